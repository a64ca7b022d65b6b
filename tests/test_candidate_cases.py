"""The candidate-class scenarios of tests/candidate_cases.py, with the oracle alone (no GPU): the
reference is right where it can be checked against an independent statement, and every scenario
moves enough outcomes that a handle which ignored the words, or read a non-candidate as an absent
node (the maxima following), would fail tests/test_gpu_candidates.py."""
import ctypes as C

import numpy as np
import pytest

import candidate_cases as cases
import oracle
import pyoracle
from yoda_amd.soa import MODE_SCV

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")

# floors: base as the issue states them; small and c4 half of what the recipe gave when it was
# first measured (460 / 199 / 6 / 134 / 7 and 581 / 881 / 43 / 196 / 4), rounded up
FLOORS = {"base": (1000, 100, 1, 100, 4), "small": (230, 100, 3, 67, 4), "c4": (291, 441, 22, 98, 2)}


@pytest.fixture(scope="module")
def snaps():
    out = {}

    def get(shape):
        if shape not in out:
            nd, pd, steps = cases.walk(shape, mixed_pods=3000)
            out[shape] = (nd, pd, steps, cases.Snapshot(cases.Model(nd), pd))
        return out[shape]
    return get


@pytest.mark.parametrize("shape", ["base", "small", "c4"])
def test_all_ones_words_equal_the_oracle(snaps, shape):
    nd, pd, _, snap = snaps(shape)
    m = cases.Model(nd)
    m.apply(("cand", 64, np.full(nd.n_nodes, cases.FULL, np.uint64)))
    m.apply(("classes", (np.arange(pd.n_pods) % 64).astype(np.uint8)))
    got, _ = cases.reference(snap, m)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(snap.full, f), err_msg=f)


def test_reference_equals_a_direct_composition(snaps):
    """40 pods of small under the recipe: pyoracle.fits and the class bit for F', the maxima of
    collect_max_values over EVERY node, and schedule_one's tail over F'."""
    nd, pd, steps, snap = snaps("small")
    m = cases.states(nd, steps)[0][1]
    scvs, plist = oracle.to_py(nd, pd)
    for p in np.random.default_rng(1).choice(pd.n_pods, 40, replace=False).tolist():
        pod, cand = plist[p], m.candidates(p)
        mv = pyoracle.collect_max_values(pod, scvs)
        fp = [i for i, s in enumerate(scvs) if pyoracle.fits(pod, s)[0] and cand[i]]
        d = cases.detail(snap, m, p)
        assert d["n_feasible"] == len(fp) and np.flatnonzero(d["feas"]).tolist() == fp
        assert snap.full.maxima[p].tolist() == mv.as_list()
        if len(fp) < 2:
            assert d["status"] == (0 if fp else 1) and d["pick"] == (fp[0] if fp else -1)
            continue
        sc = [pyoracle._score(pod, scvs[i], mv, 0, None, i) for i in fp]
        hi, lo = max(0, max(sc)), min(sc)
        lo -= hi == lo
        norm = [pyoracle._go_div(pyoracle._to_i64((v - lo) * 100), hi - lo) for v in sc]
        ties = [fp[k] for k, v in enumerate(norm) if v == max(norm)]
        assert (d["status"], d["pick"], d["n_ties"]) == (0, ties[0], len(ties))
        assert d["ties"].tolist() == ties and d["top_score"] == sc[fp.index(ties[0])]
        assert d["norm"][fp].tolist() == norm and d["raw"][fp].tolist() == sc


@pytest.mark.parametrize("shape", ["base", "small", "c4"])
def test_recipe_clears_the_floors(snaps, shape):
    nd, pd, steps, snap = snaps(shape)
    m = cases.states(nd, steps)[0][1]
    ref, _ = cases.reference(snap, m)
    ab = cases.as_absent(m, pd)
    ok = (ref.status == 0) & (ab.status == 0)
    got = ((ref.pick != snap.full.pick).sum(), (ref.n_feasible == 0).sum(),
           (ref.n_feasible == 1).sum(), (ref.top_score[ok] != ab.top_score[ok]).sum(),
           (ref.pick != ab.pick).sum())
    print(shape, "moved / none / one / top_score vs absent / picks vs absent:", got)
    assert all(g >= f for g, f in zip(got, FLOORS[shape])), (got, FLOORS[shape])


@pytest.mark.parametrize("shape", ["small", "c4", "mixed", "ranks", "f64", "u64"])
def test_every_walk_check_moves_outcomes(snaps, shape):
    """Each check of the walk differs from no candidates in picks or counts -- except the two that
    must not (every pod ANY, candidates off) -- and from the check before it."""
    nd, pd, steps, snap = snaps(shape)
    prev = None
    for k, (tag, m) in enumerate(cases.states(nd, steps)):
        ref, _ = cases.reference(snap, m)
        moved = int((ref.pick != snap.full.pick).sum() + (ref.n_feasible != snap.full.n_feasible).sum())
        if k in (cases.WALK_ANY, cases.WALK_OFF):
            assert moved == 0, tag
        else:
            assert moved >= pd.n_pods // 20, tag
        if prev is not None and k != 5:
            assert (ref.n_feasible != prev.n_feasible).any(), tag
        np.testing.assert_array_equal(ref.maxima, snap.full.maxima, err_msg=tag)
        prev = ref


def test_maxima_holder_differs_from_absence():
    nd, pd, steps, holders = cases.maxima_holder()
    m = cases.states(nd, steps)[1][1]
    snap = cases.Snapshot(cases.Model(nd), pd)
    ref, _ = cases.reference(snap, m)
    ab = cases.as_absent(m, pd)
    np.testing.assert_array_equal(ref.maxima, snap.full.maxima)
    assert (ab.maxima != ref.maxima).any(axis=1).mean() >= 0.25
    ok = (ref.status == 0) & (ab.status == 0)
    assert (ref.top_score[ok] != ab.top_score[ok]).sum() >= 100
    assert (ref.pick != ab.pick).sum() >= 1
    assert not np.isin(ref.pick[ref.pick >= 0], holders).any()


def test_zero_total_follows_the_candidates():
    nd, pd, steps, s, p = cases.zero_total()
    snap = cases.Snapshot(cases.Model(nd), pd)
    st = [cases.detail(snap, m, p) for _, m in cases.states(nd, steps)]
    assert st[0]["status"] == 2 and st[1]["status"] == 0 and st[1]["n_feasible"] >= 3
    assert (st[2]["status"], st[2]["pick"], st[2]["n_feasible"], st[2]["n_ties"]) == (0, s, 1, 1)
    assert st[3]["status"] == 2


def test_with_absent_and_overflow_scenarios():
    nd, pd, steps = cases.with_absent()
    refs = []
    for tag, m in cases.states(nd, steps):
        snap = cases.Snapshot(m, pd)
        ref, _ = cases.reference(snap, m)
        assert not np.isin(ref.pick[ref.pick >= 0], m.absent()).any(), tag
        refs.append((ref, snap.full))
    assert (refs[0][1].maxima != refs[1][1].maxima).any()  # the updates show
    # ... in what a handle that dropped them would get wrong: counts of one pod in twenty at
    # least, and some picks
    assert (refs[0][0].n_feasible != refs[1][0].n_feasible).sum() >= pd.n_pods // 20
    assert (refs[0][0].pick != refs[1][0].pick).any()
    nd, pd, steps = cases.overflow()
    (_, m0), (_, m1) = cases.states(nd, steps)
    snap = cases.Snapshot(m0, pd)
    r0, _ = cases.reference(snap, m0)
    r1, _ = cases.reference(snap, m1)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(r0, f), getattr(snap.full, f), err_msg=f)
    assert (r0.status == 3).all()
    assert (r1.n_feasible < r0.n_feasible).all() and (r1.n_feasible >= 1).all()


def test_null_handle_and_arguments():
    """A NULL handle is YODA_ERR_INVALID_ARG from every call, whatever the other arguments.  That
    is all that runs without a device: a handle needs one, so the validation of n_classes, class
    bytes and NULL arrays on a live handle is in tests/test_gpu_candidates.py
    (test_state_and_failed_calls)."""
    from yoda_amd.capi import ERRORS, lib
    L = lib()
    w = (C.c_uint64 * 4)()
    ids = (C.c_uint32 * 4)()
    cls = (C.c_uint8 * 4)()
    out = (C.c_uint32 * 3)()
    INVALID = {v: k for k, v in ERRORS.items()}["YODA_ERR_INVALID_ARG"]
    assert L.yoda_set_candidates(None, 65, w) == INVALID
    assert L.yoda_set_candidates(None, 1, w) == INVALID
    assert L.yoda_set_candidates(None, 0, None) == INVALID
    assert L.yoda_update_candidates(None, 4, ids, w) == INVALID
    assert L.yoda_update_candidates(None, 0, None, None) == INVALID
    assert L.yoda_set_pod_classes(None, 4, cls) == INVALID
    assert L.yoda_set_pod_classes(None, 0, None) == INVALID
    assert L.yoda_candidates_info(None, out) == INVALID
    assert L.yoda_candidates_profile(None, None) == INVALID
