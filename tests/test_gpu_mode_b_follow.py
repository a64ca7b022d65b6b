"""Mode B with yoda_mode_b_follow on: the batch path honours the absent nodes
(yoda_set_node_present) and the candidate classes (yoda_set_candidates).  Pod p's cycle must be
the oracle's Mode B cycle on the nodes of E(p) = present and candidates of p's class, picks as ids
of the uploaded snapshot.  Every pod is compared with mode_b_follow_cases.reference (the oracle on
the compacted snapshot, per class); tests/test_mode_b_follow_cases.py shows that the scenarios fail
a handle that ignores E.  Both launch forms (lane = node up to 64 effective classes, lane = class
above), the level-0 settle, chunks and classes with no eligible node, class 63, ANY pods among
candidates and absent nodes, the rows, the draw, greedy, and the invalidation of the lazily
built tables."""
import numpy as np
import pytest

import mode_b_follow_cases as cases
import oracle
from candidate_cases import Model
from node_present_cases import _present, remap
from test_gpu_mode_b import boundary_nodes, pods_with
from tie_draw_cases import draw
from yoda_amd import synth
from yoda_amd.capi import Yoda, YodaError, comm_run_local
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

ANY = cases.ANY
SEED = 0xB10CFACE


class Handle:
    """One long-lived handle with the setting on and the model of what it was told."""

    def __init__(self, nodes, follow=True):
        self.model = Model(nodes)
        self.dev = Yoda(0)
        self.dev.upload_nodes(nodes)
        if follow:
            self.dev.mode_b_follow(True)

    def apply(self, step):
        self.model.apply(step)
        if step[0] == "cand":
            self.dev.set_candidates(step[2], step[1])
        elif step[0] == "update":
            self.dev.update_candidates(step[1], step[2])
        elif step[0] == "classes":
            self.dev.set_pod_classes(step[1])
        elif step[0] == "present":
            self.dev.set_node_present(step[1], step[2])
        else:
            raise ValueError(step[0])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.dev.close()


def expected_info(model, pods):
    """(effective classes D', 1 when some E is not the whole snapshot) of this state."""
    cls = cases.classes_of(model, pods.n_pods)
    keyed = bool((cls != ANY).any())
    by = cls if keyed else np.zeros(pods.n_pods, np.uint8)
    d = len({(float(a), int(b), int(c)) for a, b, c in zip(pods.rio, pods.rcpu, by)})
    return d, int(keyed or not model.present.all())


def check(h, pods, tag):
    """run + download and eval against the reference; the launch form through mode_b_info."""
    want = cases.reference(h.model, pods)
    h.dev.upload_pods(pods)
    h.dev.run(MODE_DISKIO)
    cases.assert_same(h.dev.download(), want, tag)
    info = h.dev.mode_b_info()
    assert (info[1], info[2]) == expected_info(h.model, pods), tag
    cases.assert_same(h.dev.eval(pods, MODE_DISKIO), want, tag + " (eval)")
    pick, status = h.dev.download_picks()
    np.testing.assert_array_equal(pick, want.pick, err_msg=tag)
    np.testing.assert_array_equal(status, want.status, err_msg=tag)
    return want


def replay(h, pods, steps):
    k = 0
    for step in steps:
        if step[0] == "check":
            check(h, pods, step[1])
            k += 1
        else:
            h.apply(step)
    return k


@pytest.mark.parametrize("distinct", [False, True])
def test_walk(distinct):
    """candidate_cases.WALK and presence steps on 5,000 nodes x 700 pods: one spec (8 classes and
    ANY: D' = 9, lane = node) and 700 distinct requests (lane = class)."""
    nodes, pods, steps = cases.walk(distinct)
    with Handle(nodes) as h:
        for s in steps[:3]:
            h.apply(s)
        check(h, pods, steps[3][1])
        assert h.dev.mode_b_info()[1:3] == ((700, 1) if distinct else (9, 1))
        assert replay(h, pods, steps[4:]) == len(cases.cc.WALK)
        assert h.dev.mode_b_info()[2] == 0  # every node back, candidates off
        assert h.dev.nodes_absent == 0


def ragged_state(n_nodes, n_specs, seed):
    nodes, _ = synth.make_config(2, pods=1, nodes=n_nodes)
    rng = np.random.default_rng(seed)
    pods = pods_with(rng.random(n_specs) * 20.0, rng.integers(1, 2000, n_specs))
    words = rng.integers(0, 8, n_nodes).astype(np.uint64)  # 3 classes, random words
    cls = rng.integers(0, 4, n_specs).astype(np.uint8)
    cls[cls == 3] = ANY
    gone = np.flatnonzero(rng.random(n_nodes) < 0.3)
    return nodes, pods, words, cls, gone


@pytest.mark.parametrize("n_nodes", [1, 2, 63, 65, 2047, 2048, 2049, 5000])
def test_ragged_sizes(n_nodes):
    """3 classes and ANY, random words, about 30 % of the nodes absent; 3 specs (lane = node) and
    700 (lane = class).  N = 1 also with its node absent, and with its word empty."""
    for n_specs in (3, 700):
        nodes, pods, words, cls, gone = ragged_state(n_nodes, n_specs, n_nodes + n_specs)
        with Handle(nodes) as h:
            for s in (("cand", 3, words), ("classes", cls), _present(gone, 0)):
                h.apply(s)
            check(h, pods, f"N {n_nodes} specs {n_specs}")
            if n_nodes == 1:
                h.apply(("update", np.zeros(1, np.uint32), np.zeros(1, np.uint64)))
                h.apply(_present([0], 1))
                want = check(h, pods, "N 1, word 0")
                assert (want.n_feasible[cls != ANY] == 0).all()
                assert (want.n_feasible[cls == ANY] == 1).all()
                h.apply(_present([0], 0))
                want = check(h, pods, "N 1, absent")
                assert (want.status == 1).all() and (want.pick == -1).all()


def test_every_eligible_node_scores_zero():
    """cpu = 1000 (V = 10) and a NaN pod: every node is at level 0, which is settled from the
    eligible nodes seen, not from the chunk's bounds.  Nodes 0..2,100 are hidden from class 0 (the
    first lane = node chunk of 2,048 is empty) and so is the first node of every later chunk."""
    nodes, _ = synth.make_config(2, pods=1, nodes=6500)
    nodes.cpu = np.full(nodes.n_nodes, 1000.0)
    nodes = nodes.normalized()
    words = np.full(nodes.n_nodes, 3, np.uint64)
    hidden = np.concatenate([np.arange(2101), [4096, 6144]])
    words[hidden] = 2
    rng = np.random.default_rng(4)
    few = pods_with([0.0, 0.0, 10.0, 0.0], [0, 100, 1000, 0])  # NaN, alpha = 1, ...
    many = pods_with(np.concatenate([[0.0], 0.5 + rng.random(200) * 4.5]),
                     np.concatenate([[0], rng.integers(1000, 4000, 200)]))
    for pods in (few, many):
        cls = (np.arange(pods.n_pods) % 2).astype(np.uint8)
        with Handle(nodes) as h:
            for s in (("cand", 2, words), ("classes", cls), _present([2101, 2500], 0)):
                h.apply(s)
            want = check(h, pods, f"{pods.n_pods} pods")
            assert h.dev.mode_b_info()[1] > 64 or pods.n_pods == 4
            e0 = nodes.n_nodes - hidden.size - 2  # class 0: 2,101 and 2,500 are absent
            assert (want.n_ties[cls == 0] == e0).all() and (want.pick[cls == 0] == 2102).all()
            assert (want.n_ties[cls == 1] == nodes.n_nodes - 2).all()
            assert (want.pick[cls == 1] == 0).all() and (want.top_score == 0).all()


@pytest.mark.parametrize("k", range(1, 11))
def test_level_boundary_hidden_from_a_class(k):
    """test_gpu_mode_b.boundary_nodes(k): the nodes within 6 ulps of level k's threshold.  Class 1
    loses every node at level k of pod 0 (alpha = 1, beta = 0): its best level drops below k,
    while class 0 and the ANY pod keep it."""
    for extra in (0, 3000):
        nodes = boundary_nodes(k, n_extra=extra)
        pods = pods_with([0.0, 0.0, 0.0, 10.0, 0.0], [100, 100, 100, 100, 0])
        raw = oracle.pod_detail(nodes, pods, 0, MODE_DISKIO)[2]
        assert raw.max() == k
        words = np.full(nodes.n_nodes, 3, np.uint64)
        words[raw == k] = 1
        cls = np.array([1, 0, ANY, 1, 1], np.uint8)
        with Handle(nodes) as h:
            h.apply(("cand", 2, words))
            h.apply(("classes", cls))
            want = check(h, pods, f"level {k}")
            assert want.top_score[0] < k and want.top_score[1] == k and want.top_score[2] == k
            assert h.dev.mode_b_info()[2] == 1


def test_class_63_of_64():
    nodes, pods = synth.make_config(2, pods=300, nodes=2500)
    pods = synth.distinct_diskio(pods)
    rng = np.random.default_rng(63)
    words = rng.integers(0, 2 ** 63, nodes.n_nodes, dtype=np.uint64)
    words[rng.random(nodes.n_nodes) < 0.5] |= np.uint64(1 << 63)
    cls = np.where(np.arange(300) % 3 == 0, 62, 63).astype(np.uint8)
    with Handle(nodes) as h:
        h.apply(("cand", 64, words))
        h.apply(("classes", cls))
        want = check(h, pods, "class 63")
        assert (want.n_feasible[cls == 63] == int((words >> np.uint64(63)).sum())).all()
        blind = oracle.schedule(nodes, pods, MODE_DISKIO, threads=8)
        assert (want.pick != blind.pick).sum() > 100


def test_score_rows_norm_and_bitmask():
    """3 pods x 300 nodes: the feasibility bits are E, a node outside E has raw and normalized
    score -1, NormalizeScore takes highest and lowest over E."""
    nodes, _ = synth.make_config(2, pods=1, nodes=300)
    rng = np.random.default_rng(8)
    pods = pods_with(rng.random(3) * 20.0, rng.integers(1, 2000, 3))
    words = rng.integers(0, 4, 300).astype(np.uint64)
    cls = np.array([0, 1, ANY], np.uint8)
    with Handle(nodes) as h:
        for s in (("cand", 2, words), ("classes", cls), _present(rng.choice(300, 40, False), 0)):
            h.apply(s)
        h.dev.upload_pods(pods)
        feas, raw, norm = h.dev.score_rows(MODE_DISKIO, norm=True)
        feas2, raw2 = h.dev.score_rows(MODE_DISKIO)
        for p in range(3):
            d = cases.detail(h.model, pods, p)
            assert 2 <= d["feas"].sum() < 300
            np.testing.assert_array_equal(feas[p], d["feas"], err_msg=f"bits {p}")
            np.testing.assert_array_equal(raw[p], d["raw"], err_msg=f"raw {p}")
            np.testing.assert_array_equal(norm[p], d["norm"], err_msg=f"norm {p}")
            np.testing.assert_array_equal(feas2[p], d["feas"])
            np.testing.assert_array_equal(raw2[p], d["raw"])
        cases.assert_same(h.dev.download(), cases.reference(h.model, pods), "after the rows")


@pytest.mark.parametrize("distinct", [False, True])
def test_tie_draw_within_E(distinct):
    """With yoda_set_tie_draw on, every tied pod's pick is the member of its tie set within E with
    the smallest (yoda_tie_hash << 32) | node; everything else as with the draw off."""
    nodes, pods, steps = cases.scenario(distinct)
    P = 700 if not distinct else 120
    pods = pods.slice(0, P)
    with Handle(nodes) as h:
        for s in steps[:2]:
            h.apply(s)
        h.apply(("classes", steps[2][1][:P]))
        want = cases.reference(h.model, pods)
        on = want.pick.copy()
        cls = cases.classes_of(h.model, P)
        sets = {}
        for p in np.flatnonzero((want.status == 0) & (want.n_ties >= 2)).tolist():
            key = p if distinct else int(cls[p])
            if key not in sets:
                sets[key] = cases.detail(h.model, pods, p)["ties"]
            assert sets[key].size == want.n_ties[p]
            on[p] = draw(SEED, p, sets[key])
        assert (on != want.pick).sum() >= P // 4
        h.dev.set_tie_draw(SEED)
        got = h.dev.eval(pods, MODE_DISKIO)
        np.testing.assert_array_equal(got.pick, on)
        for f in ("status", "n_feasible", "n_ties", "top_score"):
            np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
        h.dev.set_tie_draw(None)
        cases.assert_same(h.dev.eval(pods, MODE_DISKIO), want, "draw off")


def test_greedy_with_absent_nodes():
    """yoda_greedy in Mode B is a batch of independent cycles in queue order: with nodes absent
    it equals oracle.greedy on the compacted snapshot; with candidates on it keeps refusing."""
    nodes, _ = synth.make_config(2, pods=1, nodes=3000)
    pods = synth.distinct_diskio(synth.make_pods(400, 17, priorities=True))
    blind, _ = oracle.greedy(nodes, pods, MODE_DISKIO, 0)
    # every node the whole snapshot's greedy picks leaves, with 500 random others
    gone = np.union1d(np.unique(blind[blind >= 0]),
                      np.random.default_rng(2).choice(3000, 500, replace=False))
    with Handle(nodes) as h:
        h.apply(_present(gone, 0))
        keep = h.model.keep()
        pick, _ = oracle.greedy(nodes.take(keep), pods, MODE_DISKIO, 0)
        assert (remap(pick, keep) != blind).all()
        np.testing.assert_array_equal(h.dev.greedy(pods, MODE_DISKIO, 0), remap(pick, keep))
        h.apply(("cand", 2, np.full(3000, 3, np.uint64)))
        with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
            h.dev.greedy(pods, MODE_DISKIO, 0)
        assert "candidate" in str(e.value)


def test_invalidation():
    """The tables follow every change of the state between two runs on the same uploaded pods,
    and the build counter (mode_b_info out[3]) moves only when a table changed."""
    nodes, pods, steps = cases.scenario(True)
    present, cand, classes = steps[:3]
    with Handle(nodes) as h:
        dev = h.dev

        def run(tag, builds):
            want = cases.reference(h.model, pods)
            dev.run(MODE_DISKIO)
            cases.assert_same(dev.download(), want, tag)
            assert dev.mode_b_info()[3] == builds, tag
            return want

        dev.upload_pods(pods)
        run("as uploaded", 0)                      # nothing to follow: no table
        h.apply(present)
        run("absent", 1)
        run("absent again", 1)
        h.apply(_present(present[1][:40], 1))      # set_node_present between two runs
        run("40 back", 2)
        h.apply(_present(present[1][:40], 1))      # unchanged flags: nothing to rebuild
        run("40 back again", 2)
        h.apply(cand)
        h.apply(classes)
        a = run("candidates", 3)
        h.apply(("classes", np.roll(classes[1], 1)))   # set_pod_classes, no upload_pods
        b = run("classes rolled", 3)
        assert (a.pick != b.pick).sum() > 100
        ids = np.flatnonzero(cand[2] == 0)[:50].astype(np.uint32)
        h.apply(("update", ids, np.full(ids.size, 0xFF, np.uint64)))
        run("update_candidates", 4)
        # a Mode A run between two Mode B runs on one handle
        snap = cases.cc.Snapshot(h.model, pods)
        want_a, _ = cases.cc.reference(snap, h.model)
        dev.run(MODE_SCV)
        got = dev.download()
        for f in ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima"):
            np.testing.assert_array_equal(getattr(got, f), getattr(want_a, f), err_msg=f)
        run("after Mode A", 4)
        h.apply(("classes", None))                 # every pod ANY: presence alone
        c = run("all ANY", 4)
        assert (c.n_feasible == int(h.model.present.sum())).all()
        # upload_nodes: every node present, candidates off
        dev.upload_nodes(nodes)
        h.model = Model(nodes)
        assert dev.mode_b_info()[0] == 1           # a setting: it stays across uploads
        dev.upload_pods(pods)
        d = run("re-uploaded", 0)
        cases.assert_same(d, oracle.schedule(nodes, pods, MODE_DISKIO, threads=8), "whole")
        assert dev.mode_b_info()[2] == 0


def test_setting_on_with_nothing_to_follow():
    """Nothing absent and candidates off, or on with every pod ANY: the oracle's answers from the
    unchanged kernels (mode_b_info out[2] == 0), no table built."""
    nodes, pods = cases.workload(True)
    want = oracle.schedule(nodes, pods, MODE_DISKIO, threads=8)
    with Handle(nodes) as h:
        cases.assert_same(h.dev.eval(pods, MODE_DISKIO), want, "on")
        assert h.dev.mode_b_info() == (1, 700, 0, 0)
        h.apply(("cand", 4, np.zeros(nodes.n_nodes, np.uint64)))
        cases.assert_same(h.dev.eval(pods, MODE_DISKIO), want, "every pod ANY")
        h.apply(("classes", np.full(700, ANY, np.uint8)))
        cases.assert_same(h.dev.eval(pods, MODE_DISKIO), want, "ANY bytes")
        assert h.dev.mode_b_info() == (1, 700, 0, 0)
        h.dev.upload_pods(pods.slice(0, 300))      # the class array must fit the batch
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            h.dev.run(MODE_DISKIO)


def test_on_then_off_and_what_stays_refused():
    """Off again, the refusals return with their messages; with the setting on the communicator
    runs and the bitmask download keep refusing."""
    nodes, pods = synth.make_config(2, pods=300, nodes=1500)
    with Handle(nodes) as h:
        dev = h.dev
        h.apply(_present([700], 0))
        check(h, pods, "on")
        dev.upload_pods(pods)
        with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
            comm_run_local([dev], MODE_DISKIO)
        assert "absent" in str(e.value)
        dev.run(MODE_DISKIO, bitmask=True)
        with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
            dev.download_bitmask()
        assert "Mode A" in str(e.value)
        dev.mode_b_follow(False)
        assert dev.mode_b_info()[0] == 0
        for call in (lambda: dev.eval(pods, MODE_DISKIO), lambda: dev.run(MODE_DISKIO),
                     lambda: dev.score_rows(MODE_DISKIO),
                     lambda: dev.greedy(pods.slice(0, 50), MODE_DISKIO, 0)):
            with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
                call()
            assert "Mode B does not honour absent nodes" in str(e.value)
        h.apply(_present([700], 1))
        h.apply(("cand", 2, np.full(1500, 1, np.uint64)))
        dev.upload_pods(pods)
        with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
            dev.run(MODE_DISKIO)
        assert "Mode B does not honour candidate classes" in str(e.value)
        dev.mode_b_follow(True)
        h.apply(("classes", np.ones(300, np.uint8)))
        want = check(h, pods, "on again")
        assert (want.status == 1).all()            # class 1 is a candidate nowhere
        with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
            comm_run_local([dev], MODE_DISKIO)
        assert "candidate" in str(e.value)
