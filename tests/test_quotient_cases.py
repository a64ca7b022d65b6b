"""CPU: the many-model fleets of tests/quotient_cases.py can fail a wrong kernel.  With the
oracle alone: each tier's declared record path is what choose_format's expression gives; the
scored (x, M) pairs are many, and a tenth of them sit on each rounding edge; the f32 quotient is
exact on every tier inside the lemma and wrong on pairs of `pack16` and `wide`; three wrong
readings of CalculateCardScore, evaluated on every tier, each move the top score of a tenth of a pod sample; and the
independent Python oracle agrees with the C one.  Run with -s for the figures."""
import functools

import numpy as np
import pytest

import oracle
import pyoracle as po
import quotient_cases as qc
from test_exactness import ru32 as ru32_lemma

U = np.uint64


@functools.lru_cache(maxsize=None)
def _want(name):
    t = qc.tier(name)
    return oracle.schedule(t.nodes, t.pods, 0, threads=8)


@functools.lru_cache(maxsize=None)
def _census(name):
    return qc.pair_census(qc.tier(name), _want(name))


def _f32_wrong(pairs):
    x, M = pairs[:, 0], pairs[:, 1]
    return qc.quot32(x, M) != x * U(100) // M


def test_reciprocal_matches_the_lemma_check():
    M = np.arange(1, 1 << 16, dtype=np.uint64)
    np.testing.assert_array_equal(qc.ru32(M), ru32_lemma(M))
    assert int(qc.quot32([77813], [78599])[0]) == 99 and 77813 * 100 // 78599 == 98
    bad = qc.f32_failing(qc.N32_FIELD_MAX)
    assert bad.size and 77813 in qc.f32_failing(78599)


@pytest.mark.parametrize("name", qc.TIERS)
def test_declared_path_is_choose_formats(name):
    t = qc.tier(name)
    path, small_max, ranks, grouped = qc.predict_format(t.nodes)
    assert path == t.path
    assert (small_max <= qc.F32_SMALL_MAX) == t.flags["small_le"]
    assert ranks == t.flags["ranks"] and grouped == t.flags["grouped"]
    assert (_want(name).status == 0).mean() > 0.8
    if name in ("pack16", "wide"):   # without the one-model shortcut every node counts as mixed
        assert qc.predict_format(t.nodes, no_uniform=True)[0] == "f64"
    if name == "pack16":
        assert qc.F32_SMALL_MAX < small_max <= qc.PACK16_MAX
        for f in qc.SMALL:
            col = getattr(t.nodes, "card_" + f)
            assert (col == 55739).any() and (col == 65535).any(), f
    if name in ("q32", "q32_grouped", "q32_mixed", "ranks"):
        for f in qc.SMALL:
            assert int(getattr(t.nodes, "card_" + f).max()) == qc.F32_SMALL_MAX, f
    real = np.arange(t.nodes.max_cards)[None, :] < t.nodes.card_count[:, None]
    clocks = np.unique(t.nodes.card_clock[real]).size
    if name in ("q32", "q32_mixed", "ranks", "pack16"):
        assert clocks >= 200
    if name == "q32_grouped":
        assert clocks <= 48


def test_score32_sits_on_the_u32_bound():
    c, k = qc.SCORE32_CLOCK, qc.SCORE32_K
    assert c == 2_684_346 and k * (800 + c * 100) == 4_294_966_400
    t = qc.tier("score32")
    ask = (t.pods.has_clock == 1) & (t.pods.clock == U(c))
    w = _want("score32")
    assert (ask & (w.status == 0)).sum() >= 30
    assert (w.maxima[ask & (w.status == 0), 0] == 1).all()      # MaxBandwidth = 1
    hot = (t.nodes.card_clock[:, 0] == U(c))
    assert (t.nodes.card_count[hot] == k).any()


def test_field44_holds_the_last_fast_value():
    for name, top in (("field44", 1 << 44), ("field44_plus1", (1 << 44) + 1)):
        nd = qc.tier(name).nodes
        assert int(nd.card_total_memory.max()) == top == int(nd.card_free_memory.max())
        assert (_want(name).maxima[:, 3] == U(top)).any()        # a pod scores against it


@pytest.mark.parametrize("name", qc.BIG_TIERS)
def test_pair_coverage(name):
    """>= 500 distinct scored (x, M) per field; >= 1/10 exact quotients; >= 1/10 near-integer."""
    figures = []
    for f in qc.FIELDS:
        pairs = _census(name)[f]
        x, M = pairs[:, 0].astype(object), pairs[:, 1].astype(object)
        r = x * 100 % M
        exact, near = int((r == 0).sum()), int((r >= M - 100).sum())
        wrong = 0 if f == "total" else int(_f32_wrong(pairs).sum())
        figures.append(f"{f} {len(pairs)} ({exact} exact, {near} near, {wrong} f32-wrong)")
        assert len(pairs) >= 500, (name, f, len(pairs))
        assert exact * 10 >= len(pairs), (name, f, exact, len(pairs))
        assert near * 10 >= len(pairs), (name, f, near, len(pairs))
    print(f"\n{name}: " + "; ".join(figures))


@pytest.mark.parametrize("name", qc.LEMMA_TIERS)
def test_f32_quotient_exact_inside_the_lemma(name):
    """No scored small-field pair of these tiers has a wrong f32 quotient."""
    for f in qc.SMALL:
        assert not _f32_wrong(_census(name)[f]).any(), (name, f)


def test_f32_quotient_wrong_on_pack16():
    """>= 20 scored pairs of `pack16` where f32 differs -- clocks in 55739..65535 over the small
    MaxBandwidth values of PACK16_BANDWIDTHS (for x <= M <= 65535 there is none) -- and a pod
    whose top score would change: f32 quotients on this tier, a kF32SmallMax misplaced anywhere
    up to 65535, do not pass."""
    lo, hi = qc.F32_SMALL_MAX + 1, qc.PACK16_MAX
    for M in qc.PACK16_BANDWIDTHS:
        assert qc.f32_failing_range(M, lo, hi).size >= 10, M
    pairs = _census("pack16")["clock"]
    bad = pairs[_f32_wrong(pairs)]
    print(f"\npack16: {len(bad)} scored clock / MaxBandwidth pairs with a wrong f32 quotient")
    assert len(bad) >= 20
    assert np.isin(bad[:, 1], qc.PACK16_BANDWIDTHS).all() and (bad[:, 0] >= U(lo)).all()
    for f in ("bandwidth", "core", "power"):       # x <= M <= 65535: none
        assert not _f32_wrong(_census("pack16")[f]).any(), f
    t, w = qc.tier("pack16"), _want("pack16")
    ask = np.flatnonzero((w.status == 0) & (t.pods.has_clock == 1) &
                         np.isin(t.pods.clock, bad[:, 0]))
    moved = sum(qc.evaluate(t.nodes, t.pods, int(p), "f32")[1] != w.top_score[p] for p in ask)
    print(f"pack16: {moved} of the {ask.size} pods that ask for such a clock move under f32")
    assert moved >= 1


def test_f32_quotient_wrong_on_wide():
    """>= 100 scored pairs of `wide` where f32 differs, and a pod whose pick or top score would
    change with f32 quotients."""
    wrong = sum(int(_f32_wrong(_census("wide")[f]).sum()) for f in qc.SMALL)
    print(f"\nwide: {wrong} scored pairs with a wrong f32 quotient")
    assert wrong >= 100
    t, w = qc.tier("wide"), _want("wide")
    moved = 0
    for p in np.flatnonzero(w.status == 0)[:48]:
        pick, top, _, _ = qc.evaluate(t.nodes, t.pods, int(p), "f32")
        moved += pick != w.pick[p] or top != w.top_score[p]
    print(f"wide: {moved} of 48 pods move under f32 quotients")
    assert moved >= 1


MUTANT_TIERS = qc.TIERS


@functools.lru_cache(maxsize=None)
def _sample(name):
    t, w = qc.tier(name), _want(name)
    ok = np.flatnonzero(w.status == 0)
    return ok[np.linspace(0, ok.size - 1, 64).astype(np.int64)]


@pytest.mark.parametrize("name", MUTANT_TIERS)
def test_integer_restatement_is_the_oracle(name):
    """card_score restated in integers (quotient_cases.evaluate) gives the C oracle's pick, top
    score and feasible count on the 64-pod sample: the mutants below differ from it only in
    their reading."""
    t, w = qc.tier(name), _want(name)
    for p in _sample(name):
        pick, top, nf, _ = qc.evaluate(t.nodes, t.pods, int(p))
        assert (pick, top, nf) == (w.pick[p], w.top_score[p], w.n_feasible[p]), (name, p)


@pytest.mark.parametrize("reading", ["nearest", "maxclock", "wrap32", "wrap31"])
def test_wrong_readings_move_top_scores(reading):
    """The reciprocal rounded to nearest, the clock over MaxClock, the card scores summed modulo
    2^32: each changes the top score of >= 10 % of the 64-pod sample of some tier.  The 2^32 wrap
    does so in score32's twin with one more clock: in score32 itself no sum reaches 2^32 (that
    is what choose_format's bound K * (800 + max clock quotient) < 2^32 guarantees, 4,294,966,400
    being the largest), so there the reading that moves the sample is a sum modulo 2^31 -- a
    signed accumulator."""
    share = {}
    for name in MUTANT_TIERS:
        t, w = qc.tier(name), _want(name)
        moved = 0
        for p in _sample(name):
            _, top, _, _ = qc.evaluate(t.nodes, t.pods, int(p), reading, f32=t.flags["small_le"])
            moved += top != w.top_score[p]
        share[name] = moved / 64
    print(f"\n{reading}: " + ", ".join(f"{k} {v:.2f}" for k, v in share.items()))
    assert max(share.values()) >= 0.1
    if reading == "wrap32":
        assert share["score32"] == 0.0 and share["score32_plus1"] >= 0.1
    if reading == "wrap31":
        assert share["score32"] >= 0.1


@pytest.mark.parametrize("name", qc.TIERS)
def test_python_oracle_agrees(name):
    t, w = qc.tier(name), _want(name)
    idx = np.linspace(0, t.pods.n_pods - 1, 16).astype(np.int64)
    scvs, plist = oracle.to_py(t.nodes, t.pods.take(idx))
    for k, p in enumerate(idx):
        r = po.schedule_one(plist[k], scvs, 0)
        assert (r.pick, r.status, r.n_feasible) == (w.pick[p], w.status[p], w.n_feasible[p]), p
        assert r.maxima == [int(v) for v in w.maxima[p]], p
        if r.status == 0:
            assert (r.top_score, r.n_ties) == (w.top_score[p], w.n_ties[p]), p
