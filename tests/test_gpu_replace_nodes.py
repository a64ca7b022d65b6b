"""A long-lived handle under whole-record replacements (yoda_replace_nodes), across every entry
point.  At every check three things are compared, exactly and in every field of assert_same: the
handle that saw only the steps, a fresh upload of the model's snapshot, and the C oracle
(scenarios: tests/replace_cases.py; tests/test_replace_cases.py shows that each of them moves the
picks, the feasible counts or the maxima).  yoda_snapshot_check then looks at what no pick shows
-- block-grouped copies, stored block summaries, host mirrors -- and on shapes without a grouped
node order the table digests of the long-lived handle equal a fresh upload's."""
import numpy as np
import pytest

import oracle
import replace_cases as cases
from test_gpu_node_present import check_present
from test_gpu_node_state import Fleet, _scatter, assert_equal_results, check_state
from test_gpu_parity import assert_same
from yoda_amd.capi import Yoda, YodaError
from yoda_amd.soa import MODE_SCV, STATUS_DIV_ZERO

pytestmark = pytest.mark.gpu

ZERO = [0, 0, 0, 0]
SEED = 0x5EEDFACE


class ReplaceFleet(Fleet):
    """The long-lived handles of a scenario; every step goes to every handle with GLOBAL ids."""

    def __init__(self, nodes, shards=False, **upload_kw):
        super().__init__(nodes, shards=shards, **upload_kw)
        self.model = cases.Model(nodes)

    def apply(self, step):
        self.model.apply(step)
        for h in self.handles():
            if step[0] == "replace":
                h.replace_nodes(step[1], step[2])
            elif step[0] == "present":
                h.set_node_present(step[1], step[2])
            else:
                raise ValueError(step[0])

    def self_check(self, tag):
        for h in self.handles():
            assert h.snapshot_check()[1].tolist() == ZERO, tag


def fresh_digest(nodes, **kw):
    with Yoda(0) as y:
        y.upload_nodes(nodes, **kw)
        d, m = y.snapshot_check()
    assert m.tolist() == ZERO
    return d


def replay(fleet, pods, steps, entry_points, digests=False):
    """entry_points: per check index (a list, cycled) or one tuple for all.  Returns the checks."""
    k = 0
    for step in steps:
        if step[0] != "check":
            fleet.apply(step)
            continue
        eps = entry_points[k % len(entry_points)] if isinstance(entry_points, list) else entry_points
        if fleet.model.present.all():
            check_state(fleet, pods, step[1], eps)
        else:
            check_present(fleet, pods, step[1], eps)
        fleet.self_check(step[1])
        if digests:
            np.testing.assert_array_equal(fleet.dev.snapshot_check()[0],
                                          fresh_digest(fleet.model.nodes(), **fleet.kw),
                                          err_msg=step[1])
        k += 1
    return k


# ---- (a) the walk ----
@pytest.mark.parametrize("handles", ["single", "shards"])
def test_walk_base(handles):
    """Grouped node order.  single: eval, score rows, top-k lists and greedy on one handle;
    shards: the node shards of worlds 2 and 3 (ragged cuts) at every check."""
    nodes, pods, steps = cases.walk("base")
    with ReplaceFleet(nodes, shards=handles == "shards") as fleet:
        assert fleet.dev.node_order_grouped and fleet.dev.path == "n32"
        eps = ("shards",) if handles == "shards" else \
            [("eval", "rows"), ("topk", "eval"), ("greedy", "rows"), ("eval",),
             ("rows", "eval"), ("eval", "topk", "greedy")]
        assert replay(fleet, pods, steps, eps) == len(cases.WALK_SIZES)


@pytest.mark.parametrize("shape", ["small", "c4", "ranks", "f64", "u64"])
def test_walk(shape):
    """small: below the grouped order; c4: K = 16, empty CardLists, CardNumber != len, another
    card count for every replaced node; ranks: memory in bytes; f64 / u64: records only."""
    nodes, pods, steps = cases.walk(shape)
    kw = cases.UPLOAD_KW.get(shape, {})
    with ReplaceFleet(nodes, **kw) as fleet:
        dev = fleet.dev
        assert dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        assert dev.memory_ranks == (shape == "ranks")
        ungrouped = shape in ("small", "f64", "u64")
        assert dev.node_order_grouped != ungrouped
        eps = [("eval",), ("eval", "greedy")] if shape in ("f64", "u64") else \
            [("eval", "rows"), ("eval", "topk"), ("greedy", "eval")]
        assert replay(fleet, pods, steps, eps, digests=ungrouped) == len(cases.WALK_SIZES)


def test_walk_mixed_grouped_order():
    """Half the nodes with mixed GPU models: the block-grouped order needs >= 32768 pods there.
    Every pod against a fresh upload, a 2000-pod sample against the oracle."""
    nodes, pods, steps = cases.walk("mixed")
    sample = np.sort(np.random.default_rng(3).choice(pods.n_pods, 2000, replace=False))
    sub = pods.take(sample)
    with ReplaceFleet(nodes) as fleet:
        dev = fleet.dev
        assert dev.node_order_grouped
        checks = 0
        for step in steps:
            if step[0] != "check":
                fleet.apply(step)
                continue
            model_nodes = fleet.model.nodes()
            got = dev.eval(pods, MODE_SCV)
            info = dev.order_info()
            assert info["kind"] == 2 and info["work"] >= 32768
            with Yoda(0) as y:
                y.upload_nodes(model_nodes)
                assert_equal_results(got, y.eval(pods, MODE_SCV), step[1])
            want = _scatter(oracle.schedule(model_nodes, sub, MODE_SCV, threads=8), sample,
                            pods.n_pods)
            assert_same(got, want, pods=sample)
            fleet.self_check(step[1])
            checks += 1
        assert checks == len(cases.WALK_SIZES)


# ---- (b) a model the snapshot did not hold: the six G maxima up and back ----
@pytest.mark.parametrize("n", [900, 4608])
def test_new_model_moves_each_g_maximum(n):
    nodes, pods, steps = cases.new_model(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    with ReplaceFleet(nodes) as fleet:
        before = fleet.dev.snapshot_check()[0]
        eps = [("eval", "rows"), ("eval", "topk")]
        assert replay(fleet, pods, steps, eps, digests=n == 900) == 13
        if n == 900:
            np.testing.assert_array_equal(fleet.dev.snapshot_check()[0], before)


# ---- (c) whole blocks ----
@pytest.mark.parametrize("n", [900, 4608])
def test_block_clocks(n):
    nodes, pods, steps = cases.block_clocks(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    with ReplaceFleet(nodes, shards=n != 900) as fleet:
        eps = ("eval", "rows", "topk", "greedy") + (("shards",) if n != 900 else ())
        assert replay(fleet, pods, steps, eps, digests=n == 900) == 3


# ---- (d) a mixed-model node in an all-one-model snapshot, and back ----
@pytest.mark.parametrize("n", [900, 4608])
def test_mixed_and_back(n):
    nodes, pods, steps = cases.mixed_and_back(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    with ReplaceFleet(nodes) as fleet:
        assert replay(fleet, pods, steps, ("eval", "rows", "topk", "greedy"),
                      digests=n == 900) == 3


# ---- (e) spare slots ----
def test_spare_slots():
    nodes, pods, steps, slots, join = cases.spare_slots()
    with ReplaceFleet(nodes, shards=True) as fleet:
        dev = fleet.dev
        assert replay(fleet, pods, steps[:4], ("eval", "rows", "topk", "shards")) == 2
        # the records are in place while the slots are out: no bit, no pick, no count
        assert dev.nodes_absent == cases.SPARE
        dev.upload_pods(pods.slice(0, 24))
        feas, rows, _ = dev.score_rows(MODE_SCV, norm=True)
        assert not feas[:, slots].any() and (rows[:, slots] == -1).all()
        assert replay(fleet, pods, steps[4:], ("eval", "rows", "topk", "shards", "greedy")) == 1
        assert dev.nodes_absent == cases.SPARE - cases.JOIN
        # a fresh upload of the full snapshot with the other 64 taken out
        rest = np.setdiff1d(slots, join).astype(np.uint32)
        got = dev.eval(pods, MODE_SCV)
        with Yoda(0) as y:
            y.upload_nodes(fleet.model.nodes())
            y.set_node_present(rest, 0)
            assert_equal_results(got, y.eval(pods, MODE_SCV), "fresh upload, 64 out")
        assert np.isin(got.pick, join).mean() >= 0.01


# ---- (f) card counts and totals ----
def test_card_counts_and_zero_total():
    nodes, pods, steps = cases.card_counts()
    with ReplaceFleet(nodes) as fleet:
        assert replay(fleet, pods, steps, ("eval", "rows", "topk", "greedy"), digests=True) == 5
        got = fleet.dev.eval(pods, MODE_SCV)
        assert (got.status == STATUS_DIV_ZERO).mean() >= 0.01
        assert got.n_feasible[-1] == 1 and got.status[-1] == 0
        assert got.pick[-1] == int(steps[-2][1][0])


# ---- (g) every range rule ----
@pytest.mark.parametrize("k", range(len(cases.RANGE_RULES)),
                         ids=[r[0].replace(" ", "_") for r in cases.RANGE_RULES])
def test_range_rule_writes_nothing(k):
    """YODA_ERR_RANGE from the LAST record of a five-node list: nothing of the earlier ones is
    kept -- digests, mismatch words, bounds and eval are those before the call; without its last
    record the list is accepted and changes the state."""
    name, shape, _ = cases.RANGE_RULES[k]
    nodes, pods, kw, good, bad = cases.range_rule(k)
    with ReplaceFleet(nodes, **kw) as fleet:
        dev = fleet.dev
        assert dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        assert dev.memory_ranks == (shape == "ranks")
        before = dev.eval(pods, MODE_SCV)
        d0 = dev.snapshot_check()[0]
        bounds = (dev.score_bound, dev.small_field_max)
        with pytest.raises(YodaError, match="YODA_ERR_RANGE"):
            dev.replace_nodes(bad[1], bad[2])
        d1, m1 = dev.snapshot_check()
        np.testing.assert_array_equal(d1, d0)
        assert m1.tolist() == ZERO
        assert (dev.score_bound, dev.small_field_max) == bounds
        assert_equal_results(dev.eval(pods, MODE_SCV), before, "after the rejected list")
        fleet.apply(good)
        check_state(fleet, pods, "accepted prefix", ("eval",))
        assert (dev.snapshot_check()[0] != d0).any()


@pytest.mark.parametrize("rule", ["small field above 0xFFFFFFFE",
                                  "mixed-model node without f32 quotients",
                                  "memory above 0xFFFFFFFE", "f64 field above 2^44",
                                  "node score f64"], ids=lambda r: r.replace(" ", "_"))
def test_u64_takes_what_the_fast_paths_refuse(rule):
    """The exact-u64 path takes every record that fits K: the lists the 32-bit and f64 paths
    refuse for a field or a score are accepted whole."""
    k = [r[0] for r in cases.RANGE_RULES].index(rule)
    nodes, pods, _, _, bad = cases.range_rule(k)
    with ReplaceFleet(nodes, force_generic=True) as fleet:
        assert fleet.dev.path == "u64"
        fleet.apply(bad)
        check_state(fleet, pods, cases.RANGE_RULES[k][0], ("eval",))
        fleet.self_check("u64")


# ---- (h) state survives ----
def test_state_survives_a_replacement():
    """8 candidate classes, a class array, 100 absent nodes, the seeded tie draw and the diagnosis
    counts: 64 nodes are replaced, some absent, some with words other than all-ones; the handle
    answers as a fresh upload brought to the same state."""
    nodes, pods, steps = cases.walk("base")
    rng = np.random.default_rng(53)
    n = nodes.n_nodes
    ids, recs = steps[0][1], steps[0][2]
    assert ids.size == 64
    words = rng.integers(0, 256, n).astype(np.uint64)
    words[rng.random(n) < 0.5] = 0xFF
    cls = rng.integers(0, 9, pods.n_pods).astype(np.uint8)
    cls[cls == 8] = 0xFF
    gone = np.concatenate([ids[:20], rng.choice(np.setdiff1d(np.arange(n), ids), 80,
                                                replace=False)]).astype(np.uint32)
    assert (words[ids] != 0xFF).any() and (words[ids] == 0xFF).any()

    def dress(y):
        y.set_candidates(words, 8)
        y.set_pod_classes(cls)
        y.set_node_present(gone, 0)
        y.set_tie_draw(SEED)

    model = cases.Model(nodes)
    model.apply(steps[0])
    with Yoda(0) as dev, Yoda(0) as ref:
        dev.upload_nodes(nodes)
        dress(dev)
        first = dev.eval(pods, MODE_SCV)
        dev.replace_nodes(ids, recs)
        assert dev.nodes_absent == 100 and dev.candidates_info()[0] == 8
        got = dev.eval(pods, MODE_SCV)
        got_diag = dev.diagnose(all=True)
        ref.upload_nodes(model.nodes())
        dress(ref)
        want = ref.eval(pods, MODE_SCV)
        assert_equal_results(got, want, "replaced under candidates, absences and the draw")
        np.testing.assert_array_equal(got_diag, ref.diagnose(all=True))
        assert ((got.pick != first.pick) | (got.n_feasible != first.n_feasible)).mean() >= 0.01
        assert not np.isin(got.pick, gone).any()
        assert dev.snapshot_check()[1].tolist() == ZERO
        # the absent replaced nodes show their new records when they return
        dev.set_node_present(gone, 1)
        ref.set_node_present(gone, 1)
        assert_equal_results(dev.eval(pods, MODE_SCV), ref.eval(pods, MODE_SCV), "returned")


# ---- conventions, invalidation, the bounds ----
def test_conventions_and_invalidation():
    import torch
    from yoda_amd.dist import ShardBuffers
    nodes, pods, steps = cases.block_clocks(nodes=900, pods=300)
    ids, recs = steps[1][1], steps[1][2]
    with Yoda(0) as y:
        with pytest.raises(YodaError, match="YODA_ERR_NO_NODES"):
            y.replace_nodes(ids, recs)
    with ReplaceFleet(nodes) as fleet:
        dev = fleet.dev
        d0 = dev.snapshot_check()[0]
        dev.replace_nodes(np.zeros(0, np.uint32), nodes.take(np.zeros(0, np.int64)))
        # ids of another shard only: nothing to do
        dev.replace_nodes(np.array([900, 5000], np.uint32), nodes.take([0, 1]))
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)
        with pytest.raises(ValueError):
            dev.replace_nodes(ids[:3], recs)
        # a run, a replacement, a run on the SAME uploaded pods reflects the replacement
        dev.upload_pods(pods)
        dev.run(MODE_SCV)
        first = dev.download()
        fleet.apply(steps[1])
        dev.run(MODE_SCV)
        second = dev.download()
        assert_same(second, oracle.schedule(fleet.model.nodes(), pods, MODE_SCV, threads=8))
        assert (second.pick != first.pick).mean() >= 0.01
        b = ShardBuffers(pods.n_pods, torch.device("cuda:0"))
        p = ShardBuffers.ptr
        dev.shard_phase1(MODE_SCV, p(b.maxima), p(b.counts))
        fleet.apply(steps[3])
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.shard_phase2(MODE_SCV, p(b.maxima), p(b.counts), p(b.best), p(b.idx), p(b.ties),
                             p(b.lowest))
        check_state(fleet, pods, "after the refused phase 2", ("eval",))
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)


def test_upper_bounds_only_grow():
    """yoda_score_bound and yoda_small_field_max follow a larger clock up and stay there."""
    nodes, _, steps = cases.new_model(nodes=900, pods=300)

    def fresh(nd):
        with Yoda(0) as y:
            y.upload_nodes(nd)
            return y.score_bound, y.small_field_max

    with ReplaceFleet(nodes) as fleet:
        dev = fleet.dev
        assert (dev.score_bound, dev.small_field_max) == fresh(nodes)
        k = 1 + 4 * cases.MAX_FIELDS.index("card_bandwidth")
        fleet.apply(steps[k])      # bandwidth: the largest small field of the fleet
        up = fresh(fleet.model.nodes())
        assert (dev.score_bound, dev.small_field_max) == up
        assert up[1] > fresh(nodes)[1]
        fleet.apply(steps[k + 2])
        assert (dev.score_bound, dev.small_field_max) == up
        k = 1 + 4 * cases.MAX_FIELDS.index("card_clock")
        fleet.apply(steps[k])      # clock: the card term of the score bound
        up2 = fresh(fleet.model.nodes())
        assert dev.score_bound == up2[0] > up[0]
        fleet.apply(steps[k + 2])
        assert dev.score_bound == up2[0] and dev.small_field_max == up[1]
