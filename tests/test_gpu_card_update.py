"""A long-lived handle under sparse card-metric updates (yoda_update_node_cards), across every
entry point.  At every check three things are compared, exactly and in every field of
assert_same: the handle that saw only the steps, a fresh upload of the model's snapshot, and the
C oracle (scenarios: tests/card_update_cases.py; tests/test_card_update_cases.py shows that each
of them moves a large share of the picks or feasible counts).  yoda_snapshot_check then looks at
what no pick shows: block-grouped copies that left the base rows, stored block summaries that
differ from a fresh k_bsum_build, host mirrors that differ from the device; and on shapes without a grouped node
order the table digests of the long-lived handle equal a fresh upload's (no stale tail word, an
exact G table)."""
import numpy as np
import pytest

import card_update_cases as cases
import oracle
import upload_cases
from test_gpu_node_state import (Fleet, _scatter, assert_equal_results, check_state)
from test_gpu_parity import assert_same
from yoda_amd.capi import Yoda, YodaError
from yoda_amd.soa import MODE_SCV

pytestmark = pytest.mark.gpu

ZERO = [0, 0, 0, 0]


class CardFleet(Fleet):
    """The long-lived handles of a scenario; card updates go to every handle with GLOBAL ids."""

    def __init__(self, nodes, shards=False, **upload_kw):
        super().__init__(nodes, shards=shards, **upload_kw)
        self.model = cases.Model(nodes)

    def apply(self, step):
        if step[0] == "cards":
            self.model.apply(step)
            for h in self.handles():
                h.update_cards(*step[1:])
        else:
            super().apply(step)

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
    """entry_points: per check index (a list) or one tuple for all.  Returns the checks made."""
    k = 0
    for step in steps:
        if step[0] != "check":
            fleet.apply(step)
            continue
        eps = entry_points[k % len(entry_points)] if isinstance(entry_points, list) else entry_points
        check_state(fleet, pods, step[1], eps)
        fleet.self_check(step[1])
        if digests:
            np.testing.assert_array_equal(fleet.dev.snapshot_check()[0],
                                          fresh_digest(fleet.model.nodes(), **fleet.kw),
                                          err_msg=step[1])
        k += 1
    return k


@pytest.mark.parametrize("handles", ["single", "shards"])
def test_walk_base(handles):
    """Grouped node order.  single: eval, score rows, top-k lists and greedy on one handle;
    shards: the node shards of worlds 2 and 3 (ragged cuts) at every check."""
    nodes, pods, steps = cases.walk("base")
    with CardFleet(nodes, shards=handles == "shards") as fleet:
        assert fleet.dev.node_order_grouped and fleet.dev.path == "n32"
        eps = ("shards",) if handles == "shards" else \
            [("eval", "rows"), ("topk", "eval"), ("rows",), ("eval",),
             ("greedy", "rows"), ("eval", "topk"), ("rows", "eval"), ("topk",)]
        assert replay(fleet, pods, steps, eps) == len(cases.WALK_SIZES)


@pytest.mark.parametrize("shape", ["small", "c4", "ranks", "f64", "u64"])
def test_walk(shape):
    """small: below the grouped order; c4: K = 16, empty CardLists, CardNumber != len; ranks:
    memory in bytes, new frees from the snapshot's own values; f64 / u64: records only."""
    nodes, pods, steps = cases.walk(shape)
    kw = cases.UPLOAD_KW.get(shape, {})
    with CardFleet(nodes, **kw) as fleet:
        dev = fleet.dev
        assert dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        assert dev.memory_ranks == (shape == "ranks")
        ungrouped = shape in ("small", "f64", "u64")
        assert dev.node_order_grouped != ungrouped
        eps = [("eval",), ("eval", "greedy")] if shape in ("f64", "u64") else \
            [("eval", "rows"), ("eval", "topk"), ("greedy", "eval")]
        assert replay(fleet, pods, steps, eps, digests=ungrouped) == len(cases.WALK_SIZES)


def test_walk_mixed_grouped_order():
    """Half the nodes with mixed GPU models (the per-card model rows and K1 tiles decide them):
    the block-grouped order needs >= 32768 pods there.  Every pod against a fresh upload, a
    2000-pod sample against the oracle."""
    nodes, pods, steps = cases.walk("mixed")
    sample = np.sort(np.random.default_rng(3).choice(pods.n_pods, 2000, replace=False))
    sub = pods.take(sample)
    with CardFleet(nodes) as fleet:
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


@pytest.mark.parametrize("n", [900, 4608])
def test_block_drain_and_fill(n):
    """Whole 64-node blocks go from every free 0 to their totals and back: the block summaries
    (mrf, hfs bounds, the maxima and their witnesses) must follow both ways."""
    nodes, pods, steps = cases.block_drain(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    with CardFleet(nodes, shards=n != 900) as fleet:
        eps = ("eval", "rows", "topk", "greedy") + (("shards",) if n != 900 else ())
        assert replay(fleet, pods, steps, eps, digests=n == 900) == 3


@pytest.mark.parametrize("n", [900, 4608])
def test_free_maximum_up_and_back(n):
    """The G maximum of FreeMemory rises with one card and returns when it is restored: the G
    table, its reciprocals and (n = 900) every digest equal a fresh upload's both times."""
    nodes, pods, steps = cases.free_maximum(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    with CardFleet(nodes) as fleet:
        before = fleet.dev.snapshot_check()[0]
        assert replay(fleet, pods, steps, ("eval", "rows", "topk"), digests=n == 900) == 3
        np.testing.assert_array_equal(fleet.dev.snapshot_check()[0], before)


def test_health_only():
    nodes, pods, steps = cases.health_only()
    with CardFleet(nodes, shards=True) as fleet:
        assert replay(fleet, pods, steps, ("eval", "rows", "topk", "shards", "greedy")) == 2


def test_rejected_update_writes_nothing():
    """(e) YODA_ERR_RANGE from the LAST entry of a list: nothing of the earlier entries is kept."""
    nodes, pods, step = cases.rejected()
    with CardFleet(nodes) as fleet:
        dev = fleet.dev
        assert dev.memory_ranks
        before = dev.eval(pods, MODE_SCV)
        d0 = dev.snapshot_check()[0]
        with pytest.raises(YodaError, match="YODA_ERR_RANGE"):
            dev.update_cards(*step[1:])
        d1, m1 = dev.snapshot_check()
        np.testing.assert_array_equal(d1, d0)
        assert m1.tolist() == ZERO
        assert_equal_results(dev.eval(pods, MODE_SCV), before, "after the rejected update")
        assert_same(before, oracle.schedule(nodes, pods, MODE_SCV, threads=8))
        # without its last entry the list is accepted, and changes the state
        ok = ("cards",) + tuple(a[:-1] for a in step[1:])
        fleet.apply(ok)
        check_state(fleet, pods, "accepted prefix", ("eval",))
        assert (dev.snapshot_check()[0] != d0).any()
        # max_cards below a listed node's card count: invalid, nothing written either
        d2 = dev.snapshot_check()[0]
        with pytest.raises(YodaError, match="YODA_ERR_INVALID_ARG"):
            dev.update_cards(step[1][:2], step[2][:2, :4], step[3][:2, :4], step[4][:2])
        np.testing.assert_array_equal(dev.snapshot_check()[0], d2)


def test_zero_count_cached_runs_and_phase_order():
    """count == 0 is a no-op; a run, an update, a run on the SAME uploaded pods reflects the
    update; yoda_shard_phase2 after an update without a new phase 1 is YODA_ERR_STATE."""
    import torch
    from yoda_amd.dist import ShardBuffers
    nodes, pods, steps = cases.block_drain()
    with CardFleet(nodes) as fleet:
        dev = fleet.dev
        d0 = dev.snapshot_check()[0]
        k = nodes.max_cards
        dev.update_cards(np.zeros(0, np.uint32), np.zeros((0, k), np.uint64),
                         np.zeros((0, k), np.uint8), np.zeros(0, np.uint64))
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)
        dev.upload_pods(pods)
        dev.run(MODE_SCV)
        first = dev.download()
        assert_same(first, oracle.schedule(nodes, pods, MODE_SCV, threads=8))
        fleet.apply(steps[1])
        dev.run(MODE_SCV)  # no new upload_pods
        second = dev.download()
        assert_same(second, oracle.schedule(fleet.model.nodes(), pods, MODE_SCV, threads=8))
        assert (second.n_feasible != first.n_feasible).mean() >= 0.40
        b = ShardBuffers(pods.n_pods, torch.device("cuda:0"))
        p = ShardBuffers.ptr
        dev.shard_phase1(MODE_SCV, p(b.maxima), p(b.counts))
        fleet.apply(steps[3])
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.shard_phase2(MODE_SCV, p(b.maxima), p(b.counts), p(b.best), p(b.idx), p(b.ties),
                             p(b.lowest))
        check_state(fleet, pods, "after the refused phase 2", ("eval",))


def test_score_bound_only_grows():
    """yoda_score_bound follows the largest Actual term up (a filled block: FreeMemorySum from 0
    to the total) and never comes down (drained again)."""
    nodes, _, steps = cases.block_drain(nodes=900, pods=10)

    def fresh_bound(nd):
        with Yoda(0) as y:
            y.upload_nodes(nd)
            return y.score_bound

    with CardFleet(nodes) as fleet:
        dev = fleet.dev
        assert dev.score_bound == fresh_bound(nodes)
        fleet.apply(steps[1])
        filled = fresh_bound(fleet.model.nodes())
        assert dev.score_bound == filled >= fresh_bound(nodes)
        fleet.apply(steps[3])
        assert dev.score_bound == filled >= fresh_bound(fleet.model.nodes())


@pytest.mark.parametrize("shape", upload_cases.NAMES)
def test_builder_equivalence_on_fresh_uploads(shape):
    """A fresh upload against tests/golden/upload_digests.json, recorded at the last commit whose
    upload built the block summaries on the host (where a zero mismatch meant host builder ==
    k_bsum_build).  Digest 5: the block summaries k_bsum_build writes at upload equal that host
    builder's, word for word; digests 0-4, 6 and 7: the records, every other base table, the G
    table, its maxima and reciprocals are the ones that upload made; path and grouped order
    too.  The mismatch words: the stored block summaries of both orders equal a build into
    zeroed scratch (no stale padding word: small_after_base uploads over a larger snapshot) and
    the block-grouped copies are the base rows permuted, before any update."""
    with Yoda(0) as y:
        for nodes, kw in upload_cases.uploads(shape):
            y.upload_nodes(nodes, **kw)
        d, m = y.snapshot_check()
        assert m.tolist() == ZERO
        assert d[0] != 0
        assert (d[1:] != 0).all() == (y.path == "n32")
        assert upload_cases.entry(y, d) == upload_cases.golden()[shape]
