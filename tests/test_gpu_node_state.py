"""A long-lived handle under node-state pushes (yoda_set_node_state / yoda_update_alloc) that
RAISE static scores and CardNumbers, across every entry point (the snapshot is
uploaded once, assumes and pod deletions arrive as pushes).  The K2 block bounds, the K1 seeds
and the block summaries' CardNumber bounds are tables of the state they were built from; after
a push that raises a score they may prune the block that holds the best node, which gives no
fault, only a wrong pick.  Every check compares the handle that saw only the pushes with a fresh
upload of the same state and with the C oracle, exactly (scenarios: tests/node_state_cases.py;
tests/test_node_state_cases.py shows that each of them moves a large share of the picks)."""
import numpy as np
import pytest

import node_state_cases as cases
import oracle
from test_gpu_parity import assert_same
from test_gpu_topk import _check as check_lists, lists_of
from yoda_amd import synth
from yoda_amd.capi import Yoda, comm_run_local
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
GREEDY_PODS = 600  # the sequential oracle's cost: a batch this size takes 0.3 s
SHARD_CUTS = {2: (0.37,), 3: (0.24, 0.63)}  # ragged shards, non-zero node offsets


def assert_equal_results(got, want, tag):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f"{tag}: {f}")


class Fleet:
    """The long-lived handles of one scenario: `dev` over all nodes and, on request, node shards
    of worlds 2 and 3.  Every push goes to every handle with GLOBAL ids."""

    def __init__(self, nodes, shards=False, **upload_kw):
        self.kw = upload_kw
        self.model = cases.Model(nodes)
        self.dev = Yoda(0)
        self.dev.upload_nodes(nodes, **upload_kw)
        self.worlds = {}
        n = nodes.n_nodes
        for world, cuts in (SHARD_CUTS.items() if shards else ()):
            b = [0] + [int(c * n) for c in cuts] + [n]
            hs = []
            for r in range(world):
                h = Yoda(0)
                h.upload_nodes(nodes.slice(b[r], b[r + 1]), node_offset=b[r], **upload_kw)
                hs.append(h)
            self.worlds[world] = (b, hs)

    def handles(self):
        return [self.dev] + [h for _, hs in self.worlds.values() for h in hs]

    def apply(self, step):
        self.model.apply(step)
        if step[0] == "push":
            for h in self.handles():
                h.set_node_state(*step[1:])
        elif step[0] == "update_alloc":
            self.dev.update_alloc(step[1])
            for b, hs in self.worlds.values():
                for r, h in enumerate(hs):
                    h.update_alloc(step[1][b[r]:b[r + 1]])

    def close(self):
        for h in self.handles():
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def row_pods(pods, n=24):
    """An n-pod slice that holds pods of at least three (number, clock) groups."""
    sub = pods.slice(0, n)
    groups = {(int(a), int(b), int(c), int(d)) for a, b, c, d in
              zip(sub.has_number, sub.number, sub.has_clock, sub.clock)}
    assert len(groups) >= 3
    return sub


def check_state(fleet, pods, tag, entry_points, topk_sample=120):
    """The long-lived handles against a fresh upload of the model's snapshot and against the C
    oracle, for each entry point named, in the order given."""
    dev, nodes = fleet.dev, fleet.model.nodes()
    want = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    ref = None
    if "eval" in entry_points or "shards" in entry_points:
        with Yoda(0) as y:
            y.upload_nodes(nodes, **fleet.kw)
            ref = y.eval(pods, MODE_SCV)
        assert_same(ref, want)
    for ep in entry_points:
        what = f"{tag}/{ep}"
        if ep == "eval":
            got = dev.eval(pods, MODE_SCV)
            assert_equal_results(got, ref, what)
            assert_same(got, want)
        elif ep == "rows":
            sub = row_pods(pods)
            dev.upload_pods(sub)
            feas, rows, norm = dev.score_rows(MODE_SCV, norm=True)
            for p in range(sub.n_pods):
                _, f, raw, nrm = oracle.pod_detail(nodes, sub, p, MODE_SCV)
                np.testing.assert_array_equal(feas[p], f, err_msg=f"{what}: pod {p}")
                np.testing.assert_array_equal(norm[p], nrm, err_msg=f"{what}: pod {p}")
                np.testing.assert_array_equal(rows[p][f], raw[f], err_msg=f"{what}: pod {p}")
                assert (rows[p][~f] == -1).all()
            assert_same(dev.download(), oracle.schedule(nodes, sub, MODE_SCV, threads=8))
        elif ep == "topk":
            counts, ts, ti = lists_of(dev, pods)
            rng = np.random.default_rng(17)
            check_lists(nodes, pods, counts, ts, ti,
                        rng.choice(pods.n_pods, min(topk_sample, pods.n_pods), replace=False))
        elif ep == "shards":
            assert fleet.worlds
            for world, (_, hs) in fleet.worlds.items():
                for h in hs:
                    h.upload_pods(pods)
                comm_run_local(hs, MODE_SCV)
                for h in hs:
                    got = h.download()
                    assert_same(got, want)   # the oracle
                    assert_same(got, ref)    # the unsharded evaluation
        elif ep == "greedy":
            batch = pods.slice(0, min(pods.n_pods, GREEDY_PODS))
            for flags in (0, 1):
                np.testing.assert_array_equal(dev.greedy(batch, MODE_SCV, flags),
                                              oracle.greedy(nodes, batch, MODE_SCV, flags)[0],
                                              err_msg=f"{what}: flags {flags}")
            # greedy restores the snapshot by pushes that raise scores; the model is unchanged
            got = dev.eval(pods, MODE_SCV)
            assert_same(got, want)
        else:
            raise ValueError(ep)


def pruned_blocks(dev, pods, want):
    """K2 blocks the bounds pruned in one more private run (which must still be right)."""
    dev.class_stats(True)
    try:
        got = dev.eval(pods, MODE_SCV)
        st = dev.class_stats()
    finally:
        dev.class_stats(False)
    assert_same(got, want)
    return st["k2_blocks"]["pruned"]


def replay(fleet, pods, steps, entry_points):
    """entry_points: per check index (or one tuple for all)."""
    k = 0
    for step in steps:
        if step[0] == "check":
            eps = entry_points[k] if isinstance(entry_points, list) else entry_points
            check_state(fleet, pods, step[1], eps)
            k += 1
        else:
            fleet.apply(step)
    return k


@pytest.mark.parametrize("after_push", [("rows", "eval", "rows", "topk", "shards"),
                                        ("shards", "topk", "eval", "rows"),
                                        ("greedy", "rows", "topk")],
                         ids=["rows_first", "shards_first", "greedy_first"])
def test_wake_prunes_and_is_exact(after_push):
    """Every node fully allocated at upload, then 150 nodes pushed to alloc 0: their static
    scores rise above what the bounds were built with (kbub_dirty).  rows_first: score rows
    see the dirty tables before any private run rebuilt them; shards_first: the sharded step
    and the candidate lists do; greedy_first: a greedy batch does -- the one entry point that
    keeps merely loose tables (its own pushes only lower scores; every other one rebuilds
    them in its phase 1 or 2 whichever flag is set).  Pruning is on before and after
    (k2_blocks.pruned > 0), so the test cannot pass on an unpruned walk.
    Known limit: a build whose note_static() books every push as a fall (loose, never dirty)
    still passes all three orders.  Only a greedy window's list pass then reads stale bounds,
    and at 4608 nodes each of its K2 chunks is a single 64-node block, so a block's bound is
    never compared with a list filled from another block."""
    nodes, pods, steps = cases.wake()
    with Fleet(nodes, shards=True) as fleet:
        dev = fleet.dev
        assert dev.node_order_grouped and dev.path == "n32"
        check_state(fleet, pods, steps[0][1], ("eval", "rows", "topk", "shards"))
        assert pruned_blocks(dev, pods, oracle.schedule(nodes, pods, MODE_SCV, threads=8)) > 0
        fleet.apply(steps[1])
        check_state(fleet, pods, steps[2][1], after_push)
        want = oracle.schedule(fleet.model.nodes(), pods, MODE_SCV, threads=8)
        assert pruned_blocks(dev, pods, want) > 0


def test_round_trip():
    """Fall, run (tables rebuilt at the lower scores), rise back, run; then a fall and a rise
    in one gap (loose and dirty before one run)."""
    nodes, pods, steps = cases.sleep_wake()
    with Fleet(nodes) as fleet:
        assert fleet.dev.node_order_grouped
        n = replay(fleet, pods, steps, [("eval",), ("eval",), ("eval", "rows", "topk"),
                                       ("topk", "rows", "eval")])
        assert n == 4


@pytest.mark.parametrize("pod_order", [True, False], ids=["sorted", "caller_order"])
def test_card_number_rise_and_fall(pod_order):
    """CardNumber 1 -> 8 on 40 % of the nodes, then 8 -> 0 on another 20 %: the K1 summaries,
    their block-grouped copies and the blocks' CardNumber bounds must all follow, with the
    pods sorted on the device and in the caller's order (no block-grouped run).  Whole blocks
    that rise: test_greedy_after_card_number_rise."""
    nodes, pods, steps = cases.cards()
    with Fleet(nodes, shards=True) as fleet:
        assert fleet.dev.node_order_grouped
        fleet.dev.set_pod_order(pod_order)
        try:
            assert replay(fleet, pods, steps, ("eval", "rows", "shards")) == 3
        finally:
            fleet.dev.set_pod_order(True)


def test_greedy_after_card_number_rise():
    """Whole 64-node blocks rise from CardNumber 1 to 8 and a greedy batch runs first: inside
    a greedy batch the block summaries are not tightened, so K1's whole-block rules read what
    k_set_static's atomics left there.  (Without its atomicMax on CnMax the greedy picks after
    the rise differ from the oracle's for a fifth of the pods.)"""
    nodes, pods, steps = cases.card_blocks()
    with Fleet(nodes) as fleet:
        assert replay(fleet, pods, steps, [("eval", "greedy"), ("greedy", "rows", "eval")]) == 2


@pytest.mark.parametrize("path", ["n32", "f64", "u64", "ranks"])
def test_walk(path):
    """Ten pushes of 0 to all nodes, alloc up and down, CardNumber 0..8, ids outside the
    snapshot: the pushed value is an f64 bit pattern on the N32 / F64 records and a u64 on the
    U64 records; `ranks` holds its memory fields as ranks."""
    shape = {"pods": 600, "nodes": 1500} if path in ("f64", "u64") else {}
    nodes, pods, steps = cases.walk(in_bytes=path == "ranks", **shape)
    kw = {"f64": {"force_f64": True}, "u64": {"force_generic": True}}.get(path, {})
    with Fleet(nodes, **kw) as fleet:
        dev = fleet.dev
        assert dev.path == ("n32" if path == "ranks" else path)
        assert dev.memory_ranks == (path == "ranks")
        eps = [("eval", "greedy") if k in (3, 8) else ("eval",) for k in range(10)]
        assert replay(fleet, pods, steps, eps) == 10


def test_walk_small_ungrouped():
    """The same walk below the grouped node order and the K1 probe."""
    nodes, pods, steps = cases.walk(pods=700, nodes=900)
    with Fleet(nodes) as fleet:
        assert not fleet.dev.node_order_grouped
        assert replay(fleet, pods, steps, ("eval", "rows")) == 10


def test_mixed_fleet_grouped_order():
    """Half the nodes with mixed GPU models: the block-grouped order needs >= 32768 pods there,
    and k_set_static must reach both orders' copies.  Every pod against a fresh upload, a
    2000-pod sample against the oracle."""
    nodes, pods, steps = cases.mixed_fleet()
    sample = np.sort(np.random.default_rng(3).choice(pods.n_pods, 2000, replace=False))
    sub = pods.take(sample)
    with Fleet(nodes) as fleet:
        dev = fleet.dev
        assert dev.node_order_grouped
        checks = 0
        for step in steps:
            if step[0] != "check":
                fleet.apply(step)
                continue
            model_nodes = fleet.model.nodes()
            got = dev.eval(pods, MODE_SCV)
            info = dev.order_info()   # counting order over >= 32768 sorted pods: perm_run
            assert info["kind"] == 2 and info["work"] >= 32768
            with Yoda(0) as y:
                y.upload_nodes(model_nodes)
                assert_equal_results(got, y.eval(pods, MODE_SCV), step[1])
            want = _scatter(oracle.schedule(model_nodes, sub, MODE_SCV, threads=8), sample,
                            pods.n_pods)
            assert_same(got, want, pods=sample)
            checks += 1
        assert checks == 3


def _scatter(res, idx, n):
    """An EvalResult over n pods holding `res` at positions idx."""
    from yoda_amd.soa import EvalResult
    out = EvalResult.empty(n)
    for f in FIELDS:
        getattr(out, f)[idx] = getattr(res, f)
    return out


def _eval_pair(dev, nodes, pods, tag, **kw):
    got = dev.eval(pods, MODE_SCV)
    with Yoda(0) as y:
        y.upload_nodes(nodes, **kw)
        assert_equal_results(got, y.eval(pods, MODE_SCV), tag)
    assert_same(got, oracle.schedule(nodes, pods, MODE_SCV, threads=8))
    return got


@pytest.mark.parametrize("path", ["n32", "u64"])
def test_push_over_allocation(path):
    """alloc = total + 1 on one node (the best one).  static_score() gives such a node an
    Allocate score of 0, as the reference and the oracle do (algorithm.go:305-307), so the
    push is accepted on every record path (no YODA_ERR_RANGE) and the node scores as a fully
    allocated one; the host copies hold the same state (an update_alloc of the model's array
    changes nothing)."""
    kw = {"force_generic": True} if path == "u64" else {}
    nodes, pods = synth.make_config(3, pods=600, nodes=1500)
    with Fleet(nodes, **kw) as fleet:
        dev = fleet.dev
        assert dev.path == path
        before = _eval_pair(dev, nodes, pods, "before", **kw)
        best = int(np.bincount(before.pick[before.status == 0]).argmax())
        step = ("push", np.array([best], np.uint32),
                np.array([nodes.total_memory_sum[best] + np.uint64(1)], np.uint64),
                np.array([nodes.card_number[best]], np.uint64))
        fleet.apply(step)
        after = _eval_pair(dev, fleet.model.nodes(), pods, "over-allocated", **kw)
        assert (after.pick != before.pick).any()
        dev.update_alloc(fleet.model.alloc)   # the host copies hold the model's state too
        _eval_pair(dev, fleet.model.nodes(), pods, "after update_alloc", **kw)


def test_push_edges():
    """Repeated ids in one list (the last entry wins, on the device and in the host copies),
    Mode B untouched by pushes, a re-upload on a handle the pushes left dirty and loose, and a
    close while a push is pending."""
    nodes, pods, _ = cases.wake()
    with Fleet(nodes) as fleet:
        dev = fleet.dev
        mode_b = dev.eval(pods, MODE_DISKIO)
        assert_same(mode_b, oracle.schedule(nodes, pods, MODE_DISKIO, threads=8), MODE_DISKIO)
        _eval_pair(dev, nodes, pods, "asleep")            # tables built at the uploaded state
        # every listed id three times with different values: first awake with 8 cards, then
        # asleep with none, last awake with 5 -- whichever entry the device kept shows in the
        # picks, the feasible counts or the scores
        rng = np.random.default_rng(11)
        sel = rng.choice(nodes.n_nodes, 200, replace=False).astype(np.uint32)
        total = nodes.total_memory_sum[sel]
        ids = np.concatenate([sel, sel[::-1], rng.permutation(sel)])
        last = ids[-sel.size:]
        alloc = np.concatenate([np.zeros(sel.size, np.uint64), total[::-1],
                                nodes.total_memory_sum[last] // np.uint64(4)])
        cn = np.concatenate([np.full(sel.size, 8), np.zeros(sel.size), np.full(sel.size, 5)])
        step = ("push", ids, alloc, cn.astype(np.uint64))
        fleet.apply(step)
        np.testing.assert_array_equal(fleet.model.alloc[last], nodes.total_memory_sum[last] // 4)
        check_state(fleet, pods, "repeated ids", ("rows", "eval", "topk"))
        # the host copies: update_alloc pushes h_card_number back, greedy starts from both
        dev.update_alloc(fleet.model.alloc)
        check_state(fleet, pods.slice(0, 600), "repeated ids, host copies", ("eval", "greedy"))
        assert_equal_results(dev.eval(pods, MODE_DISKIO), mode_b, "Mode B after the pushes")
        # dirty and loose, then another snapshot on the same handle: node count, K = 4 / 16
        for k, n in ((4, 1100), (16, 700)):
            base = fleet.model.base
            ids = rng.choice(base.n_nodes, 90, replace=False).astype(np.uint32)
            fleet.apply(("push", ids[:50], np.zeros(50, np.uint64), np.full(50, 8, np.uint64)))
            fleet.apply(("push", ids[50:], base.total_memory_sum[ids[50:]],
                         np.full(40, 8, np.uint64)))
            other = synth.make_nodes(n, seed=100 + k, cards=k)
            dev.upload_nodes(other)
            fleet.model = cases.Model(other)
            _eval_pair(dev, other, pods.slice(0, 400), f"re-upload K={k}")
    y = Yoda(0)
    y.upload_nodes(nodes)
    y.set_node_state(np.arange(64, dtype=np.uint32), np.zeros(64, np.uint64),
                     np.full(64, 8, np.uint64))
    y.close()  # a push still in flight: nothing to assert beyond a clean return
