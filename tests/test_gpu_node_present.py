"""A long-lived handle while nodes leave the node set and come back (yoda_set_node_present),
across every Mode A entry point.  The contract: while a node is absent the handle answers exactly
as one freshly uploaded with the snapshot WITHOUT it would, the survivors keeping their ids.  So
at every check the handle that saw only the steps is compared, in every field of assert_same,
with the C oracle on the compacted snapshot (picks mapped back through the survivors' ids:
node_present_cases.reference) and with a fresh upload of that compacted snapshot.
yoda_snapshot_check looks at what no pick shows -- block-grouped copies, stored block summaries
against a fresh k_bsum_build (kBsAbsent is derived there), host mirrors -- and on the shapes
without a grouped node order the table digests after the last return equal a fresh upload's.
Scenarios: tests/node_present_cases.py; tests/test_node_present_cases.py shows that each of them
moves a large share of the picks or feasible counts."""
import numpy as np
import pytest

import node_present_cases as cases
import oracle
from test_gpu_card_update import ZERO, fresh_digest
from test_gpu_node_state import GREEDY_PODS, SHARD_CUTS, Fleet, _scatter, row_pods
from test_gpu_parity import assert_same
from test_gpu_topk import lists_of, lists_of_capacity
from tie_draw_cases import draw, tie_set
from yoda_amd import synth
from yoda_amd.capi import Yoda, YodaError, comm_greedy_local, comm_run_local, topk_k, topk_k_capacity
from yoda_amd.soa import MODE_DISKIO, MODE_SCV, NodeSoA

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE


class PresentFleet(Fleet):
    """The long-lived handles of a scenario; every step goes to every handle with GLOBAL ids."""

    def __init__(self, nodes, shards=False, **upload_kw):
        super().__init__(nodes, shards=shards, **upload_kw)
        self.model = cases.Model(nodes)

    def apply(self, step):
        if step[0] == "present":
            self.model.apply(step)
            for h in self.handles():
                h.set_node_present(step[1], step[2])
        elif step[0] == "cards":
            self.model.apply(step)
            for h in self.handles():
                h.update_cards(*step[1:])
        else:
            super().apply(step)

    def self_check(self, tag):
        gone = self.model.absent().size
        assert self.dev.nodes_absent == gone, tag
        for _, hs in self.worlds.values():
            assert sum(h.nodes_absent for h in hs) == gone, tag
        for h in self.handles():
            assert h.snapshot_check()[1].tolist() == ZERO, tag


def remapped(res, keep):
    res.pick = cases.remap(res.pick, keep)
    return res


def check_lists(model, pods, counts, ts, ti, sample, k):
    """The candidate lists against the oracle's per-node detail on the compacted snapshot: the
    first k feasible nodes by (score desc, id asc), as GLOBAL ids of the full snapshot."""
    comp, keep = model.compact(), model.keep()
    assert ts.shape[0] == k and ti.shape[0] == k
    for p in sample:
        _, feas, raw, _ = oracle.pod_detail(comp, pods, int(p), MODE_SCV)
        idx = np.flatnonzero(feas)
        assert counts[0, p] == idx.size, f"pod {p}"
        top = idx[np.lexsort((idx, -raw[idx]))][:k]
        m = top.size
        np.testing.assert_array_equal(ti[:m, p], keep[top].astype(np.uint32), err_msg=f"pod {p}")
        np.testing.assert_array_equal(ts[:m, p], raw[top].astype(np.float64), err_msg=f"pod {p}")
        assert (ts[m:, p] == -1.0).all() and (ti[m:, p] == 0xFFFFFFFF).all()


def check_present(fleet, pods, tag, entry_points, topk_sample=60):
    dev, model = fleet.dev, fleet.model
    keep, comp, n = model.keep(), model.compact(), model.base.n_nodes
    want = cases.reference(model, pods)
    for ep in entry_points:
        what = f"{tag}/{ep}"
        if ep == "eval":
            got = dev.eval(pods, MODE_SCV)
            assert_same(got, want)
            assert not np.isin(got.pick[got.pick >= 0], model.absent()).any(), what
            if keep.size:  # the handle a fresh upload of the compacted snapshot gives
                with Yoda(0) as y:
                    y.upload_nodes(comp, **fleet.kw)
                    assert_same(got, remapped(y.eval(pods, MODE_SCV), keep))
        elif ep == "rows":
            sub = row_pods(pods)
            dev.upload_pods(sub)
            feas, rows, norm = dev.score_rows(MODE_SCV, norm=True)
            assert feas.shape == (sub.n_pods, n)  # n_nodes and the ids do not change
            gone = model.absent()
            assert not feas[:, gone].any() and (rows[:, gone] == -1).all() and \
                (norm[:, gone] == -1).all(), what
            for p in range(sub.n_pods):
                _, f, raw, nrm = oracle.pod_detail(comp, sub, p, MODE_SCV)
                full_f = np.zeros(n, bool)
                full_f[keep] = f
                full_n = np.full(n, -1, np.int64)
                full_n[keep] = nrm
                np.testing.assert_array_equal(feas[p], full_f, err_msg=f"{what}: pod {p}")
                np.testing.assert_array_equal(norm[p], full_n, err_msg=f"{what}: pod {p}")
                np.testing.assert_array_equal(rows[p][keep][f], raw[f], err_msg=f"{what}: pod {p}")
                assert (rows[p][~full_f] == -1).all()
            assert_same(dev.download(), cases.reference(model, sub))
        elif ep in ("topk", "witness"):
            rng = np.random.default_rng(17)
            sample = rng.choice(pods.n_pods, min(topk_sample, pods.n_pods), replace=False)
            if ep == "topk":
                counts, ts, ti = lists_of(dev, pods)
                check_lists(model, pods, counts, ts, ti, sample, topk_k())
            else:  # the witness phase 1 and the capacity windows' lists
                counts, ts, ti = lists_of_capacity(dev, pods)
                check_lists(model, pods, counts, ts, ti, sample, topk_k_capacity())
            np.testing.assert_array_equal(counts[0], want.n_feasible, err_msg=what)
        elif ep == "shards":
            assert fleet.worlds
            for world, (_, hs) in fleet.worlds.items():
                for h in hs:
                    h.upload_pods(pods)
                comm_run_local(hs, MODE_SCV)
                for h in hs:
                    assert_same(h.download(), want)
        elif ep == "greedy":
            batch = pods.slice(0, min(pods.n_pods, GREEDY_PODS))
            for flags in (0, 1):
                np.testing.assert_array_equal(
                    dev.greedy(batch, MODE_SCV, flags),
                    cases.remap(oracle.greedy(comp, batch, MODE_SCV, flags)[0], keep),
                    err_msg=f"{what}: flags {flags}")
            # greedy leaves the presence (and the node state) as it found it
            assert dev.nodes_absent == model.absent().size
            assert_same(dev.eval(pods, MODE_SCV), want)
        elif ep == "shard_greedy":
            batch = pods.slice(0, min(pods.n_pods, GREEDY_PODS))
            _, hs = fleet.worlds[3]
            for flags in (0, 1):
                np.testing.assert_array_equal(
                    comm_greedy_local(hs, model.nodes(), batch, MODE_SCV, flags),
                    cases.remap(oracle.greedy(comp, batch, MODE_SCV, flags)[0], keep),
                    err_msg=f"{what}: flags {flags}")
        else:
            raise ValueError(ep)


def replay(fleet, pods, steps, entry_points):
    """entry_points: per check index (a list, cycled) or one tuple for all.  Returns the checks."""
    k = 0
    for step in steps:
        if step[0] != "check":
            fleet.apply(step)
            continue
        eps = entry_points[k % len(entry_points)] if isinstance(entry_points, list) else entry_points
        check_present(fleet, pods, step[1], eps)
        fleet.self_check(step[1])
        k += 1
    return k


@pytest.mark.parametrize("handles", ["single", "shards"])
def test_walk_base(handles):
    """Grouped node order.  single: eval, score rows, both kinds of candidate lists and greedy
    on one handle; shards: the node shards of worlds 2 and 3 (ragged cuts) at every check, and
    the sharded greedy once nodes are absent and once after updates named absent nodes."""
    nodes, pods, steps = cases.walk("base")
    assert SHARD_CUTS == cases.SHARD_CUTS
    with PresentFleet(nodes, shards=handles == "shards") as fleet:
        assert fleet.dev.node_order_grouped and fleet.dev.path == "n32"
        if handles == "shards":
            eps = [("shards",)] * len(cases.WALK)
            eps[3] = eps[cases.WALK_UPDATES + 1] = ("shards", "shard_greedy")
        else:
            eps = [("eval", "rows"), ("topk", "eval"), ("rows", "witness"), ("eval", "greedy"),
                   ("eval",), ("rows", "eval"), ("witness", "eval"), ("eval", "topk"),
                   ("greedy", "rows"), ("eval", "rows", "topk"), ("eval", "greedy")]
        assert replay(fleet, pods, steps, eps) == len(cases.WALK)


@pytest.mark.parametrize("shape", ["small", "c4", "ranks", "f64", "u64"])
def test_walk(shape):
    """small: below the grouped order; c4: K = 16, empty CardLists, CardNumber != len; ranks:
    memory as ranks; f64 / u64: records only (the per-node K1s read kNodeAbsent).  On the
    ungrouped shapes the digests after the last return equal a fresh upload's."""
    nodes, pods, steps = cases.walk(shape)
    kw = cases.UPLOAD_KW.get(shape, {})
    with PresentFleet(nodes, **kw) as fleet:
        dev = fleet.dev
        assert dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        assert dev.memory_ranks == (shape == "ranks")
        ungrouped = shape in ("small", "f64", "u64")
        assert dev.node_order_grouped != ungrouped
        eps = [("eval",), ("eval", "greedy"), ("eval", "rows")] if shape in ("f64", "u64") else \
            [("eval", "rows"), ("eval", "topk"), ("greedy", "eval"), ("witness", "eval")]
        assert replay(fleet, pods, steps, eps) == len(cases.WALK)
        assert dev.nodes_absent == 0
        if ungrouped:
            np.testing.assert_array_equal(dev.snapshot_check()[0],
                                          fresh_digest(fleet.model.nodes(), **kw))


def test_walk_mixed_grouped_order():
    """Half the nodes with mixed GPU models (the K1 tiles and model rows are repacked with the
    node): the block-grouped order needs >= 32768 pods there.  Every pod against a fresh upload
    of the compacted snapshot, a 2000-pod sample against the oracle."""
    nodes, pods, steps = cases.walk("mixed")
    sample = np.sort(np.random.default_rng(3).choice(pods.n_pods, 2000, replace=False))
    sub = pods.take(sample)
    with PresentFleet(nodes) as fleet:
        dev = fleet.dev
        assert dev.node_order_grouped
        checks = 0
        for step in steps:
            if step[0] != "check":
                fleet.apply(step)
                continue
            model = fleet.model
            keep = model.keep()
            got = dev.eval(pods, MODE_SCV)
            info = dev.order_info()
            assert info["kind"] == 2 and info["work"] >= 32768
            if keep.size:
                with Yoda(0) as y:
                    y.upload_nodes(model.compact())
                    assert_same(got, remapped(y.eval(pods, MODE_SCV), keep))
            assert_same(got, _scatter(cases.reference(model, sub), sample, pods.n_pods),
                        pods=sample)
            fleet.self_check(step[1])
            checks += 1
        assert checks == len(cases.WALK)


def test_single_survivor_no_div_zero():
    """All nodes but one of a pod group's feasible set absent, the survivor with TotalMemorySum
    0: one feasible node is returned without scoring, so no DIV_ZERO -- the rule follows the
    REDUCED count."""
    nodes, pods, steps, s, p = cases.single_survivor()
    with PresentFleet(nodes, shards=True) as fleet:
        eps = ("eval", "rows", "topk", "shards", "greedy")
        assert replay(fleet, pods, steps[:3], eps) == 2
        got = fleet.dev.eval(pods, MODE_SCV)
        assert got.pick[p] == s and got.status[p] == 0 and got.n_feasible[p] == 1
        assert replay(fleet, pods, steps[3:], eps) == 1


def test_max_holders_move_g():
    """Every holder of the snapshot's largest bandwidth absent: the pods' maxima and the G maxima
    move.  With G recomputed over the present nodes the waves' maxima still equal it (the
    G-table K2: a non-zero uniform-maxima count); with a stale G none would."""
    nodes, pods, steps = cases.max_holders()
    with PresentFleet(nodes) as fleet:
        dev = fleet.dev
        d0 = dev.snapshot_check()[0]
        assert replay(fleet, pods, steps[:3], ("eval", "rows", "topk")) == 2
        dev.class_stats(True)
        try:
            got = dev.eval(pods, MODE_SCV)
            st = dev.class_stats()
        finally:
            dev.class_stats(False)
        assert_same(got, cases.reference(fleet.model, pods))
        assert st["k2_uniform_maxima_wave_chunks"] > 0
        assert (dev.snapshot_check()[0][7] != d0[7])  # the G maxima and reciprocals moved
        assert replay(fleet, pods, steps[3:], ("eval", "witness", "greedy")) == 1
        # the records, every base table, the G table and its maxima: as before the nodes left
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)


def test_whole_shards_absent():
    nodes, pods, steps = cases.shard_absent()
    with PresentFleet(nodes, shards=True) as fleet:
        assert replay(fleet, pods, steps, [("shards", "eval", "shard_greedy"),
                                           ("shards", "eval"), ("shards",)]) == 3


def _repeat_nodes(nodes, r):
    return NodeSoA(**{f: np.concatenate([getattr(nodes, f)] * r, axis=0)
                      for f in nodes.__dataclass_fields__}).normalized()


def test_seeded_tie_draw_over_the_survivors():
    """640 nodes repeated 8 times (every pod ties over the 8 clones); one clone set loses a whole
    block, 700 scattered nodes and every first clone of the nodes most pods pick.  With the
    seeded draw on, single and sharded, each tied pod's pick is the member of the reference's
    tie set -- the oracle's on the compacted snapshot -- with the smallest yoda_tie_hash over
    the surviving GLOBAL ids."""
    nodes = _repeat_nodes(synth.make_nodes(640, 3), 8)
    pods = synth.make_pods(300, 5)
    n = nodes.n_nodes
    rng = np.random.default_rng(8)
    full = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    gone = np.unique(np.concatenate([np.arange(1280, 1344), rng.choice(n, 700, replace=False),
                                     np.unique(full.pick[full.status == 0])]))
    with PresentFleet(nodes, shards=True) as fleet:
        fleet.apply(("present", gone.astype(np.uint32), np.zeros(gone.size, np.uint8)))
        model = fleet.model
        comp, keep = model.compact(), model.keep()
        want = cases.reference(model, pods)
        tied = np.flatnonzero((want.status == 0) & (want.n_ties >= 2))
        assert tied.size >= 150 and (want.n_ties[tied] < 8).any()
        on = want.pick.copy()
        for p in tied:
            members = tie_set(comp, pods, int(p), MODE_SCV, int(want.n_ties[p]))
            on[p] = draw(SEED, int(p), keep[members])
        assert (on != want.pick).sum() >= 50
        dev = fleet.dev
        dev.set_tie_draw(SEED)
        got = dev.eval(pods, MODE_SCV)
        np.testing.assert_array_equal(got.pick, on)
        for f in ("status", "n_feasible", "n_ties", "top_score", "maxima"):
            np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
        dev.set_tie_draw(None)
        assert_same(dev.eval(pods, MODE_SCV), want)
        for world, (_, hs) in fleet.worlds.items():
            for h in hs:
                h.set_tie_draw(SEED)
                h.shard_tie_draw(True)
                h.upload_pods(pods)
            comm_run_local(hs, MODE_SCV)
            for h in hs:
                np.testing.assert_array_equal(h.download().pick, on, err_msg=f"world {world}")
            for h in hs:
                h.set_tie_draw(None)
                h.shard_tie_draw(False)
        fleet.self_check("tie draw")


def test_mode_b_refuses_while_a_node_is_absent():
    """Mode B has no Filter and does not read the bit: YODA_ERR_STATE from every Mode B entry
    point while a node is absent, the handle usable for Mode A meanwhile, Mode B as before once
    the node is back."""
    nodes, pods = synth.make_config(3, pods=600, nodes=1500)
    with PresentFleet(nodes, shards=True) as fleet:
        dev = fleet.dev
        before = dev.eval(pods, MODE_DISKIO)
        assert_same(before, oracle.schedule(nodes, pods, MODE_DISKIO, threads=8), MODE_DISKIO)
        fleet.apply(("present", np.array([700], np.uint32), np.zeros(1, np.uint8)))
        dev.upload_pods(pods)
        for call in (lambda: dev.eval(pods, MODE_DISKIO), lambda: dev.run(MODE_DISKIO),
                     lambda: dev.score_rows(MODE_DISKIO),
                     lambda: dev.greedy(pods.slice(0, 50), MODE_DISKIO, 0)):
            with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
                call()
            assert "absent" in str(e.value)
        _, hs = fleet.worlds[2]   # node 700 is in the second shard
        for h in hs:
            h.upload_pods(pods)
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            comm_run_local(hs, MODE_DISKIO)
        check_present(fleet, pods, "Mode A meanwhile", ("eval", "shards"))
        fleet.apply(("present", np.array([700], np.uint32), np.ones(1, np.uint8)))
        after = dev.eval(pods, MODE_DISKIO)
        for f in ("pick", "status", "n_feasible", "n_ties", "top_score"):
            np.testing.assert_array_equal(getattr(after, f), getattr(before, f), err_msg=f)
        comm_run_local(hs, MODE_DISKIO)
        assert_same(hs[0].download(), before, MODE_DISKIO)


def test_conventions_and_invalidation():
    """YODA_ERR_NO_NODES before an upload; count == 0 writes nothing; a list of unchanged flags
    writes nothing; a run, an absence, a run on the SAME uploaded pods reflects it;
    yoda_shard_phase2 after an absence without a new phase 1 is YODA_ERR_STATE; an upload makes
    every node present again."""
    import torch
    from yoda_amd.dist import ShardBuffers
    nodes, pods, steps = cases.max_holders()
    with Yoda(0) as y:
        with pytest.raises(YodaError, match="YODA_ERR_NO_NODES"):
            y.set_node_present(np.array([0], np.uint32), 0)
    with PresentFleet(nodes) as fleet:
        dev = fleet.dev
        d0 = dev.snapshot_check()[0]
        dev.set_node_present(np.zeros(0, np.uint32), np.zeros(0, np.uint8))
        dev.set_node_present(np.array([1, 2, nodes.n_nodes + 9], np.uint32), 1)  # present already
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)
        assert dev.nodes_absent == 0
        dev.upload_pods(pods)
        dev.run(MODE_SCV)
        first = dev.download()
        assert_same(first, oracle.schedule(nodes, pods, MODE_SCV, threads=8))
        fleet.apply(steps[1])
        dev.run(MODE_SCV)  # no new upload_pods
        second = dev.download()
        assert_same(second, cases.reference(fleet.model, pods))
        assert (second.maxima != first.maxima).any(axis=1).mean() >= 0.25
        b = ShardBuffers(pods.n_pods, torch.device("cuda:0"))
        p = ShardBuffers.ptr
        dev.shard_phase1(MODE_SCV, p(b.maxima), p(b.counts))
        fleet.apply(steps[3])
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.shard_phase2(MODE_SCV, p(b.maxima), p(b.counts), p(b.best), p(b.idx), p(b.ties),
                             p(b.lowest))
        check_present(fleet, pods, "after the refused phase 2", ("eval",))
        fleet.apply(steps[1])
        assert dev.nodes_absent == fleet.model.absent().size > 0
        dev.upload_nodes(nodes)
        assert dev.nodes_absent == 0
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)
        assert_same(dev.eval(pods, MODE_SCV), oracle.schedule(nodes, pods, MODE_SCV, threads=8))
