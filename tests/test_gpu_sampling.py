"""Node sampling (yoda_set_node_sampling) on a long-lived handle, across the Mode A batch entry
points.  The contract: each pod's walk begins at its start id, wraps, and keeps the first
num_to_find nodes of F'; the PreScore maxima do not move; counts, NormalizeScore, ties, picks, the
seeded draw, the bitmask and the rows follow the sample; n_found is |F'| and next_start the
(M+1)-th node of the walk.  Every check compares yoda_run + yoda_download, yoda_eval, the bits of
a YODA_RUN_BITMASK run, the raw and normalized rows of 24 pods and yoda_download_sampling with
sampling_cases.reference (the oracle's feasibility, raw scores and maxima, cut on the host).
Scenarios: tests/sampling_cases.py; tests/test_sampling_cases.py shows that they separate the
specification from its near misses."""
import numpy as np
import pytest

import candidate_cases as cc
import sampling_cases as cases
from card_update_cases import UPLOAD_KW, shape_workload
from test_gpu_card_update import ZERO
from test_gpu_parity import assert_same
from tie_draw_cases import draw
from yoda_amd import synth
from yoda_amd.capi import Yoda, YodaError, comm_run_local
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE
ROW_PODS = 24


def shifted(res, off):
    """The reference's picks as GLOBAL ids of a handle uploaded at node_offset `off`."""
    if off:
        res.pick = np.where(res.pick >= 0, res.pick + off, res.pick).astype(res.pick.dtype)
    return res


def check(dev, pods, snap, model, m, start, tag, sample=None, off=0):
    """The handle against the reference at one setting; start: LOCAL ids or None."""
    n = model.base.n_nodes
    want, _, found, nxt, sm = cases.reference(snap, model, m, start, sample)
    want = shifted(want, off)
    sel = slice(None) if sample is None else np.asarray(sample)
    gstart = None if start is None else (np.asarray(start, np.uint32) + np.uint32(off))

    def sampling():
        f, x = dev.download_sampling()
        np.testing.assert_array_equal(f[sel], found[sel], err_msg=f"{tag}: n_found")
        np.testing.assert_array_equal(x[sel], nxt[sel] + off, err_msg=f"{tag}: next_start")

    dev.set_node_sampling(m, gstart)
    assert dev.sampling_info()[:2] == (m, 0 if start is None else len(start))
    dev.upload_pods(pods)
    dev.run(MODE_SCV)
    assert_same(dev.download(), want, pods=sample)
    assert dev.sampling_info()[2] == 1
    sampling()
    assert_same(dev.eval(pods, MODE_SCV), want, pods=sample)
    sampling()
    some = np.arange(pods.n_pods) if sample is None else np.asarray(sample)
    some = some[:: max(1, some.size // 40)]
    dev.upload_pods(pods)
    dev.run(MODE_SCV, bitmask=True)
    assert_same(dev.download(), want, pods=sample)
    sampling()
    bits = np.unpackbits(dev.download_bitmask()[some].view(np.uint8), axis=1,
                         bitorder="little")[:, :n].astype(bool)
    for k, p in enumerate(some.tolist()):
        np.testing.assert_array_equal(bits[k], sm.candidates(p), err_msg=f"{tag}: bitmask of pod {p}")
    # (the start and class arrays stay on the handle across pod uploads: the row batch takes its own)
    n_rows = min(ROW_PODS, pods.n_pods)
    cls = model.cls
    dev.set_pod_classes(None if cls is None else cls[:n_rows])
    dev.set_node_sampling(m, None if gstart is None else gstart[:n_rows])
    dev.upload_pods(pods.slice(0, n_rows))
    feas, raw, norm = dev.score_rows(MODE_SCV, norm=True)
    f, x = dev.download_sampling()
    np.testing.assert_array_equal(f, found[:n_rows], err_msg=f"{tag}: rows n_found")
    np.testing.assert_array_equal(x, nxt[:n_rows] + off, err_msg=f"{tag}: rows next_start")
    for p in range(n_rows):
        d = cc.detail(snap, sm, p)
        np.testing.assert_array_equal(feas[p], d["feas"], err_msg=f"{tag}: row bits {p}")
        np.testing.assert_array_equal(raw[p][d["feas"]], d["raw"][d["feas"]],
                                      err_msg=f"{tag}: raw row {p}")
        assert (raw[p][~d["feas"]] == -1).all() and (norm[p][~d["feas"]] == -1).all(), tag
        if d["status"] == 0 and d["n_feasible"] >= 2:
            np.testing.assert_array_equal(norm[p], d["norm"], err_msg=f"{tag}: norm row {p}")
    dev.set_pod_classes(cls)
    dev.set_node_sampling(m, gstart)
    assert dev.snapshot_check()[1].tolist() == ZERO, tag


@pytest.mark.parametrize("shape", ["base", "small", "c4", "ranks", "f64", "u64"])
def test_walk(shape):
    """base: sparse masks, a snapshot with a grouped order (not taken while sampling); small:
    below it; c4: K = 16, empty CardLists; ranks: memory as ranks; f64 / u64: the per-node K1's
    dense masks, u64 with the exact normalize."""
    nodes, pods = shape_workload(shape)
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=11)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes, **UPLOAD_KW.get(shape, {}))
        assert dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        for m in cases.m_values(nodes.n_nodes):
            check(dev, pods, snap, model, m, start, f"{shape} M={m}")
        # M >= N: the unsampled outputs
        dev.set_node_sampling(nodes.n_nodes, start)
        assert_same(dev.eval(pods, MODE_SCV), snap.full)


def test_walk_mixed():
    """Half the nodes with mixed GPU models, 32k pods (513 pod waves): a 1000-pod sample."""
    nodes, pods = shape_workload("mixed", 32768 + 37)
    sample = np.sort(np.random.default_rng(3).choice(pods.n_pods, 1000, replace=False))
    sample[:ROW_PODS] = np.arange(ROW_PODS)
    sample = np.unique(sample)
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=13)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        check(dev, pods, snap, model, 100, start, "mixed", sample)


@pytest.mark.parametrize("n_pods", [229, 37])
def test_directed_cuts(n_pods):
    """229 pods: ordered, padded, a partly live wave; 37: below the ordering threshold."""
    nodes, pods, words, cls, start, tags = cases.directed(n_pods)
    model = cc.Model(nodes)
    model.apply(("cand", 3, words))
    model.apply(("classes", cls))
    snap = cc.Snapshot(model, pods)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        dev.set_candidates(words, 3)
        dev.set_pod_classes(cls)
        check(dev, pods, snap, model, cases.DIRECTED_M, start, f"directed {n_pods}")
        check(dev, pods, snap, model, cases.DIRECTED_M, None, f"directed {n_pods}, no starts")


def test_with_candidates_and_absent_nodes():
    """candidate_cases.with_absent's first state (8 classes, 120 absent nodes); some walks start
    on an absent node."""
    nodes, pods, steps = cc.with_absent()
    tag, model = cc.states(nodes, steps)[0]
    snap = cc.Snapshot(model, pods)
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=17)
    gone = model.absent()
    start[: gone.size] = gone
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        dev.set_candidates(model.words, model.n_classes)
        dev.set_pod_classes(model.cls)
        dev.set_node_present(gone.astype(np.uint32), np.zeros(gone.size, np.uint8))
        for m in (7, 100):
            check(dev, pods, snap, model, m, start, f"{tag} M={m}")


def test_seeded_tie_draw_over_the_sample():
    """640 nodes repeated 8 times (every pod ties over the clones inside its sample): with the draw
    on, every drawn pick is the member of the sample's tie set with the smallest
    (yoda_tie_hash << 32) | node."""
    from test_gpu_node_present import _repeat_nodes
    nodes = _repeat_nodes(synth.make_nodes(640, 3), 8)
    pods = synth.make_pods(300, 5)
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    m = 1500
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=19)
    want, ties, found, nxt, _ = cases.reference(snap, model, m, start)
    tied = np.flatnonzero((want.status == 0) & (want.n_ties >= 2))
    assert tied.size >= 100 and (found > m).sum() >= 100
    on = want.pick.copy()
    for p in tied.tolist():
        on[p] = draw(SEED, p, ties[p])
    assert (on != want.pick).sum() >= 50
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        dev.set_node_sampling(m, start)
        dev.set_tie_draw(SEED)
        got = dev.eval(pods, MODE_SCV)
        np.testing.assert_array_equal(got.pick, on)
        for f in ("status", "n_feasible", "n_ties", "top_score", "maxima"):
            np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
        np.testing.assert_array_equal(dev.download_sampling()[1], nxt)
        dev.set_tie_draw(None)
        assert_same(dev.eval(pods, MODE_SCV), want)
        assert dev.snapshot_check()[1].tolist() == ZERO


def test_zero_total():
    """candidate_cases.zero_total's pod p and its feasible node s with TotalMemorySum 0: with s
    inside the sample p ends in DIV_ZERO, with s outside it in OK."""
    nodes, pods, _, s, p = cc.zero_total()
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    feas = np.flatnonzero(snap.pod(p)[0])
    assert feas.size >= 4 and s in feas
    m = 2
    rot = cases.rotate(feas, s)
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=23)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        for st, status in ((int(s), 2), (int(rot[1]), 0)):  # s first in the walk; s last
            start[p] = st
            check(dev, pods, snap, model, m, start, f"zero_total start {st}")
            assert dev.eval(pods, MODE_SCV).status[p] == status
        assert dev.snapshot_check()[1].tolist() == ZERO


def test_node_offset():
    nodes, pods = shape_workload("small")
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    off = 70000
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=29)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes, node_offset=off)
        check(dev, pods, snap, model, 50, start, "offset", off=off)
        check(dev, pods, snap, model, 50, None, "offset, no starts", off=off)
        with pytest.raises(YodaError, match="YODA_ERR_RANGE"):
            dev.set_node_sampling(50, np.array([off - 1], np.uint32))
        with pytest.raises(YodaError, match="YODA_ERR_RANGE"):
            dev.set_node_sampling(50, np.array([off, off + nodes.n_nodes], np.uint32))


def test_off_means_off():
    nodes, pods = shape_workload("base")
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=31)
    with Yoda(0) as fresh, Yoda(0) as dev:
        fresh.upload_nodes(nodes)
        want = fresh.eval(pods, MODE_SCV)
        dev.upload_nodes(nodes)
        dev.set_node_sampling(100, start)
        cut = dev.eval(pods, MODE_SCV)
        assert (cut.n_feasible != want.n_feasible).sum() >= pods.n_pods // 4
        dev.set_node_sampling(0)
        assert dev.sampling_info() == (0, 0, 0)
        assert_same(dev.eval(pods, MODE_SCV), want)
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.download_sampling()
        dev.set_node_sampling(100, start)
        dev.upload_nodes(nodes)
        assert dev.sampling_info()[0] == 0
        assert_same(dev.eval(pods, MODE_SCV), want)
        dev.set_node_sampling(nodes.n_nodes + 5, start)  # M >= N: no pod is cut
        assert_same(dev.eval(pods, MODE_SCV), want)
        found, nxt = dev.download_sampling()
        np.testing.assert_array_equal(found, want.n_feasible)
        np.testing.assert_array_equal(nxt, start)
        assert dev.snapshot_check()[1].tolist() == ZERO


def test_refusals_and_errors():
    """With sampling on, greedy, the shard calls, the communicator runs, Mode B, reason_rows and
    diagnose(all) return YODA_ERR_STATE and the next sampled run still answers right; a failed
    call leaves the handle's answers unchanged; with sampling off they run."""
    import torch
    from yoda_amd.dist import ShardBuffers
    nodes, pods = synth.make_config(3, pods=600, nodes=1500)
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    m = 40
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=37)
    want, _, found, nxt, _ = cases.reference(snap, model, m, start)
    few = pods.slice(0, 8)
    with Yoda(0) as y:
        with pytest.raises(YodaError, match="YODA_ERR_NO_NODES"):
            y.set_node_sampling(5)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.download_sampling()
        b = ShardBuffers(pods.n_pods, torch.device("cuda:0"))
        p = ShardBuffers.ptr
        calls = (lambda: dev.greedy(pods.slice(0, 50), MODE_SCV, 0),
                 lambda: dev.shard_phase1(MODE_SCV, p(b.maxima), p(b.counts)),
                 lambda: comm_run_local([dev], MODE_SCV),
                 lambda: dev.run(MODE_DISKIO),
                 lambda: dev.reason_rows(),
                 lambda: dev.diagnose(all=True))
        dev.set_node_sampling(m, start)
        dev.upload_pods(pods)
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):  # no run is pending
            dev.download_sampling()

        def right():
            dev.upload_pods(pods)
            dev.run(MODE_SCV)
            assert_same(dev.download(), want)
            f, x = dev.download_sampling()
            np.testing.assert_array_equal(f, found)
            np.testing.assert_array_equal(x, nxt)

        for k, call in enumerate(calls):
            if k == 4:
                dev.upload_pods(few)
            if k == 5:
                right()  # (diagnose needs a completed run)
            with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
                call()
            assert "sampling" in str(e.value), k
            right()
        np.testing.assert_array_equal(dev.diagnose()[want.n_feasible > 0], 0xFFFFFFFF)
        from yoda_amd.capi import ERRORS, lib
        state = {v: k for k, v in ERRORS.items()}["YODA_ERR_STATE"]
        L, hp, q = lib(), dev._h, p(b.maxima)
        for rc in (L.yoda_shard_draw_apply(hp, q), L.yoda_shard_prepare_merge(hp, q, q, q, q),
                   L.yoda_shard_exact_records(hp, q), L.yoda_shard_exact_merge(hp, q, 1),
                   L.yoda_shard_witness_prepare(hp, q, q, q),
                   L.yoda_shard_witness_download(hp, q, q, q, q)):
            assert rc == state and b"sampling" in L.yoda_last_error(hp)
        right()
        # a start array of another length: the run refuses and launches nothing
        dev.upload_pods(pods.slice(0, 300))
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.run(MODE_SCV)
        right()
        # a start id out of range: validated before anything is written
        bad = start.copy()
        bad[7] = nodes.n_nodes
        with pytest.raises(YodaError, match="YODA_ERR_RANGE"):
            dev.set_node_sampling(m, bad)
        assert dev.sampling_info()[:2] == (m, pods.n_pods)
        right()
        dev.set_node_sampling(0)
        for k, call in enumerate(calls):
            dev.upload_pods(few if k == 4 else pods)
            if k == 5:
                dev.run(MODE_SCV)
            call()
        assert_same(dev.eval(pods, MODE_SCV), snap.full)
        assert dev.snapshot_check()[1].tolist() == ZERO
