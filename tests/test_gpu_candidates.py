"""Other plugins' Filter results as candidate classes (yoda_set_candidates) on a long-lived handle,
across the Mode A batch entry points.  The contract: the PreScore maxima do not move; Filter,
counts, NormalizeScore, ties, picks and the seeded draw follow F' = Yoda's Filter and the pod's
class bit.  At every check the handle that saw only the steps is compared with
candidate_cases.reference (the oracle's feasibility, raw scores and maxima, narrowed on the host):
yoda_run + yoda_download, yoda_eval, the F' bits of a YODA_RUN_BITMASK run and the raw and
normalized rows.  Scenarios: tests/candidate_cases.py; tests/test_candidate_cases.py shows that
each of them fails a handle that ignores the words or lets the maxima follow them."""
import numpy as np
import pytest

import candidate_cases as cases
import oracle
from test_gpu_card_update import ZERO
from test_gpu_node_state import row_pods
from test_gpu_parity import assert_same
from tie_draw_cases import draw
from yoda_amd import synth
from yoda_amd.capi import Yoda, YodaError, comm_run_local
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

SEED = 0x5EEDFACE
ROW_PODS = 24


class Handle:
    """One long-lived handle and the model of what it was told."""

    def __init__(self, nodes, **kw):
        self.kw = kw
        self.model = cases.Model(nodes)
        self.dev = Yoda(0)
        self.dev.upload_nodes(nodes, **kw)

    def apply(self, step):
        self.model.apply(step)
        dev = self.dev
        if step[0] == "cand":
            dev.set_candidates(step[2], step[1])
        elif step[0] == "update":
            dev.update_candidates(step[1], step[2])
        elif step[0] == "classes":
            dev.set_pod_classes(step[1])
        elif step[0] == "present":
            dev.set_node_present(step[1], step[2])
        elif step[0] == "cards":
            dev.update_cards(*step[1:])
        elif step[0] == "push":
            dev.set_node_state(*step[1:])
        else:
            raise ValueError(step[0])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.dev.close()


def check(h, pods, snap, tag, sample=None):
    """The handle against the reference at one check: run + download, eval, the bitmask run's F'
    bits (of 40 pods spread over the batch or the sample: only their rows of the downloaded matrix
    are unpacked), and the raw / normalized rows of ROW_PODS pods (a smaller batch: all of it)."""
    dev, model = h.dev, h.model
    want, _ = cases.reference(snap, model, sample)
    dev.upload_pods(pods)
    dev.run(MODE_SCV)
    got = dev.download()
    assert_same(got, want, pods=sample)
    assert_same(dev.eval(pods, MODE_SCV), want, pods=sample)
    some = np.arange(pods.n_pods) if sample is None else np.asarray(sample)
    some = some[:: max(1, some.size // 40)]
    dev.upload_pods(pods)
    dev.run(MODE_SCV, bitmask=True)
    assert_same(dev.download(), want, pods=sample)
    bits = np.unpackbits(dev.download_bitmask()[some].view(np.uint8), axis=1,
                         bitorder="little")[:, :model.base.n_nodes].astype(bool)
    for k, p in enumerate(some.tolist()):
        np.testing.assert_array_equal(bits[k], cases.detail(snap, model, p)["feas"],
                                      err_msg=f"{tag}: bitmask of pod {p}")
    # (the class array stays on the handle across pod uploads: the row batch takes its own)
    cls = model.cls
    n_rows = min(ROW_PODS, pods.n_pods)
    sub = row_pods(pods, ROW_PODS) if n_rows == ROW_PODS else pods
    dev.set_pod_classes(None if cls is None else cls[:n_rows])
    dev.upload_pods(sub)
    feas, raw, norm = dev.score_rows(MODE_SCV, norm=True)
    for p in range(n_rows):
        d = cases.detail(snap, model, p)
        np.testing.assert_array_equal(feas[p], d["feas"], err_msg=f"{tag}: row bits {p}")
        np.testing.assert_array_equal(raw[p][d["feas"]], d["raw"][d["feas"]],
                                      err_msg=f"{tag}: raw row {p}")
        assert (raw[p][~d["feas"]] == -1).all() and (norm[p][~d["feas"]] == -1).all(), tag
        if d["status"] == 0 and d["n_feasible"] >= 2:
            np.testing.assert_array_equal(norm[p], d["norm"], err_msg=f"{tag}: norm row {p}")
    dev.set_pod_classes(cls)
    assert dev.snapshot_check()[1].tolist() == ZERO, tag


def replay(h, pods, steps, sample=None):
    snap, k = None, 0
    for step in steps:
        if step[0] != "check":
            h.apply(step)
            if step[0] in ("present", "cards", "push"):
                snap = None  # the maxima and raw scores follow the node values
            continue
        snap = snap or cases.Snapshot(h.model, pods)
        check(h, pods, snap, step[1], sample)
        k += 1
    return k


@pytest.mark.parametrize("shape", ["base", "small", "c4", "ranks", "f64", "u64"])
def test_walk(shape):
    """base: grouped node order; small: below it; c4: K = 16, empty CardLists; ranks: memory as
    ranks; f64 / u64: the per-node K1's dense masks."""
    nodes, pods, steps = cases.walk(shape)
    with Handle(nodes, **cases.UPLOAD_KW.get(shape, {})) as h:
        assert h.dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        assert replay(h, pods, steps) == len(cases.WALK)
        assert h.dev.candidates_info()[0] == 0
        with Yoda(0) as y:  # candidates off again: a fresh handle's answers
            y.upload_nodes(nodes, **h.kw)
            assert_same(h.dev.eval(pods, MODE_SCV), y.eval(pods, MODE_SCV))


def test_walk_mixed_grouped_order():
    """Half the nodes with mixed GPU models: the block-grouped order needs >= 32768 pods there.
    A 1000-pod sample against the reference, the bitmask run (the radix order over the mixed-model
    tiles, 513 pod waves, the upload-order candidate tables) included."""
    nodes, pods, steps = cases.walk("mixed")
    sample = np.sort(np.random.default_rng(3).choice(pods.n_pods, 1000, replace=False))
    sample[:ROW_PODS] = np.arange(ROW_PODS)  # (the row pods are the first ones)
    sample = np.unique(sample)
    with Handle(nodes) as h:
        assert h.dev.node_order_grouped
        assert replay(h, pods, steps, sample) == len(cases.WALK)
        h.dev.eval(pods, MODE_SCV)
        info = h.dev.order_info()
        assert info["kind"] == 2 and info["work"] >= 32768


@pytest.mark.parametrize("flag", ["per_node_k1", "per_node_k2", "no_gtab", "no_uniform"])
def test_walk_base_upload_flags(flag):
    """The YODA_UPLOAD_* test flags on base: the per-node K1 (dense masks) and K2, no G table, no
    uniform-node factoring."""
    nodes, pods, steps = cases.walk("base")
    with Handle(nodes, **{flag: True}) as h:
        assert replay(h, pods, steps) == len(cases.WALK)


@pytest.mark.parametrize("n_nodes", [337, 64, 65])
@pytest.mark.parametrize("n_pods", [197, 130])
def test_edge_shapes(n_pods, n_nodes):
    """Three pod waves with the last partly live (above the 128-pod ordering threshold) and two
    with two live lanes in the last; five node blocks and a 17-node tail, one block, one block and
    one node."""
    nodes, pods = synth.make_config(3, pods=n_pods, nodes=n_nodes)
    words, cls = cases.recipe(nodes, pods, seed=5, cordoned=3)
    with Handle(nodes) as h:
        steps = [("cand", 8, words), ("classes", cls), ("check", "recipe"),
                 ("classes", np.full(n_pods, 7, np.uint8)), ("check", "one class")]
        assert replay(h, pods, steps) == 2


def test_maxima_holder():
    nodes, pods, steps, holders = cases.maxima_holder()
    with Handle(nodes) as h:
        assert replay(h, pods, steps[:4]) == 2
        got = h.dev.eval(pods, MODE_SCV)
        np.testing.assert_array_equal(got.maxima,
                                      oracle.schedule(nodes, pods, MODE_SCV, threads=8).maxima)
        assert not np.isin(got.pick[got.pick >= 0], holders).any()
        assert replay(h, pods, steps[4:]) == 1


def test_zero_total():
    nodes, pods, steps, s, p = cases.zero_total()
    with Handle(nodes) as h:
        assert replay(h, pods, steps[:1]) == 1
        assert h.dev.eval(pods, MODE_SCV).status[p] == 2
        assert replay(h, pods, steps[1:4]) == 1
        assert h.dev.eval(pods, MODE_SCV).status[p] == 0
        assert replay(h, pods, steps[4:6]) == 1
        got = h.dev.eval(pods, MODE_SCV)
        assert got.pick[p] == s and got.status[p] == 0 and got.n_feasible[p] == 1
        assert replay(h, pods, steps[6:]) == 1


def test_with_absent_nodes_and_updates():
    nodes, pods, steps = cases.with_absent()
    with Handle(nodes) as h:
        assert replay(h, pods, steps) == 3


def test_overflow_exact_normalize():
    nodes, pods, steps = cases.overflow()
    with Handle(nodes, force_generic=True) as h:
        assert h.dev.path == "u64"
        assert replay(h, pods, steps) == 2


@pytest.mark.parametrize("shape", ["base", "small"])
def test_pod_order_is_invisible(shape):
    nodes, pods, steps = cases.walk(shape)
    with Handle(nodes) as h:
        for s in steps[:2]:
            h.apply(s)
        res = []
        for order in (0, 1, 2):
            h.dev.set_pod_order(order != 0, pad=order == 1)
            res.append(h.dev.eval(pods, MODE_SCV))
        for r in res[1:]:
            for f in ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima"):
                np.testing.assert_array_equal(getattr(r, f), getattr(res[0], f), err_msg=f)


def test_seeded_tie_draw_over_the_candidates():
    """640 nodes repeated 8 times (every pod ties over the clones it may use): with the draw on,
    every drawn pick is the member of the reference's tie set with the smallest
    (yoda_tie_hash << 32) | node."""
    from test_gpu_node_present import _repeat_nodes
    nodes = _repeat_nodes(synth.make_nodes(640, 3), 8)
    pods = synth.make_pods(300, 5)
    words, cls = cases.recipe(nodes, pods, seed=9, tenths=0.3, cordoned=16)
    with Handle(nodes) as h:
        h.apply(("cand", 8, words))
        h.apply(("classes", cls))
        snap = cases.Snapshot(h.model, pods)
        want, ties = cases.reference(snap, h.model)
        tied = np.flatnonzero((want.status == 0) & (want.n_ties >= 2))
        assert tied.size >= 150
        on = want.pick.copy()
        for p in tied.tolist():
            on[p] = draw(SEED, p, ties[p])
        assert (on != want.pick).sum() >= 50
        h.dev.set_tie_draw(SEED)
        got = h.dev.eval(pods, MODE_SCV)
        np.testing.assert_array_equal(got.pick, on)
        for f in ("status", "n_feasible", "n_ties", "top_score", "maxima"):
            np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
        h.dev.set_tie_draw(None)
        assert_same(h.dev.eval(pods, MODE_SCV), want)


def test_state_and_failed_calls():
    """yoda_upload_nodes turns candidates off; a failed call (a bad class byte, n_classes 65, an
    update while off, a class array of another length) leaves the handle's answers unchanged."""
    nodes, pods, steps = cases.walk("small")
    words, cls = steps[0][2], steps[1][1]
    with Yoda(0) as y:
        with pytest.raises(YodaError, match="YODA_ERR_NO_NODES"):
            y.set_candidates(np.zeros(0, np.uint64), 3)
    with Handle(nodes) as h:
        dev = h.dev
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.update_candidates(np.array([1], np.uint32), np.array([0], np.uint64))
        h.apply(steps[0])
        h.apply(steps[1])
        snap = cases.Snapshot(h.model, pods)
        want, _ = cases.reference(snap, h.model)
        assert dev.candidates_info() == (8, pods.n_pods, int(((words & 0xFF) != 0xFF).sum()))
        assert_same(dev.eval(pods, MODE_SCV), want)
        bad = cls.copy()
        bad[5] = 8
        for call, err in ((lambda: dev.set_pod_classes(bad), "YODA_ERR_INVALID_ARG"),
                          (lambda: dev.set_candidates(words, 65), "YODA_ERR_INVALID_ARG")):
            with pytest.raises(YodaError, match=err):
                call()
            assert_same(dev.eval(pods, MODE_SCV), want)
        # a NULL array where one is needed: words with n_classes > 0, ids / words with count > 0
        from yoda_amd.capi import ERRORS, lib
        invalid = {v: k for k, v in ERRORS.items()}["YODA_ERR_INVALID_ARG"]
        ids2, w2 = np.array([1, 2], np.uint32), np.zeros(2, np.uint64)
        for rc in (lib().yoda_set_candidates(dev._h, 3, None),
                   lib().yoda_update_candidates(dev._h, 2, None, w2.ctypes.data),
                   lib().yoda_update_candidates(dev._h, 2, ids2.ctypes.data, None)):
            assert rc == invalid
            assert_same(dev.eval(pods, MODE_SCV), want)
        assert dev.candidates_info()[0] == 8
        dev.update_candidates(np.zeros(0, np.uint32), np.zeros(0, np.uint64))  # a no-op
        dev.upload_pods(pods.slice(0, 300))
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            dev.run(MODE_SCV)
        assert_same(dev.eval(pods, MODE_SCV), want)
        dev.upload_nodes(nodes)
        assert dev.candidates_info()[0] == 0
        assert_same(dev.eval(pods, MODE_SCV), snap.full)


def test_refusals():
    """With candidates on, greedy, the shard calls, the communicator runs and Mode B return
    YODA_ERR_STATE and the next yoda_run still answers right; with candidates off they run."""
    import torch
    from yoda_amd.dist import ShardBuffers
    nodes, pods = synth.make_config(3, pods=600, nodes=1500)
    words, cls = cases.recipe(nodes, pods, seed=3, cordoned=8)
    with Handle(nodes) as h:
        dev = h.dev
        b = ShardBuffers(pods.n_pods, torch.device("cuda:0"))
        p = ShardBuffers.ptr
        calls = (lambda: dev.greedy(pods.slice(0, 50), MODE_SCV, 0),
                 lambda: dev.shard_phase1(MODE_SCV, p(b.maxima), p(b.counts)),
                 lambda: comm_run_local([dev], MODE_SCV),
                 lambda: dev.run(MODE_DISKIO))
        h.apply(("cand", 8, words))
        h.apply(("classes", cls))
        snap = cases.Snapshot(h.model, pods)
        want, _ = cases.reference(snap, h.model)
        dev.upload_pods(pods)
        for call in calls:
            with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
                call()
            assert "candidate" in str(e.value)
            dev.run(MODE_SCV)
            assert_same(dev.download(), want)
        # the shard calls that continue or read a step refuse too (before they touch a buffer)
        from yoda_amd.capi import ERRORS, lib
        state = {v: k for k, v in ERRORS.items()}["YODA_ERR_STATE"]
        L, hp, q = lib(), dev._h, p(b.maxima)
        for rc in (L.yoda_shard_draw_apply(hp, q), L.yoda_shard_prepare_merge(hp, q, q, q, q),
                   L.yoda_shard_exact_records(hp, q), L.yoda_shard_exact_merge(hp, q, 1),
                   L.yoda_shard_witness_prepare(hp, q, q, q),
                   L.yoda_shard_witness_download(hp, q, q, q, q)):
            assert rc == state and b"candidate" in L.yoda_last_error(hp)
        dev.run(MODE_SCV)
        assert_same(dev.download(), want)
        h.apply(("cand", 0, None))
        for call in calls:
            dev.upload_pods(pods)
            call()
        assert_same(dev.eval(pods, MODE_SCV), snap.full)
