"""Filter diagnosis on libyoda (include/yoda.h "Filter diagnosis"): yoda_diagnose's per-pod reason
counts and yoda_reason_rows' per-node codes against the numpy reference of
tests/diagnosis_cases.py, on a long-lived handle that saw only the scenario's steps.  Every
comparison is exact (integers).  tests/test_diagnosis_cases.py shows without a GPU that the
reference is right and that no scenario passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import diagnosis_cases as cases
import node_present_cases as npc
from test_gpu_candidates import Handle
from test_gpu_card_update import ZERO
from yoda_amd import capi
from yoda_amd.capi import Yoda, YodaError, lib
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
ROW_PODS = 24


def same_download(a, b, what):
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f"{what}: {f}"


def check_counts(dev, pods, ref, tag):
    """After a run: the default and the YODA_DIAG_ALL diagnosis equal the reference, twice the
    same, and the run's download is untouched."""
    dev.upload_pods(pods)
    dev.run(MODE_SCV)
    before = dev.download()
    np.testing.assert_array_equal(before.n_feasible, ref.n_feasible, err_msg=tag)
    got = dev.diagnose()
    print(f"{tag}: {int(ref.selected().sum())} of {pods.n_pods} pods selected")
    np.testing.assert_array_equal(got, ref.counts(), err_msg=f"{tag}: default selection")
    assert (got[~ref.selected()] == cases.UNSELECTED).all(), tag
    np.testing.assert_array_equal(dev.diagnose(all=True), ref.counts(all=True),
                                  err_msg=f"{tag}: every pod")
    np.testing.assert_array_equal(dev.diagnose(), got, err_msg=f"{tag}: a second diagnose")
    same_download(dev.download(), before, tag)


def check_rows(dev, pods, ref, model, tag):
    """The first pods as a row batch: the codes, code 0 == score_rows' feasibility, and each
    row's histogram == that pod's YODA_DIAG_ALL counts (the diagnosis of score_rows' own run)."""
    n_rows = min(ROW_PODS, pods.n_pods)
    cls = model.cls
    dev.set_pod_classes(None if cls is None else cls[:n_rows])
    dev.upload_pods(pods.slice(0, n_rows))
    rows = dev.reason_rows()
    for p in range(n_rows):
        np.testing.assert_array_equal(rows[p], ref.codes(p), err_msg=f"{tag}: reason row {p}")
    feas, _ = dev.score_rows(MODE_SCV)
    np.testing.assert_array_equal(rows == 0, feas, err_msg=f"{tag}: code 0 against score_rows")
    counts = dev.diagnose(all=True)
    hist = np.stack([(rows == c).sum(axis=1) for c in cases.COUNTED], axis=1)
    np.testing.assert_array_equal(counts, hist, err_msg=f"{tag}: row histograms")
    dev.set_pod_classes(cls)


def replay(h, pods, steps, name, rows=True):
    k = 0
    for step in steps:
        if step[0] != "check":
            h.apply(step)
            continue
        tag = f"{name} / {step[1]}"
        ref = cases.Reference(h.model, pods)
        check_counts(h.dev, pods, ref, tag)
        if rows:
            check_rows(h.dev, pods, ref, h.model, tag)
        assert h.dev.snapshot_check()[1].tolist() == ZERO, tag
        k += 1
    return k


@pytest.mark.parametrize("shape", cases.WALK_SHAPES)
def test_walk(shape):
    """small: below the grouped node order; c4: K = 16, empty CardLists, CardNumber !=
    len(CardList); ranks: memory thresholds in rank space; mixed: per-card clocks (no
    kNodeUniform4 shortcut); f64 / u64: the other two record formats."""
    nodes, pods, steps = cases.walk(shape)
    with Handle(nodes, **cases.cu.UPLOAD_KW.get(shape, {})) as h:
        assert h.dev.path == {"f64": "f64", "u64": "u64"}.get(shape, "n32")
        if shape == "ranks":
            assert lib().yoda_memory_ranks(h.dev._h) == 1
        assert replay(h, pods, steps, "walk " + shape) == len(cases.WALK)


@pytest.mark.parametrize("name", [n for n in sorted(cases.scenarios()) if n != "long chunks"])
def test_scenario(name):
    """Fleets of 1 .. 193 nodes, batches of 1 .. 130 pods, K of 1 .. 16, the scv/number labels,
    an empty selection."""
    nodes, pods, steps = cases.scenarios()[name]
    with Handle(nodes) as h:
        assert replay(h, pods, steps, name) == sum(s[0] == "check" for s in steps)


@pytest.mark.parametrize("order", [1, 0])
def test_pod_order(order):
    """700 pods: sorted on the device and padded to waves (a padding position is a copy of its
    pod: counted once), or with yoda_set_pod_order(h, 0); the counts come back in caller order."""
    nodes, pods, steps = cases.ordered_batch()
    with Handle(nodes) as h:
        h.dev.set_pod_order(bool(order))
        replay(h, pods, steps, f"order {order}", rows=False)
        info = np.zeros(4, np.uint32)
        lib().yoda_order_info(h.dev._h, info.ctypes.data_as(C.c_void_p))
        assert (info[3] != 0) == bool(order)


def test_long_chunks():
    """66,000 pods x 2,150 nodes: with every pod selected the sweep's chunks are two 64-node
    blocks long and the last one ends mid-block; the default selection takes one-block chunks."""
    nodes, pods, steps = cases.long_chunks()
    with Handle(nodes) as h:
        replay(h, pods, steps, "long chunks", rows=False)


def test_eval_is_diagnosed_like_run():
    """The C entry point yoda_eval (Yoda.eval is upload + run + download in Python) on a batch
    that differs from the one run before it: the diagnosis after it is that batch's, and equals
    the one after upload_pods + yoda_run."""
    from yoda_amd.soa import CEvalOut
    nodes, pods, steps = cases.tiny_fleet(193)
    with Handle(nodes) as h:
        for s in steps:
            if s[0] != "check":
                h.apply(s)
        cls = h.model.cls
        other = np.arange(pods.n_pods)[::-1][:97].copy()  # another batch: 97 pods, reversed
        h.dev.upload_pods(pods)
        h.dev.run(MODE_SCV)
        first = h.dev.diagnose()
        np.testing.assert_array_equal(first, cases.Reference(h.model, pods).counts())
        sub = pods.take(other)
        h.model.apply(("classes", cls[other]))
        h.dev.set_pod_classes(cls[other])
        ref = cases.Reference(h.model, sub)
        assert 0 < ref.selected().sum() < sub.n_pods
        pick = np.zeros(sub.n_pods, np.int32)
        nf = np.zeros(sub.n_pods, np.uint32)
        out = CEvalOut(pick=pick.ctypes.data_as(C.POINTER(C.c_int32)),
                       n_feasible=nf.ctypes.data_as(C.POINTER(C.c_uint32)))
        cp = sub.c()
        assert lib().yoda_eval(h.dev._h, C.byref(cp), MODE_SCV, C.byref(out)) == 0
        h.dev.n_pods = sub.n_pods
        np.testing.assert_array_equal(nf, ref.n_feasible)
        after_eval = h.dev.diagnose()
        np.testing.assert_array_equal(after_eval, ref.counts())
        np.testing.assert_array_equal(h.dev.diagnose(all=True), ref.counts(all=True))
        h.dev.upload_pods(sub)
        h.dev.run(MODE_SCV)
        np.testing.assert_array_equal(h.dev.diagnose(), after_eval)


# ---- node shards ---------------------------------------------------------------------------------
@pytest.mark.parametrize("caller_order", [True, False])
@pytest.mark.parametrize("shape", ["small", "u64"])
@pytest.mark.parametrize("world", [2, 3])
def test_shards(world, shape, caller_order):
    """The snapshot cut into ragged node shards, yoda_shard_candidates on, one step through
    yoda_comm_run_local: every shard selects the single handle's pods (the GLOBAL n_feasible) and
    the shards' counts add up to the single handle's."""
    nodes, pods, steps = cases.walk(shape)
    kw = cases.cu.UPLOAD_KW.get(shape, {})
    n = nodes.n_nodes
    b = [0] + [int(n * c) for c in npc.SHARD_CUTS[world]] + [n]
    hs = [Yoda(0) for _ in range(world)]
    try:
        for y, lo, hi in zip(hs, b[:-1], b[1:]):
            y.upload_nodes(nodes.slice(lo, hi), node_offset=lo, **kw)
            y.shard_candidates(True)
            y.shard_exchange_order(caller_order)
        with Handle(nodes, **kw) as one:
            assert one.dev.path == ("u64" if shape == "u64" else "n32")
            k = 0
            for step in steps:
                if step[0] != "check":
                    one.apply(step)
                    for y, lo, hi in zip(hs, b[:-1], b[1:]):
                        if step[0] == "cand":
                            y.set_candidates(None if step[2] is None else step[2][lo:hi], step[1])
                        elif step[0] == "update":
                            y.update_candidates(step[1], step[2])
                        elif step[0] == "classes":
                            y.set_pod_classes(step[1])
                        elif step[0] == "present":
                            y.set_node_present(step[1], step[2])
                        elif step[0] == "cards":
                            y.update_cards(*step[1:])
                        else:
                            y.set_node_state(*step[1:])
                    continue
                k += 1
                tag = f"{shape} world {world} / {step[1]}"
                ref = cases.Reference(one.model, pods)
                one.dev.upload_pods(pods)
                one.dev.run(MODE_SCV)
                want, want_all = one.dev.diagnose(), one.dev.diagnose(all=True)
                np.testing.assert_array_equal(want, ref.counts(), err_msg=tag)
                for y in hs:
                    y.upload_pods(pods)
                capi.comm_run_local(hs, MODE_SCV)
                got = [y.diagnose() for y in hs]
                for g in got:
                    np.testing.assert_array_equal(g[:, 0] == cases.UNSELECTED,
                                                  ~ref.selected(), err_msg=f"{tag}: selection")
                sel = ref.selected()
                total = sum(g[sel].astype(np.int64) for g in got)
                np.testing.assert_array_equal(total, want[sel], err_msg=f"{tag}: sum of shards")
                total = sum(y.diagnose(all=True).astype(np.int64) for y in hs)
                np.testing.assert_array_equal(total, want_all, err_msg=f"{tag}: every pod")
            assert k == len(cases.WALK)
    finally:
        for y in hs:
            y.close()


# ---- the state matrix ----------------------------------------------------------------------------
def refused(code, fn, *a, **kw):
    with pytest.raises(YodaError, match=code):
        fn(*a, **kw)


def test_state_matrix():
    """Every YODA_ERR_STATE / YODA_ERR_INVALID_ARG case of the contract; after each refusal the
    handle still runs and diagnoses correctly."""
    nodes, pods, steps = cases.tiny_fleet(193)
    L = lib()
    with Handle(nodes) as h:
        dev = h.dev
        ref = cases.Reference(h.model, pods)
        counts = np.zeros((pods.n_pods, 4), np.uint32)
        cp = counts.ctypes.data_as(C.c_void_p)

        def good(tag):
            dev.upload_pods(pods)
            dev.run(MODE_SCV)
            np.testing.assert_array_equal(dev.diagnose(), ref.counts(), err_msg=tag)

        # before anything ran; NULL handle and buffer; unknown flags; bad sizes
        refused("YODA_ERR_STATE", dev.diagnose)
        assert L.yoda_diagnose(None, 0) == -1 and L.yoda_download_diagnosis(None, cp, 0) == -1
        assert L.yoda_reason_rows(None, cp, 0) == -1
        dev.upload_pods(pods)
        refused("YODA_ERR_STATE", dev.diagnose)  # pods uploaded, nothing run
        dev.run(MODE_SCV)
        assert L.yoda_download_diagnosis(dev._h, cp, counts.size) == -7  # before this run's diagnose
        assert L.yoda_diagnose(dev._h, 2) == -1 and L.yoda_diagnose(dev._h, 0x80000001) == -1
        assert L.yoda_diagnose(dev._h, 0) == 0
        assert L.yoda_download_diagnosis(dev._h, None, counts.size) == -1
        assert L.yoda_download_diagnosis(dev._h, cp, counts.size - 1) == -1
        assert L.yoda_download_diagnosis(dev._h, cp, counts.size + 4) == -1
        assert L.yoda_download_diagnosis(dev._h, cp, counts.size) == 0
        np.testing.assert_array_equal(counts, ref.counts())
        # a new run needs its own diagnose
        dev.run(MODE_SCV)
        assert L.yoda_download_diagnosis(dev._h, cp, counts.size) == -7
        good("after the refusals")
        # Mode B, yoda_greedy
        dev.run(MODE_DISKIO)
        refused("YODA_ERR_STATE", dev.diagnose)
        good("after Mode B")
        dev.greedy(pods, MODE_SCV)
        refused("YODA_ERR_STATE", dev.diagnose)
        good("after greedy")
        # every call that invalidates a pending run
        some = np.array([5], np.uint32)
        words = np.full(nodes.n_nodes, 3, np.uint64)
        k = nodes.max_cards
        invalidating = [
            ("upload_pods", lambda: dev.upload_pods(pods)),
            ("upload_nodes", lambda: dev.upload_nodes(nodes)),
            ("update_cards", lambda: dev.update_cards(some, nodes.card_free_memory[some],
                                                      nodes.card_healthy[some],
                                                      nodes.free_memory_sum[some])),
            ("set_node_present", lambda: dev.set_node_present(some, np.ones(1, np.uint8))),
            ("set_candidates", lambda: dev.set_candidates(words, 2)),
            ("update_candidates", lambda: dev.update_candidates(some, np.array([3], np.uint64))),
            ("set_pod_classes", lambda: dev.set_pod_classes(np.zeros(pods.n_pods, np.uint8))),
            ("set_pod_classes off", lambda: dev.set_pod_classes(None)),
            ("candidates off", lambda: dev.set_candidates(None, 0)),
            ("reason_rows", lambda: dev.reason_rows()),
        ]
        assert k == nodes.card_free_memory.shape[1]
        for name, call in invalidating:
            good("before " + name)
            call()
            refused("YODA_ERR_STATE", dev.diagnose)
            assert L.yoda_download_diagnosis(dev._h, cp, counts.size) == -7, name
        good("after the invalidating calls")
        # the class array's length rule of yoda_run, for the row call
        dev.set_candidates(words, 2)
        dev.set_pod_classes(np.zeros(pods.n_pods + 1, np.uint8))
        refused("YODA_ERR_STATE", dev.reason_rows)
        dev.set_pod_classes(None)
        dev.set_candidates(None, 0)
        # bad sizes of the row call
        rows = np.zeros((pods.n_pods, nodes.n_nodes), np.uint8)
        rp = rows.ctypes.data_as(C.c_void_p)
        assert L.yoda_reason_rows(dev._h, rp, rows.size - 1) == -1
        assert L.yoda_reason_rows(dev._h, rp, rows.size + 1) == -1
        assert L.yoda_reason_rows(dev._h, None, rows.size) == -1
        assert L.yoda_reason_rows(dev._h, rp, rows.size) == 0
        for p in range(pods.n_pods):
            np.testing.assert_array_equal(rows[p], ref.codes(p))
        good("at the end")
    # the row call before the uploads
    with Yoda(0) as y:
        refused("YODA_ERR_NO_NODES", y.reason_rows)
        y.upload_nodes(nodes)
        refused("YODA_ERR_NO_PODS", y.reason_rows)
        refused("YODA_ERR_STATE", y.diagnose)


def test_a_sharded_step_in_progress_has_no_diagnosis():
    """yoda_shard_phase1 and yoda_shard_phase1_witness start a step: the earlier run is no longer
    pending; the step through
    yoda_comm_run_local on the same handle is diagnosed as a run is."""
    import torch
    nodes, pods, _ = cases.tiny_fleet(193)
    with Handle(nodes) as h:
        dev = h.dev
        ref = cases.Reference(h.model, pods)
        dev.upload_pods(pods)
        dev.run(MODE_SCV)
        np.testing.assert_array_equal(dev.diagnose(), ref.counts())
        buf = torch.zeros(8 * pods.n_pods, dtype=torch.int64, device="cuda")
        dev.shard_phase1(MODE_SCV, buf.data_ptr(), buf.data_ptr() + 48 * pods.n_pods)
        refused("YODA_ERR_STATE", dev.diagnose)
        dev.upload_pods(pods)
        dev.run(MODE_SCV)
        np.testing.assert_array_equal(dev.diagnose(), ref.counts())
        # the witness phase 1 of the capacity windows starts a step as well
        wit = torch.zeros(12 * pods.n_pods, dtype=torch.int32, device="cuda")
        dev.shard_phase1_witness(buf.data_ptr(), buf.data_ptr() + 48 * pods.n_pods, wit.data_ptr())
        refused("YODA_ERR_STATE", dev.diagnose)
        dev.upload_pods(pods)
        capi.comm_run_local([dev], MODE_SCV)
        np.testing.assert_array_equal(dev.diagnose(), ref.counts())
