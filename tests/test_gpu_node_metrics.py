"""Mode B's node inputs on a long-lived handle (yoda_update_node_metrics, and yoda_replace_nodes
carrying cpu / disk_io): NodeInfo.Cpu and NodeInfo.DiskIO are live metrics, so a handle must take
them every cycle without a re-upload -- and without losing its absent nodes and candidate classes
under yoda_mode_b_follow.  At every check the handle that saw only the steps is compared with a
fresh upload of the model's snapshot and with the C oracle in MODE_DISKIO (scenarios:
tests/replace_cases.py metrics_walk; tests/test_replace_cases.py shows that every list moves the
Mode B picks)."""
import copy

import numpy as np
import pytest

import candidate_cases as cc
import mode_b_follow_cases as mbf
import oracle
import replace_cases as cases
from test_gpu_node_state import assert_equal_results
from test_gpu_parity import assert_same
from yoda_amd import synth
from yoda_amd.capi import Yoda, YodaError
from yoda_amd.soa import MODE_DISKIO, MODE_SCV

pytestmark = pytest.mark.gpu

B_FIELDS = ("status", "pick", "n_feasible", "n_ties", "top_score")


def assert_same_b(got, want, tag):
    for f in B_FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f"{tag}: {f}")


def apply(dev, model, step):
    model.apply(step)
    if step[0] == "metrics":
        dev.update_node_metrics(*step[1:])
    elif step[0] == "replace":
        dev.replace_nodes(step[1], step[2])
    else:
        raise ValueError(step[0])


@pytest.mark.parametrize("distinct", [False, True], ids=["one_spec", "distinct"])
def test_metrics_walk(distinct):
    """Sparse lists of 1, 64 and 700 nodes (each with an id outside the snapshot and a repeated id
    whose real entry is last) and the dense form, on one pod spec (lane = node) and on a distinct
    request per pod (lane = class)."""
    nodes, pods, steps = cases.metrics_walk()
    if distinct:
        pods = synth.distinct_diskio(pods)
    model = cases.Model(nodes)
    checks, prev = 0, None
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        for step in steps:
            if step[0] != "check":
                apply(dev, model, step)
                continue
            nd = model.nodes()
            want = oracle.schedule(nd, pods, MODE_DISKIO, threads=8)
            got = dev.eval(pods, MODE_DISKIO)
            assert_same_b(got, want, step[1])
            with Yoda(0) as y:
                y.upload_nodes(nd)
                assert_same_b(got, y.eval(pods, MODE_DISKIO), step[1] + " (fresh upload)")
            # the same uploaded pods, no new upload_pods: the run reads the new records
            dev.run(MODE_DISKIO)
            assert_same_b(dev.download(), want, step[1] + " (cached pods)")
            if prev is not None and distinct:
                assert (got.pick != prev.pick).mean() >= 0.01, step[1]
            prev = got
            checks += 1
        assert checks == 1 + len(cases.METRIC_SIZES)
        assert dev.mode_b_info()[3] == 0  # no eligibility table was ever needed


def test_follow_state_survives_and_no_table_rebuild():
    """yoda_mode_b_follow with 8 classes, a class array and absent nodes: a metrics update keeps
    all of it, is answered as the oracle on each pod's eligible nodes, and does not rebuild the
    eligibility table (the build counter of yoda_mode_b_info stays)."""
    nodes, pods, steps = mbf.scenario(True)
    rng = np.random.default_rng(61)
    n = nodes.n_nodes
    model = cc.Model(nodes)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        dev.mode_b_follow(True)
        for s in steps[:3]:
            model.apply(s)
        dev.set_node_present(steps[0][1], steps[0][2])
        dev.set_candidates(steps[1][2], steps[1][1])
        dev.set_pod_classes(steps[2][1])
        first = dev.eval(pods, MODE_DISKIO)
        mbf.assert_same(first, mbf.reference(model, pods), "before")
        builds = dev.mode_b_info()[3]
        assert builds >= 1 and dev.mode_b_info()[2] == 1
        for tag, ids in (("dense", None), ("sparse", rng.choice(n, 700, replace=False))):
            size = n if ids is None else ids.size
            cpu, disk = rng.random(size) * 100.0, rng.random(size) * 100.0
            dev.update_node_metrics(ids, cpu, disk)
            nd = cases.copy_nodes(model.base)
            sel = slice(None) if ids is None else ids
            nd.cpu[sel], nd.disk_io[sel] = cpu, disk
            moved = copy.copy(model)
            moved.base = nd.normalized()
            model = moved
            got = dev.eval(pods, MODE_DISKIO)
            mbf.assert_same(got, mbf.reference(model, pods), tag)
            # (most pods tie on the top level and pick the lowest eligible id: the tie counts move)
            assert ((got.pick != first.pick) | (got.n_ties != first.n_ties)).mean() >= 0.10, tag
            assert dev.mode_b_info()[3] == builds, tag
            assert dev.mode_b_info()[2] == 1, tag
            assert dev.nodes_absent == steps[0][1].size and dev.candidates_info()[0] == 8
            first = got
        # a fresh upload brought to the same state answers the same
        with Yoda(0) as y:
            y.upload_nodes(model.base)
            y.mode_b_follow(True)
            y.set_node_present(steps[0][1], steps[0][2])
            y.set_candidates(steps[1][2], steps[1][1])
            y.set_pod_classes(steps[2][1])
            mbf.assert_same(got, y.eval(pods, MODE_DISKIO), "fresh upload, same state")


def test_errors_and_conventions():
    nodes, pods, _ = cases.metrics_walk()
    n = nodes.n_nodes
    cpu, disk = nodes.cpu.copy(), nodes.disk_io.copy()
    with Yoda(0) as y:
        with pytest.raises(YodaError, match="YODA_ERR_NO_NODES"):
            y.update_node_metrics(None, cpu, disk)
        y.upload_nodes(nodes)
        before = y.eval(pods, MODE_DISKIO)
        with pytest.raises(YodaError, match="YODA_ERR_INVALID_ARG"):
            y.update_node_metrics(None, cpu[:-1], disk[:-1])  # dense: n_nodes entries
        with pytest.raises(ValueError):
            y.update_node_metrics(np.arange(3, dtype=np.uint32), cpu[:2], disk[:2])
        y.update_node_metrics(np.zeros(0, np.uint32), cpu[:0], disk[:0])       # count == 0
        y.update_node_metrics(np.array([n, n + 9], np.uint32), cpu[:2], disk[:2])  # other shards'
        assert_same_b(y.eval(pods, MODE_DISKIO), before, "after the no-ops")


def test_state_error_without_mode_b_records():
    """A snapshot uploaded without cpu / disk_io has no Mode B records to update; a replacement
    on it ignores the record's cpu / disk_io."""
    import ctypes as C
    from yoda_amd.capi import lib
    nodes, pods = synth.make_config(3, pods=200, nodes=900)
    c = nodes.c()  # (`nodes` is normalized and outlives the call)
    c.cpu = C.cast(None, C.POINTER(C.c_double))
    c.disk_io = C.cast(None, C.POINTER(C.c_double))
    with Yoda(0) as y:
        y._check(lib().yoda_upload_nodes(y._h, C.byref(c), 0, 0), "yoda_upload_nodes")
        y.n_nodes = nodes.n_nodes
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            y.update_node_metrics(None, nodes.cpu, nodes.disk_io)
        ids = np.array([3, 500], np.uint32)
        y.replace_nodes(ids, nodes.take([7, 8]))
        m = cases.Model(nodes)
        m.apply(("replace", ids, nodes.take([7, 8])))
        assert_same(y.eval(pods, MODE_SCV), oracle.schedule(m.nodes(), pods, MODE_SCV, threads=8))


def test_replace_nodes_carries_the_metrics():
    """yoda_replace_nodes writes cpu / disk_io with the rest of the record: Mode B and Mode A both
    follow, and a record without them is refused when the snapshot holds them."""
    import ctypes as C
    from yoda_amd.capi import lib, _np_ptr
    nodes, pods, _ = cases.metrics_walk()
    pods = synth.distinct_diskio(pods)
    rng = np.random.default_rng(67)
    ids = rng.choice(nodes.n_nodes, 300, replace=False).astype(np.uint32)
    recs = nodes.take((ids.astype(np.int64) + 11) % nodes.n_nodes)
    model = cases.Model(nodes)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        first = dev.eval(pods, MODE_DISKIO)
        apply(dev, model, ("replace", ids, recs))
        nd = model.nodes()
        got = dev.eval(pods, MODE_DISKIO)
        assert_same_b(got, oracle.schedule(nd, pods, MODE_DISKIO, threads=8), "mode B")
        assert (got.pick != first.pick).mean() >= 0.01
        assert_same(dev.eval(pods, MODE_SCV), oracle.schedule(nd, pods, MODE_SCV, threads=8))
        d0 = dev.snapshot_check()[0]
        r = recs.normalized()
        c = r.c()
        c.cpu = C.cast(None, C.POINTER(C.c_double))
        rc = lib().yoda_replace_nodes(dev._h, ids.size, _np_ptr(ids), C.byref(c))
        assert rc == -1  # YODA_ERR_INVALID_ARG
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)
        assert_same_b(dev.eval(pods, MODE_DISKIO), got, "after the refused list")


def test_mode_a_is_unchanged_by_a_metrics_update():
    nodes, pods = synth.make_config(3, pods=700, nodes=900)
    rng = np.random.default_rng(71)
    with Yoda(0) as dev:
        dev.upload_nodes(nodes)
        before = dev.eval(pods, MODE_SCV)
        d0 = dev.snapshot_check()[0]
        dev.update_node_metrics(None, rng.random(900) * 100.0, rng.random(900) * 100.0)
        after = dev.eval(pods, MODE_SCV)
        assert_equal_results(after, before, "mode A after a metrics update")
        assert_same(after, oracle.schedule(nodes, pods, MODE_SCV, threads=8))
        np.testing.assert_array_equal(dev.snapshot_check()[0], d0)
