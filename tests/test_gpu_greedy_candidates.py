"""yoda_greedy with candidate classes (yoda_greedy_candidates) on the device: every pick of every
pod against tests/greedy_candidate_cases.reference, on the three Mode A paths and in Mode B.

The shapes: the config-5 generator at 2,500 pods x 600 nodes (tests/test_gpu_greedy_single.py's)
with the recipe classes (8 classes + ANY, 8 cordoned nodes); 6,500 pods, which is more than one
6,144-pod window, so the second window's class slice starts past 0; a mixed-model fleet, whose
capacity windows take the dense-mask witness kernel; a handle with a node offset; 120 absent
nodes.  test_paths_taken reads the work counters: the flags-0 batch evaluates pods one by one on
the narrowed masks (k_greedy_one), the capacity batch restarts windows and schedules pods exactly
with the one-pod kernels' candidate variant."""
import numpy as np
import pytest

import candidate_cases as cc
import greedy_candidate_cases as gc
import mode_b_follow_cases as mb
import node_present_cases as npc
import oracle
from yoda_amd import synth
from yoda_amd.capi import Yoda, YodaError
from yoda_amd.soa import MODE_DISKIO, MODE_SCV, PICK_NONE

pytestmark = pytest.mark.gpu

OFFSET = 1000
FIELDS = ("status", "pick", "n_feasible", "n_ties", "top_score")


@pytest.fixture
def dev():
    y = Yoda(0)
    yield y
    y.close()


def setup(dev, nd, words, cls, n_classes=8, **upload):
    dev.upload_nodes(nd, **upload)
    dev.set_candidates(words, n_classes)
    dev.set_pod_classes(cls)
    dev.greedy_candidates(True)


def model_of(nd, words, cls, n_classes=8, gone=None):
    m = cc.Model(nd)
    m.apply(("cand", n_classes, words))
    m.apply(("classes", cls))
    if gone is not None:
        m.apply(npc._present(gone, 0))
    return m


def assert_state_intact(dev, pods, model, sample=300, offset=0):
    """The snapshot, the words and the caller's class array (as long as `pods`) are what they
    were: a plain evaluation of the whole batch answers as candidate_cases.reference."""
    snap = cc.Snapshot(model, pods)
    want, _ = cc.reference(snap, model, sample=np.arange(sample))
    got = dev.eval(pods, MODE_SCV)
    for f in FIELDS:
        w = getattr(want, f)[:sample]
        if f == "pick":
            w = np.where(w >= 0, w + offset, w)
        np.testing.assert_array_equal(getattr(got, f)[:sample], w, err_msg=f)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("path", ["n32", "f64", "u64"])
def test_config5_paths(dev, path, flags):
    nd, pd, words, cls = gc.workload()
    want = gc.want(flags=flags)
    setup(dev, nd, words, cls, force_f64=path == "f64", force_generic=path == "u64")
    assert dev.path == path
    got = dev.greedy(pd, MODE_SCV, flags)
    np.testing.assert_array_equal(got, want)
    assert_state_intact(dev, pd, model_of(nd, words, cls))
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), want)


@pytest.mark.parametrize("flags", [0, 1])
def test_more_than_one_window(dev, flags):
    nd, pd, words, cls = gc.workload(pods=6500)
    setup(dev, nd, words, cls)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), gc.want(pods=6500, flags=flags))
    assert dev.greedy_stats()[0] >= 2


def test_mixed_models_dense_witness(dev):
    nd, pd, words, cls = gc.workload(pods=1200, mixed=True)
    setup(dev, nd, words, cls)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, 1),
                                  gc.want(pods=1200, mixed=True, flags=1))


def test_node_offset(dev):
    nd, pd, words, cls = gc.workload()
    want = gc.want(flags=1)
    setup(dev, nd, words, cls, node_offset=OFFSET)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, 1),
                                  np.where(want >= 0, want + OFFSET, want))
    assert_state_intact(dev, pd, model_of(nd, words, cls), offset=OFFSET)


@pytest.mark.parametrize("flags", [0, 1])
def test_absent_nodes(dev, flags):
    nd, pd, words, cls = gc.workload()
    gone = np.random.default_rng(9).choice(nd.n_nodes, 120, replace=False)
    present = np.ones(nd.n_nodes, bool)
    present[gone] = False
    want = gc.reference(nd, pd, words, cls, flags, present=present)
    setup(dev, nd, words, cls)
    dev.set_node_present(gone.astype(np.uint32), 0)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), want)
    assert_state_intact(dev, pd, model_of(nd, words, cls, gone=gone))


def test_paths_taken(dev):
    """The fallbacks of both modes ran on this workload (2,500 x 600, n32): flags 0 evaluates
    pods one by one on the window's narrowed masks; the capacity batch restarts windows and
    schedules pods exactly against the current state (the one-pod kernels' candidate variant for
    a pod that names a class)."""
    nd, pd, words, cls = gc.workload()
    setup(dev, nd, words, cls)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, 0), gc.want(flags=0))
    windows, fallbacks = dev.greedy_stats()
    print("flags 0: windows", windows, "fallbacks", fallbacks)
    assert fallbacks >= 1
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, 1), gc.want(flags=1))
    windows, fallbacks = dev.greedy_stats()
    restarts = dev.greedy_restarts()
    print("capacity: windows", windows, "fallbacks", fallbacks, "restarts", restarts)
    assert restarts >= 1 and fallbacks >= 1


@pytest.mark.parametrize("flags", [0, 1])
def test_every_pod_any(dev, flags):
    nd, pd, words, _ = gc.workload(pods=1200)
    want = oracle.greedy(nd, pd, MODE_SCV, flags)[0]
    setup(dev, nd, words, np.full(pd.n_pods, gc.ANY, np.uint8))
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), want)
    dev.set_pod_classes(None)  # no class array at all
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), want)


@pytest.mark.parametrize("flags", [0, 1])
def test_a_class_nowhere(dev, flags):
    nd, pd, words, cls = gc.workload(pods=1200)
    words = words & ~np.uint64(1 << 1)  # no node carries class 1
    want = gc.reference(nd, pd, words, cls, flags)
    assert (want[cls == 1] == PICK_NONE).all() and (want[cls != 1] >= 0).any()
    setup(dev, nd, words, cls)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), want)


@pytest.mark.parametrize("flags", [0, 1])
def test_class_63(dev, flags):
    nd, pd, _, _ = gc.workload(pods=1200)
    rng = np.random.default_rng(4)
    n = nd.n_nodes
    w64 = rng.integers(0, 2 ** 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    w64[rng.choice(n, 3 * n // 10, replace=False)] &= np.uint64((1 << 63) - 1)
    cls = np.full(pd.n_pods, 63, np.uint8)
    want = gc.reference(nd, pd, w64, cls, flags)
    assert (want != oracle.greedy(nd, pd, MODE_SCV, flags)[0]).any()
    setup(dev, nd, w64, cls, n_classes=64)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, flags), want)


def test_wrong_length_class_array(dev):
    nd, pd, words, cls = gc.workload(pods=1200)
    setup(dev, nd, words, cls[:700])
    with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
        dev.greedy(pd, MODE_SCV, 1)
    assert "class array" in str(e.value)
    sub = pd.slice(0, 700)
    assert_state_intact(dev, sub, model_of(nd, words, cls[:700]))


def test_setting_off_refuses(dev):
    nd, pd, words, cls = gc.workload(pods=1200)
    setup(dev, nd, words, cls)
    dev.greedy_candidates(False)
    for mode in (MODE_SCV, MODE_DISKIO):
        with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
            dev.greedy(pd, mode, 0)
        assert "candidate" in str(e.value)
    # a setting: it stays across uploads
    dev.greedy_candidates(True)
    dev.upload_nodes(nd)
    dev.set_candidates(words, 8)
    dev.set_pod_classes(cls)
    np.testing.assert_array_equal(dev.greedy(pd, MODE_SCV, 0), gc.want(pods=1200, flags=0))


def test_mode_b(dev):
    """Mode B: independent cycles in queue order, each pod with its own class -- per class the
    oracle on the nodes of E (mode_b_follow_cases.reference), in input order."""
    nodes, _ = synth.make_config(2, pods=1, nodes=3000)
    pods = synth.distinct_diskio(synth.make_pods(400, 17, priorities=True))
    absent, words, cls = mb.recipe(nodes, pods)
    m = model_of(nodes, words, cls, gone=absent)
    want = mb.reference(m, pods).pick
    assert (want != oracle.greedy(nodes, pods, MODE_DISKIO, 0)[0]).all()
    # (the queue order is not the input order: the class array really is permuted)
    assert (oracle.queue_order(pods) != np.arange(pods.n_pods)).any()
    setup(dev, nodes, words, cls)
    dev.set_node_present(absent, 0)
    with pytest.raises(YodaError, match="YODA_ERR_STATE") as e:
        dev.greedy(pods, MODE_DISKIO, 0)
    assert "Mode B does not honour" in str(e.value)
    dev.mode_b_follow(True)
    np.testing.assert_array_equal(dev.greedy(pods, MODE_DISKIO, 0), want)
    # the caller's class array is back in input order: a plain run answers by it
    mb.assert_same(dev.eval(pods, MODE_DISKIO), mb.reference(m, pods), "after greedy")
    np.testing.assert_array_equal(dev.greedy(pods, MODE_DISKIO, 0), want)
