"""The seeded selectHost draw of yoda_run / yoda_eval (include/yoda.h yoda_set_tie_draw): a pod
that ends OK with n_ties >= 2 is placed on the node of its tie set with the smallest draw word;
every other output, and every other entry point, is as with the draw off.

The expected pick never comes from libyoda: the tie set is read from the oracle's per-node
detail (its size asserted equal to the oracle's n_ties) and the draw word from the numpy
restatement of the header's formula (tie_draw_cases.py)."""
import os

import numpy as np
import pytest

import oracle
import pyoracle as po
from yoda_amd import capi, synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import MODE_DISKIO, MODE_SCV, NodeSoA, PodSoA

from tie_draw_cases import expected, tie_set

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 20240607, 3
OUT = ("status", "n_feasible", "n_ties", "top_score", "maxima")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def repeat_nodes(nodes, r):
    return NodeSoA(**{f: np.concatenate([getattr(nodes, f)] * r, axis=0)
                      for f in nodes.__dataclass_fields__}).normalized()


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    nodes = NodeSoA(**{k[5:]: z[k] for k in z.files if k.startswith("node_")})
    pods = PodSoA(**{k[4:]: z[k] for k in z.files if k.startswith("pod_")})
    return nodes.normalized(), pods.normalized()


@pytest.fixture()
def dev():
    y = Yoda(0)
    yield y
    y.close()


class Case:
    """A workload with its oracle result and the expected picks per (seed, base, offset)."""

    def __init__(self, nodes, pods, mode=MODE_SCV):
        self.nodes, self.pods, self.mode = nodes, pods, mode
        self.want = oracle.schedule(nodes, pods, mode, threads=8)
        self._exp = {}

    def picks(self, seed, pod_base=0, node_offset=0):
        key = (seed, pod_base, node_offset)
        if key not in self._exp:
            _, off, on, tied = expected(self.nodes, self.pods, self.mode, seed, pod_base,
                                        node_offset, self.want)
            self._exp[key] = (off, on, tied)
        return self._exp[key]


def dense_case(base):
    """`base` (640 nodes) repeated 8 times: the clones of a node sit 640 ids apart, in different
    64-node blocks and chunks, and tie on every pod."""
    return Case(repeat_nodes(base, 8), synth.make_pods(300, 5))


@pytest.fixture(scope="module")
def dense():
    c = dense_case(synth.make_nodes(640, 3))
    ok = c.want.status == 0
    assert ok.sum() >= 200 and (c.want.n_ties[ok] == 8).all()  # 227 of 227 when written
    return c


@pytest.fixture(scope="module")
def dense_mixed():
    c = dense_case(synth.mixed_models(synth.make_nodes(640, 3), 0.5))
    ok = c.want.status == 0
    assert ok.sum() >= 100 and (c.want.n_ties[ok] >= 8).all()
    return c


def assert_off(got, case, off):
    np.testing.assert_array_equal(got.pick, off, err_msg="pick (draw off)")
    for f in ("status", "n_feasible", "n_ties"):
        np.testing.assert_array_equal(getattr(got, f), getattr(case.want, f), err_msg=f)


def run_both(dev, case, seeds=(SEED_A,), pod_base=0, node_offset=0, mode=None):
    """Draw off against the oracle, then each seed: the expected picks, and every other output
    bit for bit as with the draw off.  Returns the seeds' pick vectors."""
    mode = case.mode if mode is None else mode
    dev.set_tie_draw(None)
    base = dev.eval(case.pods, mode)
    assert_off(base, case, case.picks(seeds[0], pod_base, node_offset)[0])
    out = []
    for s in seeds:
        _, on, tied = case.picks(s, pod_base, node_offset)
        dev.set_tie_draw(s, pod_base)
        got = dev.eval(case.pods, mode)
        bad = np.flatnonzero(got.pick != on)
        assert bad.size == 0, (f"seed {s}: {bad.size} picks differ, first pod {bad[:5]}: got "
                               f"{got.pick[bad[:5]]}, want {on[bad[:5]]}")
        for f in OUT:
            np.testing.assert_array_equal(getattr(got, f), getattr(base, f), err_msg=f)
        out.append(got.pick)
    dev.set_tie_draw(None)
    return out


# ---- 1. dense ties, Mode A, every record path ------------------------------------------------
VARIANTS = {
    "n32": ({}, "n32"),
    "f64": ({"force_f64": True}, "f64"),
    "u64": ({"force_generic": True}, "u64"),
    "mem_ranks": ({"mem_ranks": True}, "n32"),
    "f64_quotients": ({"f64_quotients": True}, "n32"),
    "per_node": ({"per_node_k1": True, "per_node_k2": True}, "n32"),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_dense_ties(dev, dense, name):
    kw, path = VARIANTS[name]
    dev.upload_nodes(dense.nodes, **kw)
    assert dev.path == path
    if name == "mem_ranks":
        assert dev.memory_ranks
    a, b = run_both(dev, dense, (SEED_A, SEED_B))
    assert (a != b).any()  # another seed, another draw
    tied = dense.picks(SEED_A)[2]
    assert (a[tied] != dense.picks(SEED_A)[0][tied]).any()  # and not the lowest node


def test_dense_ties_mixed_models(dev, dense_mixed):
    dev.upload_nodes(dense_mixed.nodes)
    assert dev.path == "n32"
    a, b = run_both(dev, dense_mixed, (SEED_A, SEED_B))
    assert (a != b).any()


# ---- 2. sparse ties ----------------------------------------------------------------------------
def test_sparse_ties(dev):
    case = Case(*synth.make_config(3, pods=2000, nodes=20000))
    tied = case.picks(SEED_A)[2]
    assert tied.size >= 20  # 41 of 1500 schedulable pods when written
    dev.upload_nodes(case.nodes)
    run_both(dev, case)


# ---- 3. pod orders and node orders ---------------------------------------------------------------
def test_unordered_small_batch(dev, dense):
    """100 pods: below the ordering threshold, the kernels see the caller's order."""
    sub = Case.__new__(Case)
    sub.nodes, sub.pods, sub.mode = dense.nodes, dense.pods.slice(0, 100), MODE_SCV
    sub.want = oracle.schedule(sub.nodes, sub.pods, MODE_SCV, threads=8)
    sub._exp = {}
    dev.upload_nodes(dense.nodes)
    run_both(dev, sub)
    assert dev.order_info()["kind"] == 0
    # pods 0..99 of the whole batch hash the same indices: the same picks
    np.testing.assert_array_equal(sub.picks(SEED_A)[1], dense.picks(SEED_A)[1][:100])


def padded_pods():
    """Two (clock, number, has-memory) groups of 190 and 126 pods, interleaved: padding each
    to whole waves adds 4 positions (<= 1/8 of the batch), so a private run takes the padded
    counting order, which evaluates two pods twice."""
    pool = synth.make_pods(6000, 5)
    one = (pool.has_clock == 0) & ((pool.has_number == 0) | (pool.number == 1))
    g1 = np.flatnonzero(one & (pool.has_memory == 1))[:190]
    g2 = np.flatnonzero(one & (pool.has_memory == 0))[:126]
    assert g1.size == 190 and g2.size == 126
    return pool.take(np.sort(np.concatenate([g1, g2])))


def test_pod_orders(dev, dense):
    case = Case(dense.nodes, padded_pods())
    assert case.picks(SEED_A)[2].size >= 100
    dev.upload_nodes(case.nodes)
    seen = {}
    for enable, pad in ((False, True), (True, True), (True, False)):
        dev.set_pod_order(enable, pad)
        run_both(dev, case)
        info = dev.order_info()
        seen[(enable, pad)] = info
    dev.set_pod_order(True, True)
    P = case.pods.n_pods
    assert seen[(False, True)]["kind"] == 0
    assert seen[(True, True)]["kind"] == 2 and seen[(True, True)]["work"] > P  # padded copies
    assert seen[(True, False)]["kind"] == 2 and seen[(True, False)]["work"] == P


def test_run_with_the_bitmask(dev, dense):
    """yoda_run with YODA_RUN_BITMASK takes the radix order (no padding) and keeps the masks for
    download: the same draw."""
    dev.upload_nodes(dense.nodes)
    dev.set_tie_draw(SEED_A)
    dev.upload_pods(dense.pods)
    dev.run(MODE_SCV, bitmask=True)
    got = dev.download()
    assert dev.order_info()["kind"] == 1
    np.testing.assert_array_equal(got.pick, dense.picks(SEED_A)[1])
    _, feas, _, _ = oracle.pod_detail(dense.nodes, dense.pods, 0, MODE_SCV)
    words = dev.download_bitmask()
    bits = np.unpackbits(words[0].view(np.uint8), bitorder="little")[:dense.nodes.n_nodes]
    np.testing.assert_array_equal(bits.astype(bool), feas)
    dev.set_tie_draw(None)


def test_node_orders(dev, dense):
    """The block-grouped node order on (5120 nodes) and off (3840 nodes: below its threshold):
    the hashed id is the upload-order id either way."""
    dev.upload_nodes(dense.nodes)
    assert dev.node_order_grouped
    run_both(dev, dense)
    small = Case(dense.nodes.slice(0, 640 * 6), dense.pods)
    ok = small.want.status == 0
    assert (small.want.n_ties[ok] == 6).all()
    dev.upload_nodes(small.nodes)
    assert not dev.node_order_grouped
    run_both(dev, small)


# ---- 4. ids --------------------------------------------------------------------------------------
def test_node_offset_hashes_global_ids(dev, dense):
    dev.upload_nodes(dense.nodes, node_offset=70000)
    (a,) = run_both(dev, dense, node_offset=70000)
    tied = dense.picks(SEED_A, 0, 70000)[2]
    assert (a[tied] >= 70000).all()
    # not the offset-0 draw shifted: the word hashes the global id
    assert (a[tied] - 70000 != dense.picks(SEED_A)[1][tied]).any()


def test_pod_base_reproduces_the_whole_batch(dev, dense):
    dev.upload_nodes(dense.nodes)
    whole = dense.picks(SEED_A)[1]
    got = []
    for lo, hi in ((0, 150), (150, 300)):
        dev.set_tie_draw(SEED_A, lo)
        got.append(dev.eval(dense.pods.slice(lo, hi), MODE_SCV).pick)
    dev.set_tie_draw(None)
    np.testing.assert_array_equal(np.concatenate(got), whole)


# ---- 5. Mode B -----------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [False, True])
def test_mode_b(dev, distinct):
    nodes, pods = synth.make_config(2)  # 1000 x 5000, tie sets up to 1001 nodes
    if distinct:
        pods = synth.distinct_diskio(pods)
    case = Case(nodes, pods, MODE_DISKIO)
    tied = case.picks(SEED_A)[2]
    assert tied.size >= 900
    dev.upload_nodes(nodes)
    (a,) = run_both(dev, case)
    if not distinct:  # one (rio, rcpu) class: one tie set, but a draw per pod
        assert np.unique(a[tied]).size > 100


# ---- 6. U64: exact-normalize pods and the other outcomes -------------------------------------------
def H(free, clock=1500, bw=1):
    return po.Card(free_memory=free, total_memory=16000, clock=clock, bandwidth=bw, core=1,
                   power=1, health="Healthy")


def normalize_cluster():
    """raw = 100 * clock + const (clock / MaxBandwidth with MaxBandwidth 1, algorithm.go:283).
    Clocks 1 (lowest), 9e14 and 2^62 / 100 (highest): highest - lowest overflows times 100, the
    highest nodes' product wraps to a small negative (normalized 0), the middle nodes normalize
    to 1 -- so the top NORMALIZED set is the middle nodes, not the raw maximizers.  Plus a
    node only one pod can use and pods nothing fits."""
    hi, mid = (1 << 62) // 100, 9 * 10 ** 14
    scvs = []
    for clock in (hi, 1, mid, hi, mid, 1, mid, 7):
        scvs.append(po.Scv(card_number=1, card_list=[H(10, clock=clock)], free_memory_sum=10,
                           total_memory_sum=16000))
    pods = [po.Pod(), po.Pod(number=1), po.Pod(clock=7), po.Pod(number=5), po.Pod(clock=mid),
            po.Pod(clock=hi), po.Pod(memory=5)] * 3
    return oracle.from_py(scvs, pods, max_cards=1)


def test_exact_normalize_pods_draw_over_the_normalized_top(dev):
    case = Case(*normalize_cluster())
    w = case.want
    off, on, tied = case.picks(SEED_A)
    # preconditions, from the oracle: some tied pod's set is NOT its raw maximizers; and the
    # other outcomes are present
    differs = 0
    for p in tied:
        _, feas, raw, _ = oracle.pod_detail(case.nodes, case.pods, int(p), MODE_SCV)
        members = tie_set(case.nodes, case.pods, int(p), MODE_SCV, int(w.n_ties[p]))
        idx = np.flatnonzero(feas)
        differs += set(members) != set(idx[raw[idx] == raw[idx].max()])
    assert differs >= 3
    assert (w.status == 1).any() and ((w.status == 0) & (w.n_feasible == 1)).any()
    dev.upload_nodes(case.nodes)
    assert dev.path == "u64"
    run_both(dev, case, (SEED_A, SEED_B))


@pytest.mark.parametrize("name", ["overflow.npz", "edges.npz"])
def test_other_outcomes_keep_theirs(dev, name):
    """overflow.npz: every pod ends STATUS_SCORE_RANGE; edges.npz: DIV_ZERO, UNSCHEDULABLE and
    one-node pods beside tied ones.  On the U64 path."""
    case = Case(*load_golden(name))
    if name == "overflow.npz":
        assert (case.want.status == 3).all()
    else:
        assert {1, 2} <= set(case.want.status.tolist())
    dev.upload_nodes(case.nodes, force_generic=True)
    assert dev.path == "u64"
    run_both(dev, case)


# ---- 7. live state -------------------------------------------------------------------------------
def test_after_set_node_state(dev, dense):
    """Raising the allocated memory of one clone of every base node lowers its score: it leaves
    the tie sets, and the draw runs over the rest."""
    dev.upload_nodes(dense.nodes)
    run_both(dev, dense)  # (the draw has run on the old state)
    sel = (np.arange(640) + 640 * (np.arange(640) % 8)).astype(np.uint32)
    mod = dense.nodes.slice(0, dense.nodes.n_nodes)
    alloc = mod.alloc_memory.copy()
    alloc[sel] += np.uint64(4096)
    mod.alloc_memory = alloc
    dev.set_node_state(sel, alloc[sel], mod.card_number[sel])
    case = Case(mod.normalized(), dense.pods)
    ok = case.want.status == 0
    assert (case.want.n_ties[ok] < 8).any()
    run_both(dev, case)


def test_after_update_node_cards(dev, dense):
    """The same through yoda_update_node_cards: one clone of each base node loses free memory
    on its first card."""
    dev.upload_nodes(dense.nodes)
    run_both(dev, dense)
    sel = (np.arange(640) + 640 * ((np.arange(640) + 3) % 8)).astype(np.uint32)
    mod = dense.nodes.slice(0, dense.nodes.n_nodes)
    free = mod.card_free_memory.copy()
    cut = np.minimum(free[sel, 0], np.uint64(1000))
    free[sel, 0] -= cut
    fsum = mod.free_memory_sum.copy()
    fsum[sel] -= cut
    mod.card_free_memory, mod.free_memory_sum = free, fsum
    dev.update_cards(sel, free[sel], mod.card_healthy[sel], fsum[sel])
    case = Case(mod.normalized(), dense.pods)
    ok = case.want.status == 0
    assert (case.want.n_ties[ok] < 8).any()
    run_both(dev, case)


# ---- 8. off is off ---------------------------------------------------------------------------------
def test_disable_restores_the_lowest_node(dev, dense):
    dev.upload_nodes(dense.nodes)
    dev.set_tie_draw(SEED_A)
    dev.eval(dense.pods, MODE_SCV)
    dev.set_tie_draw(None)
    again = dev.eval(dense.pods, MODE_SCV)
    with Yoda(0) as fresh:
        fresh.upload_nodes(dense.nodes)
        want = fresh.eval(dense.pods, MODE_SCV)
    for f in ("pick",) + OUT:
        np.testing.assert_array_equal(getattr(again, f), getattr(want, f), err_msg=f)


def test_other_entry_points_keep_the_lowest_node(dev, dense):
    nodes, pods = dense.nodes, dense.pods
    few = pods.slice(0, 4)

    def others(y):
        y.upload_pods(few)
        feas, scores = y.score_rows(MODE_SCV)
        rows_pick = y.download().pick
        greedy = y.greedy(pods, MODE_SCV, 0)
        greedy_b = y.greedy(pods, MODE_DISKIO, 0)
        return feas, scores, rows_pick, greedy, greedy_b

    dev.upload_nodes(nodes)
    off = others(dev)
    dev.set_tie_draw(SEED_A)
    on = others(dev)
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
    # the sharded step: two shard handles, the draw enabled on both
    half = nodes.n_nodes // 2
    res = []
    for seed in (None, SEED_A):
        hs = [Yoda(0), Yoda(0)]
        for i, h in enumerate(hs):
            h.upload_nodes(nodes.slice(i * half, (i + 1) * half), node_offset=i * half)
            h.upload_pods(pods)
            h.set_tie_draw(seed)
        capi.comm_run_local(hs, MODE_SCV)
        res.append(hs[0].download())
        for h in hs:
            h.close()
    for f in ("pick",) + OUT[:4]:
        np.testing.assert_array_equal(getattr(res[1], f), getattr(res[0], f), err_msg=f)
    np.testing.assert_array_equal(res[0].pick, dense.picks(SEED_A)[0])
