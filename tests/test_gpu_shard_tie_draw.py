"""The seeded selectHost draw carried across node shards (include/yoda.h yoda_shard_tie_draw,
yoda_shard_draw_keys, yoda_shard_draw_apply): with the shard draw on, a batch
split over several shard handles places every tied pod on the node one handle holding the whole
snapshot would draw -- whatever the split, the record path, the transport or the pod order --
and changes nothing else; with it off the sharded step keeps the lowest node.

The expected pick never comes from libyoda: tie_draw_cases.expected runs over the WHOLE
snapshot, with the oracle's tie set and the numpy draw word.  Every test runs several shard
handles on device 0, through yoda_comm_run_local or dist.ShardExchange.local."""
import contextlib
import os

import numpy as np
import pytest

import oracle
import pyoracle as po
from yoda_amd import capi, synth
from yoda_amd.capi import Yoda, YodaError
from yoda_amd.soa import MODE_DISKIO, MODE_SCV, NodeSoA, PodSoA

from tie_draw_cases import expected, tie_set

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 20240607, 3
OUT = ("status", "n_feasible", "n_ties", "top_score", "maxima")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DENSE_BOUNDS = {2: (0, 2560, 5120), 3: (0, 1700, 3400, 5120)}  # world 3: no multiple of 64


def repeat_nodes(nodes, r):
    return NodeSoA(**{f: np.concatenate([getattr(nodes, f)] * r, axis=0)
                      for f in nodes.__dataclass_fields__}).normalized()


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    nodes = NodeSoA(**{k[5:]: z[k] for k in z.files if k.startswith("node_")})
    pods = PodSoA(**{k[4:]: z[k] for k in z.files if k.startswith("pod_")})
    return nodes.normalized(), pods.normalized()


def even_bounds(n_nodes, world):
    return tuple(int(x) for x in np.linspace(0, n_nodes, world + 1))


class Case:
    """A workload with its oracle result over the whole snapshot and the expected picks per
    (seed, base, offset), computed once."""

    def __init__(self, nodes, pods, mode=MODE_SCV):
        self.nodes, self.pods, self.mode = nodes, pods, mode
        self.want = oracle.schedule(nodes, pods, mode, threads=8)
        self._exp = {}

    def picks(self, seed, pod_base=0, node_offset=0):
        """(picks with the draw off, picks with the draw, tied pods)"""
        key = (seed, pod_base, node_offset)
        if key not in self._exp:
            _, off, on, tied = expected(self.nodes, self.pods, self.mode, seed, pod_base,
                                        node_offset, self.want)
            self._exp[key] = (off, on, tied)
        return self._exp[key]


@contextlib.contextmanager
def fleet(nodes, bounds, node_offset=0, **kw):
    """One shard handle per [bounds[r], bounds[r + 1]), uploaded at its global offset."""
    hs = []
    try:
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            y = Yoda(0)
            hs.append(y)
            y.upload_nodes(nodes.slice(lo, hi), node_offset=node_offset + lo, **kw)
        yield hs
    finally:
        for y in hs:
            y.close()


def configure(hs, draw):
    """draw: None (everything off) or (seed, pod_base): both switches on, on every shard."""
    for h in hs:
        h.set_tie_draw(*(draw if draw else (None,)))
        h.shard_tie_draw(draw is not None)


def step(hs, pods, mode, draw=None):
    """One yoda_comm_run_local step; every shard must hold the same result."""
    configure(hs, draw)
    for h in hs:
        h.upload_pods(pods)
    capi.comm_run_local(hs, mode)
    res = [h.download() for h in hs]
    for r in res[1:]:
        for f in ("pick",) + OUT:
            np.testing.assert_array_equal(getattr(r, f), getattr(res[0], f), err_msg=f)
    return res[0]


def assert_picks(got, want, what=""):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} picks differ, first pods {bad[:5]}: got "
                           f"{got[bad[:5]]}, want {want[bad[:5]]}")


def run_both(hs, case, seeds=(SEED_A,), pod_base=0, node_offset=0, pods=None):
    """The step with the draw off against the oracle, then with each seed: the expected picks,
    and every other output bit for bit the draw-off step's.  Returns the seeds' picks."""
    pods = case.pods if pods is None else pods
    base = step(hs, pods, case.mode)
    assert_picks(base.pick, case.picks(seeds[0], pod_base, node_offset)[0], "draw off")
    for f in ("status", "n_feasible", "n_ties"):
        np.testing.assert_array_equal(getattr(base, f), getattr(case.want, f), err_msg=f)
    out = []
    for s in seeds:
        got = step(hs, pods, case.mode, (s, pod_base))
        assert_picks(got.pick, case.picks(s, pod_base, node_offset)[1], f"seed {s}")
        for f in OUT:
            np.testing.assert_array_equal(getattr(got, f), getattr(base, f), err_msg=f)
        out.append(got.pick)
    return out


@pytest.fixture(scope="module")
def dense():
    """synth.make_nodes(640, 3) repeated 8 times: the clones of a node sit 640 ids apart and tie
    on every pod, so every tie set of 8 spans both halves and all three thirds."""
    c = Case(repeat_nodes(synth.make_nodes(640, 3), 8), synth.make_pods(300, 5))
    ok = c.want.status == 0
    assert ok.sum() >= 200 and (c.want.n_ties[ok] == 8).all()
    off, on, tied = c.picks(SEED_A)
    assert tied.size >= 200
    for world, b in DENSE_BOUNDS.items():
        shard = lambda n: np.searchsorted(np.asarray(b), n, side="right")
        # the drawn node in another shard than the lowest one: lowest-node code cannot pass
        assert (shard(on[tied]) != shard(off[tied])).sum() >= 50, world
    return c


# ---- 1. dense ties, every record path, both splits, libyoda's transport ---------------------
VARIANTS = {
    "n32": ({}, "n32"),
    "f64": ({"force_f64": True}, "f64"),
    "u64": ({"force_generic": True}, "u64"),
    "mem_ranks": ({"mem_ranks": True}, "n32"),
    "f64_quotients": ({"f64_quotients": True}, "n32"),
}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_dense_ties(dense, name, world):
    kw, path = VARIANTS[name]
    with fleet(dense.nodes, DENSE_BOUNDS[world], **kw) as hs:
        assert all(h.path == path for h in hs)
        if name == "mem_ranks":
            assert all(h.memory_ranks for h in hs)
        a, b = run_both(hs, dense, (SEED_A, SEED_B))
    assert (a != b).any()  # another seed, another draw
    off, _, tied = dense.picks(SEED_A)
    assert (a[tied] != off[tied]).any()


# ---- 2. the Python driver ---------------------------------------------------------------------
@pytest.mark.parametrize("caller_order", [True, False])
@pytest.mark.parametrize("compact", [True, False])
def test_shard_exchange_driver(dense, compact, caller_order):
    """dist.ShardExchange.local with tie_draw: the packed-key and the three-reduce merges, the
    caller-order and the shared radix-order exchange buffers -- the keys are in the caller's
    order either way."""
    import torch
    from yoda_amd.dist import ShardExchange
    b = DENSE_BOUNDS[3]
    with fleet(dense.nodes, b) as hs:
        for h in hs:
            h.upload_pods(dense.pods)
        shards = [dense.nodes.slice(lo, hi) for lo, hi in zip(b[:-1], b[1:])]
        ex = ShardExchange.local(hs, torch.device("cuda:0"), shards, list(b[:-1]),
                                 compact=compact, caller_order=caller_order,
                                 tie_draw=(SEED_A, 0))
        assert (ex.ib is not None) == compact
        got = ex.run(MODE_SCV)
        assert_picks(got.pick, dense.picks(SEED_A)[1], "ShardExchange")
        for f in ("status", "n_feasible", "n_ties"):
            np.testing.assert_array_equal(getattr(got, f), getattr(dense.want, f), err_msg=f)
        for h in hs[1:]:
            np.testing.assert_array_equal(h.download().pick, got.pick)


# ---- 3. one handle holding the whole snapshot draws the same ----------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_equals_the_single_handle(dense, world):
    with Yoda(0) as one:
        one.upload_nodes(dense.nodes)
        one.set_tie_draw(SEED_A)
        whole = one.eval(dense.pods, MODE_SCV)
    with fleet(dense.nodes, DENSE_BOUNDS[world]) as hs:
        got = step(hs, dense.pods, MODE_SCV, (SEED_A, 0))
    for f in ("pick",) + OUT:
        np.testing.assert_array_equal(getattr(got, f), getattr(whole, f), err_msg=f)


def test_rccl_world1(dense):
    """yoda_comm_run over a one-rank RCCL communicator: exchange 4 through ncclAllReduce(MIN)
    itself (more ranks need more GPUs than a test has)."""
    with Yoda(0) as y:
        y.upload_nodes(dense.nodes)
        y.upload_pods(dense.pods)
        y.comm_init(capi.comm_unique_id(), 0, 1)
        y.comm_run(MODE_SCV)
        assert_picks(y.download().pick, dense.picks(SEED_A)[0], "draw off")
        y.set_tie_draw(SEED_A)
        y.shard_tie_draw(True)
        y.comm_run(MODE_SCV)
        got = y.download()
        assert_picks(got.pick, dense.picks(SEED_A)[1], "RCCL world 1")
        np.testing.assert_array_equal(got.n_ties, dense.want.n_ties)


# ---- 4. padded pod order ----------------------------------------------------------------------
def padded_pods():
    """Two (clock, number, has-memory) groups of 190 and 126 pods, interleaved: padding each to
    whole waves adds 4 positions (<= 1/8 of the batch), so a shard's private order (the sharded
    step's caller-order exchange) is the padded counting order, which evaluates two pods twice."""
    pool = synth.make_pods(6000, 5)
    one = (pool.has_clock == 0) & ((pool.has_number == 0) | (pool.number == 1))
    g1 = np.flatnonzero(one & (pool.has_memory == 1))[:190]
    g2 = np.flatnonzero(one & (pool.has_memory == 0))[:126]
    assert g1.size == 190 and g2.size == 126
    return pool.take(np.sort(np.concatenate([g1, g2])))


def test_padded_pod_order(dense):
    case = Case(dense.nodes, padded_pods())
    assert case.picks(SEED_A)[2].size >= 100
    with fleet(case.nodes, DENSE_BOUNDS[2]) as hs:
        run_both(hs, case)
        info = hs[0].order_info()
        assert info["work"] > case.pods.n_pods  # padded copies exist: they share a key slot


# ---- 5. sparse ties, shards without a top-scored node -----------------------------------------
@pytest.fixture(scope="module")
def sparse():
    case = Case(*synth.make_config(3, pods=2000, nodes=20000))
    tied = case.picks(SEED_A)[2]
    assert tied.size >= 20  # 41 of 1500 schedulable pods when written, all over nodes 9841, 14256
    case.sets = [tie_set(case.nodes, case.pods, int(p), MODE_SCV, int(case.want.n_ties[p]))
                 for p in tied]
    return case


# inside: the tie sets within the middle shard; across: the even split cuts them in two
@pytest.mark.parametrize("split", ["inside", "across"])
def test_sparse_ties_and_empty_shards(sparse, split):
    b = (0, 9000, 15000, 20000) if split == "inside" else even_bounds(20000, 3)
    held = [np.unique(np.searchsorted(np.asarray(b), m, side="right")) for m in sparse.sets]
    # a shard with no top-scored node of a tied pod: its key of that pod stays ~0
    assert sum(h.size < 3 for h in held) >= 1
    if split == "inside":  # a whole tie set in one shard: every other shard's key is ~0
        assert sum(h.size == 1 for h in held) >= 1
    else:
        assert sum(h.size == 2 for h in held) >= 1
    with fleet(sparse.nodes, b) as hs:
        run_both(hs, sparse)


# ---- 6. global ids -------------------------------------------------------------------------------
def test_node_offset_hashes_global_ids(dense):
    with fleet(dense.nodes, DENSE_BOUNDS[3], node_offset=70000) as hs:
        (a,) = run_both(hs, dense, node_offset=70000)
    tied = dense.picks(SEED_A, 0, 70000)[2]
    assert (a[tied] >= 70000).all()
    assert (a[tied] - 70000 != dense.picks(SEED_A)[1][tied]).any()  # not the offset-0 draw shifted


def test_pod_base_reproduces_the_whole_batch(dense):
    whole = dense.picks(SEED_A)[1]
    got = []
    with fleet(dense.nodes, DENSE_BOUNDS[2]) as hs:
        for lo, hi in ((0, 150), (150, 300)):
            got.append(step(hs, dense.pods.slice(lo, hi), MODE_SCV, (SEED_A, lo)).pick)
    np.testing.assert_array_equal(np.concatenate(got), whole)


# ---- 7. Mode B -----------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [False, True])
def test_mode_b(distinct):
    nodes, pods = synth.make_config(2)  # 1000 x 5000, tie sets up to 1001 nodes
    if distinct:
        pods = synth.distinct_diskio(pods)
    case = Case(nodes, pods, MODE_DISKIO)
    tied = case.picks(SEED_A)[2]
    assert tied.size >= 900
    with fleet(nodes, even_bounds(nodes.n_nodes, 2)) as hs:
        (a,) = run_both(hs, case)
    if not distinct:  # one (rio, rcpu) class: one tie set, but a draw per pod
        assert np.unique(a[tied]).size > 100


# ---- 8. U64: exact-normalize pods and the other outcomes ----------------------------------------
def H(free, clock=1500, bw=1):
    return po.Card(free_memory=free, total_memory=16000, clock=clock, bandwidth=bw, core=1,
                   power=1, health="Healthy")


def normalize_cluster():
    """raw = 100 * clock + const (clock / MaxBandwidth with MaxBandwidth 1, algorithm.go:283).
    Clocks 1 (lowest), 9e14 and 2^62 / 100 (highest): highest - lowest overflows times 100, the
    highest nodes' product wraps to a small negative (normalized 0), the middle nodes normalize
    to 1 -- so the top NORMALIZED set is the middle nodes 2, 4, 6, not the raw maximizers; split
    at node 4 they straddle the two shards, and the raw maximizers 0, 3 sit in the first."""
    hi, mid = (1 << 62) // 100, 9 * 10 ** 14
    scvs = []
    for clock in (hi, 1, mid, hi, mid, 1, mid, 7):
        scvs.append(po.Scv(card_number=1, card_list=[H(10, clock=clock)], free_memory_sum=10,
                           total_memory_sum=16000))
    pods = [po.Pod(), po.Pod(number=1), po.Pod(clock=7), po.Pod(number=5), po.Pod(clock=mid),
            po.Pod(clock=hi), po.Pod(memory=5)] * 3
    return oracle.from_py(scvs, pods, max_cards=1)


@pytest.fixture(scope="module")
def normalized():
    case = Case(*normalize_cluster())
    w = case.want
    differs = 0
    for p in case.picks(SEED_A)[2]:
        _, feas, raw, _ = oracle.pod_detail(case.nodes, case.pods, int(p), MODE_SCV)
        members = tie_set(case.nodes, case.pods, int(p), MODE_SCV, int(w.n_ties[p]))
        idx = np.flatnonzero(feas)
        differs += set(members) != set(idx[raw[idx] == raw[idx].max()])
    assert differs >= 3  # tied pods that draw over a set that is NOT their raw maximizers
    return case


def test_exact_normalize_pods_comm_run_local(normalized):
    with fleet(normalized.nodes, (0, 4, 8)) as hs:
        assert all(h.path == "u64" for h in hs)
        run_both(hs, normalized, (SEED_A, SEED_B))
        assert hs[0].shard_overflow_count() > 0  # the step did go through the exact merge


def test_exact_normalize_pods_shard_exchange(normalized):
    import torch
    from yoda_amd.dist import ShardExchange
    case = normalized
    with fleet(case.nodes, (0, 4, 8)) as hs:
        for h in hs:
            h.upload_pods(case.pods)
        shards = [case.nodes.slice(0, 4), case.nodes.slice(4, 8)]
        ex = ShardExchange.local(hs, torch.device("cuda:0"), shards, [0, 4],
                                 tie_draw=(SEED_A, 0))
        got = ex.run(MODE_SCV)
        assert hs[0].shard_overflow_count() > 0
        assert_picks(got.pick, case.picks(SEED_A)[1], "ShardExchange, exact normalize")
        for f in ("status", "n_feasible", "n_ties"):
            np.testing.assert_array_equal(getattr(got, f), getattr(case.want, f), err_msg=f)
        np.testing.assert_array_equal(hs[1].download().pick, got.pick)


@pytest.mark.parametrize("name", ["overflow.npz", "edges.npz"])
def test_other_outcomes_keep_theirs(name):
    """overflow.npz: every pod ends STATUS_SCORE_RANGE; edges.npz: DIV_ZERO, UNSCHEDULABLE and
    one-node pods beside tied ones.  On the U64 path."""
    case = Case(*load_golden(name))
    if name == "overflow.npz":
        assert (case.want.status == 3).all()
    else:
        assert {1, 2} <= set(case.want.status.tolist())
    with fleet(case.nodes, even_bounds(case.nodes.n_nodes, 2), force_generic=True) as hs:
        assert all(h.path == "u64" for h in hs)
        run_both(hs, case)


# ---- 9. live state -------------------------------------------------------------------------------
def test_after_set_node_state(dense):
    """Raising the allocated memory of one clone of every base node lowers its score: it leaves
    the tie sets, and the sharded draw runs over the rest."""
    sel = (np.arange(640) + 640 * (np.arange(640) % 8)).astype(np.uint32)
    mod = dense.nodes.slice(0, dense.nodes.n_nodes)
    alloc = mod.alloc_memory.copy()
    alloc[sel] += np.uint64(4096)
    mod.alloc_memory = alloc
    case = Case(mod.normalized(), dense.pods)  # a fresh oracle run on the modified snapshot
    ok = case.want.status == 0
    assert (case.want.n_ties[ok] < 8).any()
    with fleet(dense.nodes, DENSE_BOUNDS[3]) as hs:
        run_both(hs, dense)  # (the draw has run on the old state)
        for h in hs:  # global ids: each shard takes its own
            h.set_node_state(sel, alloc[sel], mod.card_number[sel])
        run_both(hs, case)


# ---- 10. off is off ------------------------------------------------------------------------------
def test_off_is_off(dense):
    off = dense.picks(SEED_A)[0]
    b = DENSE_BOUNDS[2]
    with fleet(dense.nodes, b) as fresh:
        want = step(fresh, dense.pods, MODE_SCV)
    assert_picks(want.pick, off, "fresh handles")
    with fleet(dense.nodes, b) as hs:
        # yoda_set_tie_draw alone: the lowest node
        configure(hs, (SEED_A, 0))
        for h in hs:
            h.shard_tie_draw(False)
            h.upload_pods(dense.pods)
        capi.comm_run_local(hs, MODE_SCV)
        assert_picks(hs[0].download().pick, off, "set_tie_draw alone")
        # on, then off again
        on = step(hs, dense.pods, MODE_SCV, (SEED_A, 0))
        assert_picks(on.pick, dense.picks(SEED_A)[1], "on")
        for h in hs:
            h.shard_tie_draw(False)
        capi.comm_run_local(hs, MODE_SCV)
        for h in hs:
            again = h.download()
            for f in ("pick",) + OUT:
                np.testing.assert_array_equal(getattr(again, f), getattr(want, f), err_msg=f)


@pytest.mark.parametrize("flags", [0, 1])  # 1: YODA_GREEDY_CARD_CAPACITY
def test_sharded_greedy_keeps_the_lowest_node(dense, flags):
    with fleet(dense.nodes, DENSE_BOUNDS[2]) as hs:
        configure(hs, None)
        a = capi.comm_greedy_local(hs, dense.nodes, dense.pods, MODE_SCV, flags)
        configure(hs, (SEED_A, 0))
        b = capi.comm_greedy_local(hs, dense.nodes, dense.pods, MODE_SCV, flags)
    np.testing.assert_array_equal(a, b)


# ---- 11. errors: host-side refusals --------------------------------------------------------------
def raises(code):
    return pytest.raises(YodaError, match=code)


def keys_buffer(n):
    import torch
    return torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda:0")


def test_state_errors(dense):
    keys = keys_buffer(dense.pods.n_pods)
    with fleet(dense.nodes, DENSE_BOUNDS[2]) as hs:
        h = hs[0]
        configure(hs, (SEED_A, 0))
        for x in hs:
            x.upload_pods(dense.pods)
        with raises("YODA_ERR_STATE"):  # before any sharded finalize
            h.shard_draw_keys(MODE_SCV, keys.data_ptr())
        capi.comm_run_local(hs, MODE_SCV)
        before = h.download().pick
        with raises("YODA_ERR_STATE"):  # the step's keys were applied: none pending
            h.shard_draw_apply(keys.data_ptr())
        with raises("YODA_ERR_INVALID_ARG"):
            h.shard_draw_keys(MODE_SCV, 0)
        with raises("YODA_ERR_INVALID_ARG"):
            h.shard_draw_apply(0)
        h.shard_tie_draw(False)
        with raises("YODA_ERR_STATE"):  # the shard draw disabled
            h.shard_draw_keys(MODE_SCV, keys.data_ptr())
        h.shard_tie_draw(True)
        h.set_tie_draw(None)
        with raises("YODA_ERR_STATE"):  # the handle's draw disabled
            h.shard_draw_keys(MODE_SCV, keys.data_ptr())
        h.set_tie_draw(SEED_A)
        np.testing.assert_array_equal(h.download().pick, before)  # the picks as they were
        # the completed step still serves a key pass and ONE apply of it
        h.shard_draw_keys(MODE_SCV, keys.data_ptr())
        h.shard_draw_apply(keys.data_ptr())
        with raises("YODA_ERR_STATE"):
            h.shard_draw_apply(keys.data_ptr())
        h.eval(dense.pods, MODE_SCV)
        with raises("YODA_ERR_STATE"):  # after a private run
            h.shard_draw_keys(MODE_SCV, keys.data_ptr())
        with raises("YODA_ERR_STATE"):
            h.shard_draw_apply(keys.data_ptr())


def test_pending_exact_normalize_refuses_the_keys(normalized):
    """The yoda_shard_* step of the normalize cluster stopped after yoda_shard_finalize: pods
    wait for the exact merge, and the key pass refuses until it ran."""
    import torch
    from yoda_amd.dist import ShardBuffers, ShardExchange, merge_phase1, merge_phase2
    case = normalized
    p = ShardBuffers.ptr
    with fleet(case.nodes, (0, 4, 8)) as hs:
        for h in hs:
            h.upload_pods(case.pods)
        ex = ShardExchange.local(hs, torch.device("cuda:0"), tie_draw=(SEED_A, 0))
        for h, b in zip(hs, ex.bufs):
            h.shard_phase1(MODE_SCV, p(b.maxima), p(b.counts))
        merge_phase1(ex.reduce, ex.bufs)
        for h, b in zip(hs, ex.bufs):
            h.shard_phase2(MODE_SCV, p(b.maxima), p(b.counts), p(b.best), p(b.idx), p(b.ties),
                           p(b.lowest))
        hb = dict(zip(map(id, ex.bufs), hs))
        merge_phase2(ex.reduce, ex.bufs, lambda b: ex._prepare(hb[id(b)], b))
        for h, b in zip(hs, ex.bufs):
            h.shard_finalize(MODE_SCV, p(b.counts), p(b.best_g), p(b.idx), p(b.ties), p(b.lowest))
        assert hs[0].shard_overflow_count() > 0
        for h, b in zip(hs, ex.bufs):
            with raises("YODA_ERR_STATE"):
                h.shard_draw_keys(MODE_SCV, p(b.keys))
        # a whole step on the same handles afterwards draws as expected
        assert_picks(ex.run(MODE_SCV).pick, case.picks(SEED_A)[1], "after the refusal")


def test_shards_must_agree_on_the_draw(dense):
    with fleet(dense.nodes, DENSE_BOUNDS[2]) as hs:
        for h in hs:
            h.upload_pods(dense.pods)
        # two seeds
        configure(hs, (SEED_A, 0))
        hs[1].set_tie_draw(SEED_B)
        with pytest.raises(YodaError, match="YODA_ERR_STATE.*draw"):
            capi.comm_run_local(hs, MODE_SCV)
        # two pod bases
        hs[1].set_tie_draw(SEED_A, 150)
        with pytest.raises(YodaError, match="YODA_ERR_STATE.*draw"):
            capi.comm_run_local(hs, MODE_SCV)
        # one shard's draw off
        hs[1].set_tie_draw(SEED_A)
        hs[1].shard_tie_draw(False)
        with pytest.raises(YodaError, match="YODA_ERR_STATE.*draw"):
            capi.comm_run_local(hs, MODE_SCV)
        # the same handles complete a step once the settings agree
        got = step(hs, dense.pods, MODE_SCV, (SEED_A, 0))
        assert_picks(got.pick, dense.picks(SEED_A)[1], "after the disagreement")
