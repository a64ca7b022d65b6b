"""GPU: the score quotients x*100/M on the many-model fleets of tests/quotient_cases.py, through
every entry point that computes them, bit-exact against the C oracle (oracle.schedule /
oracle.pod_detail / oracle.greedy).  tests/test_quotient_cases.py shows on the CPU that these
fleets hold thousands of distinct (x, M) pairs per quotient, a tenth of them on each rounding
edge, and that a wrong reciprocal, divisor or sum moves the picks.  Each tier also pins the
host's choice of record format (choose_format): the path, the f32 / f64 quotient threshold, the
16-bit packing, memory ranks and the grouped node order."""
import functools

import numpy as np
import pytest

import card_update_cases
import oracle
import quotient_cases as qc
from test_gpu_node_present import _repeat_nodes
from test_gpu_parity import assert_same
from test_gpu_topk import _check as check_lists, lists_of, lists_of_capacity
from tie_draw_cases import expected as draw_expected
from yoda_amd.capi import Yoda, comm_run_local, topk_k_capacity
from yoda_amd.soa import MODE_SCV, NodeSoA

pytestmark = pytest.mark.gpu
CAP = 1  # YODA_GREEDY_CARD_CAPACITY
SEED = 0x51DEC0DE
FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")


@pytest.fixture(scope="module")
def dev():
    y = Yoda(0)
    yield y
    y.close()


@functools.lru_cache(maxsize=None)
def want_of(name, small=False):
    t = qc.tier(name, small)
    return oracle.schedule(t.nodes, t.pods, MODE_SCV, threads=8)


def upload(y, t, **kw):
    y.upload_nodes(t.nodes, **kw)


def check_format(y, t):
    assert y.path == t.path
    assert (y.small_field_max <= qc.F32_SMALL_MAX) == t.flags["small_le"]
    assert y.memory_ranks == t.flags["ranks"]
    assert y.node_order_grouped == t.flags["grouped"]


def check_rows(y, nodes, pods, tag):
    """Raw rows == pod_detail on the feasible nodes and -1 elsewhere; normalized rows where the
    pod is scheduled among at least two feasible nodes."""
    y.upload_pods(pods)
    feas, rows, norm = y.score_rows(MODE_SCV, norm=True)
    for p in range(pods.n_pods):
        rc, f, raw, nrm = oracle.pod_detail(nodes, pods, p, MODE_SCV)
        bad = np.flatnonzero(f & (rows[p] != raw))
        if bad.size:   # the failing (tier, pod, node) and its card fields
            n = int(bad[0])
            pytest.fail(f"{tag}: pod {p} node {n}: row {rows[p][n]} oracle {raw[n]}; bandwidth "
                        f"{nodes.card_bandwidth[n]} clock {nodes.card_clock[n]} core "
                        f"{nodes.card_core[n]} power {nodes.card_power[n]} total "
                        f"{nodes.card_total_memory[n]}; {bad.size} nodes differ")
        np.testing.assert_array_equal(feas[p], f, err_msg=f"{tag}: pod {p}")
        assert (rows[p][~f] == -1).all(), f"{tag}: pod {p}"
        if f.sum() >= 2 and rc == 0:
            np.testing.assert_array_equal(norm[p], nrm, err_msg=f"{tag}: pod {p}")


def bits_of(y, n):
    words = y.download_bitmask()
    return np.unpackbits(words.view(np.uint8), bitorder="little", axis=1)[:, :n].astype(bool)


@pytest.mark.parametrize("name", qc.TIERS)
def test_tier(dev, name):
    """eval of every pod, yoda_run with the bitmask, and the raw and normalized rows of 24 pods."""
    t, want = qc.tier(name), want_of(name)
    upload(dev, t)
    check_format(dev, t)
    assert_same(dev.eval(t.pods, MODE_SCV), want)
    dev.upload_pods(t.pods)
    dev.run(MODE_SCV, bitmask=True)
    assert_same(dev.download(), want)
    bits = bits_of(dev, t.nodes.n_nodes)
    np.testing.assert_array_equal(bits.sum(axis=1), want.n_feasible)
    for p in range(0, t.pods.n_pods, 37):
        fit, _ = qc.scored_cards(t.nodes, t.pods, p)
        np.testing.assert_array_equal(bits[p], fit, err_msg=f"pod {p}")
    check_rows(dev, t.nodes, qc.row_pods(t), name)


@pytest.mark.parametrize("name", ["q32", "wide"])
def test_one_block_one_node_chunk(dev, name):
    """130 pods x 65 nodes: one pod block and a partly live wave over two node blocks."""
    t, want = qc.tier(name, True), want_of(name, True)
    upload(dev, t)
    assert dev.path == t.path and not dev.node_order_grouped
    assert (dev.small_field_max <= qc.F32_SMALL_MAX) == t.flags["small_le"]
    assert_same(dev.eval(t.pods, MODE_SCV), want)
    check_rows(dev, t.nodes, qc.row_pods(t), name + "/small")


VARIANTS = ("per_node_k1", "per_node_k2", "no_gtab", "no_uniform", "force_f64", "force_generic")


@pytest.mark.parametrize("name", qc.N32_TIERS)
def test_upload_flags(dev, name):
    """The per-node K1 / K2, the K2 without the G table, the per-card branch (no_uniform) and the
    F64 / U64 records of the same fleet: every output equals the oracle's.  Beyond 55738
    no_uniform leaves no one-model node, so the snapshot must come out F64."""
    t, want = qc.tier(name), want_of(name)
    for flag in VARIANTS:
        upload(dev, t, **{flag: True})
        path = qc.predict_format(t.nodes, **{flag: True})[0]
        assert dev.path == path, flag
        if flag == "no_uniform" and name in ("pack16", "wide", "score32"):
            assert path == "f64"
        if flag in ("force_f64", "force_generic"):
            assert path == ("f64" if flag == "force_f64" else "u64")
        assert_same(dev.eval(t.pods, MODE_SCV), want)


@pytest.mark.parametrize("name", ["q32", "q32_grouped", "pack16", "wide", "q32_mixed", "ranks"])
def test_pod_order(dev, name):
    """No order, the padded and the unpadded counting order (private runs), the radix order:
    identical outputs, each kind seen.  The radix order is reached through the bitmask run, which
    always takes it; a private run falls back to it only with more than 16384 pod groups, which a
    600-pod batch cannot have (tests/test_gpu_order.py::test_too_many_groups_radix does that)."""
    t, want = qc.tier(name), want_of(name)
    upload(dev, t)
    outs, masks = [], []
    try:
        for order in (0, 1, 2):
            dev.set_pod_order(order != 0, pad=order != 2)
            outs.append(dev.eval(t.pods, MODE_SCV))
            assert dev.order_info()["kind"] == (2 if order else 0)
            dev.run(MODE_SCV, bitmask=True)
            assert dev.order_info()["kind"] == (1 if order else 0)
            outs.append(dev.download())
            masks.append(dev.download_bitmask())
    finally:
        dev.set_pod_order(True)
    for got in outs:
        assert_same(got, want)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(got, f), getattr(outs[0], f), err_msg=f)
    for m in masks[1:]:
        np.testing.assert_array_equal(m, masks[0])


@pytest.mark.parametrize("name", ["q32", "wide", "score32"])
def test_candidate_lists(name):
    """shard_phase1 + shard_topk, and the capacity depth after shard_phase1_witness: top_score is
    f64 and equals the oracle's raw scores exactly."""
    t = qc.tier(name)
    sample = np.linspace(0, t.pods.n_pods - 1, 48).astype(np.int64)
    with Yoda(0) as y:
        upload(y, t)
        assert y.path == "n32"
        counts, ts, ti = lists_of(y, t.pods)
        check_lists(t.nodes, t.pods, counts, ts, ti, sample)
        counts, ts, ti = lists_of_capacity(y, t.pods)
        check_lists(t.nodes, t.pods, counts, ts, ti, sample, k=topk_k_capacity())


def _holders_first(nodes):
    """The fleet with every node that holds a field's largest value moved to the front."""
    real = np.arange(nodes.max_cards)[None, :] < nodes.card_count[:, None]
    top = np.zeros(nodes.n_nodes, bool)
    for f in ("bandwidth", "clock", "core", "power", "total_memory", "free_memory"):
        a = np.where(real, getattr(nodes, "card_" + f), 0)
        top |= (a == a.max()).any(axis=1)
    order = np.argsort(~top, kind="stable")
    return nodes.take(order).normalized(), int(top.sum())


@pytest.mark.parametrize("name", ["q32", "wide", "field44"])
def test_node_shards_divide_by_maxima_they_never_saw(name):
    """comm_run_local over 2 and 3 shards with every holder of a field's maximum in shard 0."""
    t = qc.tier(name)
    nodes, n_top = _holders_first(t.nodes)
    want = oracle.schedule(nodes, t.pods, MODE_SCV, threads=8)
    kw = {"force_f64": True} if t.path == "f64" else {}   # (one shard alone would pick N32)
    for world in (2, 3):
        b = np.linspace(0, nodes.n_nodes, world + 1).astype(int)
        assert n_top < b[1]
        hs = [Yoda(0) for _ in range(world)]
        try:
            for r, h in enumerate(hs):
                h.upload_nodes(nodes.slice(b[r], b[r + 1]), node_offset=int(b[r]), **kw)
                assert h.path == t.path
                assert (h.small_field_max <= qc.F32_SMALL_MAX) == t.flags["small_le"] or r > 0
                h.upload_pods(t.pods)
            comm_run_local(hs, MODE_SCV)
            for h in hs:
                assert_same(h.download(), want)
        finally:
            for h in hs:
                h.close()


def _concat(a, b):
    return NodeSoA(**{f: np.concatenate([getattr(a, f), getattr(b, f)], axis=0)
                      for f in a.__dataclass_fields__}).normalized()


@pytest.mark.parametrize("one_model", [True, False])
def test_exchange_reuploads_the_narrow_shard(one_model):
    """A q32 shard next to a wide one (ShardExchange.local): agree_on_path re-uploads the narrow
    shard with f64 quotients -- it stays N32 when all its nodes hold one model, else both shards
    end on F64 -- and the picks equal the oracle's on the whole fleet."""
    import torch
    from yoda_amd.dist import ShardExchange
    q, w = qc.tier("q32"), qc.tier("wide")
    keep = np.arange(q.nodes.n_nodes)
    if one_model:
        real = np.arange(q.nodes.max_cards)[None, :] < q.nodes.card_count[:, None]
        one = q.nodes.card_count > 0
        for f in ("clock", "bandwidth", "core", "power", "total_memory"):
            a = getattr(q.nodes, "card_" + f)
            one &= (np.where(real, a, a[:, :1]) == a[:, :1]).all(axis=1)
        keep = np.flatnonzero(one)
    shards = [q.nodes.take(keep[:1500]).normalized(), w.nodes.slice(0, 1500)]
    nodes = _concat(*shards)
    pods = q.pods.take(np.arange(0, 600, 4))
    wp = w.pods.take(np.arange(0, 600, 4))
    pods = type(pods)(**{f: np.concatenate([getattr(pods, f), getattr(wp, f)])
                         for f in pods.__dataclass_fields__}).normalized()
    want = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    assert (want.status == 0).mean() > 0.5
    handles = []
    try:
        for i, sh in enumerate(shards):
            y = Yoda(0)
            y.upload_nodes(sh, node_offset=1500 * i)
            y.upload_pods(pods)
            handles.append(y)
        assert handles[0].small_field_max <= qc.F32_SMALL_MAX < handles[1].small_field_max
        assert [h.path for h in handles] == ["n32", "n32"]
        ex = ShardExchange.local(handles, torch.device("cuda:0"), shards, [0, 1500])
        assert [h.path for h in handles] == (["n32", "n32"] if one_model else ["f64", "f64"])
        assert_same(ex.run(MODE_SCV), want)
    finally:
        for y in handles:
            y.close()


def test_tie_draw_rescoring(dev):
    """q32_grouped four times over (every pod ties over the clones): with the seeded draw on, each
    pick is the drawn member of the oracle's tie set -- the draw pass rescores the pairs with
    quotient code of its own."""
    t = qc.tier("q32_grouped")
    nodes = _repeat_nodes(t.nodes, 4)
    pods = t.pods.slice(0, 160)
    want, _, on, tied = draw_expected(nodes, pods, MODE_SCV, SEED)
    assert tied.size >= 100 and (want.n_ties[tied] % 4 == 0).all()
    dev.upload_nodes(nodes)
    assert dev.path == "n32" and dev.node_order_grouped
    try:
        dev.set_tie_draw(SEED)
        got = dev.eval(pods, MODE_SCV)
    finally:
        dev.set_tie_draw(None)
    np.testing.assert_array_equal(got.pick, on)
    assert (got.pick[tied] != want.pick[tied]).any()
    got.pick = want.pick
    assert_same(got, want)


@pytest.mark.parametrize("flags", [0, CAP])
@pytest.mark.parametrize("name", ["q32", "wide"])
def test_greedy(name, flags):
    t = qc.tier(name)
    pods = qc.make_pods(SEED & 0xFFFF, 700, t.nodes, priorities=True)
    with Yoda(0) as y:
        upload(y, t)
        assert y.path == "n32"
        got = y.greedy(pods, MODE_SCV, flags)
    pick, _ = oracle.greedy(t.nodes, pods, MODE_SCV, flags)
    np.testing.assert_array_equal(got, pick)
    assert (pick >= 0).mean() > 0.5


@pytest.mark.parametrize("name", ["q32_grouped", "wide"])
def test_live_updates(name):
    """yoda_update_node_cards on 200 nodes with frees on the pods' thresholds, then
    yoda_set_node_state on 200 nodes: eval equals the oracle on the modified snapshot and the
    handle's tables equal what it would rebuild (yoda_snapshot_check)."""
    t = qc.tier(name)
    nodes, pods = t.nodes, t.pods
    rng = np.random.default_rng(SEED)
    model = card_update_cases.Model(nodes)
    ids = rng.choice(nodes.n_nodes, 200, replace=False).astype(np.uint32)
    real = np.arange(nodes.max_cards)[None, :] < nodes.card_count[ids][:, None]
    mem = pods.memory[pods.has_memory == 1]
    near = mem[rng.integers(0, mem.size, size=real.shape)].astype(np.int64) + \
        rng.integers(-1, 2, size=real.shape)
    free = np.minimum(np.clip(near, 0, None).astype(np.uint64), nodes.card_total_memory[ids])
    free = np.where(real, free, 0).astype(np.uint64)
    healthy = ((nodes.card_healthy[ids] != 0) ^ (rng.random(real.shape) < 0.1)) & real
    cards = ("cards", ids, free, healthy.astype(np.uint8), free.sum(axis=1, dtype=np.uint64))
    ids2 = rng.choice(nodes.n_nodes, 200, replace=False).astype(np.uint32)
    total = nodes.total_memory_sum[ids2]
    alloc = np.minimum((rng.random(200) * (total.astype(np.float64) + 1)).astype(np.uint64), total)
    push = ("push", ids2, alloc, rng.integers(0, 9, 200).astype(np.uint64))
    with Yoda(0) as y:
        upload(y, t)
        check_format(y, t)
        for step in (cards, push):
            model.apply(step)
            if step[0] == "cards":
                y.update_cards(*step[1:])
            else:
                y.set_node_state(*step[1:])
        now = model.nodes()
        want = oracle.schedule(now, pods, MODE_SCV, threads=8)
        before = want_of(name)
        assert (want.pick != before.pick).mean() > 0.02
        assert_same(y.eval(pods, MODE_SCV), want)
        assert y.snapshot_check()[1].tolist() == [0, 0, 0, 0]
