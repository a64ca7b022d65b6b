"""The device outputs a capacity greedy window is certified from (yoda_shard_phase1_witness,
include/yoda.h): per pod the feasible / zero-total counts, the six PreScore maxima and, per
maxima field, the witness count and the lowest witness node -- compared for EVERY pod, exactly,
with the numpy reference of tests/witness_cases.py (tests/test_witness_cases.py pins that
reference to the oracle and shows that the inputs have small, varied counts).  The greedy
tests see these words only through the picks, which a wrong count rarely moves: a window whose
certificate fails is evaluated again.

Which kernel a case reaches follows phase1_witness() in yoda_capi.cpp: the block-classified
witness K1 (k1_block_n32 WIT) when the record path is N32 and every node is one GPU model with
one TotalMemory, else the per-node k1_witness<N32 | F64>; then k_reduce_wit up to 48 node
chunks and the two-phase k_reduce_wit_split beyond.  The block K1 takes 64-node chunks at
these batch sizes, the per-node K1 the batch's K1 chunks (64 nodes too: few pod blocks).

Where a maximum is the floor 1 the witness words are unspecified (yoda.h) and not compared."""
import functools

import numpy as np
import pytest

import witness_cases as cases
from yoda_amd.capi import Yoda, YodaError, topk_k_capacity
from yoda_amd.dist import HandleShard, Reducer, merge_witness, shard_bounds
from yoda_amd.soa import MODE_SCV

pytestmark = pytest.mark.gpu

BUILDERS = {"tied_free": cases.tied_free, "mixed": cases.mixed, "het": cases.het,
            "no_qualifying": cases.no_qualifying, "wide_chunks": cases.wide_chunks,
            "tied_top": cases.tied_top}


@functools.lru_cache(maxsize=None)
def _case(name, P, N, shuffle=False):
    """(nodes, pods, reference), computed once and shared: do not write to them."""
    nodes, pods = BUILDERS[name](P, N)
    if shuffle:
        pods = pods.take(np.random.default_rng(P + N).permutation(P))
    return nodes, pods, cases.reference(nodes, pods)


def witness_of(y, pods):
    """(counts [2, P], maxima [6, P], wit [12, P]) of `pods` on handle `y` as it stands."""
    import torch
    y.upload_pods(pods)
    P = max(pods.n_pods, 1)
    dmax = torch.zeros(6 * P, dtype=torch.int64, device="cuda:0")
    dcnt = torch.zeros(2 * P, dtype=torch.int32, device="cuda:0")
    dwit = torch.zeros(12 * P, dtype=torch.int32, device="cuda:0")
    y.shard_phase1_witness(dmax.data_ptr(), dcnt.data_ptr(), dwit.data_ptr())
    assert y.shard_topk_depth() == topk_k_capacity()
    counts, _, _ = y.shard_topk(dmax.data_ptr(), dcnt.data_ptr())
    mx, wit = y.shard_witness_download(dmax.data_ptr(), dwit.data_ptr())
    torch.cuda.synchronize()
    return counts, mx, wit


def assert_witness(got, ref, tag=""):
    counts, mx, wit = got
    np.testing.assert_array_equal(counts[0], ref["n_feasible"], err_msg=f"{tag}: n_feasible")
    np.testing.assert_array_equal(counts[1], ref["n_zero_total"], err_msg=f"{tag}: n_zero_total")
    np.testing.assert_array_equal(mx, ref["maxima"], err_msg=f"{tag}: maxima")
    live = ref["maxima"] > 1
    assert (ref["wit_count"][live] >= 1).all()
    # (flattened over the (field, pod) pairs np.argwhere(live) lists, in that order)
    np.testing.assert_array_equal(wit[:6][live], ref["wit_count"][live],
                                  err_msg=f"{tag}: witness counts")
    np.testing.assert_array_equal(wit[6:][live], ref["wit_node"][live],
                                  err_msg=f"{tag}: lowest witnesses")


def _run(name, P, N, shuffle=False, want_path="n32", **upload_kw):
    nodes, pods, ref = _case(name, P, N, shuffle)
    with Yoda(0) as y:
        y.upload_nodes(nodes, **upload_kw)
        assert y.path == want_path
        got = witness_of(y, pods)
        ranks = y.memory_ranks
    assert_witness(got, ref, f"{name} {P}x{N}")
    return ranks


@pytest.mark.parametrize("P,N", [(1, 1), (64, 64), (65, 63), (130, 577), (300, 1500),
                                 (130, 4700)])
def test_block_witness_sizes(P, N):
    """tied_free is one GPU model per node on N32: the block-classified witness K1.  One pod
    and one node; exactly one wave and one block; a second, one-lane wave over a partly live
    block; 130 pods (the last wave has 2 live lanes) over 577 nodes = 10 chunks rounded to 16
    (trailing chunks empty, the last block with one node); 300 shuffled pods (the batch is
    reordered above 128: the download maps back); 4700 nodes = 74 chunks rounded to 80, beyond
    the 48 that k_reduce_wit takes: k_reduce_wit_split over 5 chunk slices."""
    _run("tied_free", P, N, shuffle=P > 128)


def test_block_witness_chunks_of_several_blocks():
    """wide_chunks: 128 pod blocks, so plan_chunks gives K1 node chunks of several 64-node
    blocks (the window sizes of a real greedy batch do too).  Within a chunk the block K1 folds
    the blocks it decides as a whole BEFORE the nodes of the undecided blocks, lane = block
    then lane = node: the lowest witness has to come out of a fold that is not in id order."""
    _run("wide_chunks", 32768, 8192)


def test_block_witness_whole_blocks_tie():
    """tied_top: two whole 64-node blocks of identical nodes, which the block K1 decides as a
    whole for most waves: their witness counts (64 a block) come from the block summaries."""
    _run("tied_top", 300, 1500)


SHAPES = [(300, 1500), (130, 577)]


@pytest.mark.parametrize("P,N", SHAPES)
def test_per_node_n32_mixed_models(P, N):
    """mixed: half the nodes hold several GPU models, so all_one_model is false and the per-node
    k1_witness<N32> runs: its one-model branch on the other half, the per-card branch here."""
    _run("mixed", P, N)


@pytest.mark.parametrize("P,N", SHAPES)
def test_per_node_f64(P, N):
    """force_f64: the path is not N32, so k1_witness<F64> (per-card branch only)."""
    _run("tied_free", P, N, want_path="f64", force_f64=True)


@pytest.mark.parametrize("P,N", SHAPES + [(130, 4700)])
def test_block_witness_memory_ranks(P, N):
    """mem_ranks: the block witness K1 over FreeMemory / TotalMemory ranks; the maxima come back
    as values (rank_value in k_reduce_wit; k_rank_maxima after k_reduce_wit_split at 4700)."""
    assert _run("tied_free", P, N, mem_ranks=True)


@pytest.mark.parametrize("P,N", SHAPES)
def test_per_node_n32_sixteen_cards(P, N):
    """het: K = 16 with per-card TotalMemory, so no node is one-model: k1_witness<16, N32>,
    per-card branch; cardless nodes, card_count != CardNumber, pods feasible nowhere."""
    _run("het", P, N)


@pytest.mark.parametrize("P,N", SHAPES)
def test_no_qualifying_cards(P, N):
    """no_qualifying: feasible nodes without a card (they count, with their zero totals, and
    contribute nothing) and pods whose every maximum stays at the floor.  A cardless node is not
    one-model (pack_node), so all_one_model is false: the per-node k1_witness<N32>, the
    cardless nodes in its per-card branch, the others in its one-model branch."""
    _run("no_qualifying", P, N)


def test_u64_path_is_refused():
    """The U64 record path has no witness phase 1: YODA_ERR_STATE, and the handle goes on."""
    nodes, pods, ref = _case("tied_free", 130, 577)
    with Yoda(0) as y:
        y.upload_nodes(nodes, force_generic=True)
        assert y.path == "u64"
        with pytest.raises(YodaError, match="YODA_ERR_STATE"):
            witness_of(y, pods)
        res = y.eval(pods, MODE_SCV)
        np.testing.assert_array_equal(res.n_feasible, ref["n_feasible"])
        np.testing.assert_array_equal(res.maxima.T, ref["maxima"])
        y.upload_nodes(nodes)
        assert_witness(witness_of(y, pods), ref, "after the refusal")


@pytest.mark.parametrize("name", ["tied_free", "mixed"])
def test_witness_after_node_state_push(name):
    """A long-lived handle: a yoda_set_node_state push lowers CardNumber of ~100 nodes (every
    tied one), then the old values come back.  The block K1 decides whole blocks from the block
    summaries' CardNumber bounds and takes their witness counts from tables built at upload;
    the per-node K1 (mixed) reads the records the push rewrites."""
    P, N = 300, 1500
    nodes, pods, ref = _case(name, P, N)
    ids, alloc, cn, after = cases.decrement(nodes, seed=3)
    ref_after = cases.reference(after, pods)
    with Yoda(0) as y:
        y.upload_nodes(nodes)
        assert y.path == "n32"
        assert_witness(witness_of(y, pods), ref, "as uploaded")
        y.set_node_state(ids, alloc, cn)
        assert_witness(witness_of(y, pods), ref_after, "after the push")
        y.set_node_state(ids, alloc, nodes.card_number[ids])
        assert_witness(witness_of(y, pods), ref, "pushed back")


def _shards(nodes, pods, bounds):
    import torch
    dev = torch.device("cuda:0")
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        y = Yoda(0)
        y.upload_nodes(nodes.slice(int(lo), int(hi)), node_offset=int(lo))
        s = HandleShard(y, dev)
        s.upload_pods(pods)
        out.append(s)
    return out


def _shard_download(s):
    counts, _, _ = s.topk()
    mx, wit = s.witness()
    return counts, mx, wit


def _merge_and_check(shards, whole, tag):
    bufs = [s.phase1_witness() for s in shards]
    sb = dict(zip(map(id, bufs), shards))
    merge_witness(Reducer(local=True), bufs, lambda b: sb[id(b)].witness_prepare(b))
    for r, s in enumerate(shards):
        assert_witness(_shard_download(s), whole, f"{tag}: merged, shard {r}")


@pytest.mark.parametrize("name", ["tied_free", "mixed"])
def test_shards_local_then_merged(name):
    """Three shards on one GPU over shard_bounds(1500, 3): 500 and 1000 are no multiples of 64
    and node_offset != 0.  Each shard's own download carries GLOBAL ids; after merge_witness
    (k_wit_prepare clears a shard below the global maximum, counts SUM, nodes MIN) every shard
    holds the unsharded result."""
    P, N = 300, 1500
    nodes, pods, whole = _case(name, P, N)
    bounds = shard_bounds(N, 3)
    shards = _shards(nodes, pods, bounds)
    try:
        for r, s in enumerate(shards):
            s.phase1_witness()
            ref = cases.reference(nodes, pods, int(bounds[r]), int(bounds[r + 1]))
            assert_witness(_shard_download(s), ref, f"{name}: shard {r} alone")
        _merge_and_check(shards, whole, name)
    finally:
        for s in shards:
            s.h.close()


def test_empty_shard_between_real_ones():
    """A shard without nodes next to two real ones: counts 0, maxima 1, and the merged result
    is the unsharded one."""
    P, N = 300, 1500
    nodes, pods, whole = _case("tied_free", P, N)
    shards = _shards(nodes, pods, [0, 700, 700, N])
    try:
        shards[1].phase1_witness()
        counts, mx, wit = _shard_download(shards[1])
        assert (counts == 0).all() and (mx == 1).all()
        assert_witness((counts, mx, wit), cases.reference(nodes, pods, 700, 700), "empty shard")
        _merge_and_check(shards, whole, "with an empty shard")
    finally:
        for s in shards:
            s.h.close()
