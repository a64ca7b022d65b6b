"""Greedy candidate lists (yoda_shard_topk on one handle): each pod's best k (score, node)
pairs, (score desc, node asc), against the oracle's per-node raw scores (oracle_pod_detail,
algorithm.go:96 + scheduler.go:154).  N32 batches run the block-classified K2 with packed keys
(k2_block_n32 TKO, k_topk_merge_keys); K = 16 and the F64 path the per-pair k2_score.
After the witness phase 1 (capacity windows) the lists are 16 deep, or -- yoda_shard_topk_deep
-- as deep as yoda_greedy_cap_depth() and exact as far as they reach."""
import functools

import numpy as np
import pytest

import oracle
from yoda_amd import synth
from yoda_amd.capi import Yoda, greedy_cap_depth, topk_k, topk_k_capacity
from yoda_amd.soa import MODE_SCV

pytestmark = pytest.mark.gpu


def lists_of(y, pods):
    """The lists of `pods` on handle `y` as it stands (its snapshot and node-state pushes)."""
    import torch
    y.upload_pods(pods)
    P = pods.n_pods
    dmax = torch.zeros(6 * P, dtype=torch.int64, device="cuda:0")
    dcnt = torch.zeros(2 * P, dtype=torch.int32, device="cuda:0")
    y.shard_phase1(MODE_SCV, dmax.data_ptr(), dcnt.data_ptr())
    out = y.shard_topk(dmax.data_ptr(), dcnt.data_ptr())
    torch.cuda.synchronize()
    return out


def _lists(nodes, pods, force_f64=False, alloc=None):
    y = Yoda(0)
    y.upload_nodes(nodes, force_f64=force_f64)
    if alloc is not None:
        y.update_alloc(alloc)
    out = lists_of(y, pods)
    path = y.path
    y.close()
    return out, path


def lists_of_capacity(y, pods, deep=0):
    """The capacity windows' lists of `pods` on handle `y`: the witness phase 1, then the
    handle's depth (yoda_topk_k_capacity), or -- deep > 0 -- yoda_shard_topk_deep."""
    import torch
    y.upload_pods(pods)
    P = pods.n_pods
    dmax = torch.zeros(6 * P, dtype=torch.int64, device="cuda:0")
    dcnt = torch.zeros(2 * P, dtype=torch.int32, device="cuda:0")
    dwit = torch.zeros(12 * P, dtype=torch.int32, device="cuda:0")
    y.shard_phase1_witness(dmax.data_ptr(), dcnt.data_ptr(), dwit.data_ptr())
    assert y.shard_topk_depth() == topk_k_capacity()
    out = y.shard_topk(dmax.data_ptr(), dcnt.data_ptr(), deep=deep)
    torch.cuda.synchronize()
    return out


def _check(nodes, pods, counts, ts, ti, sample, k=None):
    k = topk_k() if k is None else k
    assert ts.shape[0] == k and ti.shape[0] == k
    for p in sample:
        rc, feas, raw, _ = oracle.pod_detail(nodes, pods, int(p), MODE_SCV)
        idx = np.flatnonzero(feas)
        assert counts[0, p] == idx.size
        top = idx[np.lexsort((idx, -raw[idx]))][:k]
        m = top.size
        np.testing.assert_array_equal(ti[:m, p], top.astype(np.uint32), err_msg=f"pod {p}")
        np.testing.assert_array_equal(ts[:m, p], raw[top].astype(np.float64), err_msg=f"pod {p}")
        assert (ts[m:, p] == -1.0).all() and (ti[m:, p] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("cfg,P,N,want_path", [(2, 700, 3000, "n32"), (3, 1200, 5000, "n32"),
                                               (4, 300, 2500, "n32")])
def test_topk_lists_match_oracle(cfg, P, N, want_path):
    nodes, pods = synth.make_config(cfg, pods=P, nodes=N)
    (counts, ts, ti), path = _lists(nodes, pods)
    assert path == want_path
    rng = np.random.default_rng(cfg)
    _check(nodes, pods, counts, ts, ti, rng.choice(P, 120, replace=False))


def test_topk_lists_mixed_models_and_alloc():
    """Mixed-model nodes (per-pod exact scores), several reciprocal sets and allocations that
    reorder the static part: the same lists as the oracle; F64 records agree with N32."""
    nodes, pods = synth.make_config(2, pods=640, nodes=2600)
    rng = np.random.default_rng(5)
    mix = rng.random(nodes.n_nodes) < 0.5
    k = nodes.card_clock.shape[1]
    half = k // 2
    nodes.card_clock[mix, half:] = np.where(nodes.card_clock[mix, half:] > 0, 1500, 0)
    nodes.card_bandwidth[mix, half:] = np.where(nodes.card_bandwidth[mix, half:] > 0, 1200, 0)
    alloc = (rng.random(nodes.n_nodes) * nodes.total_memory_sum.astype(np.float64)).astype(np.uint64)
    nodes.alloc_memory = alloc
    (counts, ts, ti), path = _lists(nodes, pods)
    assert path == "n32"
    _check(nodes, pods, counts, ts, ti, rng.choice(pods.n_pods, 120, replace=False))
    (c2, ts2, ti2), path2 = _lists(nodes, pods, force_f64=True)
    assert path2 == "f64"
    np.testing.assert_array_equal(ts2, ts)
    np.testing.assert_array_equal(ti2, ti)
    np.testing.assert_array_equal(c2, counts)


def _tie_case():
    """Identical nodes (every score ties: lowest ids first), pods feasible nowhere, one node."""
    nodes, pods = synth.make_config(2, pods=200, nodes=1)
    one = nodes.slice(0, 1)
    many = nodes.slice(0, 1)
    for name in ("card_number", "card_count", "free_memory_sum", "total_memory_sum",
                 "alloc_memory", "cpu", "disk_io"):
        setattr(many, name, np.repeat(getattr(one, name), 300, axis=0))
    for name in ("card_free_memory", "card_total_memory", "card_clock", "card_bandwidth",
                 "card_core", "card_power", "card_healthy"):
        setattr(many, name, np.repeat(getattr(one, name), 300, axis=0))
    pods.number[:50] = 64  # no node has 64 cards
    pods.has_number[:50] = 1
    return many, pods


def test_topk_lists_ties_and_empty():
    """Identical nodes (every score ties: lowest ids first), pods feasible nowhere, one node."""
    many, pods = _tie_case()
    (counts, ts, ti), _ = _lists(many, pods)
    _check(many, pods, counts, ts, ti, range(pods.n_pods))


def test_topk_lists_many_chunks():
    """A small batch over many nodes: hundreds of chunk lists per pod, so every thread of the
    merge (k_topk_merge_keys: one workgroup per pod) folds several lists before the wave and
    workgroup extraction rounds."""
    nodes, pods = synth.make_config(3, pods=128, nodes=40000)
    (counts, ts, ti), path = _lists(nodes, pods)
    assert path == "n32"
    rng = np.random.default_rng(11)
    _check(nodes, pods, counts, ts, ti, rng.choice(pods.n_pods, 40, replace=False))


# ---- the capacity windows' lists: 16 deep after the witness phase 1, and the deep lists ----
P_CAP, N_CAP = 300, 1500


def _cap_case(name):
    """(nodes, pods, upload kwargs, record path, the block top-k kernels run) of a named case."""
    import witness_cases
    if name == "ties":
        nodes, pods = _tie_case()
        return nodes, pods, {}, "n32", True
    base = name.split("/")[0]
    nodes, pods = getattr(witness_cases, base)(P_CAP, N_CAP)
    f64 = name.endswith("/f64")
    # (topk_block_ok in yoda_capi.cpp: N32 with at most 8 card slots)
    return (nodes, pods, {"force_f64": True} if f64 else {}, "f64" if f64 else "n32",
            not f64 and nodes.max_cards <= 8)


_ORDERS = {}


def _oracle_orders(name, nodes, pods):
    """Per pod the feasible nodes in (score desc, node asc) order and their raw scores: computed
    once per case, shared by the 16-deep and the deep check."""
    name = name.split("/")[0]  # (the record path does not change the oracle's view)
    if name not in _ORDERS:
        out = []
        for p in range(pods.n_pods):
            _, feas, raw, _ = oracle.pod_detail(nodes, pods, p, MODE_SCV)
            idx = np.flatnonzero(feas)
            top = idx[np.lexsort((idx, -raw[idx]))]
            out.append((top.astype(np.uint32), raw[top].astype(np.float64)))
        _ORDERS[name] = out
    return _ORDERS[name]


def _cap_lists(name, deep=0):
    nodes, pods, kw, want_path, block = _cap_case(name)
    assert pods.n_pods <= 300  # every pod is checked
    with Yoda(0) as y:
        y.upload_nodes(nodes, **kw)
        assert y.path == want_path
        counts, ts, ti = lists_of_capacity(y, pods, deep)
    return nodes, pods, block, counts, ts, ti


CAP_CASES = ["tied_free", "tied_free/f64", "mixed", "het", "ties", "tied_top"]


@pytest.mark.parametrize("name", CAP_CASES)
def test_capacity_lists_match_oracle(name):
    """The 16-deep lists of a capacity window (the kTopKCap instantiations): tied_free the block
    top-k K2 with packed keys and k_topk_merge_keys, mixed its per-pod exact scores, f64 and
    het (K = 16) the per-pair k2_topk with k_topk_merge_wave; every pod, the rule of the 8-deep
    lists with k = 16."""
    nodes, pods, _, counts, ts, ti = _cap_lists(name)
    k = topk_k_capacity()
    assert k == 16
    for p, (top, raw) in enumerate(_oracle_orders(name, nodes, pods)):
        assert counts[0, p] == top.size
        m = min(k, top.size)
        np.testing.assert_array_equal(ti[:m, p], top[:m], err_msg=f"pod {p}")
        np.testing.assert_array_equal(ts[:m, p], raw[:m], err_msg=f"pod {p}")
        assert (ts[m:, p] == -1.0).all() and (ti[m:, p] == 0xFFFFFFFF).all()


@functools.lru_cache(maxsize=None)
def _deep_lengths(name):
    """Every pod's deep list against the oracle as far as it reaches (one device run per case,
    shared by the tests below); returns (L [P], n_feasible [P], deep, block kernels run)."""
    deep = greedy_cap_depth()
    nodes, pods, block, counts, ts, ti = _cap_lists(name, deep)
    assert ts.shape[0] == deep and ti.shape[0] == deep and deep > topk_k_capacity()
    Ls, nfs = [], []
    for p, (top, raw) in enumerate(_oracle_orders(name, nodes, pods)):
        nf = top.size
        assert counts[0, p] == nf
        full = ti[:, p] != 0xFFFFFFFF
        L = int(full.sum())
        assert full[:L].all(), f"pod {p}: a gap in the list"
        assert (ts[L:, p] == -1.0).all() and (ti[L:, p] == 0xFFFFFFFF).all()
        # (the lower bound min(16, nf) has a test of its own: the figures of every pod first)
        assert min(topk_k(), nf) <= L <= min(deep, nf), f"pod {p}: L = {L}, n_feasible = {nf}"
        np.testing.assert_array_equal(ti[:L, p], top[:L], err_msg=f"pod {p}")
        np.testing.assert_array_equal(ts[:L, p], raw[:L], err_msg=f"pod {p}")
        Ls.append(L)
        nfs.append(nf)
    L, nf = np.array(Ls), np.array(nfs)
    k = topk_k_capacity()
    short = L < np.minimum(k, nf)
    print(f"{name}: deep = {deep}, pods with L < min({k}, n_feasible): {int(short.sum())} of "
          f"{L.size}, their L {np.unique(L[short]).tolist()}; L > {k}: {int((L > k).sum())}; "
          f"L < min(deep, n_feasible): {int((L < np.minimum(deep, nf)).sum())}")
    return L, nf, deep, block


@pytest.mark.parametrize("name", CAP_CASES)
def test_deep_lists_exact_as_far_as_they_reach(name):
    """yoda_shard_topk_deep with deep = yoda_greedy_cap_depth(): per pod the first L entries are
    the oracle's first L, node and score, everything past them is empty and L <=
    min(deep, n_feasible); without the block kernels (f64, K = 16) the 16-deep lists padded."""
    L, nf, _, block = _deep_lengths(name)
    if not block:
        np.testing.assert_array_equal(L, np.minimum(topk_k_capacity(), nf))


@pytest.mark.parametrize("name", CAP_CASES)
def test_deep_lists_reach_the_capacity_depth(name):
    """min(16, n_feasible) <= L for every pod: a deep list is no shorter than the 16-deep list
    yoda_shard_topk gives after the same phase 1.  k_topk_merge_deep keeps max(TK, candidates
    above every full chunk list's TK-th key) entries, TK the chunk lists' depth: with every
    score tied (`ties`) that is TK.  (With 8-deep chunk lists under the merge, 24 of the 200
    tie pods had L = 8 of 300 feasible nodes; shard_topk_impl now asks for 16-deep ones.)"""
    L, nf, _, _ = _deep_lengths(name)
    short = np.flatnonzero(L < np.minimum(topk_k_capacity(), nf))
    assert short.size == 0, (f"{short.size} pods, e.g. pod {short[0]}: L = {L[short[0]]}, "
                             f"n_feasible = {nf[short[0]]}")


@pytest.mark.parametrize("name", ["tied_top"])
def test_deep_lists_exercise_the_merge(name):
    """On the block path k_topk_merge_deep decides where a list ends: a pod whose feasible nodes
    are sparse in every chunk gets all of them (up to deep), one dense in some chunk ends where
    a node its chunk left unlisted could enter.  Both kinds must occur, or the merge's cut is
    untested.  With 16-deep lists of 64-node chunks no pod of tied_free or mixed at 300 x 1500
    is cut short (every list is min(deep, n_feasible) long: 210 and 246 pods above 16), so the
    case is tied_top, whose two leading chunks tie at the top of most pods' lists."""
    L, nf, deep, block = _deep_lengths(name)
    assert block
    assert (L > topk_k_capacity()).any()
    assert (L < np.minimum(deep, nf)).any()
