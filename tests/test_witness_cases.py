"""The witness reference of tests/witness_cases.py is right (against the C oracle and against a
brute-force loop over pyoracle's Filter and card loop), and its inputs can fail a wrong kernel:
with the reference alone, the witness counts are small and varied, the lowest witnesses spread
over lanes, blocks and shards, and a CardNumber push moves them.  These are conditions on the
inputs, not on libyoda (tests/test_gpu_witness.py compares libyoda with the reference)."""
import numpy as np
import pytest

import oracle
import pyoracle
import witness_cases as cases
from yoda_amd.dist import shard_bounds
from yoda_amd.soa import MODE_SCV

P, N = 300, 1500
BUILDERS = {"base": cases.base, "tied_free": cases.tied_free, "mixed": cases.mixed,
            "het": cases.het, "no_qualifying": cases.no_qualifying, "tied_top": cases.tied_top}


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_reference_matches_oracle(name):
    nodes, pods = BUILDERS[name](P, N)
    ref = cases.reference(nodes, pods)
    res = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    np.testing.assert_array_equal(ref["n_feasible"], res.n_feasible)
    np.testing.assert_array_equal(ref["maxima"], res.maxima.T)
    # a maximum above the floor has a witness, and the lowest one is a node of the snapshot
    above = ref["maxima"] > 1
    assert (ref["wit_count"][above] >= 1).all()
    assert (ref["wit_node"][above] < N).all()
    assert (ref["wit_count"] <= ref["n_feasible"][None, :]).all()


def _brute(nodes, pods, lo, hi):
    """Filter by pyoracle.fits, maxima by the card loop of collect_max_values (collection.go:
    41-53), witnesses by running that loop again per node."""
    scvs, plist = oracle.to_py(nodes, pods)
    get = (lambda c: c.bandwidth, lambda c: c.clock, lambda c: c.core, lambda c: c.free_memory,
           lambda c: c.power, lambda c: c.total_memory)
    Pn = len(plist)
    nf, nz = np.zeros(Pn, np.uint32), np.zeros(Pn, np.uint32)
    mx = np.ones((6, Pn), np.uint64)
    wc = np.zeros((6, Pn), np.uint32)
    wn = np.full((6, Pn), cases.NONE, np.uint32)
    for p, pod in enumerate(plist):
        contrib = {}
        for i in range(lo, hi):
            ok, memory, clock = pyoracle.fits(pod, scvs[i])
            if not ok:
                continue
            nf[p] += 1
            nz[p] += scvs[i].total_memory_sum == 0
            qual = [c for c in scvs[i].card_list if c.free_memory >= memory and c.clock >= clock]
            if qual:
                contrib[i] = [max(g(c) for c in qual) for g in get]
        for f in range(6):
            best = max([1] + [v[f] for v in contrib.values()])
            hit = [i for i, v in contrib.items() if v[f] == best]
            mx[f, p], wc[f, p] = best, len(hit)
            if hit:
                wn[f, p] = min(hit)
    return {"n_feasible": nf, "n_zero_total": nz, "maxima": mx, "wit_count": wc, "wit_node": wn}


@pytest.mark.parametrize("name", ["het", "tied_free", "no_qualifying"])
@pytest.mark.parametrize("lo,hi", [(0, 40), (13, 29)])
def test_reference_matches_brute_force(name, lo, hi):
    nodes, pods = BUILDERS[name](20, 40)
    ref, want = cases.reference(nodes, pods, lo, hi), _brute(nodes, pods, lo, hi)
    for k in want:
        np.testing.assert_array_equal(ref[k], want[k], err_msg=k)


def test_reference_merges_over_shards():
    nodes, pods = cases.mixed(P, N)
    b = shard_bounds(N, 3)
    parts = [cases.reference(nodes, pods, int(b[r]), int(b[r + 1])) for r in range(3)]
    parts.append(cases.reference(nodes, pods, N, N))  # an empty shard changes nothing
    whole, got = cases.reference(nodes, pods), cases.merged(parts)
    for k in whole:
        np.testing.assert_array_equal(got[k], whole[k], err_msg=k)


@pytest.mark.parametrize("Pn,Nn", [(130, 577), (300, 1500), (130, 4700)])
def test_tied_free_ties_the_free_maximum(Pn, Nn):
    nodes, pods = cases.tied_free(Pn, Nn)
    ref = cases.reference(nodes, pods)
    live = ref["maxima"][cases.FREE] > 1
    assert live.sum() >= 50
    cnt = ref["wit_count"][cases.FREE][live]
    for c in (1, 2, 4, 6, 8):
        assert (cnt == c).mean() >= 0.05, (c, float((cnt == c).mean()))
    assert np.unique(ref["wit_node"][cases.FREE][live]).size >= 5


def test_het_counts_are_small_and_many_pods_infeasible():
    nodes, pods = cases.het(P, N)
    assert nodes.max_cards == 16 and (nodes.card_count != nodes.card_number).any()
    assert (nodes.card_count == 0).any()
    ref = cases.reference(nodes, pods)
    assert (ref["n_feasible"] == 0).mean() >= 0.10
    small = ref["wit_count"][list(cases.SMALL)]
    live = ref["maxima"][list(cases.SMALL)] > 1
    assert (((small >= 2) & (small <= 8) & live).any(axis=0)).mean() >= 0.10


def test_no_qualifying_leaves_maxima_at_the_floor():
    nodes, pods = cases.no_qualifying(P, N)
    ref = cases.reference(nodes, pods)
    floor = (ref["n_feasible"] > 0) & (ref["maxima"] == 1).all(axis=0)
    assert floor.sum() >= 1
    assert (ref["n_zero_total"][floor] > 0).all()  # the zero-total count is exercised too
    assert (ref["wit_count"][:, floor] == 0).all()
    # and feasible nodes that contribute nothing next to ones that do
    cardless = nodes.card_count == 0
    some = (ref["n_feasible"] > cardless.sum()) & (pods.has_memory == 0) & (pods.has_clock == 0)
    assert some.sum() >= 3


def test_wide_chunks_lowest_witness_precedes_a_tied_block():
    nodes, pods = cases.wide_chunks(32768, 8192)
    assert pods.n_pods == 32768 and nodes.n_nodes == 8192
    ref = cases.reference(nodes, pods)
    free = cases.FREE
    hit = (ref["wit_node"][free] == 1) & (ref["wit_count"][free] >= 65)
    assert hit.mean() >= 0.25
    # node 0 is no witness for them, and whole sorted waves of 64 pods share the outcome
    assert (ref["wit_node"][free] != 0).all()


@pytest.mark.parametrize("name", ["tied_free", "mixed"])
def test_decrement_moves_counts_and_witnesses(name):
    nodes, pods = BUILDERS[name](P, N)
    ids, alloc, cn, after = cases.decrement(nodes, seed=3)
    assert 90 <= ids.size <= 100 and np.isin(cases.tied_ids(N), ids).all()
    assert (cn < nodes.card_number[ids]).all() and (cn == 0).any()
    np.testing.assert_array_equal(alloc, nodes.alloc_memory[ids])
    a, b = cases.reference(nodes, pods), cases.reference(after, pods)
    assert (a["n_feasible"] != b["n_feasible"]).mean() >= 0.25
    moved = ((a["wit_count"][cases.FREE] != b["wit_count"][cases.FREE]) |
             (a["wit_node"][cases.FREE] != b["wit_node"][cases.FREE]))
    assert moved.mean() >= 0.10


def test_shards_leave_witnesses_to_clear_and_to_merge():
    nodes, pods = cases.tied_free(P, N)
    b = shard_bounds(N, 3)
    assert all(int(x) % 64 for x in b[1:-1])  # the shards do not start on block boundaries
    parts = [cases.reference(nodes, pods, int(b[r]), int(b[r + 1])) for r in range(3)]
    whole = cases.reference(nodes, pods)
    live = whole["maxima"][cases.FREE] > 1
    reach = np.stack([r["maxima"][cases.FREE] == whole["maxima"][cases.FREE] for r in parts])
    assert ((~reach).any(axis=0))[live].mean() >= 0.50   # k_wit_prepare has something to clear
    assert (reach.sum(axis=0) >= 2)[live].mean() >= 0.10  # SUM and MIN merge real values
