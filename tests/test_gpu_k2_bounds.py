"""The block K2's un-gated window bounds and candidate mask, and the block kernels' level indices
from a ballot (k2_block_n32 / k1_block_n32), against the per-pair kernels for every pod and all
six outputs, plus the C oracle on a pod sample.

  sparse   2,000 pods x 1,000 nodes: 16 one-block chunks.  A fifth of the pods get large memory
           requests (maxima below the snapshot's: the decoupled bounds), another fifth an
           scv/clock that only five nodes have, so most of their windows list no block at all:
           the bounds are loaded for a window that does not use them, and the candidate mask is
           empty.
  wide     24,000 pods x 10,000 nodes (32 chunks of 5 blocks; windows that straddle list words).
           A quarter of the nodes are a model with bandwidth 1 and clock 55,738 (the largest
           small field the f32 quotients take), so a pod that asks for that clock has bandwidth
           maximum 1 and basic scores of 8 x 55,738 x 100: top scores beyond 2^20 (44.6 million),
           the largest block bounds the N32 path compares.  The snapshot stays on the N32 path
           (asserted), the oracle sample has such scores (asserted).  With pods of scv/memory 0
           and pods whose scv/memory is above every free.
  k1 / k1b 2,000 x 1,000 and 5,000 x 3,000 for the K1's wave record and level index: the last
           wave is partly live, the label mix varies within waves, some pods ask for more cards
           than the K = 8 slots, and the first 128 pods ask for more cards (9) than any node has.
           Each shape runs in the device's pod order and in the caller's order
           (set_pod_order(False)), where pods 0..127 are waves 0 and 1 by construction: two whole
           waves that no node satisfies.  Evaluated as a private batch run (yoda_run, the only
           entry point whose probe writes the K1 wave record and whose K1 reads it), again
           through score_rows (its phase 1 has no final maxima, so it passes no record and the
           same block K1 computes its set-up per chunk task, level ballot included), and by the
           per-pair kernels: all three agree.  Both shapes have at least 8 pod blocks, the
           threshold from which a run probes and orders its pod blocks at all.
"""
import numpy as np
import pytest

import oracle
from yoda_amd import synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import MODE_SCV

from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
WIDE_CLOCK = 55_738


@pytest.fixture(scope="module")
def dev():
    y = Yoda(0)
    yield y
    y.close()


def big_memory(pods, rng, frac=0.2):
    few = rng.random(pods.n_pods) < frac
    pods.has_memory[few] = 1
    pods.memory[few] = rng.integers(70000, 81921, size=int(few.sum())).astype(np.uint64)


def sparse_case():
    nodes, pods = synth.make_config(3, pods=2_000, nodes=1_000)
    rng = np.random.default_rng(101)
    big_memory(pods, rng)
    rare = rng.choice(nodes.n_nodes, size=5, replace=False)  # the only nodes with this clock
    nodes.card_clock[rare] = 1600
    ask = rng.random(pods.n_pods) < 0.2
    pods.has_clock[ask] = 1
    pods.clock[ask] = 1600
    return nodes, pods.normalized()


def wide_case():
    nodes, pods = synth.make_config(3, pods=24_000, nodes=10_000)
    rng = np.random.default_rng(202)
    wide = rng.random(nodes.n_nodes) < 0.25
    nodes.card_bandwidth[wide] = 1
    nodes.card_clock[wide] = WIDE_CLOCK
    ask = rng.random(pods.n_pods) < 0.25
    pods.has_clock[ask] = 1
    pods.clock[ask] = WIDE_CLOCK
    zero = rng.random(pods.n_pods) < 0.1   # scv/memory 0: every card qualifies
    pods.has_memory[zero] = 1
    pods.memory[zero] = 0
    over = rng.random(pods.n_pods) < 0.05  # above every free: feasible nowhere
    pods.has_memory[over] = 1
    pods.memory[over] = int(nodes.card_free_memory.max()) + 1
    return nodes, pods.normalized()


def k1_case(n_pods, n_nodes, seed):
    nodes, pods = synth.make_config(3, pods=n_pods, nodes=n_nodes)
    rng = np.random.default_rng(seed)
    big_memory(pods, rng, 0.1)
    many = rng.random(pods.n_pods) < 0.05  # more cards than the K = 8 slots (no node has them)
    pods.has_number[many] = 1
    pods.number[many] = 16
    # pods 0..127 ask for more cards than any node has, whatever their labels: in the caller's
    # order they are waves 0 and 1
    pods.has_number[:128] = 1
    pods.number[:128] = 9
    return nodes, pods.normalized()


def check_block_against_pairs(dev, nodes, pods, rng, rows=False):
    dev.upload_nodes(nodes)
    assert dev.path == "n32"
    got = dev.eval(pods, MODE_SCV)  # a private batch run: the block kernels
    row = None
    if rows:  # the row entry point: the same outputs from its own K1 / K2 launches
        dev.upload_pods(pods)
        dev.score_rows(MODE_SCV)
        row = dev.download()
    dev.upload_nodes(nodes, per_node_k1=True, per_node_k2=True)
    pair = dev.eval(pods, MODE_SCV)
    for f in FIELDS:  # every pod, every output
        np.testing.assert_array_equal(getattr(got, f), getattr(pair, f), err_msg=f)
        if row is not None:
            np.testing.assert_array_equal(getattr(row, f), getattr(got, f), err_msg="rows " + f)
    sample = np.sort(rng.choice(pods.n_pods, size=400, replace=False))
    want = oracle.schedule(nodes, pods.take(sample), MODE_SCV, threads=16)
    sub = type(got)(**{f: getattr(got, f)[sample] for f in got.__dataclass_fields__})
    assert_same(sub, want)
    return got, sample, want


def test_ungated_bounds_and_empty_candidate_mask(dev):
    nodes, pods = sparse_case()
    got, _, _ = check_block_against_pairs(dev, nodes, pods, np.random.default_rng(1))
    rare = (pods.has_clock == 1) & (pods.clock == 1600)
    assert rare.sum() > 200 and (got.n_feasible[rare] <= 5).all()
    assert (got.n_feasible[rare] > 0).any()


def test_scores_beyond_2_20(dev):
    nodes, pods = wide_case()
    got, sample, want = check_block_against_pairs(dev, nodes, pods, np.random.default_rng(2))
    assert (want.top_score[want.status == 0] >= 1 << 20).any()  # (the oracle's own scores)
    assert (got.top_score[got.status == 0] >= 1 << 20).sum() > 1000
    over = pods.memory > nodes.card_free_memory.max()
    assert over.sum() > 500 and (got.n_feasible[over] == 0).all()
    assert ((pods.has_memory == 1) & (pods.memory == 0)).sum() > 1000


@pytest.mark.parametrize("ordered", [True, False], ids=["sorted", "caller_order"])
@pytest.mark.parametrize("shape", [(2_000, 1_000, 303), (5_000, 3_000, 404)],
                         ids=["k1", "k1b"])
def test_k1_wave_bounds_private_run_and_rows(dev, shape, ordered):
    n_pods, n_nodes, seed = shape
    nodes, pods = k1_case(n_pods, n_nodes, seed)
    assert n_pods % 64 != 0  # the last wave is partly live
    assert (n_pods + 255) // 256 >= 8  # enough pod blocks for the probe (and its record) to run
    # waves 0 and 1 of the caller's order: every pod needs 9 cards, no node has more than 8
    assert (pods.number[:128] == 9).all() and int(nodes.card_number.max()) == 8
    dev.set_pod_order(ordered)
    try:
        got, _, _ = check_block_against_pairs(dev, nodes, pods, np.random.default_rng(3),
                                              rows=True)
    finally:
        dev.set_pod_order(True)
    assert (got.n_feasible[pods.number > 8] == 0).all()
