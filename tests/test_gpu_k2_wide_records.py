"""The block K2's node records on waves of several reciprocal sets (k2_block_n32, WIDE): a node
whose qualifying-card count takes up to four values over the wave keeps four basic scores per
set -- sets 0 and 1 in the record, sets 2 and 3 in the node's row of the prefix table -- and is
served by the record pass instead of the per-node loop that computes every lane's card terms.
WIDE is on for one release kernel only (argmax, K = 8, one-model snapshot, no memory ranks, f32
small fields) and for the traced kernel of the same K; synth config 3 is that shape.

Every case compares all six outputs of every pod with the per-pair kernels, and a pod sample
with the C oracle.  A case but the last passes only if the K2 trace (YODA_K2_TRACE) shows tasks of
non-uniform waves with the case's number of sets (the third and fourth set are the word groups
of the table row) that served such nodes: bits 8-15 of a slot's word 3 count the record nodes
with more than two values, bits 4-6 the sets, bit 0 uniform maxima.

  ordered    the default pod order: the waves at the boundaries of its groups mix clock labels
             (any number of sets)
  unordered  yoda_set_pod_order(0): every wave mixes the three clock labels and the pods without
             one (4 sets)
  three      unordered, two clock labels and the pods without one (3 sets)
  two        unordered, one clock label and the pods without one (2 sets)
  spread     unordered, scv/memory over the whole free-memory range: the counts of nearly every
             node take more than four values over a wave, so the per-node loop serves them as
             before, beside two-valued record nodes at most (no count asked of the trace)

All but the last draw scv/memory from a 12,000 MiB band, about one card of a node's eight, so the
counts of most nodes take two to four values over a wave.  6,000 nodes are 94 blocks, the last
one partial; 8,000 pods are 125 waves."""
import numpy as np
import pytest

import oracle
from yoda_amd import synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import MODE_SCV

from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")
N_PODS, N_NODES, SLOTS = 8_000, 6_000, 60_000
# name -> (pod order on, scv/memory range, clock labels in use, the sets the trace must show:
# None: any, 0: no count asked)
CASES = {"ordered": (True, (30_000, 42_001), 3, None),
         "unordered": (False, (30_000, 42_001), 3, 4), "three": (False, (30_000, 42_001), 2, 3),
         "two": (False, (30_000, 42_001), 1, 2), "spread": (False, (0, 81_921), 3, 0)}


@pytest.fixture(scope="module")
def dev():
    y = Yoda(0)
    yield y
    y.close()


@pytest.mark.parametrize("case", list(CASES))
def test_several_set_records_match_per_pair_and_oracle(dev, case, monkeypatch):
    ordered, (m_lo, m_hi), n_clocks, want_sets = CASES[case]
    nodes, pods = synth.make_config(3, pods=N_PODS, nodes=N_NODES)
    rng = np.random.default_rng(11)
    pods.has_memory[:] = 1
    pods.memory[:] = rng.integers(m_lo, m_hi, size=pods.n_pods).astype(np.uint64)
    if n_clocks < 3:
        pods.has_clock[:] = rng.random(pods.n_pods) < 0.66
        pods.clock[:] = np.where(pods.has_clock == 1,
                                 synth.CLOCKS[rng.integers(0, n_clocks, size=pods.n_pods)], 0)
    pods = pods.normalized()
    dev.set_pod_order(ordered)
    try:
        dev.upload_nodes(nodes)
        assert dev.path == "n32"
        got = dev.eval(pods, MODE_SCV)
        monkeypatch.setenv("YODA_K2_TRACE", str(SLOTS))
        dev.class_stats(True)
        dev.run(MODE_SCV)
        dev.synchronize()
        dev.class_stats(False)
        monkeypatch.delenv("YODA_K2_TRACE")
        tr = dev.k2_trace(SLOTS)
        tr = tr[tr[:, 1] > 0]
        w3 = tr[:, 3]
        multi = (w3 & np.uint64(1)) == 0
        nsets = ((w3 >> np.uint64(4)) & np.uint64(7)).astype(np.int64)
        nwide = ((w3 >> np.uint64(8)) & np.uint64(0xff)).astype(np.int64)
        by_sets = {s: int(nwide[multi & (nsets == s)].sum()) for s in (2, 3, 4)}
        print(f"{case}: {len(tr)} tasks, {int(multi.sum())} of non-uniform waves; record nodes "
              f"with more than two values by sets: {by_sets}")
        assert nwide[~multi].sum() == 0
        if want_sets != 0:
            assert (by_sets[want_sets] if want_sets else sum(by_sets.values())) > 0, (case, by_sets)
        dev.upload_nodes(nodes, per_node_k1=True, per_node_k2=True)
        pair = dev.eval(pods, MODE_SCV)
    finally:
        dev.set_pod_order(True)
    for f in FIELDS:  # every pod, every output
        np.testing.assert_array_equal(getattr(got, f), getattr(pair, f), err_msg=f)
    sample = np.sort(rng.choice(pods.n_pods, size=400, replace=False))
    want = oracle.schedule(nodes, pods.take(sample), MODE_SCV, threads=16)
    sub = type(got)(**{f: getattr(got, f)[sample] for f in got.__dataclass_fields__})
    assert_same(sub, want)
