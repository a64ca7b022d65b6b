"""The block K2's chunk-relative window walk (k2_block_n32: 64 listed blocks at a time from
window_bits, one bound evaluation per window) on chunk geometries the flagship shape does not
have, against the per-pair kernels for every pod and the C oracle on a pod sample.

The geometries follow the chunk plan (plan_chunks_for) at the K2's resident capacity of 1280
workgroups (5 waves per SIMD); the test reads each chunk count back from the slot count of the
K2 trace (YODA_K2_TRACE: slot = wave * chunks + chunk) and asserts it, so a change of the plan
that moves a geometry shows here and not as a silent loss of coverage:

  straddle  24,000 pods x 10,000 nodes: 32 chunks of 320 nodes = 5 blocks.  Small chunks whose
            one window starts at every shift 0, 5, 10, ...; chunk 12 covers blocks 60-64, across
            list words 0 and 1 (the window merges two words); the last chunk is cut short by
            n_nodes, and the row's 157 blocks are no multiple of 64 (the last window's second
            word would be the one after the row).
  windows   300,000 pods x 40,000 nodes: 8 chunks of 5056 nodes = 79 blocks.  Several windows
            per chunk (64 + 15 blocks) whose starts sit at non-zero shifts (0, 15, 30, ...), so
            a chunk's hot-first order is per window.
  single    660,000 pods x 1,000 nodes: ONE chunk of 16 blocks -- one partial window that ends
            in the last (only) word of a one-word row.  (The plan gives one K2 chunk only from
            2560 pod blocks on, 655,360 pods.)
  ones      2,000 pods x 1,000 nodes: 16 chunks of one block each -- one-bit windows at every
            shift 0..15 of a one-word row.

A fifth of the pods get large memory requests (as test_g_table_on_off), so that some waves'
maxima are not the snapshot's and they prune with the decoupled bounds too."""
import numpy as np
import pytest

import oracle
from yoda_amd import synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import MODE_SCV

from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

# name -> (pods, nodes, K2 chunks)
SHAPES = {"straddle": (24_000, 10_000, 32), "windows": (300_000, 40_000, 8),
          "single": (660_000, 1_000, 1), "ones": (2_000, 1_000, 16)}
FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score", "maxima")


@pytest.fixture(scope="module")
def dev():
    y = Yoda(0)
    yield y
    y.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_window_walk_matches_per_pair_and_oracle(dev, shape, monkeypatch):
    n_pods, n_nodes, chunks = SHAPES[shape]
    nodes, pods = synth.make_config(3, pods=n_pods, nodes=n_nodes)
    rng = np.random.default_rng(77)
    few = rng.random(pods.n_pods) < 0.2  # big requests: maxima below the snapshot's on many waves
    pods.has_memory[few] = 1
    pods.memory[few] = rng.integers(70000, 81921, size=int(few.sum())).astype(np.uint64)
    pods = pods.normalized()
    dev.upload_nodes(nodes)
    assert dev.path == "n32"
    got = dev.eval(pods, MODE_SCV)
    # the K2 chunk count of this geometry: the trace's slots are wave * chunks + chunk, the waves
    # those of the padded pod order (a few more than n_pods / 64; another multiple-of-8 chunk
    # count would put used / chunks outside that range)
    waves = (n_pods + 63) // 64
    slots = (waves + waves // 10 + 8) * chunks
    monkeypatch.setenv("YODA_K2_TRACE", str(slots))
    dev.class_stats(True)
    dev.run(MODE_SCV)
    dev.synchronize()
    dev.class_stats(False)
    monkeypatch.delenv("YODA_K2_TRACE")
    used = int(np.nonzero(dev.k2_trace(slots)[:, 1] > 0)[0].max()) + 1
    print(f"{shape}: trace slots used {used} = {used / chunks:.2f} waves x {chunks} chunks "
          f"({waves} unpadded waves)")
    assert used % chunks == 0 and waves <= used // chunks < slots // chunks, (used, chunks, waves)
    dev.upload_nodes(nodes, per_node_k1=True, per_node_k2=True)
    pair = dev.eval(pods, MODE_SCV)
    for f in FIELDS:  # every pod, every output
        np.testing.assert_array_equal(getattr(got, f), getattr(pair, f), err_msg=f)
    sample = np.sort(rng.choice(pods.n_pods, size=600, replace=False))
    want = oracle.schedule(nodes, pods.take(sample), MODE_SCV, threads=16)
    sub = type(got)(**{f: getattr(got, f)[sample] for f in got.__dataclass_fields__})
    assert_same(sub, want)
