"""Fresh-upload shapes as plain data (no fixtures): what tests/golden/make_upload_digests.py
records and test_gpu_card_update.test_builder_equivalence_on_fresh_uploads replays.

uploads(name) returns the [(nodes, upload kwargs)] that go into ONE handle, in order; the
record is taken after the last.  Every shape is small: one upload and one yoda_snapshot_check."""
import json
import os

import numpy as np

import card_update_cases as cases
from yoda_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upload_digests.json")

BLOCK_EDGES = (1, 63, 64, 65, 4097)  # a lone block, a partial last block, a new tile row
NAMES = (tuple(cases.SHAPES) + ("six_clocks", "wide_clocks") +
         tuple(f"n{n}" for n in BLOCK_EDGES) + ("k1", "k2", "small_after_base"))


def six_clock_fleet():
    """test_gpu_robust.test_mixed_block_rules' fleet: blocks with six healthy-card clocks (no
    per-clock table), mixed models, nodes without cards."""
    rng = np.random.default_rng(7300)
    n = 4096
    nodes = synth.mixed_models(synth.make_nodes(n, 77), 0.7, seed=78)
    clocks6 = np.array([1200, 1300, 1410, 1500, 1600, 1755], dtype=np.uint64)
    real = np.arange(8)[None, :] < nodes.card_count[:, None]
    six = np.arange(n) < 1024
    nodes.card_clock[six] = np.where(real[six], clocks6[rng.integers(0, 6, size=(1024, 8))], 0)
    empty = rng.random(n) < 0.02
    for a in (nodes.card_free_memory, nodes.card_total_memory, nodes.card_clock,
              nodes.card_bandwidth, nodes.card_core, nodes.card_power, nodes.card_healthy):
        a[empty] = 0
    nodes.card_count[empty] = 0
    return nodes.normalized()


def wide_clock_fleet():
    big, _ = synth.make_config(2, pods=10, nodes=3000)
    big.card_clock[:] = np.where(big.card_clock > 0, big.card_clock * 100, 0)
    return big.normalized()


def _shape(shape):
    return cases.shape_workload(shape, mixed_pods=10)[0], cases.UPLOAD_KW.get(shape, {})


def uploads(name):
    if name == "six_clocks":
        return [(six_clock_fleet(), {})]
    if name == "wide_clocks":
        return [(wide_clock_fleet(), {})]
    if name[0] == "n" and name[1:].isdigit():
        return [(synth.make_config(3, pods=10, nodes=int(name[1:]))[0], {})]
    if name in ("k1", "k2"):  # the largest card count 1 / 2: K = 1 / K = 2
        return [(synth.make_nodes(900, 5, cards=int(name[1])), {})]
    if name == "small_after_base":  # grow-only buffers: a smaller snapshot over a larger one
        return [_shape("base"), _shape("small")]
    return [_shape(name)]


def entry(y, digest):
    """What the fixture holds of a handle, given its yoda_snapshot_check digests."""
    return {"digest": [f"{int(x):016x}" for x in digest], "path": y.path,
            "node_order_grouped": bool(y.node_order_grouped)}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
