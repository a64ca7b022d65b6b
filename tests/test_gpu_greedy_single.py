"""yoda_greedy on one handle, where its three Mode A paths (flags 0, card capacity, the U64
exact sequence) share one driver over the host session: an Allocate sum that really wraps past
2^64 inside the batch, and a handle whose node ids carry an offset."""
import numpy as np
import pytest

import oracle
from yoda_amd import synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import MODE_SCV

pytestmark = pytest.mark.gpu

OFFSET = 1000


@pytest.fixture
def dev():
    y = Yoda(0)
    yield y
    y.close()


@pytest.fixture(scope="module")
def wrap_case():
    """Every third node starts 1000 below 2^64 of allocated memory: the oracle's Allocate wraps
    4 times (flags 0, first at queue position 34) / 30 times (flags 1, first at position 20),
    and hundreds of pods are resolved after the first wrap."""
    nodes, pods = synth.make_config(5, pods=600, nodes=300)
    nodes.alloc_memory[::3] = np.uint64((1 << 64) - 1000)
    nodes, pods = nodes.normalized(), pods.normalized()
    want = {flags: oracle.greedy(nodes, pods, MODE_SCV, flags)[0] for flags in (0, 1)}
    # the wrap is real: some node's start value + the memory of the pods it took passes 2^64
    mem = np.where(pods.has_memory == 1, pods.memory, 0).astype(object)
    for flags in (0, 1):
        total = np.array(nodes.alloc_memory, object)
        for p in np.flatnonzero(want[flags] >= 0):
            total[want[flags][p]] += int(mem[p])
        assert (total >= (1 << 64)).any()
    sub = pods.slice(0, 64)
    return nodes, pods, want, sub, oracle.schedule(nodes, sub, MODE_SCV, threads=8)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("path", ["n32", "f64"])
def test_greedy_allocate_wraps(dev, wrap_case, path, flags):
    nodes, pods, want, sub, sub_want = wrap_case
    dev.upload_nodes(nodes, force_f64=path == "f64")
    assert dev.path == path
    np.testing.assert_array_equal(dev.greedy(pods, MODE_SCV, flags), want[flags])
    # the uploaded snapshot is unchanged afterwards
    np.testing.assert_array_equal(dev.eval(sub, MODE_SCV).pick, sub_want.pick)


@pytest.fixture(scope="module")
def offset_case():
    nodes, pods = synth.make_config(5, pods=2500, nodes=600)
    nodes, pods = nodes.normalized(), pods.normalized()
    want = {flags: oracle.greedy(nodes, pods, MODE_SCV, flags)[0] for flags in (0, 1)}
    # a later node-state change, by global id: more allocated memory, fewer cards
    rng = np.random.default_rng(5)
    ids = rng.choice(nodes.n_nodes, size=40, replace=False)
    moved = nodes.slice(0, nodes.n_nodes)
    moved.alloc_memory = np.array(nodes.alloc_memory, np.uint64)
    moved.card_number = np.array(nodes.card_number, np.uint64)
    moved.alloc_memory[ids] += np.uint64(4096)
    moved.card_number[ids] //= np.uint64(2)
    sub = pods.slice(0, 300)
    return nodes, pods, want, ids, moved, sub, oracle.schedule(moved, sub, MODE_SCV, threads=8)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("path", ["n32", "f64", "u64"])
def test_greedy_with_node_offset(dev, offset_case, path, flags):
    nodes, pods, want, ids, moved, sub, sub_want = offset_case
    dev.upload_nodes(nodes, node_offset=OFFSET, force_f64=path == "f64",
                     force_generic=path == "u64")
    got = dev.greedy(pods, MODE_SCV, flags)
    exp = want[flags]
    np.testing.assert_array_equal(got, np.where(exp >= 0, exp + OFFSET, exp))
    # the handle still answers to its global ids, on the snapshot the batch left as it was
    dev.set_node_state(ids + OFFSET, moved.alloc_memory[ids], moved.card_number[ids])
    res = dev.eval(sub, MODE_SCV)
    np.testing.assert_array_equal(res.status, sub_want.status)
    np.testing.assert_array_equal(res.pick, np.where(sub_want.pick >= 0, sub_want.pick + OFFSET,
                                                     sub_want.pick))
