"""The node-state scenarios of tests/node_state_cases.py can fail: with the oracle alone, every
push moves the picks (or the feasible counts) of a large share of the pods, so a handle that
ignored a push, or pruned with tables of the state before it, cannot pass the GPU tests
(tests/test_gpu_node_state.py).  These are conditions on the inputs, not on libyoda."""
import numpy as np
import pytest

import node_state_cases as cases
import oracle
from yoda_amd.soa import MODE_SCV


def _results(scenario):
    nodes, pods, steps = scenario
    return [(tag, oracle.schedule(nd, pods, MODE_SCV, threads=8))
            for tag, nd in cases.states(nodes, steps)]


def _pick_change(a, b):
    """Share of the pods feasible in either state whose pick differs."""
    feas = (a.status == 0) | (b.status == 0)
    assert feas.sum() > 500
    return float((a.pick != b.pick)[feas].mean())


def test_model_applies_steps():
    nodes, _, _ = cases.wake(pods=10, nodes=50, woken=20)
    m = cases.Model(nodes)
    ids = np.array([3, 60, 3, 7, 0xFFFFFFFF], np.uint32)
    m.apply(("push", ids, np.array([11, 12, 13, 14, 15], np.uint64),
             np.array([1, 2, 3, 4, 5], np.uint64)))
    got = m.nodes()
    assert got.alloc_memory[3] == 13 and got.card_number[3] == 3   # the last entry of id 3
    assert got.alloc_memory[7] == 14 and got.card_number[7] == 4
    keep = np.setdiff1d(np.arange(50), [3, 7])                     # ids >= n_nodes: ignored
    np.testing.assert_array_equal(got.alloc_memory[keep], nodes.alloc_memory[keep])
    np.testing.assert_array_equal(got.card_number[keep], nodes.card_number[keep])
    m.apply(("update_alloc", np.arange(50, dtype=np.uint64)))
    np.testing.assert_array_equal(m.nodes().alloc_memory, np.arange(50, dtype=np.uint64))
    assert m.nodes().card_number[3] == 3
    np.testing.assert_array_equal(nodes.alloc_memory[3], nodes.total_memory_sum[3])  # untouched


def test_wake_moves_picks_and_raises_scores():
    (_, before), (_, after) = _results(cases.wake())
    assert _pick_change(before, after) >= 0.40
    feas = (before.status == 0) & (after.status == 0)
    assert feas.sum() > 500
    assert (after.top_score > before.top_score)[feas].mean() >= 0.40
    assert (after.top_score >= before.top_score)[feas].all()


def test_sleep_wake_moves_picks_at_every_step():
    res = _results(cases.sleep_wake())
    assert len(res) == 4
    for (ta, a), (tb, b) in zip(res, res[1:]):
        assert _pick_change(a, b) >= 0.25, (ta, tb)


def test_cards_move_feasible_counts():
    (_, one), (_, rise), (_, fall) = _results(cases.cards())
    assert (one.n_feasible != rise.n_feasible).mean() >= 0.30
    assert (rise.n_feasible != fall.n_feasible).mean() >= 0.50
    assert (rise.n_feasible >= one.n_feasible).all() and (fall.n_feasible <= rise.n_feasible).all()


def test_card_blocks_move_feasible_counts():
    nodes, pods, steps = cases.card_blocks()
    assert (nodes.card_number.reshape(-1, 64).max(axis=1) == 1).sum() == nodes.n_nodes // 192
    (_, one), (_, rise) = _results((nodes, pods, steps))
    assert (one.n_feasible != rise.n_feasible).mean() >= 0.30
    assert _pick_change(one, rise) >= 0.05   # (greedy is compared by its picks alone)


@pytest.mark.parametrize("shape", ["base", "ranks", "per_pair", "small"])
def test_walk_moves_picks(shape):
    kw = {"base": {}, "ranks": {"in_bytes": True}, "per_pair": {"pods": 600, "nodes": 1500},
          "small": {"pods": 700, "nodes": 900}}[shape]
    nodes, pods, steps = cases.walk(**kw)
    pushes = [s for s in steps if s[0] != "check"]
    assert len(pushes) == 10 and pushes[cases.WALK_EMPTY][1].size == 0
    assert sum(s[0] == "update_alloc" for s in pushes) == 1
    assert (pushes[cases.WALK_OUTSIDE][1] >= nodes.n_nodes).sum() == 4
    sizes = {int((s[1] < nodes.n_nodes).sum()) for s in pushes if s[0] == "push"}
    assert sizes == {0, 1, 7, 64, 700}
    res = [oracle.schedule(nd, pods, MODE_SCV, threads=8) for _, nd in cases.states(nodes, steps)]
    prev = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    for k, r in enumerate(res):
        if k == cases.WALK_EMPTY:
            np.testing.assert_array_equal(r.pick, prev.pick)
        else:
            feas = (r.status == 0) | (prev.status == 0)
            assert feas.sum() > 100
            assert (r.pick != prev.pick)[feas].mean() >= 0.05, f"walk {k}"
        prev = r


def test_mixed_fleet_moves_picks():
    nodes, pods, steps = cases.mixed_fleet(pods=3000)
    prev = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    for tag, nd in cases.states(nodes, steps):
        r = oracle.schedule(nd, pods, MODE_SCV, threads=8)
        moved = ((r.pick != prev.pick) | (r.n_feasible != prev.n_feasible) |
                 (r.top_score != prev.top_score))
        assert moved.mean() >= 0.25, tag
        prev = r
