"""The stream scenarios of tests/stream_cases.py can fail: with the oracle alone, the answer a
wrong ordering on a busy stream would give -- the previous batch's pods, the state before an
update, a burst with one call lost or out of order, the other snapshot's value table -- differs
from the right one, so tests/test_gpu_streams.py cannot pass on it.  These are conditions on the
inputs, not on libyoda."""
import numpy as np
import pytest

import stream_cases as cases


def _differ(a, b):
    """Pods whose pick or feasible count differs."""
    return int(((a.pick != b.pick) | (a.n_feasible != b.n_feasible)).sum())


@pytest.mark.parametrize("name", cases.SIZE_SEQUENCES)
def test_back_to_back_batches_disagree(name):
    """Scenario 3: position by position, batch A's results are not batch B's -- in n_feasible or a
    maximum for at least half of the compared positions, in the pick for at least a quarter."""
    nodes, a, b = cases.batch_pair(name)
    state, pick = cases.disagreement(cases.schedule(nodes, a), cases.schedule(nodes, b))
    print(f"{name}: counts or maxima differ at {state:.3f} of the positions, picks at {pick:.3f}")
    assert state >= 0.5
    assert pick >= 0.25


def test_burst_needs_every_call_in_order():
    """Scenario 4: the burst's answer is the last writer's -- dropping any one of the five calls,
    or moving one across a call that writes the same node, changes some pod's pick or count; and
    the one call that commutes with the others (set_node_present) does."""
    nodes, pods, steps = cases.burst()
    assert [s[0] for s in steps] == ["push", "push", "cards", "present", "replace"]
    want = cases.schedule(cases.after(nodes, steps).compact(), pods)
    assert _differ(want, cases.schedule(nodes, pods)) >= pods.n_pods // 4
    for name, other in cases.burst_variants().items():
        got = cases.schedule(cases.after(nodes, other).compact(), pods)
        n = _differ(got, want)
        print(f"{name}: {n} pods differ")
        assert n >= 1, name
    # overlapping lists, different values: the two pushes share 20 nodes, the replaced node is in
    # both and in the card update, and is not one of the absent ones
    a, b, c, d, x = (set(s[1].tolist()) for s in steps)
    assert len(a & b) == 20 and x <= (a & b & c) and not (x & d)
    moved = list(steps)
    moved.insert(0, moved.pop(3))  # set_node_present first: the same state
    m0, m1 = cases.after(nodes, steps), cases.after(nodes, tuple(moved))
    assert (m0.present == m1.present).all() and not m0.present.all()
    assert _differ(cases.schedule(m1.compact(), pods), want) == 0


def test_burst_model_takes_the_last_entry():
    nodes, _, _ = cases.burst()
    m = cases.Model(nodes)
    ids = np.array([3, 900, 3, 0xFFFFFFFF], np.uint32)
    m.apply(("push", ids, np.array([11, 12, 13, 14], np.uint64), np.array([1, 2, 3, 4], np.uint64)))
    got = m.nodes()
    assert got.alloc_memory[3] == 13 and got.card_number[3] == 3
    keep = np.setdiff1d(np.arange(nodes.n_nodes), [3])
    np.testing.assert_array_equal(got.alloc_memory[keep], nodes.alloc_memory[keep])
    k = nodes.max_cards
    m.apply(("cards", np.array([5], np.uint32), np.full((1, k), 7, np.uint64),
             np.ones((1, k), np.uint8), np.array([7 * k], np.uint64)))
    real = np.arange(k) < nodes.card_count[5]
    np.testing.assert_array_equal(m.nodes().card_free_memory[5], np.where(real, 7, 0))
    assert m.nodes().free_memory_sum[5] == 7 * k


def test_mode_b_batch_is_not_its_reverse():
    """Scenario 2: the batch run before each pass is the same pods reversed; position by position
    its Mode B answer is another one (the tie count nearly everywhere, the pick for a quarter)."""
    from yoda_amd.soa import MODE_DISKIO
    import oracle
    nodes, pods = cases.mode_b_batch()
    w = oracle.schedule(nodes, pods, MODE_DISKIO, threads=8)
    assert (w.n_ties != w.n_ties[::-1]).mean() >= 0.9
    assert (w.pick != w.pick[::-1]).mean() >= 0.25


@pytest.mark.parametrize("shape", list(cases.RANK_SHAPES))
def test_rank_snapshots_have_other_memory_maxima(shape):
    """Scenario 7: the two memory-ranks snapshots hold as many distinct memory values, every one
    another, and give every pod with a feasible node (in either) another FreeMemory or TotalMemory
    maximum -- a phase 1 of the first that read the second's value table shows in every such pod."""
    first, second, pods = cases.ranks_pair(shape)
    for f in ("card_free_memory", "card_total_memory"):
        u1, u2 = np.unique(getattr(first, f)), np.unique(getattr(second, f))
        assert u1.size == u2.size and u1.size > 2
        assert (u1 != u2)[u1 > 0].all()  # rank by rank (0 stays 0)
    r1, r2 = cases.schedule(first, pods), cases.schedule(second, pods)
    feas = (r1.n_feasible > 0) | (r2.n_feasible > 0)
    assert feas.sum() >= pods.n_pods // 2
    mem = [cases.MAX_FREE, cases.MAX_TOTAL]
    assert (r1.maxima[feas][:, mem] != r2.maxima[feas][:, mem]).any(axis=1).all()


def test_state_push_moves_the_counts():
    """Scenario 7, the node-state variant: the push changes n_feasible of nine in ten pods that
    had a feasible node, and the pick of more than half."""
    nodes, pods, push, moved = cases.state_pair()
    m = cases.after(nodes, (push,))
    np.testing.assert_array_equal(m.nodes().card_number, moved.card_number)
    np.testing.assert_array_equal(m.nodes().alloc_memory, moved.alloc_memory)
    r1, r2 = cases.schedule(nodes, pods), cases.schedule(moved, pods)
    feas = r1.n_feasible > 0
    assert feas.sum() >= pods.n_pods // 2
    assert (r1.n_feasible != r2.n_feasible)[feas].mean() >= 0.9
    assert (r1.pick != r2.pick)[feas].mean() >= 0.5
