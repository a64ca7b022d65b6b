"""The card-update scenarios of tests/card_update_cases.py can fail: with the oracle alone, every
update moves the picks, the feasible counts or the maxima of a large share of the pods, so a
handle that ignored an update, or decided with tables of the state before it, cannot pass the
GPU tests (tests/test_gpu_card_update.py).  These are conditions on the inputs, not on libyoda."""
import numpy as np
import pytest

import card_update_cases as cases
import oracle
from yoda_amd.soa import MODE_SCV


def _schedule(nd, pods):
    return oracle.schedule(nd, pods, MODE_SCV, threads=8)


def _results(scenario):
    nodes, pods, steps = scenario
    return [(tag, _schedule(nd, pods)) for tag, nd in cases.states(nodes, steps)]


def _moved(a, b):
    """Share of the pods whose feasible count or pick differs."""
    return float(((a.n_feasible != b.n_feasible) | (a.pick != b.pick)).mean())


def test_model_applies_card_steps():
    nodes, _ = cases.shape_workload("c4")
    k = nodes.max_cards
    i = int(np.flatnonzero((nodes.card_count > 0) & (nodes.card_count < k))[0])
    cnt = int(nodes.card_count[i])
    m = cases.Model(nodes)
    ids = np.array([i, nodes.n_nodes + 3, i, 0xFFFFFFFF], np.uint32)
    free = np.arange(4 * k, dtype=np.uint64).reshape(4, k) + 1
    healthy = np.ones((4, k), np.uint8)
    m.apply(("cards", ids, free, healthy, np.array([10, 20, 30, 40], np.uint64)))
    got = m.nodes()
    np.testing.assert_array_equal(got.card_free_memory[i, :cnt], free[2, :cnt])  # the last entry
    assert (got.card_free_memory[i, cnt:] == 0).all() and (got.card_healthy[i, cnt:] == 0).all()
    assert got.free_memory_sum[i] == 30
    keep = np.setdiff1d(np.arange(nodes.n_nodes), [i])
    np.testing.assert_array_equal(got.card_free_memory[keep], nodes.card_free_memory[keep])
    np.testing.assert_array_equal(got.free_memory_sum[keep], nodes.free_memory_sum[keep])
    assert nodes.free_memory_sum[i] != 30  # the scenario's own arrays are untouched


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_walk_moves_picks(shape):
    nodes, pods, steps = cases.walk(shape, mixed_pods=3000)
    lists = [s for s in steps if s[0] != "check"]
    assert [s[0] for s in lists].count("push") == 1 and lists[cases.WALK_EMPTY][1].size == 0
    out = lists[cases.WALK_OUTSIDE][1]
    assert (out >= nodes.n_nodes).sum() == 4 and np.unique(out).size == out.size - 40
    sizes = {int(np.unique(s[1][s[1] < nodes.n_nodes]).size) for s in lists if s[0] == "cards"}
    assert sizes == {0, 1, 7, 64, 700}
    if shape == "ranks":  # every new free is a value the snapshot's cards hold
        pool = cases._free_pool(nodes)
        for s in lists:
            if s[0] == "cards":
                real = cases._real(nodes, np.minimum(s[1], nodes.n_nodes - 1).astype(np.int64))
                assert np.isin(s[2][real & (s[1] < nodes.n_nodes)[:, None]], pool).all()
    prev = _schedule(nodes, pods)
    for k, (tag, nd) in enumerate(cases.states(nodes, steps)):
        r = _schedule(nd, pods)
        if k == cases.WALK_EMPTY:
            np.testing.assert_array_equal(r.pick, prev.pick)
        else:
            feas = (r.status == 0) | (prev.status == 0)
            assert feas.sum() > 100
            share = float((r.pick != prev.pick)[feas].mean())
            print(shape, tag, "pick share", round(share, 3), "moved", round(_moved(r, prev), 3))
            assert share >= 0.10, tag
        prev = r


@pytest.mark.parametrize("n", [900, 4608])
def test_block_drain_changes_feasible_counts_and_picks(n):
    res = _results(cases.block_drain(nodes=n, pods=700 if n == 900 else cases.BASE_PODS))
    assert len(res) == 3
    for (ta, a), (tb, b) in zip(res, res[1:]):
        feas = (a.status == 0) | (b.status == 0)
        assert feas.sum() > 100
        nf, pk = float((a.n_feasible != b.n_feasible).mean()), float((a.pick != b.pick)[feas].mean())
        print(n, ta, "->", tb, "n_feasible", round(nf, 3), "pick", round(pk, 3))
        assert nf >= 0.40 and pk >= 0.90, (ta, tb)


@pytest.mark.parametrize("n", [900, 4608])
def test_free_maximum_moves_maxima_both_ways(n):
    res = _results(cases.free_maximum(nodes=n, pods=700 if n == 900 else cases.BASE_PODS))
    (_, base), (_, up), (_, back) = res
    rose = float((up.maxima != base.maxima).any(axis=1).mean())
    fell = float((back.maxima != up.maxima).any(axis=1).mean())
    print(n, "maxima changed: up", round(rose, 3), "back", round(fell, 3))
    assert rose >= 0.20 and fell >= 0.20
    np.testing.assert_array_equal(back.maxima, base.maxima)
    np.testing.assert_array_equal(back.pick, base.pick)


def test_health_only_moves_counts_or_picks():
    nodes, pods, steps = cases.health_only()
    assert np.array_equal(steps[1][2], nodes.card_free_memory[steps[1][1]])
    assert np.array_equal(steps[1][4], nodes.free_memory_sum[steps[1][1]])
    (_, a), (_, b) = _results((nodes, pods, steps))
    print("health only moved", round(_moved(a, b), 3))
    assert _moved(a, b) >= 0.10


def test_rejected_list_is_alien_only_in_its_last_entry():
    nodes, _, step = cases.rejected()
    pool = cases._free_pool(nodes)
    real = cases._real(nodes, step[1].astype(np.int64))
    assert np.isin(step[2][:-1][real[:-1]], pool).all()
    assert not np.isin(step[2][-1][real[-1]], pool).all()
