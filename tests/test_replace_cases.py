"""The replacement and metric scenarios of tests/replace_cases.py can fail: with the oracle alone,
every check of every scenario differs from the check before it -- in the pick or the feasible
count of at least one pod in a hundred, or in a PreScore maximum where the scenario is about
maxima -- so a handle that ignored a replacement, or decided with tables of the state before it,
cannot pass the GPU tests (tests/test_gpu_replace_nodes.py, tests/test_gpu_node_metrics.py).
These are conditions on the inputs, not on libyoda.  soa.node_delta is tested here too."""
import numpy as np
import pytest

import oracle
import replace_cases as cases
from yoda_amd import synth
from yoda_amd.soa import MODE_DISKIO, MODE_SCV, node_delta

STATUS_DIV_ZERO = 2  # include/yoda.h YODA_STATUS_DIV_ZERO


def _moved(a, b):
    """Share of the pods whose feasible count or pick differs."""
    return float(((a.n_feasible != b.n_feasible) | (a.pick != b.pick)).mean())


def _results(nodes, pods, steps):
    return [(tag, cases.reference(m, pods)) for tag, m in cases.states(nodes, steps)]


def _assert_bites(res, floor=0.01, maxima=False):
    for (ta, a), (tb, b) in zip(res, res[1:]):
        share = _moved(a, b)
        mx = float((a.maxima != b.maxima).any(axis=1).mean())
        print(ta, "->", tb, "moved", round(share, 4), "maxima", round(mx, 4))
        assert (mx > 0 if maxima else share >= floor), (ta, tb)


def test_model_applies_whole_records():
    nodes, _ = cases.shape_workload("c4")
    n = nodes.n_nodes
    i = int(np.flatnonzero(nodes.card_count == 2)[0])
    j = int(np.flatnonzero(nodes.card_count == 16)[0])
    m = cases.Model(nodes)
    ids = np.array([i, n + 3, i, 0xFFFFFFFF], np.uint32)
    m.apply(("replace", ids, nodes.take([0, 1, j, 2])))
    m.apply(("present", np.array([i], np.uint32), np.array([0], np.uint8)))
    got = m.nodes()
    for f in cases.FIELDS:  # the last entry, every field
        np.testing.assert_array_equal(getattr(got, f)[i], getattr(nodes, f)[j], err_msg=f)
    keep = np.setdiff1d(np.arange(n), [i])
    for f in cases.FIELDS:
        np.testing.assert_array_equal(getattr(got, f)[keep], getattr(nodes, f)[keep], err_msg=f)
    assert nodes.card_count[i] == 2  # the scenario's own arrays are untouched
    assert m.absent().tolist() == [i] and m.compact().n_nodes == n - 1
    m.apply(("metrics", np.array([i, i], np.uint32), np.array([1.0, 2.0]), np.array([3.0, 4.0])))
    assert m.nodes().cpu[i] == 2.0 and m.nodes().disk_io[i] == 4.0


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_walk_moves_picks(shape):
    nodes, pods, steps = cases.walk(shape, mixed_pods=3000)
    n = nodes.n_nodes
    lists = [s for s in steps if s[0] == "replace"]
    assert len(lists) == len(cases.WALK_SIZES) and lists[cases.WALK_EMPTY][1].size == 0
    out = lists[cases.WALK_OUTSIDE][1]
    assert (out >= n).sum() == 4 and 0xFFFFFFFF in out
    assert np.unique(out).size == out.size - 40
    sizes = [int(np.unique(s[1][s[1] < n]).size) for s in lists]
    assert sizes == list(cases.WALK_SIZES)
    if np.unique(nodes.card_count).size > 1:  # another card count wherever the shape has several
        for s in lists[:cases.WALK_OUTSIDE]:
            assert (s[2].card_count != nodes.card_count[s[1]]).all()
    prev = oracle.schedule(nodes, pods, MODE_SCV, threads=8)
    for k, (tag, m) in enumerate(cases.states(nodes, steps)):
        r = cases.reference(m, pods)
        if k == cases.WALK_EMPTY:
            np.testing.assert_array_equal(r.pick, prev.pick)
        else:
            print(shape, tag, "moved", round(_moved(r, prev), 4))
            assert _moved(r, prev) >= 0.01, tag
        prev = r


@pytest.mark.parametrize("n", [900, 4608])
def test_new_model_moves_each_maximum_both_ways(n):
    nodes, pods, steps = cases.new_model(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    res = _results(nodes, pods, steps)
    assert len(res) == 13
    _assert_bites(res, maxima=True)
    base = res[0][1]
    for f, (_, up), (_, back) in zip(cases.MAX_FIELDS, res[1::2], res[2::2]):
        changed = (up.maxima != base.maxima).any(axis=0)
        assert changed.any(), f  # (a new clock also moves the Filter, and other maxima with it)
        np.testing.assert_array_equal(back.maxima, base.maxima)
        np.testing.assert_array_equal(back.pick, base.pick)


@pytest.mark.parametrize("n", [900, 4608])
def test_block_clocks_move_picks(n):
    res = _results(*cases.block_clocks(nodes=n, pods=700 if n == 900 else cases.BASE_PODS))
    assert len(res) == 3
    _assert_bites(res)
    np.testing.assert_array_equal(res[2][1].pick, res[0][1].pick)


@pytest.mark.parametrize("n", [900, 4608])
def test_mixed_and_back_moves_picks(n):
    nodes, pods, steps = cases.mixed_and_back(nodes=n, pods=700 if n == 900 else cases.BASE_PODS)
    st = cases.states(nodes, steps)

    def one_model(nd):
        real = np.arange(nd.max_cards)[None, :] < nd.card_count[:, None]
        return np.array([all(np.unique(a[i][real[i]]).size <= 1 for a in
                             (nd.card_clock, nd.card_bandwidth, nd.card_core, nd.card_power))
                         for i in range(nd.n_nodes)])

    assert one_model(st[0][1].nodes()).all() and one_model(st[2][1].nodes()).all()
    assert (~one_model(st[1][1].nodes())).sum() == 10
    _assert_bites(_results(nodes, pods, steps))


def test_spare_slots_join_the_picks():
    nodes, pods, steps, slots, join = cases.spare_slots()
    assert (nodes.card_count[slots] == 0).all() and slots.size == cases.SPARE
    (_, out), (_, absent), (_, joined) = _results(nodes, pods, steps)
    # records given to absent slots change nothing; once back, they take picks
    np.testing.assert_array_equal(absent.pick, out.pick)
    np.testing.assert_array_equal(absent.n_feasible, out.n_feasible)
    assert not np.isin(absent.pick, slots).any()
    print("joined: moved", round(_moved(joined, absent), 4))
    assert _moved(joined, absent) >= 0.01
    assert np.isin(joined.pick, join).mean() >= 0.01
    assert not np.isin(joined.pick, np.setdiff1d(slots, join)).any()


def test_card_counts_and_zero_total():
    nodes, pods, steps = cases.card_counts()
    res = _results(nodes, pods, steps)
    assert len(res) == 5
    _assert_bites(res)
    np.testing.assert_array_equal(res[3][1].pick, res[0][1].pick)
    last = res[4][1]
    node = int(steps[-2][1][0])
    assert (last.status == STATUS_DIV_ZERO).mean() >= 0.01
    # the pod labelled with the lone clock: one feasible node, picked without a score
    assert last.n_feasible[-1] == 1 and last.status[-1] == 0 and last.pick[-1] == node
    assert res[3][1].n_feasible[-1] == 0


def test_range_lists_differ_only_in_their_last_record():
    for k, (name, shape, _) in enumerate(cases.RANGE_RULES):
        nodes, pods, kw, good, bad = cases.range_rule(k)
        assert good[1].size == 4 and bad[1].size == 5, name
        a, b = good[2].normalized(), bad[2].normalized()
        for f in cases.FIELDS:
            x, y = getattr(a, f), getattr(b, f)[:4]
            if f in cases.CARD_FIELDS:
                y = y[:, :x.shape[1]]
            np.testing.assert_array_equal(x, y, err_msg=f"{name}: {f}")
        # the accepted prefix itself moves the state
        res = _results(nodes, pods, [("check", "before"), good, ("check", "after")])
        assert _moved(res[0][1], res[1][1]) > 0, name


def test_metrics_walk_moves_mode_b_picks():
    nodes, pods, steps = cases.metrics_walk()
    pods = synth.distinct_diskio(pods)
    prev = None
    for tag, m in cases.states(nodes, steps):
        r = oracle.schedule(m.nodes(), pods, MODE_DISKIO, threads=8)
        if prev is not None:
            share = float((r.pick != prev.pick).mean())
            print(tag, "mode B picks moved", round(share, 4))
            assert share >= 0.01, tag
        prev = r


# ---- soa.node_delta ----
def test_node_delta_splits_the_changed_nodes():
    old, _ = synth.make_config(4, pods=1, nodes=300)
    new = cases.copy_nodes(old)
    real = np.flatnonzero(old.card_count >= 2)
    a, b, c, d, e = (int(x) for x in real[:5])
    new.card_free_memory[a, 0] += np.uint64(5)          # dynamic only
    new.free_memory_sum[a] += np.uint64(5)
    new.card_healthy[b, 1] ^= 1                          # dynamic, and metrics
    new.cpu[b] += 1.0
    new.card_clock[c, 0] += np.uint64(3)                 # static, and everything else
    new.card_free_memory[c, 0] += np.uint64(1)
    new.cpu[c] += 2.0
    new.card_count[d] -= 1                               # a card count
    new.disk_io[e] += 0.5                                # metrics only
    new.alloc_memory[a] += np.uint64(9)                  # not its business
    dl = node_delta(old, new)
    assert dl.cards[0].tolist() == sorted([a, b])
    assert dl.replace[0].tolist() == sorted([c, d])
    assert dl.metrics[0].tolist() == sorted([b, e])
    nn = new.normalized()
    for f in cases.FIELDS:
        np.testing.assert_array_equal(getattr(dl.replace[1], f), getattr(nn, f)[dl.replace[0]], f)
    np.testing.assert_array_equal(dl.cards[1], nn.card_free_memory[dl.cards[0]])
    np.testing.assert_array_equal(dl.cards[2], nn.card_healthy[dl.cards[0]])
    np.testing.assert_array_equal(dl.cards[3], nn.free_memory_sum[dl.cards[0]])
    np.testing.assert_array_equal(dl.metrics[1], nn.cpu[dl.metrics[0]])
    np.testing.assert_array_equal(dl.metrics[2], nn.disk_io[dl.metrics[0]])
    # applying the three lists to a model of `old` gives `new` (but for the allocation of a)
    m = cases.Model(old)
    m.apply(("replace",) + dl.replace)
    m.apply(("metrics",) + dl.metrics)
    got = m.nodes()
    for f in ("card_count", "card_clock", "total_memory_sum", "cpu", "disk_io", "card_number"):
        np.testing.assert_array_equal(getattr(got, f), getattr(nn, f), err_msg=f)


def test_node_delta_edges():
    old, _ = synth.make_config(3, pods=1, nodes=50)
    same = node_delta(old, cases.copy_nodes(old))
    assert same.cards[0].size == same.replace[0].size == same.metrics[0].size == 0
    assert same.replace[1].n_nodes == 0
    assert node_delta(old, old.slice(0, 49)) is None
    # another card stride: the unused slots are zeros, nothing changed
    wide = cases.copy_nodes(old)
    for f in cases.CARD_FIELDS:
        setattr(wide, f, np.pad(getattr(wide, f), ((0, 0), (0, 8))))
    d = node_delta(old, wide)
    assert d.cards[0].size == d.replace[0].size == d.metrics[0].size == 0
    wide.card_count[7] = 9
    wide.card_total_memory[7, 8] = 5
    assert node_delta(old, wide).replace[0].tolist() == [7]
    nan = cases.copy_nodes(old)
    nan.cpu[3] = np.nan
    assert node_delta(old, nan).metrics[0].tolist() == [3]
    assert node_delta(nan, cases.copy_nodes(nan)).metrics[0].size == 0
