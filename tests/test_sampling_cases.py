"""The node-sampling scenarios of tests/sampling_cases.py, with the oracle alone (no GPU): the known
answers of numFeasibleNodesToFind, and floors that show the scenarios separate the specification
from its near misses -- no sampling at all, a cut that ignores the start index, and a reading that
treats the unsampled nodes as absent (the maxima following)."""
import ctypes as C

import numpy as np
import pytest

import candidate_cases as cc
import oracle
import sampling_cases as cases
from card_update_cases import shape_workload
from yoda_amd.soa import MODE_SCV

N_PODS, M = 600, 100


@pytest.mark.parametrize("n,pct,want", cases.KNOWN)
def test_num_feasible_to_find_known_answers(n, pct, want):
    assert cases.num_feasible_to_find(n, pct) == want


@pytest.fixture(scope="module")
def base():
    nd, pd = shape_workload("base")
    pd = pd.slice(0, N_PODS)
    model = cc.Model(nd)
    snap = cc.Snapshot(model, pd)
    start = cases.random_starts(nd.n_nodes, N_PODS)
    ref = cases.reference(snap, model, M, start)
    return nd, pd, model, snap, start, ref


def test_sampling_moves_the_picks(base):
    """At least a quarter of the pods pick another node than the unsampled cycle does (measured:
    61 %), and than a cut that ignores the start index (61 %)."""
    nd, pd, model, snap, start, (ref, _, found, nxt, _) = base
    unsampled = int((ref.pick != snap.full.pick).sum())
    no_start = cases.reference(snap, model, M, start, ignore_start=True)[0]
    ignoring = int((ref.pick != no_start.pick).sum())
    print("differs from unsampled / from a start-ignoring cut:", unsampled, ignoring, "of", N_PODS)
    assert unsampled >= N_PODS // 4 and ignoring >= N_PODS // 4
    np.testing.assert_array_equal(ref.maxima, snap.full.maxima)
    np.testing.assert_array_equal(found, snap.full.n_feasible)
    np.testing.assert_array_equal(ref.n_feasible, np.minimum(found, M))
    assert (nxt[found <= M] == start[found <= M]).all() and (found > M).sum() >= N_PODS // 4


def test_unsampled_nodes_are_not_absent(base):
    """The maxima are over every SCV: on a snapshot cut down to a pod's sample they differ."""
    nd, pd, model, snap, start, (ref, _, found, _, sm) = base
    moved = 0
    for p in np.flatnonzero(found > M)[:12].tolist():
        keep = np.flatnonzero(sm.candidates(p))
        r = oracle.schedule(nd.take(keep), pd.slice(p, p + 1), MODE_SCV, threads=1)
        assert r.n_feasible[0] == ref.n_feasible[p] == M
        moved += bool((r.maxima[0] != ref.maxima[p]).any())
    assert moved >= 1


def test_walk_restated(base):
    """n_found, next_start and the sample against a plain loop over the rotated ids."""
    nd, pd, model, snap, start, (ref, _, found, nxt, sm) = base
    n = nd.n_nodes
    for p in range(0, N_PODS, 37):
        feas = np.zeros(n, bool)
        feas[snap.keep] = snap.pod(p)[0]
        got, nx = [], int(start[p])
        for k in range(n):
            i = (int(start[p]) + k) % n
            if feas[i]:
                if len(got) == M:
                    nx = i
                    break
                got.append(i)
        assert sorted(got) == np.flatnonzero(sm.candidates(p)).tolist()
        assert (found[p], nxt[p]) == (feas.sum(), nx)


@pytest.mark.parametrize("n_pods", [229, 37])
def test_directed_cuts_land_where_they_say(n_pods):
    nd, pods, words, cls, start, tags = cases.directed(n_pods)
    model = cc.Model(nd)
    model.apply(("cand", 3, words))
    model.apply(("classes", cls))
    snap = cc.Snapshot(model, pods)
    sm = cases.Sampled(snap, model, cases.DIRECTED_M, start)
    M, n = cases.DIRECTED_M, nd.n_nodes
    last = {}
    for i, tag in enumerate(tags):
        mask, found, nxt = sm.walk(i)
        rot = cases.rotate(np.flatnonzero(mask), int(start[i]))
        last[tag] = (int(rot[-1]), found, nxt, int(start[i]))
    assert last["last node of a block"][0] % 64 == 63
    assert last["first node of a block"][0] % 64 == 0
    assert last["last node of window 0"][0] < 4096 <= last["last node of window 0"][2]
    assert last["in the last block"][0] >= n - 64
    assert last["after a wrap"][0] < last["after a wrap"][3]
    e, found, nxt, s = last["head of the start's block"]
    assert found == M + 1 and e // 64 == s // 64 == nxt // 64 and e < nxt < s
    assert last["|F'| == M"][1] == M and last["|F'| == M"][2] == last["|F'| == M"][3]
    assert last["|F'| == M + 1"][1] == M + 1
    assert all(v[1] > M for t, v in last.items() if not t.startswith("|F'| == M"))
    assert (last["start 0"][3], last["start N-1"][3]) == (0, n - 1)


def test_plugin_cycle_mirror_walks_the_same_way(base):
    """plugin.find_nodes_that_pass_filters (the framework mirror's walk) against the reference."""
    from yoda_amd.plugin import Status, find_nodes_that_pass_filters
    nd, pd, model, snap, start, (ref, _, found, nxt, sm) = base

    class OnlyFilter:
        node_names = [f"n{i}" for i in range(nd.n_nodes)]

        def __init__(self, feas):
            self.feas = feas

        def filter(self, state, pod, name):
            return Status() if self.feas[int(name[1:])] else Status(1, "no")

    for p in (0, 5, 77):
        feas = np.zeros(nd.n_nodes, bool)
        feas[snap.keep] = snap.pod(p)[0]
        got, nx = find_nodes_that_pass_filters(OnlyFilter(feas), None, None, M, int(start[p]))
        assert sorted(int(n[1:]) for n in got) == np.flatnonzero(sm.candidates(p)).tolist()
        assert nx == nxt[p]
        every, nx = find_nodes_that_pass_filters(OnlyFilter(feas), None, None, 0, int(start[p]))
        assert len(every) == found[p] and nx == start[p]


def test_plugin_schedule_one_matches_the_reference():
    """The framework mirror's whole cycle with num_to_find / start, over the oracle's rows."""
    from test_host import OracleRows
    from yoda_amd import synth
    from yoda_amd.pack import pods_to_dicts
    from yoda_amd.plugin import YodaPlugin, schedule_one
    nodes, pods = synth.make_config(2, pods=40, nodes=300)
    names = [f"node-{i}" for i in range(nodes.n_nodes)]
    plugin = YodaPlugin(OracleRows(nodes), names, nodes, MODE_SCV)
    model = cc.Model(nodes)
    snap = cc.Snapshot(model, pods)
    start = cases.random_starts(nodes.n_nodes, pods.n_pods, seed=3)
    want = cases.reference(snap, model, 20, start)[0]
    assert (want.pick != snap.full.pick).sum() >= 10
    for p, pod in enumerate(pods_to_dicts(pods)):
        node, st = schedule_one(plugin, pod, num_to_find=20, start=int(start[p]))
        if want.status[p] == 0:
            assert st.is_success() and node == names[want.pick[p]], p
        else:
            assert node is None and not st.is_success(), p


def test_null_handle_and_arguments():
    """A NULL handle is YODA_ERR_INVALID_ARG from every call; yoda_num_feasible_to_find needs no
    handle.  The validation on a live handle is in tests/test_gpu_sampling.py."""
    from yoda_amd.capi import ERRORS, Yoda, lib
    L = lib()
    s = (C.c_uint32 * 4)()
    out = (C.c_uint32 * 3)()
    INVALID = {v: k for k, v in ERRORS.items()}["YODA_ERR_INVALID_ARG"]
    assert L.yoda_set_node_sampling(None, 5, 4, s) == INVALID
    assert L.yoda_set_node_sampling(None, 0, 0, None) == INVALID
    assert L.yoda_download_sampling(None, s, s) == INVALID
    assert L.yoda_sampling_info(None, out) == INVALID
    assert L.yoda_sampling_profile(None, None) == INVALID
    for n, pct, want in cases.KNOWN:
        assert Yoda.num_feasible_to_find(n, pct) == want
