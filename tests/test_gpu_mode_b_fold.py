"""The two instances of each Mode B kernel (ELIG = false, the unrestricted run; ELIG = true, a
run with yoda_mode_b_follow and something to follow) pinned to each other, not each to the oracle.
Handle A holds N nodes with the setting off.  Handle B holds the same N nodes and one more, which
is absent, with the setting on: its run takes the eligibility instances and must give A's answers
on every pod.  The appended node is a lure: it would score 10 for every pod (cpu = disk_io = 0:
|alpha*V - beta*U| = 0), so a batch or rows kernel that ignores eligibility picks it; for the draw,
which looks only at the nodes at the pod's best score, it is a copy of node 0 among identical
nodes, so a draw that ignores eligibility has it in every tie set.  Shapes: the smallest at which
a chunk edge, the 8-per-trip tail or the wave merge can go wrong, in both launch forms (3 specs:
lane = node; 65 distinct specs: lane = class, the first count above the lane = node limit of 64)."""
import numpy as np
import pytest

import oracle
from test_gpu_mode_b import boundary_nodes, pods_with
from tie_draw_cases import draw
from yoda_amd import synth
from yoda_amd.capi import Yoda
from yoda_amd.soa import MODE_DISKIO

pytestmark = pytest.mark.gpu

SEED = 0xF01DED
FIELDS = ("pick", "status", "n_feasible", "n_ties", "top_score")


def with_lure(both, perfect=True):
    """(the first N nodes, all N + 1): the last node made the lure -- perfect, or a copy of node 0."""
    n = both.n_nodes - 1
    both.cpu[n] = 0.0 if perfect else both.cpu[0]
    both.disk_io[n] = 0.0 if perfect else both.disk_io[0]
    both = both.normalized()
    return both.take(np.arange(n)), both


def same(a, b, tag):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{tag}: {f}")


def compare(nodes, both, pods, rows=True):
    """Every entry point of a single handle on A and on B.  Returns A's result without and with
    the draw, and the effective pod classes of A's and B's batch runs."""
    n_nodes = nodes.n_nodes
    tag = f"N {n_nodes} pods {pods.n_pods}"
    with Yoda(0) as a, Yoda(0) as b:
        a.upload_nodes(nodes)
        b.upload_nodes(both)
        b.mode_b_follow(True)
        b.set_node_present([n_nodes], 0)
        out = []
        for dev in (a, b):
            dev.upload_pods(pods)
            dev.run(MODE_DISKIO)
            out.append([dev.download(), dev.mode_b_info()])
            out[-1].append(dev.eval(pods, MODE_DISKIO))
            out[-1].append(dev.score_rows(MODE_DISKIO) if rows else None)
            dev.set_tie_draw(SEED)
            out[-1].append(dev.eval(pods, MODE_DISKIO))
        (ra, ia, va, rows_a, da), (rb, ib, vb, rows_b, db) = out
    assert (ia[2], ib[2]) == (0, 1), tag  # A: the unrestricted instances, B: the eligibility ones
    same(ra, rb, tag + " run")
    same(va, vb, tag + " eval")
    same(ra, va, tag + " run against eval")
    same(da, db, tag + " draw")
    for f in FIELDS[1:]:
        np.testing.assert_array_equal(getattr(da, f), getattr(ra, f), err_msg=f"{tag}: draw {f}")
    if rows:
        (feas_a, raw_a), (feas_b, raw_b) = rows_a, rows_b
        np.testing.assert_array_equal(raw_b[:, :n_nodes], raw_a, err_msg=tag + " rows")
        np.testing.assert_array_equal(feas_b[:, :n_nodes], feas_a, err_msg=tag + " bits")
        assert (raw_b[:, n_nodes] == -1).all() and not feas_b[:, n_nodes].any(), tag
        assert (raw_a >= 0).all() and feas_a.all(), tag
    return ra, da, (ia[1], ib[1])


def lure_scores_10(both, pods):
    lure = oracle.schedule(both.take(np.array([both.n_nodes - 1])), pods, MODE_DISKIO, threads=1)
    return bool((lure.top_score == 10).all())


@pytest.mark.parametrize("n_specs", [3, 65])
@pytest.mark.parametrize("n_nodes", [1, 63, 65, 2047, 2049])
def test_instances_agree(n_nodes, n_specs):
    rng = np.random.default_rng(1000 * n_specs + n_nodes)
    pods = pods_with(rng.random(n_specs) * 20.0, rng.integers(1, 2000, n_specs))
    nodes, both = with_lure(synth.make_config(2, pods=1, nodes=n_nodes + 1)[0])
    assert lure_scores_10(both, pods)  # ignoring eligibility shows on every pod
    ra, da, classes = compare(nodes, both, pods)
    assert classes == (n_specs, n_specs)  # 3: lane = node, 65: lane = class, on both handles
    assert (ra.status == 0).all() and (ra.n_feasible == n_nodes).all()
    assert (da.pick[ra.n_ties == 1] == ra.pick[ra.n_ties == 1]).all()


@pytest.mark.parametrize("k", [1, 5, 10])
def test_level_boundaries(k):
    """test_gpu_mode_b.boundary_nodes(k): nodes within 6 ulps of level k's threshold, in both
    launch forms (4 specs; 400 more for lane = class)."""
    for extra, more in ((0, 0), (3000, 400)):
        rng = np.random.default_rng(k)
        pods = pods_with(np.concatenate([[0.0, 10.0, 0.0, 10.0], rng.random(more) * 50.0]),
                         np.concatenate([[100, 100, 500, 100], rng.integers(1, 4000, more)]))
        nodes, both = with_lure(boundary_nodes(k, n_extra=extra + 1))
        assert lure_scores_10(both, pods)
        ra, _, classes = compare(nodes, both, pods, rows=not more)
        assert ra.top_score[0] == k  # alpha = 1, beta = 0: the best level is k
        assert (classes[0] > 64) == bool(more) and classes[0] == classes[1]


def test_every_node_scores_zero():
    """cpu = 1000 (V = 10) on the N nodes: every pod ends at level 0, which the unrestricted
    instances settle from the chunk's bounds and the eligibility ones from the nodes they saw.
    2,100 nodes: two lane = node chunks, the second ragged."""
    for rio, rcpu in (([0.0] * 4, [100] * 4), (np.zeros(200), np.arange(1, 201))):
        both, _ = synth.make_config(2, pods=1, nodes=2101)
        both.cpu = np.full(2101, 1000.0)
        nodes, both = with_lure(both)
        pods = pods_with(rio, rcpu)
        assert lure_scores_10(both, pods)
        ra, da, _ = compare(nodes, both, pods, rows=False)
        assert (ra.n_ties == 2100).all() and (ra.pick == 0).all()
        assert (da.pick != 0).any()  # the draw moves off the lowest node, alike on both


@pytest.mark.parametrize("n_specs,n_pods", [(3, 24), (65, 65)])
def test_draw_stays_within_E(n_specs, n_pods):
    """Five identical nodes and an absent sixth like them: every pod ties over the five, and a
    draw that ignored eligibility would hold the sixth in every tie set.  The picks must be the
    draw over the five; that the seed would send some pod to the sixth is checked first."""
    both, _ = synth.make_config(2, pods=1, nodes=6)
    both.cpu = np.full(6, 40.0)
    both.disk_io = np.full(6, 25.0)
    nodes, both = with_lure(both, perfect=False)
    rng = np.random.default_rng(n_specs)
    spec = np.arange(n_pods) % n_specs
    pods = pods_with((rng.random(n_specs) * 20.0)[spec], rng.integers(1, 2000, n_specs)[spec])
    within = np.array([draw(SEED, p, np.arange(5)) for p in range(n_pods)])
    blind = np.array([draw(SEED, p, np.arange(6)) for p in range(n_pods)])
    assert (blind == 5).any()
    ra, da, classes = compare(nodes, both, pods)
    assert classes == (n_specs, n_specs)
    assert (ra.n_ties == 5).all() and (ra.pick == 0).all()
    np.testing.assert_array_equal(da.pick, within)
