"""CPU only: the walk plan of Mode B under node sampling against a brute-force walk (the
stand-alone program), and -- with the oracle alone -- that the scenarios of
tests/mode_b_sampling_cases.py separate the specification from its near misses.

tools/check_modeb_sampling.cpp is built here with AddressSanitizer and UBSan as an ordinary
executable with its own main: a read past a rank row, or a shift out of range in the in-word
select, fails the run."""
import os
import subprocess

import numpy as np
import pytest

import mode_b_follow_cases as mbf
import mode_b_sampling_cases as cases
import oracle
from yoda_amd.soa import MODE_DISKIO, STATUS_OK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
M = 500  # sampling_cases.num_feasible_to_find(5000, 0)


def test_plan_select_and_walk_predicate_match_brute_force(tmp_path):
    exe = str(tmp_path / "check_modeb_sampling")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_modeb_sampling.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_modeb_sampling ok" in out.stdout, out.stdout


@pytest.mark.parametrize("name", ["one-spec", "distinct"])
def test_ignoring_sampling_fails(name):
    """Random starts on the whole snapshot, M = 500 of 5,000: at least half the picks and every
    n_ties differ from the unsampled cycle (measured with the oracle: 634 and 700 of 700)."""
    nodes, pods, _, model = cases.state(name, "whole")
    assert cases.sc.num_feasible_to_find(nodes.n_nodes, 0) == M
    want, found, nxt = cases.reference(model, pods, M, cases.starts(name))
    blind = oracle.schedule(nodes, pods, MODE_DISKIO, threads=8)
    P = pods.n_pods
    assert (want.pick != blind.pick).sum() >= P // 2
    assert (want.n_ties != blind.n_ties).all()
    assert (want.n_feasible == M).all() and (found == nodes.n_nodes).all()
    np.testing.assert_array_equal(nxt, (cases.starts(name).astype(np.int64) + M) % nodes.n_nodes)


def test_ignoring_start_fails():
    nodes, pods, _, model = cases.state("distinct", "whole")
    st = cases.starts("distinct")
    want, _, nxt = cases.reference(model, pods, M, st)
    miss, _, nxt0 = cases.reference(model, pods, M, st, ignore_start=True)
    assert (want.pick != miss.pick).sum() >= pods.n_pods // 2
    assert (nxt != nxt0).sum() >= pods.n_pods - 5


def test_counting_m_over_node_ids_fails_under_the_recipe():
    """M counts nodes of E, not node ids: with absent nodes and classes the first M ids from the
    start hold fewer than M nodes of E."""
    nodes, pods, _, model = cases.state("distinct", "recipe")
    st = cases.starts("distinct")
    want, found, nxt = cases.reference(model, pods, M, st)
    miss, _, nxt_ids = cases.reference(model, pods, M, st, over_ids=True)
    big = np.flatnonzero(found > M)
    assert big.size > pods.n_pods // 2
    assert (want.n_feasible[big] == M).all() and (miss.n_feasible[big] < M).all()
    assert (nxt[big] != nxt_ids[big]).sum() > big.size // 2
    assert (want.n_ties[big] != miss.n_ties[big]).sum() > big.size // 2
    # the one-node class and the empty class, whatever the start
    cls = mbf.classes_of(model, pods.n_pods)
    one, none = np.flatnonzero(cls == 6), np.flatnonzero(cls == 7)
    assert one.size and none.size
    assert (want.n_feasible[one] == 1).all() and (want.n_ties[one] == 1).all()
    assert (found[one] == 1).all() and (nxt[one] == st[one]).all()
    assert (want.status[none] == 1).all() and (found[none] == 0).all()
    assert (nxt[none] == st[none]).all()


def test_directed_pods_separate_the_near_misses():
    nodes, pods, steps, start, tags = cases.directed()
    model = cases.directed_model()
    Md, n = cases.DIRECTED_M, nodes.n_nodes
    k = len(tags)
    want, found, nxt = cases.reference(model, pods, Md, start)
    assert (want.status[:k] == STATUS_OK).all()
    at = {t: i for i, t in enumerate(tags)}

    def last(p):
        return int(cases.sc.rotate(cases.walk_of(model, p, start[p], Md)[0], start[p])[-1])

    assert last(at["cut on the last node of a block"]) % 64 == 63
    assert last(at["cut on the first node of a block"]) % 64 == 0
    assert last(at["cut in the last partial block"]) >= n - 8
    assert start[at["start in the last partial block"]] >= n - 8
    assert not model.present[start[at["start on an absent node"]]]
    p = at["start on a non-candidate"]
    assert model.present[start[p]] and not mbf.eligible(model, p)[start[p]]
    # the lowest id, not the first in walk order: after a wrap the pick lies in the head segment
    p = at["after a wrap"]
    walk_first, _, _ = cases.reference(model, pods, Md, start, sample=[p], first_in_walk=True)
    assert want.pick[p] < nxt[p] < start[p]
    assert walk_first.pick[p] >= start[p] and walk_first.pick[p] != want.pick[p]
    # next_start is the (M+1)-th node of E, not the id after the M-th
    p = at["gap after the cut"]
    _, _, adj = cases.reference(model, pods, Md, start, sample=[p], adjacent_next=True)
    assert adj[p] != nxt[p] and not mbf.eligible(model, p)[adj[p]]
    # the cut in the head of the start's own block: the walk came round to it
    p = at["cut in the head of the start's block"]
    assert found[p] == Md + 1 and nxt[p] // 64 == start[p] // 64 and nxt[p] < start[p]
    assert last(p) // 64 == start[p] // 64 and last(p) < nxt[p]
    # |E| == M: nothing cut, the walk went full circle; |E| == M + 1: one node past the cut
    p, q = at["|E| == M"], at["|E| == M + 1"]
    assert found[p] == Md == want.n_feasible[p] and nxt[p] == start[p]
    assert found[q] == Md + 1 and want.n_feasible[q] == Md and nxt[q] != start[q]
    unsampled = mbf.reference(model, pods)
    for f in cases.FIELDS:
        assert getattr(want, f)[p] == getattr(unsampled, f)[p], f
    # the best level over S is below the best over E
    p = at["top_score drops"]
    assert want.top_score[p] < unsampled.top_score[p]
    # ignoring the start fails every directed pod with a node of its E below its start and a cut
    miss, _, nxt0 = cases.reference(model, pods, Md, start, ignore_start=True)
    moved = [i for i in range(k)
             if found[i] > Md and mbf.eligible(model, i)[:start[i]].any()]
    assert all(nxt0[i] != nxt[i] for i in moved) and len(moved) >= k - 3


def test_rows_and_tie_sets_agree_with_the_reference():
    nodes, pods, steps, start, tags = cases.directed()
    model = cases.directed_model()
    want, _, _ = cases.reference(model, pods, cases.DIRECTED_M, start)
    for p in range(len(tags)):
        d = cases.detail(model, pods, p, start[p], cases.DIRECTED_M)
        assert int(d["feas"].sum()) == want.n_feasible[p]
        assert (d["raw"][~d["feas"]] == -1).all() and (d["norm"][~d["feas"]] == -1).all()
        assert d["ties"].size == want.n_ties[p] and d["ties"][0] == want.pick[p]
        assert d["raw"][want.pick[p]] == want.top_score[p]
        assert d["norm"][d["feas"]].max() == 100


def test_m_at_least_e_is_the_unsampled_cycle():
    for name in ("small", "tiny"):
        nodes, pods, _, model = cases.state(name, "recipe")
        want, found, nxt = cases.reference(model, pods, nodes.n_nodes, cases.starts(name))
        cases.assert_same(want, mbf.reference(model, pods), name)
        np.testing.assert_array_equal(nxt, cases.starts(name))
