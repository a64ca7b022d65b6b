"""CPU only: every scenario of tests/mode_b_follow_cases.py fails a handle that ignores E (the
oracle on the whole uploaded snapshot), by construction -- and the stand-alone program that walks
the shared accumulator, settle and merges (yoda_modeb.h) against a brute-force loop over E.

tools/check_modeb_elig.cpp is built here with AddressSanitizer and UBSan as an ordinary executable
with its own main: a walk past a chunk's records or words, or a shift out of range, fails the
run."""
import os
import subprocess

import numpy as np
import pytest

import mode_b_follow_cases as cases
import oracle
from yoda_amd.soa import MODE_DISKIO, STATUS_OK, STATUS_UNSCHEDULABLE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_accumulator_settle_and_merges_match_brute_force(tmp_path):
    exe = str(tmp_path / "check_modeb_elig")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_modeb_elig.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_modeb_elig ok" in out.stdout, out.stdout


@pytest.mark.parametrize("distinct", [False, True])
def test_recipe_fails_a_handle_that_ignores_E(distinct):
    nodes, pods, steps = cases.scenario(distinct)
    (_, model), = cases.states(nodes, steps)
    P = pods.n_pods
    cls = cases.classes_of(model, P)
    blind = cases.unrestricted(model, pods)
    want = cases.reference(model, pods)
    # every spec's unrestricted pick is absent or a non-candidate of its class
    for p in range(P):
        assert blind.pick[p] >= 0 and not cases.eligible(model, p)[blind.pick[p]], p
    assert (want.pick != blind.pick).all()
    assert (want.n_feasible < blind.n_feasible).all()
    # the ANY pods see the present nodes
    anyp = np.flatnonzero(cls == cases.ANY)
    assert anyp.size and (want.n_feasible[anyp] == int(model.present.sum())).all()
    # class 0 hides every node at pod 0's best level: its top_score drops
    among_present = oracle.schedule(model.compact(), pods, MODE_DISKIO, threads=8)
    assert cls[0] == 0 and want.status[0] == STATUS_OK
    assert want.top_score[0] < among_present.top_score[0]
    # classes 1..5: the node each pod would pick among the present ones is hidden from it
    mid = np.flatnonzero((cls >= 1) & (cls <= 5))
    assert mid.size > 300
    assert (want.pick[mid] != cases.npc.remap(among_present.pick, model.keep())[mid]).all()
    # class 6 keeps exactly one node (returned with its raw score), class 7 none
    one, none = np.flatnonzero(cls == 6), np.flatnonzero(cls == 7)
    assert one.size and none.size
    assert (want.n_feasible[one] == 1).all() and (want.n_ties[one] == 1).all()
    assert (want.status[one] == STATUS_OK).all() and np.unique(want.pick[one]).size == 1
    d = cases.detail(model, pods, int(one[0]))
    assert want.top_score[one[0]] == d["raw"][want.pick[one[0]]]
    assert (want.status[none] == STATUS_UNSCHEDULABLE).all() and (want.pick[none] == -1).all()
    assert (want.n_feasible[none] == 0).all() and (want.top_score[none] == 0).all()
    # lane = node for one spec (8 classes and ANY), lane = class for distinct requests
    keys = {(pods.rio[p], pods.rcpu[p], cls[p]) for p in range(P)}
    assert len(keys) == (P if distinct else 9)


@pytest.mark.parametrize("distinct", [False, True])
def test_walk_states_differ_from_the_unrestricted_run(distinct):
    """Each state of the walk but the last (candidates off, every node back) changes picks."""
    nodes, pods, steps = cases.walk(distinct)
    states = cases.states(nodes, steps)
    assert [t for t, _ in states][:9] == list(cases.cc.WALK)
    blind = oracle.schedule(nodes, pods, MODE_DISKIO, threads=8)
    for tag, model in states[:-1]:
        want = cases.reference(model, pods)
        assert (want.pick != blind.pick).any() or (want.n_ties != blind.n_ties).any(), tag
        assert (want.n_feasible < nodes.n_nodes).all(), tag
    cases.assert_same(cases.reference(states[-1][1], pods), blind, "everyone back")


def test_rows_and_tie_sets_agree_with_the_reference():
    nodes, pods, steps = cases.scenario(True)
    (_, model), = cases.states(nodes, steps)
    want = cases.reference(model, pods)
    for p in range(12):
        d = cases.detail(model, pods, p)
        assert int(d["feas"].sum()) == want.n_feasible[p]
        assert (d["raw"][~d["feas"]] == -1).all() and (d["norm"][~d["feas"]] == -1).all()
        if want.status[p] == STATUS_OK:
            assert d["ties"].size == want.n_ties[p] and d["ties"][0] == want.pick[p]
            assert d["raw"][want.pick[p]] == want.top_score[p]
