"""tests/greedy_candidate_cases.py checked without a GPU: its reference against the oracle, how far
the recipe moves the picks, and the capacity session's F / F' accounting (yoda_gs_set_candidates)
on hand-built windows -- through the library's host entry points and, under AddressSanitizer and
UBSan, through the stand-alone tools/check_gs_candidates.cpp."""
import os
import subprocess

import numpy as np
import pytest

import greedy_candidate_cases as gc
import oracle
from yoda_amd.capi import GreedySession, YodaError
from yoda_amd.soa import MODE_SCV

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(pods=1200, nodes=600)


@pytest.fixture(scope="module")
def case():
    nd, pd, words, cls = gc.workload(**SHAPE)
    blind = {f: oracle.greedy(nd, pd, MODE_SCV, f)[0] for f in (0, 1)}
    ref = {f: gc.want(flags=f, **SHAPE) for f in (0, 1)}
    return nd, pd, words, cls, blind, ref


@pytest.mark.parametrize("flags", [0, 1])
def test_any_reference_is_the_oracle(case, flags):
    """(a) Every pod ANY (and no class array at all): the restated loop is oracle.greedy."""
    nd, pd, words, _, blind, _ = case
    any_cls = np.full(pd.n_pods, gc.ANY, np.uint8)
    np.testing.assert_array_equal(gc.reference(nd, pd, words, any_cls, flags), blind[flags])
    np.testing.assert_array_equal(gc.reference(nd, pd, words, None, flags), blind[flags])


@pytest.mark.parametrize("flags", [0, 1])
def test_recipe_moves_the_picks(case, flags):
    """(b) A handle that ignores the words fails at least a quarter of the pods; one that narrows
    the maxima with the candidates (the absent-node reading) fails some; single-candidate pods
    and pods without a candidate both occur."""
    nd, pd, words, cls, blind, ref = case
    differ = int((ref[flags] != blind[flags]).sum())
    assert differ >= pd.n_pods // 4, differ
    absent = gc.as_absent(nd, pd, words, cls, flags)
    assert (ref[flags] != absent).any()
    one, none = gc.single_and_none(nd, pd, words, cls, flags)
    assert one >= 1 and none >= 1, (one, none)


def test_absent_nodes_leave_the_reference(case):
    """With `present`, no absent node is picked and the picks are ids of the full snapshot."""
    nd, pd, words, cls, _, _ = case
    present = np.ones(nd.n_nodes, bool)
    present[np.random.default_rng(2).choice(nd.n_nodes, 120, replace=False)] = False
    sub = pd.slice(0, 200)
    got = gc.reference(nd, sub, words, cls[:200], 1, present=present)
    assert present[got[got >= 0]].all()
    assert (got >= 0).any() and got.max() < nd.n_nodes


@pytest.mark.parametrize("variant", gc.KAT_VARIANTS)
def test_session_kat(variant):
    """(c) The hand-built capacity windows: a lost node that passed Yoda's Filter counts against
    the feasible set only if it is the pod's candidate."""
    nxt, pick = gc.kat_run(variant)
    want_next, want_pick = gc.KAT_WANT[variant]
    assert nxt == want_next
    assert pick[0] == gc.KAT_X and pick[1] == gc.KAT_A
    if want_pick is not None:
        assert pick[2] == want_pick


def test_session_kat_discriminates():
    """The same windows in a session that never heard of the words take the other branch: the
    KATs would catch a scan_lost that does not ask cand()."""
    assert gc.kat_run("base", with_candidates=False)[0] == 3
    assert gc.kat_run("zero", with_candidates=False)[0] == 2


def test_session_set_candidates_arguments():
    nd, pd = gc.kat_nodes("base"), gc.kat_pods()
    w = gc.kat_window("base")
    for flags in (0, gc.CAPACITY):
        g = GreedySession(nd, pd, flags)
        with pytest.raises(YodaError, match="RANGE"):
            g.set_candidates(w["words"], 1, np.array([0, 1, gc.ANY], np.uint8))
        g.set_candidates(w["words"], 3, w["cls"])
        g.set_candidates(w["words"], 3, None)
        g.set_candidates(None, 0)
        g.set_candidates(w["words"], 3, w["cls"])
        g.begin_window(0, 1, w["counts"], w["top_score"], w["top_node"])
        with pytest.raises(YodaError, match="STATE"):
            g.set_candidates(w["words"], 3, w["cls"])
        g.close()


def test_gs_candidates_host_check(tmp_path):
    """(d) tools/check_gs_candidates.cpp: the same KATs on yoda_greedy_session.cpp built with
    AddressSanitizer and UBSan as an ordinary executable."""
    exe = str(tmp_path / "check_gs_candidates")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(REPO, "tools", "check_gs_candidates.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_gs_candidates ok" in out.stdout, out.stdout
