"""The shard scenarios of tests/shard_candidate_cases.py, with the oracle and candidate_cases alone
(no GPU): every split of every scenario bites, so that no test of
tests/test_gpu_shard_candidates.py can pass vacuously -- a shard step that summed the wrong counts,
took the maxima over F', drew over one shard's ties or read a non-candidate as absent would differ
from the reference on the pods counted here.  Also the dist.ShardExchange digest of the candidate
arguments, with stub handles."""
import functools

import numpy as np
import pytest

import candidate_cases as cases
import oracle
import shard_candidate_cases as sc
from yoda_amd.soa import MODE_SCV


@functools.lru_cache(maxsize=None)
def recipe_state(shape):
    """The walk's first state of a shape with its references, shared by the splits."""
    s = sc.walk(shape)
    tag, m = sc.checks(s)[0]
    snap = cases.Snapshot(m, s.pods)
    ref, ties = cases.reference(snap, m)
    return s, m, ref, ties, snap.full, cases.as_absent(m, s.pods)


# (F' spans shards, picks vs no candidates, picks vs the absent-node reading, pods with one node
# beyond shard 0, tie sets spanning shards) of the walk's recipe state when written
COUNTS = {("small", 2): (492, 454, 5, 3, 4), ("small", 3): (496, 454, 5, 3, 4),
          ("base", 2): (1713, 1568, 6, 3, 3), ("base", 3): (1725, 1568, 6, 5, 3),
          ("f64", 2): (437, 405, 1, 1, 7), ("f64", 3): (437, 405, 1, 8, 7),
          ("u64", 2): (437, 405, 1, 1, 7), ("u64", 3): (437, 405, 1, 8, 7)}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape", sc.WALK_SHAPES)
def test_walk_recipe_bites_on_every_split(shape, world):
    """The walk's first state (the recipe) per shape and split: pods whose F' spans at least two
    shards, picks that differ from the no-candidate reading, picks that differ from the
    absent-node reading, pods with |F'| = 1 beyond shard 0, tied pods whose tie set spans shards.
    Every count above zero (shard_candidate_cases.WALK_SEED is chosen so), and equal to COUNTS:
    small 492 / 454 / 5 / 3 / 4 at world 2 and 496 / 454 / 5 / 3 / 4 at world 3; base 1713 / 1568 /
    6 / 3 / 3 and 1725 / 1568 / 6 / 5 / 3; f64 and u64 437 / 405 / 1 / 1 / 7 and 437 / 405 / 1 / 8 /
    7 -- so a change of a generator or a seed shows here before it weakens a GPU test."""
    s, m, ref, ties, plain, absent = recipe_state(shape)
    b = s.splits[world - 2]
    got = sc.counts(s, b, m, ref, ties, plain, absent)
    print(shape, b, got)
    assert all(g > 0 for g in got), got
    assert got == COUNTS[shape, world], (got, COUNTS[shape, world])


def test_rules_scenario():
    """Classes whose candidates lie in one shard while the maxima holders lie in the others, a
    class nowhere, a first shard of non-candidates, one-candidate pods beyond shard 0.  The five
    counts of the split (0, 77, 2500, N) when written: 449 pods whose F' spans shards, 1,378 picks
    that differ from no candidates, 116 from the absent-node reading, 38 pods with one node beyond
    shard 0, 16 tie sets spanning shards."""
    (s, holders, ones) = sc.rules()
    b = s.splits[0]
    tag, m = sc.checks(s)[0]
    assert (m.words[:b[1]] == 0).all()  # shard 0: every node a non-candidate of every class
    assert np.unique(sc.shard_of(b, holders)).size == 3  # holders in every shard
    snap = cases.Snapshot(m, s.pods)
    ref, ties = cases.reference(snap, m)
    # classes 0 and 1: F' inside one shard, and the shard's own maxima are NOT the snapshot's for
    # most of their pods -- they come from shards that hold none of the pod's candidates
    for c, k in ((0, 1), (1, 2)):
        pods = np.flatnonzero((m.cls == c) & (ref.n_feasible > 0))
        assert pods.size >= 100
        for p in pods[:50].tolist():
            f = np.flatnonzero(cases.detail(snap, m, p)["feas"])
            assert (sc.shard_of(b, f) == k).all()
        own = oracle.schedule(s.nodes.slice(b[k], b[k + 1]).take(
            np.flatnonzero(m.candidates(int(pods[0]))[b[k]:b[k + 1]])), s.pods.take(pods),
            MODE_SCV, threads=8)
        assert (own.maxima != snap.full.maxima[pods]).any(axis=1).mean() >= 0.25
    np.testing.assert_array_equal(ref.maxima, snap.full.maxima)
    # class 2: nowhere
    nowhere = m.cls == 2
    assert nowhere.sum() >= 400 and (ref.n_feasible[nowhere] == 0).all()
    assert (snap.full.n_feasible[nowhere] > 0).sum() >= 300
    # the one-candidate pods: OK, one feasible node, beyond shard 0
    assert ones.size == sc.RULE_ONE
    assert (ref.n_feasible[ones] == 1).all() and (ref.status[ones] == 0).all()
    assert (sc.shard_of(b, ref.pick[ones]) > 0).all()
    got = sc.counts(s, b, m, ref, ties, snap.full, cases.as_absent(m, s.pods))
    print("rules:", got)
    assert all(g > 0 for g in got) and got == (449, 1378, 116, 38, 16), got
    # the empty shard holds nothing and moves no id
    e = s.splits[1]
    assert e[1] == e[2] and (sc.shard_of(e, ref.pick[ones]) > 1).all()


def test_zero_split_scenario():
    s, z, p = sc.zero_split()
    (b,) = s.splits
    assert b[1] % 64 and b[2] % 64
    st = sc.checks(s)
    snap = cases.Snapshot(st[0][1], s.pods)
    feas = np.flatnonzero(oracle.pod_detail(s.nodes, s.pods, p, MODE_SCV)[1])
    others = feas[feas != z]
    assert sc.shard_of(b, [z])[0] == 1 and (sc.shard_of(b, others) != 1).all()
    assert {0, 2} <= set(sc.shard_of(b, others).tolist())  # the others on both sides of s
    d = [cases.detail(snap, m, p) for _, m in st]
    assert [x["status"] for x in d] == [2, 0, 0, 2]
    assert d[1]["n_feasible"] == others.size and (d[2]["n_feasible"], d[2]["pick"]) == (1, z)


# half of the dense scenario's figures when written, per world: tie sets spanning shards, draws
# that leave the lowest node's shard
FLOOR_DENSE = {2: (22, 17), 3: (112, 61)}  # of 45 / 35 and 224 / 122, 227 tied pods


def test_overflow_and_dense_scenarios():
    s = sc.overflow()
    (b,) = s.splits
    _, m = sc.checks(s)[1]
    snap = cases.Snapshot(m, s.pods)
    ref, ties = cases.reference(snap, m)
    span = sum(np.unique(sc.shard_of(b, np.flatnonzero(cases.detail(snap, m, p)["feas"]))).size == 2
               for p in range(s.pods.n_pods))
    print("overflow: pods whose F' spans both shards:", span, "of", s.pods.n_pods)
    assert span >= s.pods.n_pods // 2
    assert (ref.n_feasible < snap.full.n_feasible).all()
    s = sc.dense()
    _, m = sc.checks(s)[0]
    snap = cases.Snapshot(m, s.pods)
    ref, ties = cases.reference(snap, m)
    tied = np.flatnonzero((ref.status == 0) & (ref.n_ties >= 2))
    assert tied.size >= 150
    from tie_draw_cases import draw
    for b in s.splits:
        spans = sum(np.unique(sc.shard_of(b, ties[p])).size >= 2 for p in tied.tolist())
        # the drawn node in another shard than the lowest one: lowest-node code cannot pass
        moved = sum(sc.shard_of(b, [draw(sc.SEED, p, ties[p])])[0] != sc.shard_of(b, [ref.pick[p]])[0]
                    for p in tied.tolist())
        print("dense", b, "tied pods / tie sets spanning shards / draws leaving the lowest node's "
              "shard:", tied.size, spans, moved)
        assert spans >= FLOOR_DENSE[len(b) - 1][0] and moved >= FLOOR_DENSE[len(b) - 1][1]


def test_with_absent_scenario():
    s = sc.with_absent()
    for b in s.splits:
        tag, m = sc.checks(s)[0]
        gone = m.absent()
        assert np.unique(sc.shard_of(b, gone)).size == len(b) - 1  # absent nodes in every shard
        hidden = np.flatnonzero((m.words & np.uint64(0xFF)) != np.uint64(0xFF))
        assert np.unique(sc.shard_of(b, hidden)).size == len(b) - 1


class StubHandle:
    """What ShardExchange's constructor calls on a handle, recorded."""
    n_pods, n_nodes, node_offset, score_bound, memory_ranks = 4, 8, 0, 1 << 20, False

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name,) + a)


def test_shard_exchange_candidate_digest():
    """dist.ShardExchange raises when the ranks pass different candidates (n_classes, the class
    array or none at all) before it touches a handle; different words per shard are by design."""
    import torch
    from yoda_amd.dist import Reducer, ShardExchange, _cand_digest
    cls = np.array([0, 1, 0xFF, 2], np.uint8)
    w = [np.full(8, 7, np.uint64), np.zeros(8, np.uint64)]
    same = _cand_digest((3, [w[0]], cls))
    assert same == _cand_digest((3, [w[1]], cls.copy())) and same & 1 and same < 1 << 63
    assert _cand_digest(None) == 0
    others = [(4, w, cls), (3, w, cls[::-1].copy()), (3, w, cls[:3]), (3, w, None), None]
    assert len({_cand_digest(c) for c in others} | {same}) == len(others) + 1

    class TwoRanks(Reducer):
        """A local reducer that plays a second rank contributing `other` to the digest check."""

        def __init__(self, other):
            super().__init__(local=True)
            self.other, self.reduces = other, 0

        def __call__(self, ts, op):
            if ts[0].numel() == 4 and op == "max":  # the one digest reduce: tie_draw, candidates
                self.reduces += 1
                a, d = self.other
                ts = list(ts) + [torch.tensor([a, ~a, d, ~d], dtype=torch.int64)]
            super().__call__(ts, op)

    dev = torch.device("cpu")
    for other in others:
        hs = [StubHandle(), StubHandle()]
        with pytest.raises(ValueError, match="candidates"):
            ShardExchange(hs, TwoRanks([0, _cand_digest(other)]), dev, candidates=(3, w, cls))
        assert not any(c[0].startswith(("set_", "shard_candidates")) for h in hs for c in h.calls)
    hs = [StubHandle(), StubHandle()]
    red = TwoRanks([0, same])
    ShardExchange(hs, red, dev, candidates=(3, w, cls))
    assert red.reduces == 1
    with pytest.raises(ValueError, match="tie_draw"):  # the other half of the same reduce
        ShardExchange(hs, TwoRanks([5, same]), dev, candidates=(3, w, cls))
    for k, h in enumerate(hs):
        names = [c[0] for c in h.calls]
        assert names.index("set_candidates") < names.index("shard_candidates")
        (call,) = [c for c in h.calls if c[0] == "set_candidates"]
        assert call[1] is w[k] and call[2] == 3
        assert ("shard_candidates", True) in h.calls
    hs = [StubHandle()]
    ShardExchange(hs, Reducer(local=True), dev)  # no candidates: the handle's are left alone
    assert not any(c[0] in ("set_candidates", "set_pod_classes", "shard_candidates")
                   for c in hs[0].calls)


def test_null_handle():
    from yoda_amd.capi import ERRORS, lib
    invalid = {v: k for k, v in ERRORS.items()}["YODA_ERR_INVALID_ARG"]
    assert lib().yoda_shard_candidates(None, 1) == invalid
    assert lib().yoda_shard_candidates(None, 0) == invalid
