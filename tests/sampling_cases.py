"""Node-sampling scenarios as plain data (no fixtures), and the reference (yoda_set_node_sampling).

kube-scheduler v1.22.3 scores only the first numFeasibleNodesToFind nodes that pass Filter, walking
the node list from a rotating start index.  Read at parallelism 1, for pod p with F'(p) the
feasible set without sampling (present, Yoda's Filter, a candidate of the pod's class):

    rotated order   GLOBAL ids start[p], start[p] + 1, ..., last, first, ..., start[p] - 1
    S(p)            the first min(M, |F'|) nodes of F' in that order
    n_found[p]      |F'(p)|
    next_start[p]   the (M+1)-th node of F' in that order when |F'| > M, else start[p]

The PreScore maxima do not move; everything downstream of Filter follows S.  So a sampled cycle is
the candidate-class cycle whose candidate set is the sample: the reference is
candidate_cases.detail / reference through a model whose candidates(p) returns the sample mask.
Ids here are LOCAL (0 .. n_nodes - 1); a handle uploaded at a node_offset adds it.

tests/test_sampling_cases.py shows with the oracle alone that the scenarios separate the
specification from its near misses; tests/test_gpu_sampling.py replays them on libyoda."""
import functools

import numpy as np

import candidate_cases as cc
import oracle
from card_update_cases import shape_workload
from yoda_amd.soa import MODE_SCV

ANY = cc.ANY


def num_feasible_to_find(n, pct):
    """numFeasibleNodesToFind (generic_scheduler.go, k8s v1.22.3) in 64-bit integers."""
    n, pct = np.int64(n), np.int64(pct)
    if n < 100 or pct >= 100:
        return int(n)
    a = pct if pct > 0 else max(np.int64(5), np.int64(50) - n // np.int64(125))
    return int(max(n * a // np.int64(100), np.int64(100)))


# (n, pct) -> result, as the issue lists them
KNOWN = ((99, 0, 99), (100, 0, 100), (1000, 0, 420), (4608, 0, 645), (5000, 0, 500),
         (100000, 0, 5000), (100000, 30, 30000), (100000, 100, 100000), (150, 10, 100))


def rotate(ids, start):
    """The ascending ids in the rotated order that begins at `start`."""
    ids = np.asarray(ids)
    return np.concatenate([ids[ids >= start], ids[ids < start]])


class Sampled:
    """A candidate_cases.Model seen through the sample: candidates(p) is S(p)'s mask.  start: LOCAL
    ids [P], or None (every pod starts at node 0)."""

    def __init__(self, snap, model, num_to_find, start=None, ignore_start=False):
        self.snap, self.model, self.m = snap, model, int(num_to_find)
        self.start = None if start is None else np.asarray(start, np.int64)
        self.ignore_start = ignore_start
        self.base = model.base
        self._walk = {}

    def fprime(self, p):
        """LOCAL ids of F'(p), ascending."""
        feas, _ = self.snap.pod(p)
        keep = self.snap.keep
        return keep[feas & self.model.candidates(p)[keep]]

    def walk(self, p):
        """(mask bool[n_nodes], n_found, next_start) of pod p."""
        if p not in self._walk:
            s = 0 if self.start is None else int(self.start[p])
            rot = rotate(self.fprime(p), 0 if self.ignore_start else s)
            mask = np.zeros(self.base.n_nodes, bool)
            mask[rot[:self.m]] = True
            self._walk[p] = (mask, rot.size, int(rot[self.m]) if rot.size > self.m else s)
        return self._walk[p]

    def candidates(self, p):
        return self.walk(p)[0]


def reference(snap, model, num_to_find, start=None, sample=None, **kw):
    """(EvalResult, tie sets, n_found, next_start) of the sampled cycle; pods outside `sample` are
    left empty."""
    sm = Sampled(snap, model, num_to_find, start, **kw)
    res, ties = cc.reference(snap, sm, sample)
    P = snap.pods.n_pods
    found, nxt = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    for p in (range(P) if sample is None else np.asarray(sample).tolist()):
        _, found[p], nxt[p] = sm.walk(p)
    return res, ties, found, nxt, sm


def random_starts(n_nodes, n_pods, seed=5):
    return np.random.default_rng(seed).integers(0, n_nodes, n_pods).astype(np.uint32)


def m_values(n_nodes):
    """The sample sizes of the walk tests: one node, a few, about a block and a half, the
    deployed default, and no cut at all."""
    return (1, 7, 100, num_feasible_to_find(n_nodes, 0), n_nodes)


# ---- directed cuts on base ------------------------------------------------------------------
DIRECTED_M = 100


def _labelless(pods, k):
    """`pods` with its first k pods stripped of every label (feasible wherever a node has a card
    to give: the sample is predictable)."""
    pd = pods.take(np.arange(pods.n_pods))
    for f in ("has_number", "has_memory", "has_clock"):
        a = getattr(pd, f).copy()
        a[:k] = 0
        setattr(pd, f, a)
    return pd


@functools.lru_cache(maxsize=None)
def directed(n_pods):
    """base (4,608 nodes = 72 blocks, two 64-block windows), M = 100: label-less pods whose starts
    put the cut at chosen places, then ordinary pods with random starts.  (4,608 is a whole number
    of blocks, so "the last block" is a whole one here; the walk tests' small and f64 / u64 shapes,
    900 and 1,500 nodes, end in a partial block.)
    Returns (nodes, pods, words, cls, start, tags): words / cls are candidate classes (3 classes)
    that give three of the label-less pods a small F'; tags[i] names directed pod i."""
    nd, base = shape_workload("base")
    M, n = DIRECTED_M, nd.n_nodes
    probe = _labelless(base.slice(0, 1), 1)
    ids = np.flatnonzero(oracle.pod_detail(nd, probe, 0, MODE_SCV)[1])  # F of a label-less pod
    assert ids.size > 20 * M and n == 4608

    def start_for(last):
        """The start whose M-th node is ids[last] (no wrap)."""
        assert last >= M - 1
        return int(ids[last - (M - 1)])

    def first(cond):
        return int(np.flatnonzero(cond & (np.arange(ids.size) >= M))[0])

    rows = [("last node of a block", start_for(first(ids % 64 == 63)), ANY),
            ("first node of a block", start_for(first(ids % 64 == 0)), ANY),
            ("last node of window 0", start_for(int(np.flatnonzero(ids < 4096)[-1])), ANY),
            ("in the last block", start_for(first((ids >= n - 64) & (ids % 64 < 40))), ANY),
            ("after a wrap", int(ids[-(M // 2)]), ANY),
            ("start 0", 0, ANY), ("start N-1", n - 1, ANY), ("mid-block", 1000 + 21, ANY)]
    words = np.zeros(n, np.uint64)
    # class 0: four feasible nodes g0..g3 of one block and 97 elsewhere, start g2: the walk takes
    # g2, g3, the 97, then g0 -- the cut lands in the HEAD of the start's own block; g1 is next
    blk = next(b for b in range(8, 60) if ((ids // 64) == b).sum() >= 4)
    g = ids[(ids // 64) == blk][:4]
    other = ids[(ids // 64) != blk]
    words[g] |= np.uint64(1)
    words[other[5::max(1, other.size // 97)][:97]] |= np.uint64(1)
    rows.append(("head of the start's block", int(g[2]), 0))
    # class 1: |F'| == M; class 2: |F'| == M + 1 (one node past the cut)
    words[ids[3::7][:M]] |= np.uint64(2)
    words[ids[2::5][:M + 1]] |= np.uint64(4)
    rows += [("|F'| == M", int(ids[3::7][M // 2]), 1), ("|F'| == M + 1", int(ids[2::5][M // 2]), 2)]
    k = len(rows)
    assert n_pods > k
    pods = _labelless(base.slice(0, n_pods), k)
    start = random_starts(n, n_pods, seed=n_pods)
    cls = np.full(n_pods, ANY, np.uint8)
    for i, (_, s, c) in enumerate(rows):
        start[i], cls[i] = s, c
    return nd, pods, words, cls, start, tuple(r[0] for r in rows)
