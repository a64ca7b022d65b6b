"""Mode B under node sampling (yoda_mode_b_sampling), as plain data (no fixtures): scenarios and
their reference.

With sampling on (M = num_to_find, start[p]) and the setting on, pod p's cycle is the oracle's
Mode B cycle on the sub-snapshot that holds only the nodes of

    S(p) = sampling_cases.rotate(ids of E(p), start[p])[:M]

where E(p) is mode_b_follow_cases.eligible (present and a candidate of p's class).  Picks are ids
of the uploaded snapshot; n_found[p] = |E(p)|; next_start[p] is the (M+1)-th node of E in rotated
order when |E| > M, else start[p].  Rows come through oracle.pod_detail on S and
candidate_cases._normalize, tie sets from the rows.  Ids here are LOCAL.

tests/test_mode_b_sampling_cases.py shows with the oracle alone that the scenarios separate the
specification from its near misses; tests/test_gpu_mode_b_sampling.py replays them on libyoda."""
import functools

import numpy as np

import candidate_cases as cc
import mode_b_follow_cases as mbf
import node_present_cases as npc
import oracle
import sampling_cases as sc
from yoda_amd import synth
from yoda_amd.soa import MODE_DISKIO, PICK_NONE, STATUS_UNSCHEDULABLE, EvalResult

ANY = cc.ANY
FIELDS = mbf.FIELDS
DIRECTED_M = 100


def walk_of(model, p, start, m, ignore_start=False, over_ids=False, adjacent_next=False):
    """(ids of S(p) ascending, n_found, next_start) of pod p.  The keyword flags are the near
    misses of tests/test_mode_b_sampling_cases.py: the walk from node 0; M counted over node ids
    (the first M ids from start, then cut to E); next_start as the id after the M-th node."""
    n = model.base.n_nodes
    s = 0 if ignore_start else int(start)
    ids = np.flatnonzero(mbf.eligible(model, p))
    if over_ids:
        span = (s + np.arange(min(m, n))) % n
        return np.sort(np.intersect1d(span, ids)), ids.size, (s + m) % n if n > m else s
    rot = sc.rotate(ids, s)
    nxt = int(rot[m]) if rot.size > m else int(start)
    if adjacent_next and rot.size > m:
        nxt = (int(rot[m - 1]) + 1) % n
    return np.sort(rot[:m]), rot.size, nxt


def reference(model, pods, m, start, sample=None, first_in_walk=False, **miss):
    """(EvalResult, n_found, next_start) of the sampled cycle; pods outside `sample` are left
    empty.  start: LOCAL ids [P], or None (every walk starts at node 0).  first_in_walk: the near
    miss that picks the first top-scored node in walk order instead of the lowest id."""
    P = pods.n_pods
    res = EvalResult.empty(P)
    found, nxt = np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    nodes = model.nodes()
    for p in (range(P) if sample is None else np.asarray(sample).tolist()):
        s = 0 if start is None else int(start[p])
        keep, found[p], nxt[p] = walk_of(model, p, s, m, **miss)
        if keep.size == 0:
            res.pick[p], res.status[p] = PICK_NONE, STATUS_UNSCHEDULABLE
            res.n_feasible[p] = res.n_ties[p] = res.top_score[p] = 0
            continue
        r = oracle.schedule(nodes.take(keep), pods.take(np.array([p])), MODE_DISKIO, threads=1)
        res.pick[p] = npc.remap(r.pick, keep)[0]
        for f in ("status", "n_feasible", "n_ties", "top_score"):
            getattr(res, f)[p] = getattr(r, f)[0]
        if first_in_walk and r.status[0] == 0 and r.n_ties[0] >= 2:
            ties = detail(model, pods, p, s, m)["ties"]
            res.pick[p] = int(sc.rotate(ties, s)[0])
    return res, found, nxt


def detail(model, pods, p, start, m):
    """Pod p's full-width rows (feasibility bits, raw and normalized scores, -1 outside S) and its
    tie set within S (ids of the uploaded snapshot, ascending)."""
    n = model.base.n_nodes
    keep, _, _ = walk_of(model, p, start, m)
    feas = np.zeros(n, bool)
    feas[keep] = True
    raw = np.full(n, -1, np.int64)
    norm = np.full(n, -1, np.int64)
    ties = np.zeros(0, np.int64)
    if keep.size:
        _, _, r, _ = oracle.pod_detail(model.nodes().take(keep), pods, int(p), MODE_DISKIO)
        raw[keep] = r
        nm = cc._normalize(r)
        assert nm is not None  # Mode B scores lie in [0, 10]
        norm[keep] = nm
        ties = keep[r == r.max()]
    return dict(feas=feas, raw=raw, norm=norm, ties=ties)


def assert_same(got, want, tag="", sample=None):
    sel = slice(None) if sample is None else np.asarray(sample)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f)[sel], getattr(want, f)[sel],
                                      err_msg=f"{tag}: {f}")


# ---- shapes and states ------------------------------------------------------------------------
SHAPES = ("one-spec", "distinct", "small", "tiny")


@functools.lru_cache(maxsize=None)
def shape(name):
    """(nodes, pods): 5,000 nodes x 700 pods (78 whole blocks and 8 nodes; one pod spec, or a
    distinct request per pod), 900 x 200 (14 blocks and 4 nodes) and 50 x 40 (less than a block)."""
    if name in ("one-spec", "distinct"):
        return mbf.workload(name == "distinct")
    n, p = (900, 200) if name == "small" else (50, 40)
    nodes, pods = synth.make_config(2, pods=p, nodes=n)
    return nodes, synth.distinct_diskio(pods)


@functools.lru_cache(maxsize=None)
def state(name, which):
    """(nodes, pods, steps, Model) of a shape: "whole" (every E the whole snapshot: no step) or
    "recipe" (mode_b_follow_cases.recipe: absent nodes and 8 classes, the one-node class 6 and the
    empty class 7 among them)."""
    nodes, pods = shape(name)
    steps = []
    if which == "recipe":
        absent, words, cls = mbf.recipe(nodes, pods, n_absent=min(120, nodes.n_nodes // 8))
        steps = [npc._present(absent, 0), ("cand", 8, words), ("classes", cls)]
    m = cc.Model(nodes)
    for s in steps:
        m.apply(s)
    return nodes, pods, steps, m


def starts(name, seed=41):
    nodes, pods = shape(name)
    return sc.random_starts(nodes.n_nodes, pods.n_pods, seed=seed)


# ---- directed cuts ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def directed():
    """The recipe on 5,000 nodes with four more classes (8: 101 nodes, four of them in one block;
    9: exactly M nodes; 10: M + 1; 11: M nodes below a pod's best level, then some at it),
    M = 100, and pods whose starts put the cut at chosen places.
    Returns (nodes, pods, steps, start, tags): tags[i] names pod i; the pods after the tagged
    ones keep the recipe's classes and take random starts."""
    nodes, base = mbf.workload(True)
    M, n = DIRECTED_M, nodes.n_nodes
    absent, words, rcls = mbf.recipe(nodes, base)
    present = np.ones(n, bool)
    present[absent] = False
    ids = np.flatnonzero(present)  # E of an ANY pod
    assert n == 5000 and n % 64 == 8 and ids.size > 20 * M

    def start_for(e, last):
        """The start whose M-th node is e[last] (no wrap)."""
        assert last >= M - 1
        return int(e[last - (M - 1)])

    def first(e, cond):
        return int(np.flatnonzero(cond & (np.arange(e.size) >= M))[0])

    rows = [("cut on the last node of a block", start_for(ids, first(ids, ids % 64 == 63)), ANY),
            ("cut on the first node of a block", start_for(ids, first(ids, ids % 64 == 0)), ANY),
            ("cut in the last partial block",
             start_for(ids, first(ids, (ids >= n - 8) & (ids < n - 1))), ANY),
            ("start in the last partial block", n - 5, ANY),
            ("after a wrap", int(ids[-(M // 2)]), ANY),
            ("start 0", 0, ANY), ("start N-1", n - 1, ANY),
            ("start on an absent node", int(absent[absent > 1000][0]), ANY)]
    # class 3 lacks 40 % of the nodes: a start that is present and no candidate, and a cut whose
    # M-th and (M+1)-th nodes are not adjacent ids
    e3 = ids[((words[ids] >> np.uint64(3)) & np.uint64(1)).astype(bool)]
    non = ids[(((words[ids] >> np.uint64(3)) & np.uint64(1)) == 0) & (ids > 2000)]
    rows.append(("start on a non-candidate", int(non[0]), 3))
    gap = first(e3, np.append(np.diff(e3) > 1, False))
    rows.append(("gap after the cut", start_for(e3, gap), 3))
    words = words.copy()
    # class 8: four present nodes g0..g3 of one block and 97 elsewhere, start g2: the walk takes
    # g2, g3, the 97, then g0 -- the cut lands in the HEAD of the start's own block; g1 is next
    blk = next(b for b in range(8, 60) if ((ids // 64) == b).sum() >= 4)
    g = ids[(ids // 64) == blk][:4]
    other = ids[(ids // 64) != blk]
    words[g] |= np.uint64(1 << 8)
    words[other[5::max(1, other.size // 97)][:97]] |= np.uint64(1 << 8)
    rows.append(("cut in the head of the start's block", int(g[2]), 8))
    # class 9: |E| == M; class 10: |E| == M + 1 (one node past the cut)
    words[ids[3::7][:M]] |= np.uint64(1 << 9)
    words[ids[2::5][:M + 1]] |= np.uint64(1 << 10)
    rows += [("|E| == M", int(ids[3::7][M // 2]), 9), ("|E| == M + 1", int(ids[2::5][M // 2]), 10)]
    # the pod after the tagged ones: a stretch of 100 present nodes without any node at its best
    # level over E, so its top_score drops under sampling
    # class 11: M present nodes below that pod's best level, then 30 nodes at it
    k = len(rows)
    raw = oracle.pod_detail(nodes.take(ids), base, k, MODE_DISKIO)[2]
    low = ids[raw < raw.max()][:M]
    top = ids[(raw == raw.max()) & (ids > low[-1])][:30]
    assert low.size == M and top.size
    words[low] |= np.uint64(1 << 11)
    words[top] |= np.uint64(1 << 11)
    rows.append(("top_score drops", int(low[0]), 11))
    n_pods = 80
    pods = base.slice(0, n_pods)
    start = sc.random_starts(n, n_pods, seed=n_pods)
    cls = rcls[:n_pods].copy()
    for i, (_, s, c) in enumerate(rows):
        start[i], cls[i] = s, c
    steps = [npc._present(absent, 0), ("cand", 12, words), ("classes", cls)]
    return nodes, pods, steps, start, tuple(r[0] for r in rows)


def directed_model():
    nodes, _, steps, _, _ = directed()
    m = cc.Model(nodes)
    for s in steps:
        m.apply(s)
    return m
