"""Candidate-class scenarios as plain data (no fixtures): the snapshot as uploaded, the pods, and
the steps a long-lived handle would see while other plugins' Filter results arrive as candidate
classes (yoda_set_candidates, yoda_update_candidates, yoda_set_pod_classes).
tests/test_candidate_cases.py checks with the oracle alone that every scenario would fail a handle
that ignored the words or treated a non-candidate as an absent node;
tests/test_gpu_candidates.py replays them on libyoda.

Each scenario returns (nodes, pods, steps); a step is one of
    ("cand", n_classes, words u64 | None)   yoda_set_candidates (n_classes 0: off)
    ("update", ids u32, words u64)          yoda_update_candidates (GLOBAL ids)
    ("classes", cls u8 | None)              yoda_set_pod_classes (None: every pod ANY)
    ("present", ...), ("cards", ...), ("push", ...)   as tests/node_present_cases.py
    ("check", tag)                          compare the handle with the reference here

The reference needs no oracle of its own.  CollectMaxValues (collection.go:39-52) never sees
another plugin's Filter, so the maxima are oracle.schedule's, unchanged; oracle.pod_detail gives
pod p's Yoda feasibility and its raw scores under those maxima; the pod's class bit is applied to
the feasibility and the cycle's tail (one node, DIV_ZERO, NormalizeScore in Go int64 arithmetic,
top normalized score, lowest node, tie set) is restated here as oracle/yoda_oracle.c has it (a
single feasible node reports its raw score)."""
import copy
import functools
import os

import numpy as np

import node_present_cases as npc
import oracle
from card_update_cases import BASE_NODES, BASE_PODS, SHAPES, UPLOAD_KW, shape_workload  # noqa: F401
from yoda_amd import synth
from yoda_amd.soa import (MODE_SCV, PICK_ERROR, PICK_NONE, STATUS_DIV_ZERO, STATUS_OK,
                          STATUS_SCORE_RANGE, STATUS_UNSCHEDULABLE, EvalResult, NodeSoA, PodSoA)

ANY = 0xFF
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Model(npc.Model):
    """node_present_cases.Model and the candidate state: n_classes (0: off), one word per node,
    the pods' class bytes (None: every pod ANY)."""

    def __init__(self, nodes):
        super().__init__(nodes)
        self.n_classes = 0
        self.words = np.full(nodes.n_nodes, FULL, np.uint64)
        self.cls = None

    def apply(self, step):
        if step[0] == "cand":
            self.n_classes = int(step[1])
            self.words = (np.full(self.base.n_nodes, FULL, np.uint64) if not self.n_classes
                          else np.array(step[2], np.uint64))
        elif step[0] == "update":
            n = self.base.n_nodes  # ids outside the snapshot are ignored; the last entry wins
            for i, w in zip(np.asarray(step[1]).tolist(), np.asarray(step[2]).tolist()):
                if i < n:
                    self.words[i] = w
        elif step[0] == "classes":
            self.cls = None if step[1] is None else np.array(step[1], np.uint8)
        else:
            return super().apply(step)

    def candidates(self, p):
        """bool[n_nodes]: cand(p, n) of pod p in this state."""
        c = ANY if self.cls is None else int(self.cls[p])
        if not self.n_classes or c == ANY:
            return np.ones(self.base.n_nodes, bool)
        return ((self.words >> np.uint64(c)) & np.uint64(1)).astype(bool)


class Snapshot:
    """What does not depend on the candidates: the oracle's result on the present nodes (the
    maxima) and each pod's Yoda feasibility and raw scores, computed once per pod."""

    def __init__(self, model, pods):
        self.keep, self.comp, self.pods = model.keep(), model.compact(), pods
        self.n = model.base.n_nodes
        self.full = oracle.schedule(self.comp, pods, MODE_SCV, threads=8)
        self.zero = self.comp.total_memory_sum == 0
        self._pod = {}

    def pod(self, p):
        if p not in self._pod:
            _, feas, raw, _ = oracle.pod_detail(self.comp, self.pods, int(p), MODE_SCV)
            self._pod[p] = (feas, raw)
        return self._pod[p]


def _normalize(sc):
    """NormalizeScore (scheduler.go:158-183) over the int64 scores sc, as oracle/yoda_oracle.c:
    None when a normalized score leaves [0, 100]."""
    highest, lowest = max(0, int(sc.max())), int(sc.min())
    if highest == lowest:
        lowest -= 1
    with np.errstate(over="ignore"):
        diff = sc - np.int64(lowest) if -2 ** 63 <= lowest < 2 ** 63 else None
    if diff is None or not -2 ** 63 < highest - lowest < 2 ** 63:
        return None
    prod = (diff.astype(np.uint64) * np.uint64(100)).astype(np.int64)
    den = highest - lowest
    if den > 0 and (prod >= 0).all():
        norm = prod // np.int64(den)
    else:  # Go's division truncates toward zero
        norm = np.array([abs(int(v)) // abs(den) * (1 if (int(v) < 0) == (den < 0) else -1)
                         for v in prod], np.int64)
    return None if ((norm < 0) | (norm > 100)).any() else norm


def detail(snap, model, p):
    """Pod p under the candidates of `model`: dict with the cycle's outcome, the tie set (GLOBAL
    ids) and the full-width rows (feasibility bits, raw and normalized scores, -1 outside F')."""
    feas, raw = snap.pod(p)
    f2 = feas & model.candidates(p)[snap.keep]
    idx = np.flatnonzero(f2)
    ids = snap.keep[idx]
    out = dict(pick=PICK_NONE, status=STATUS_UNSCHEDULABLE, n_feasible=idx.size, n_ties=0,
               top_score=0, ties=np.zeros(0, np.int64))
    bits = np.zeros(snap.n, bool)
    bits[ids] = True
    rows = np.full(snap.n, -1, np.int64)
    rows[ids] = raw[idx]
    norm_row = np.full(snap.n, -1, np.int64)
    out.update(feas=bits, raw=rows, norm=norm_row)
    if idx.size == 0:
        return out
    if idx.size == 1:  # returned without scoring
        out.update(pick=int(ids[0]), status=STATUS_OK, n_ties=1, top_score=int(raw[idx[0]]),
                   ties=ids)
        return out
    if snap.zero[idx].any():
        out.update(pick=PICK_ERROR, status=STATUS_DIV_ZERO)
        return out
    norm = _normalize(raw[idx])
    if norm is None:
        out.update(pick=PICK_ERROR, status=STATUS_SCORE_RANGE)
        return out
    norm_row[ids] = norm
    t = np.flatnonzero(norm == norm.max())
    out.update(pick=int(ids[t[0]]), status=STATUS_OK, n_ties=t.size, top_score=int(raw[idx[t[0]]]),
               ties=ids[t])
    return out


def reference(snap, model, sample=None):
    """EvalResult of the pods in `sample` (all when None; the others left empty) and the tie sets
    {pod: GLOBAL ids}.  The maxima are the oracle's: candidates do not move them."""
    P = snap.pods.n_pods
    res = EvalResult.empty(P)
    tie_sets = {}
    for p in (range(P) if sample is None else np.asarray(sample).tolist()):
        d = detail(snap, model, p)
        res.pick[p], res.status[p] = d["pick"], d["status"]
        res.n_feasible[p], res.n_ties[p], res.top_score[p] = d["n_feasible"], d["n_ties"], d["top_score"]
        res.maxima[p] = snap.full.maxima[p]
        tie_sets[p] = d["ties"]
    return res, tie_sets


def as_absent(model, pods):
    """The same state read as ABSENCE, per class: the oracle on the snapshot without the class's
    non-candidates (its maxima follow), picks as ids of the full snapshot.  What a caller gets who
    marks non-candidates absent; test_candidate_cases.py counts how far it is from the reference."""
    P = pods.n_pods
    res = EvalResult.empty(P)
    cls = np.full(P, ANY, np.uint8) if model.cls is None or not model.n_classes else model.cls
    for c in np.unique(cls).tolist():
        sel = np.flatnonzero(cls == c)
        keep = np.flatnonzero(model.present & model.candidates(int(sel[0])))
        r = oracle.schedule(model.nodes().take(keep), pods.take(sel), MODE_SCV, threads=8)
        res.pick[sel] = npc.remap(r.pick, keep) if keep.size else r.pick
        for f in ("status", "n_feasible", "n_ties", "top_score", "maxima"):
            getattr(res, f)[sel] = getattr(r, f)
    return res


def recipe(nodes, pods, seed=7, n_classes=8, tenths=None, cordoned=64):
    """(words, cls): class c lacks a random (c + 1) / 10 of the nodes (tenths: that share for
    every class instead), the `cordoned` most-picked nodes (fewer when fewer are picked) have
    every bit clear, the pod classes are uniform over the classes and ANY."""
    rng = np.random.default_rng(seed)
    n = nodes.n_nodes
    words = np.full(n, np.uint64((1 << n_classes) - 1), np.uint64)
    for c in range(n_classes):
        share = (c + 1) / 10 if tenths is None else tenths
        words[rng.choice(n, int(n * share), replace=False)] &= ~np.uint64(1 << c)
    r = oracle.schedule(nodes, pods.slice(0, min(pods.n_pods, 3000)), MODE_SCV, threads=8)
    ids, cnt = np.unique(r.pick[r.status == 0], return_counts=True)
    words[ids[np.argsort(-cnt, kind="stable")][:cordoned]] = 0
    cls = rng.integers(0, n_classes + 1, pods.n_pods).astype(np.uint8)
    cls[cls == n_classes] = ANY
    return words, cls


def states(nodes, steps):
    """[(tag, Model copy)] of every check, in order."""
    m, out = Model(nodes), []
    for s in steps:
        m.apply(s)
        if s[0] == "check":
            out.append((s[1], copy.deepcopy(m)))
    return out


WALK = ("recipe", "one class", "all any", "class 63", "uncordon half", "outside and repeated",
        "two blocks", "a class nowhere", "off")
WALK_ANY = 2      # every pod ANY: equals no candidates
WALK_OFF = 8      # candidates off


# the recipe's seed per shape: the first whose reference clears the floors of
# tests/test_candidate_cases.py (the small counts -- pods with one candidate, picks that differ
# from the absent-node reading -- move with the draw)
RECIPE_SEED = {"base": 1}


@functools.lru_cache(maxsize=None)
def walk(shape="base", seed=None, mixed_pods=32768 + 37):
    """A seeded walk through WALK on a shape of card_update_cases.shape_workload.  Cached: the
    arrays are shared, do not write to them."""
    seed = RECIPE_SEED.get(shape, 7) if seed is None else seed
    nd, pd = shape_workload(shape, mixed_pods)
    rng = np.random.default_rng(seed + 100)
    n, P = nd.n_nodes, pd.n_pods
    words, cls = recipe(nd, pd, seed)
    cordoned = np.flatnonzero(words == 0)
    steps = [("cand", 8, words), ("classes", cls), ("check", WALK[0]),
             ("classes", np.full(P, 3, np.uint8)), ("check", WALK[1]),
             ("classes", np.full(P, ANY, np.uint8)), ("check", WALK[2])]
    # 64 classes, every pod in class 63 (which lacks three nodes in ten); the other bits random
    w64 = rng.integers(0, 2 ** 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    w64[rng.choice(n, 3 * n // 10, replace=False)] &= np.uint64((1 << 63) - 1)
    steps += [("cand", 64, w64), ("classes", np.full(P, 63, np.uint8)), ("check", WALK[3])]
    # the recipe again; half the cordoned nodes return for every class
    back = rng.choice(cordoned, cordoned.size // 2, replace=False)
    steps += [("cand", 8, words), ("classes", cls),
              ("update", back.astype(np.uint32), np.full(back.size, 0xFF, np.uint64)),
              ("check", WALK[4])]
    # ignored by contract: n_nodes, beyond it, u32 max.  Repeated ids, the LAST entry wins: 20
    # nodes cleared and then set whole (they stay candidates), 20 set whole and then cleared
    a, b = rng.choice(n, 40, replace=False).reshape(2, 20)
    out = np.array([n, n + 5, 0xFFFFFFFF], np.uint64)
    ids = np.concatenate([a, b, out[:2], a, b, out[2:]]).astype(np.uint32)
    wd = np.concatenate([np.zeros(20), np.full(20, 0xFF), [0, 0xFF], np.full(20, 0xFF),
                         np.zeros(20), [0]]).astype(np.uint64)
    steps += [("update", ids, wd), ("check", WALK[5])]
    # two whole 64-node blocks lose class 2 (positions of the upload order)
    m = Model(nd)
    for s in steps:
        m.apply(s)
    blocks = rng.choice(n // 64, 2, replace=False)
    ids = np.concatenate([np.arange(64 * k, 64 * k + 64) for k in blocks])
    steps += [("update", ids.astype(np.uint32), m.words[ids] & ~np.uint64(1 << 2)),
              ("check", WALK[6])]
    m.apply(steps[-2])
    steps += [("cand", 8, m.words & ~np.uint64(1 << 1)), ("check", WALK[7]),
              ("cand", 0, None), ("check", WALK[8])]
    return nd, pd, steps


def maxima_holder(nodes=BASE_NODES, pods=BASE_PODS):
    """Every node that holds a card of the snapshot's largest bandwidth is a candidate of no
    class: the maxima must not move, while top scores and picks differ from the absent-node
    reading.  Returns (nodes, pods, steps, holders)."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    ids = np.flatnonzero((nd.card_bandwidth == nd.card_bandwidth.max()).any(axis=1))
    words = np.full(nd.n_nodes, 0xF, np.uint64)
    words[ids] = 0
    cls = (np.arange(pd.n_pods) % 4).astype(np.uint8)
    steps = [("check", "as uploaded"), ("cand", 4, words), ("classes", cls),
             ("check", "holders hidden"), ("cand", 0, None), ("check", "off")]
    return nd, pd, steps, ids


def zero_total():
    """node_present_cases.single_survivor: a pod p whose few feasible nodes include s with
    TotalMemorySum 0.  As uploaded p ends in DIV_ZERO; with s hidden from its class in OK; with
    every OTHER feasible node hidden in OK with one feasible node, s.
    Returns (nodes, pods, steps, s, p)."""
    nd, pd, _, s, p = npc.single_survivor()
    feas = np.flatnonzero(oracle.pod_detail(nd, pd, p, MODE_SCV)[1])
    others = feas[feas != s]
    cls = np.full(pd.n_pods, ANY, np.uint8)
    cls[p] = 1
    hide_s = np.full(nd.n_nodes, 3, np.uint64)
    hide_s[s] = 1
    hide_others = np.full(nd.n_nodes, 3, np.uint64)
    hide_others[others] = 1
    steps = [("check", "as uploaded"), ("cand", 2, hide_s), ("classes", cls),
             ("check", "zero node hidden"), ("cand", 2, hide_others), ("check", "one survivor"),
             ("cand", 0, None), ("check", "off")]
    return nd, pd, steps, s, p


def with_absent(seed=11):
    """Candidates and absent nodes together on the small shape, then a card update and a
    node-state push on non-candidate nodes: the values show (the maxima and the scores of the
    others follow them), the nodes stay non-candidates."""
    import card_update_cases as cu
    nd, pd = shape_workload("small")
    rng = np.random.default_rng(seed)
    n = nd.n_nodes
    words, cls = recipe(nd, pd, seed)
    m = Model(nd)
    gone = rng.choice(n, 120, replace=False)
    steps = [("cand", 8, words), ("classes", cls), npc._present(gone, 0),
             ("check", "candidates and absent")]
    for s in steps:
        m.apply(s)
    hidden = np.flatnonzero((words & np.uint64(0xFF)) != np.uint64(0xFF))
    ids = rng.permutation(np.concatenate([rng.choice(hidden, 60, replace=False),
                                          rng.choice(gone, 20, replace=False)]))
    ids = np.unique(ids)
    free, healthy, fsum = cu._draw(rng, m, ids)
    total = nd.total_memory_sum[ids]
    alloc = np.minimum((rng.random(ids.size) * (total.astype(np.float64) + 1)).astype(np.uint64),
                       total)
    cn = rng.integers(0, 9, ids.size).astype(np.uint64)
    steps += [cu._cards(ids, free, healthy, fsum), ("push", ids.astype(np.uint32), alloc, cn),
              ("check", "updates on non-candidates"), npc._present(gone, 1),
              ("check", "absent back")]
    return nd, pd, steps


def overflow():
    """The U64 exact-normalize pods of tests/golden/overflow.npz with half of each pod's feasible
    nodes hidden: class c hides every second feasible node of pod c."""
    z = np.load(os.path.join(GOLDEN, "overflow.npz"), allow_pickle=False)
    nd = NodeSoA(**{k[5:]: z[k] for k in z.files if k.startswith("node_")}).normalized()
    pd = PodSoA(**{k[4:]: z[k] for k in z.files if k.startswith("pod_")}).normalized()
    P = min(pd.n_pods, 64)
    pd = pd.slice(0, P)
    words = np.full(nd.n_nodes, FULL, np.uint64)
    for p in range(P):
        feas = np.flatnonzero(oracle.pod_detail(nd, pd, p, MODE_SCV)[1])
        words[feas[1::2]] &= ~np.uint64(1 << p)
    steps = [("check", "as uploaded"), ("cand", P, words),
             ("classes", np.arange(P, dtype=np.uint8)), ("check", "half hidden")]
    return nd, pd, steps
