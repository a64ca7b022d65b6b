"""Mode B with yoda_mode_b_follow on, as plain data (no fixtures): scenarios and their reference.

Mode B's Filter is a pass-through and it has no PreScore maxima, so pod p's cycle under
E(p) = {n : n present and cand(p, n)} is exactly the oracle's Mode B cycle on the snapshot that
holds only the nodes of E(p) -- the reading candidate_cases.as_absent shows to be WRONG for Mode A
is the right one here.  The state is candidate_cases.Model (presence, words, class bytes); per
distinct class the reference is oracle.schedule on the compacted snapshot with the picks mapped back
through `keep`; rows come from oracle.pod_detail on it and candidate_cases._normalize; tie sets
from the rows.  tests/test_mode_b_follow_cases.py shows with the oracle alone that every scenario
fails a handle that ignores E; tests/test_gpu_mode_b_follow.py replays them on libyoda."""
import copy
import functools

import numpy as np

import candidate_cases as cc
import node_present_cases as npc
import oracle
from yoda_amd import synth
from yoda_amd.soa import MODE_DISKIO, PICK_NONE, STATUS_UNSCHEDULABLE, EvalResult

ANY = cc.ANY
FIELDS = ("status", "pick", "n_feasible", "n_ties", "top_score")
N_NODES, N_PODS = 5000, 700


def classes_of(model, n_pods):
    """The class byte of every pod in this state (ANY while candidates are off or unset)."""
    if model.cls is None or not model.n_classes:
        return np.full(n_pods, ANY, np.uint8)
    return np.asarray(model.cls, np.uint8)


def eligible(model, p):
    """bool[n_nodes]: E(p)."""
    return model.present & model.candidates(p)


def reference(model, pods):
    """EvalResult of every pod: per distinct class the oracle on the nodes of E, picks as ids of
    the uploaded snapshot."""
    P = pods.n_pods
    res = EvalResult.empty(P)
    cls = classes_of(model, P)
    nodes = model.nodes()
    for c in np.unique(cls).tolist():
        sel = np.flatnonzero(cls == c)
        keep = np.flatnonzero(eligible(model, int(sel[0])))
        if keep.size == 0:
            res.pick[sel], res.status[sel] = PICK_NONE, STATUS_UNSCHEDULABLE
            for f in ("n_feasible", "n_ties", "top_score"):
                getattr(res, f)[sel] = 0
            continue
        r = oracle.schedule(nodes.take(keep), pods.take(sel), MODE_DISKIO, threads=8)
        res.pick[sel] = npc.remap(r.pick, keep)
        for f in ("status", "n_feasible", "n_ties", "top_score"):
            getattr(res, f)[sel] = getattr(r, f)
    return res


def unrestricted(model, pods):
    """What a handle that ignores E answers: the oracle on every uploaded node."""
    return oracle.schedule(model.nodes(), pods, MODE_DISKIO, threads=8)


def detail(model, pods, p):
    """Pod p's full-width rows (feasibility bits, raw and normalized scores, -1 outside E) and its
    tie set (ids of the uploaded snapshot)."""
    n = model.base.n_nodes
    feas = eligible(model, p)
    keep = np.flatnonzero(feas)
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


def assert_same(got, want, tag=""):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f"{tag}: {f}")


def workload(distinct):
    """5,000 nodes x 700 pods: one spec (every pod the same (alpha, beta): lane = node), or a
    distinct request per pod (lane = class)."""
    nodes, pods = synth.make_config(2, pods=N_PODS, nodes=N_NODES)
    return nodes, (synth.distinct_diskio(pods) if distinct else pods)


def recipe(nodes, pods, seed=5, n_absent=120):
    """(absent ids, words, cls) over 8 classes, built so that ignoring E fails every pod:
    - every node some pod picks on the whole snapshot is absent (with random others), so every
      spec's unrestricted pick is outside its E -- for ANY pods only absence can do that;
    - class 0 (pod 0's) hides every present node at pod 0's best level: its top_score drops;
    - classes 1..5 lack a random (c + 1) / 10 of the nodes and the node each of their pods would
      pick among the present ones;
    - class 6 keeps exactly one present node, class 7 keeps none."""
    rng = np.random.default_rng(seed)
    n, P = nodes.n_nodes, pods.n_pods
    r0 = oracle.schedule(nodes, pods, MODE_DISKIO, threads=8)
    absent = np.union1d(np.unique(r0.pick[r0.pick >= 0]), rng.choice(n, n_absent, replace=False))
    present = np.ones(n, bool)
    present[absent] = False
    keep = np.flatnonzero(present)
    cls = rng.integers(0, 9, P).astype(np.uint8)
    cls[:9] = np.arange(9)  # every class and ANY has a pod; pod 0 is in class 0
    cls[cls == 8] = ANY
    words = np.full(n, np.uint64(0xFF), np.uint64)
    for c in range(1, 6):
        words[rng.choice(n, int(n * (c + 1) / 10), replace=False)] &= ~np.uint64(1 << c)
    r1 = oracle.schedule(nodes.take(keep), pods, MODE_DISKIO, threads=8)
    p1 = npc.remap(r1.pick, keep)
    for c in range(1, 6):
        words[p1[cls == c]] &= ~np.uint64(1 << c)
    raw0 = oracle.pod_detail(nodes.take(keep), pods, 0, MODE_DISKIO)[2]
    words[keep[raw0 == raw0.max()]] &= ~np.uint64(1)
    words &= ~np.uint64(1 << 6 | 1 << 7)
    words[keep[keep.size // 2]] |= np.uint64(1 << 6)
    return absent.astype(np.uint32), words, cls


@functools.lru_cache(maxsize=None)
def scenario(distinct):
    """(nodes, pods, steps): the recipe as steps of candidate_cases.Model, one check."""
    nodes, pods = workload(distinct)
    absent, words, cls = recipe(nodes, pods)
    return nodes, pods, [npc._present(absent, 0), ("cand", 8, words), ("classes", cls),
                         ("check", "recipe")]


@functools.lru_cache(maxsize=None)
def walk(distinct, seed=21):
    """The steps of candidate_cases.WALK on the Mode B workload, with presence steps between
    them.  Cached: the arrays are shared, do not write to them."""
    nodes, pods = workload(distinct)
    n, P = nodes.n_nodes, pods.n_pods
    rng = np.random.default_rng(seed)
    absent, words, cls = recipe(nodes, pods)
    cordoned = np.flatnonzero(words == 0)
    W = cc.WALK
    steps = [npc._present(absent, 0), ("cand", 8, words), ("classes", cls), ("check", W[0]),
             ("classes", np.full(P, 3, np.uint8)), ("check", W[1]),
             ("classes", np.full(P, ANY, np.uint8)), ("check", W[2])]
    w64 = rng.integers(0, 2 ** 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    w64[rng.choice(n, 3 * n // 10, replace=False)] &= np.uint64((1 << 63) - 1)
    back = absent[: absent.size // 2]
    steps += [("cand", 64, w64), ("classes", np.full(P, 63, np.uint8)), npc._present(back, 1),
              ("check", W[3])]
    some = rng.choice(cordoned, max(1, cordoned.size // 2), replace=False)
    steps += [("cand", 8, words), ("classes", cls),
              ("update", some.astype(np.uint32), np.full(some.size, 0xFF, np.uint64)),
              ("check", W[4])]
    a, b = rng.choice(n, 40, replace=False).reshape(2, 20)
    out = np.array([n, n + 5, 0xFFFFFFFF], np.uint64)
    ids = np.concatenate([a, b, out[:2], a, b, out[2:]]).astype(np.uint32)
    wd = np.concatenate([np.zeros(20), np.full(20, 0xFF), [0, 0xFF], np.full(20, 0xFF),
                         np.zeros(20), [0]]).astype(np.uint64)
    steps += [("update", ids, wd), npc._present(rng.choice(n, 300, replace=False), 0),
              ("check", W[5])]
    m = cc.Model(nodes)
    for s in steps:
        m.apply(s)
    # two whole 64-node blocks lose class 2; the first 2,100 nodes leave (lane = node: a whole
    # first chunk of 2,048 without an eligible node)
    blocks = rng.choice(n // 64, 2, replace=False)
    ids = np.concatenate([np.arange(64 * k, 64 * k + 64) for k in blocks])
    steps += [("update", ids.astype(np.uint32), m.words[ids] & ~np.uint64(1 << 2)),
              npc._present(np.arange(2100), 0), ("check", W[6])]
    m.apply(steps[-3])
    steps += [("cand", 8, m.words & ~np.uint64(1 << 1)), ("check", W[7]),
              ("cand", 0, None), ("check", W[8]),
              npc._present(np.arange(n), 1), ("check", "everyone back")]
    return nodes, pods, steps


def states(nodes, steps):
    """[(tag, Model copy)] of every check, in order."""
    m, out = cc.Model(nodes), []
    for s in steps:
        m.apply(s)
        if s[0] == "check":
            out.append((s[1], copy.deepcopy(m)))
    return out
