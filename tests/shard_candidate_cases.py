"""Candidate classes on node shards (yoda_shard_candidates) as plain data (no fixtures): the
scenarios of tests/candidate_cases.py and a few built for the cross-shard rules, each with the
node splits it is replayed on.  tests/test_shard_candidate_cases.py shows with the oracle alone that
every scenario bites -- feasible sets, tie sets and one-node pods straddle the cuts, picks differ
from the no-candidate and from the absent-node reading; tests/test_gpu_shard_candidates.py replays
them on shard handles against candidate_cases.reference and one handle holding the whole snapshot.

A scenario is (nodes, pods, steps, splits, kw): steps as candidate_cases has them (a "cand" step
carries the words of the WHOLE snapshot by global id: shard [lo, hi) takes words[lo:hi]; every
other step goes to every shard unchanged, its ids are global), splits the node bounds to run on,
kw the upload flags.  The cuts are never multiples of 64 (a node block), so every shard but the
first starts inside a block of the whole snapshot."""
import collections
import functools

import numpy as np

import candidate_cases as cases
import oracle
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV, NodeSoA

Scenario = collections.namedtuple("Scenario", "nodes pods steps splits kw")

ANY = cases.ANY
SEED = 0x5EEDFACE  # the draw's


def bounds(n, world):
    """(0, 1000, n) and (0, 77, 2500, n) where the snapshot is large enough; a smaller one keeps
    the 77-node first shard and cuts the rest at 2/5 (world 2) or 5/9 (world 3) of n."""
    b = {2: (0, 1000, n), 3: (0, 77, 2500, n)}[world]
    if b[-2] >= n:
        cut = 2 * n // 5 if world == 2 else 5 * n // 9
        cut += cut % 64 == 0
        b = (0, cut, n) if world == 2 else (0, 77, cut, n)
    assert all(c % 64 for c in b[1:-1]) and list(b) == sorted(b)
    return b


def with_empty(b):
    """The split with an empty shard (lo == hi) after the first one."""
    return b[:2] + b[1:]


def shard_of(b, ids):
    """The shard index of each global node id under the bounds b (an empty shard holds none)."""
    return np.searchsorted(np.asarray(b[1:]), np.asarray(ids), side="right")


def split_words(b, words):
    return [None if words is None else words[lo:hi] for lo, hi in zip(b[:-1], b[1:])]


# the walk's recipe seed per shape: the first whose reference clears every floor of
# tests/test_shard_candidate_cases.py on both splits (candidate_cases.RECIPE_SEED's rule)
WALK_SHAPES = ("small", "base", "f64", "u64")
WALK_SEED = {"small": 1, "base": 28, "f64": 4, "u64": 4}


@functools.lru_cache(maxsize=None)
def walk(shape):
    nd, pd, steps = cases.walk(shape, WALK_SEED[shape])
    n = nd.n_nodes
    return Scenario(nd, pd, steps, (bounds(n, 2), bounds(n, 3)), cases.UPLOAD_KW.get(shape, {}))


RULE_ONE = 32  # pods of `rules` left with one candidate
RULE_CLONES = 600


def concat(parts):
    return NodeSoA(**{f: np.concatenate([getattr(x, f) for x in parts], axis=0)
                      for f in parts[0].__dataclass_fields__}).normalized()


@functools.lru_cache(maxsize=None)
def rules():
    """The cross-shard rules on candidate_cases.maxima_holder's snapshot, split (0, 77, 2500, N):
    class 0's candidates all lie in shard 1 and class 1's in shard 2, while the nodes that hold
    the largest bandwidth (in every shard) are candidates of no class -- the maxima must come from
    shards that hold no candidate; class 2 has no candidate anywhere; class 3 may use every node
    beyond shard 0 but the holders; every node of shard 0 has word 0; classes 4 .. 4 + RULE_ONE - 1
    have ONE candidate each, a feasible node of the one pod in the class, beyond shard 0.  The
    snapshot ends in RULE_CLONES copies of shard 1's first nodes, so that tie sets span shards 1
    and 2 here too.  Also run with an empty shard after shard 0."""
    nd, pd, _, _ = cases.maxima_holder()
    b = bounds(nd.n_nodes + RULE_CLONES, 3)
    nd = concat([nd, nd.slice(b[1], b[1] + RULE_CLONES)])
    holders = np.flatnonzero((nd.card_bandwidth == nd.card_bandwidth.max()).any(axis=1))
    n, P = nd.n_nodes, pd.n_pods
    ids = np.arange(n)
    free = ~np.isin(ids, holders)
    words = np.zeros(n, np.uint64)
    words[(ids >= b[1]) & (ids < b[2]) & free] |= np.uint64(1 << 0)
    words[(ids >= b[2]) & free] |= np.uint64(1 << 1)
    words[(ids >= b[1]) & free] |= np.uint64(1 << 3)
    cls = (np.arange(P) % 4).astype(np.uint8)
    cls[::7] = ANY
    full = oracle.schedule(nd, pd, MODE_SCV, threads=8)
    some = np.flatnonzero((full.status == 0) & (full.n_feasible >= 2))
    some = some[:: max(1, some.size // RULE_ONE)][:RULE_ONE]
    for j, p in enumerate(some.tolist()):
        feas = np.flatnonzero(oracle.pod_detail(nd, pd, p, MODE_SCV)[1])
        words[feas[-1]] |= np.uint64(1 << (4 + j))
        cls[p] = 4 + j
    steps = [("cand", 4 + some.size, words), ("classes", cls), ("check", "rules")]
    return Scenario(nd, pd, steps, (b, with_empty(b)), {}), holders, some


@functools.lru_cache(maxsize=None)
def zero_split():
    """candidate_cases.zero_total with the zero-total node s alone in the middle shard: the pod's
    other feasible nodes sit in the shards around it.  DIV_ZERO, then s hidden, then s the one
    survivor -- each decided by counts summed over the shards.  Returns (scenario, s, p)."""
    nd, pd, steps, s, p = cases.zero_total()
    return Scenario(nd, pd, steps, ((0, s, s + 1, nd.n_nodes),), {}), s, p


@functools.lru_cache(maxsize=None)
def overflow():
    """candidate_cases.overflow (U64, every pod through the exact normalize, half of each pod's
    feasible nodes hidden) at world 2."""
    nd, pd, steps = cases.overflow()
    cut = nd.n_nodes // 2
    cut += cut % 64 == 0
    return Scenario(nd, pd, steps, ((0, cut, nd.n_nodes),), {"force_generic": True})


@functools.lru_cache(maxsize=None)
def dense():
    """640 nodes repeated 8 times (the clones of a node sit 640 ids apart and tie on every pod that
    may use them), 8 classes that each lack three nodes in ten: every tie set straddles the cuts."""
    nd = concat([synth.make_nodes(640, 3)] * 8)
    pd = synth.make_pods(300, 5)
    words, cls = cases.recipe(nd, pd, seed=9, tenths=0.3, cordoned=16)
    steps = [("cand", 8, words), ("classes", cls), ("check", "dense")]
    n = nd.n_nodes
    return Scenario(nd, pd, steps, (bounds(n, 2), bounds(n, 3)), {})


@functools.lru_cache(maxsize=None)
def with_absent():
    """candidate_cases.with_absent: absent nodes beside the candidates, card updates and pushes on
    non-candidates, the nodes back -- every list in global ids, the same for every shard."""
    nd, pd, steps = cases.with_absent()
    n = nd.n_nodes
    return Scenario(nd, pd, steps, (bounds(n, 2), bounds(n, 3)), {})


def checks(sc):
    """[(tag, Model copy)] of every check of the scenario."""
    return cases.states(sc.nodes, sc.steps)


def counts(sc, b, model, ref, ties, plain, absent):
    """What makes a split of a state bite, from the reference alone: pods whose F' spans at least
    two shards, picks that differ from the no-candidate reading (`plain`) and from the absent-node
    reading (`absent`), pods with |F'| = 1 beyond shard 0, tied pods whose tie set spans shards."""
    snap = None
    span = one_out = tie_span = 0
    for p in range(sc.pods.n_pods):
        if ref.n_feasible[p] == 0:
            continue
        snap = snap or cases.Snapshot(model, sc.pods)
        f = np.flatnonzero(cases.detail(snap, model, p)["feas"])
        sh = np.unique(shard_of(b, f))
        span += sh.size >= 2
        one_out += f.size == 1 and sh[0] != 0
        if ref.status[p] == 0 and ref.n_ties[p] >= 2:
            tie_span += np.unique(shard_of(b, ties[p])).size >= 2
    return (int(span), int((ref.pick != plain.pick).sum()), int((ref.pick != absent.pick).sum()),
            int(one_out), int(tie_span))
