"""Node-presence scenarios as plain data (no fixtures): the snapshot as uploaded, the pods, and
the steps a long-lived handle would see between uploads while nodes leave the node set and come
back (yoda_set_node_present).  tests/test_node_present_cases.py checks with the oracle alone that
every scenario moves enough picks or feasible counts to fail a handle that ignored an absence;
tests/test_gpu_node_present.py replays them on libyoda.

Each scenario returns (nodes, pods, steps); a step is one of
    ("present", ids u32, flags u8)   yoda_set_node_present of that list (GLOBAL ids; 0 = absent)
    ("cards", ...), ("push", ...)    as tests/card_update_cases.py
    ("check", tag)                   compare the handle with the reference here
The reference needs no oracle of its own: while nodes are absent a handle answers as one freshly
uploaded with the snapshot WITHOUT them would, the survivors keeping their ids.  So the oracle
runs on the compacted snapshot, nodes().take(keep()), and its picks are mapped through keep()."""
import functools

import numpy as np

import card_update_cases as cu
import oracle
from card_update_cases import BASE_NODES, BASE_PODS, SHAPES, UPLOAD_KW, shape_workload  # noqa: F401
from yoda_amd import synth
from yoda_amd.soa import MODE_SCV

# the ragged node shards of tests/test_gpu_node_state.py (worlds 2 and 3)
SHARD_CUTS = {2: (0.37,), 3: (0.24, 0.63)}


class Model(cu.Model):
    """The state a handle holds after the steps applied so far: the dynamic fields of
    card_update_cases.Model and who is present.  An update that names an absent node applies its
    values and leaves it absent."""

    def __init__(self, nodes):
        super().__init__(nodes)
        self.present = np.ones(nodes.n_nodes, bool)

    def apply(self, step):
        if step[0] != "present":
            return super().apply(step)
        _, ids, flags = step
        n = self.base.n_nodes
        # ids outside the snapshot are ignored by contract; a repeated id keeps its last entry
        for i, f in zip(np.asarray(ids).tolist(), np.asarray(flags).tolist()):
            if i < n:
                self.present[i] = f != 0

    def keep(self):
        """Ids of the present nodes, ascending: position in the compacted snapshot -> id."""
        return np.flatnonzero(self.present)

    def absent(self):
        return np.flatnonzero(~self.present)

    def compact(self):
        """The snapshot without the absent nodes (every node's CURRENT values)."""
        return self.nodes().take(self.keep())


def remap(pick, keep):
    """Picks over the compacted snapshot -> ids of the full one (negative picks as they are)."""
    out = np.array(pick, copy=True)
    ok = out >= 0
    out[ok] = np.asarray(keep)[out[ok]].astype(out.dtype)
    return out


def reference(model, pods, threads=8):
    """What every Mode A evaluation must answer in this state: the oracle on the compacted
    snapshot, picks as ids of the full one."""
    res = oracle.schedule(model.compact(), pods, MODE_SCV, threads=threads)
    res.pick = remap(res.pick, model.keep())
    return res


def states(nodes, steps):
    """[(tag, Model copy)] of every check, in order."""
    import copy
    m, out = Model(nodes), []
    for s in steps:
        m.apply(s)
        if s[0] == "check":
            out.append((s[1], copy.deepcopy(m)))
    return out


def _present(ids, flags):
    ids = np.asarray(ids, np.uint32)
    return ("present", ids, np.ascontiguousarray(np.broadcast_to(np.asarray(flags, np.uint8),
                                                                 ids.shape)))


def _most_picked(m, pods, k):
    """The k present nodes most pods pick in this state: the picked nodes by pick count, then,
    while fewer than k, those picked once these are gone, and so on."""
    full, present = m.nodes(), m.present.copy()
    out = np.zeros(0, np.int64)
    while out.size < k and present.any():
        keep = np.flatnonzero(present)
        r = oracle.schedule(full.take(keep), pods, MODE_SCV, threads=8)
        ids, cnt = np.unique(r.pick[r.status == 0], return_counts=True)
        if ids.size == 0:
            break
        out = np.concatenate([out, keep[ids[np.argsort(-cnt, kind="stable")]]])[:k]
        present[out] = False
    return out


WALK = ("top 1", "top 64", "two blocks", "700 scattered", "empty list", "outside and repeated",
        "half back", "updates while absent", "their return", "every node absent",
        "every node back")
WALK_EMPTY = 4      # the check after the count == 0 list
WALK_OUTSIDE = 5    # ids at or beyond n_nodes, repeated ids with conflicting flags
WALK_UPDATES = 7    # a card update and a push that name absent nodes
WALK_NONE = 9       # no node left


@functools.lru_cache(maxsize=None)
def walk(shape="base", seed=33, mixed_pods=32768 + 37):
    """A seeded walk through WALK on a shape of card_update_cases.shape_workload.  Cached: the
    arrays are shared, do not write to them."""
    nd, pd = shape_workload(shape, mixed_pods)
    rng = np.random.default_rng(seed)
    n = nd.n_nodes
    pool = cu._free_pool(nd) if shape == "ranks" else None
    sample = pd.slice(0, min(pd.n_pods, 3000))
    m = Model(nd)
    steps = []

    def add(tag, *ss):
        for s in ss:
            m.apply(s)
        steps.extend(list(ss) + [("check", tag)])

    add(WALK[0], _present(_most_picked(m, sample, 1), 0))
    add(WALK[1], _present(_most_picked(m, sample, 64), 0))
    blocks = rng.choice(n // 64, 2, replace=False)
    add(WALK[2], _present(np.concatenate([np.arange(64 * b, 64 * b + 64) for b in blocks]), 0))
    here = m.keep()
    # (700, or what a small shape can spare with 100 nodes left for the steps after it)
    add(WALK[3], _present(rng.choice(here, min(700, here.size - 100), replace=False), 0))
    add(WALK[4], _present(np.zeros(0, np.uint32), 0))
    # ignored by contract: n_nodes, beyond it, u32 max.  Repeated ids, the LAST entry wins: 20
    # absent nodes "returned" and then taken out again (they stay absent), 20 present nodes
    # taken out and then returned (they stay), 20 present nodes returned and then taken out
    # (they leave: the state moves)
    gone, here = m.absent(), m.keep()
    a = rng.choice(gone, min(20, gone.size), replace=False)
    b = rng.choice(here, 40, replace=False)
    stay, leave = b[:20], b[20:]
    out = np.array([n, n + 5, n + 100000, 0xFFFFFFFF], np.uint64)
    ids = np.concatenate([a, stay, leave, out[:2], a, stay, leave, out[2:]]).astype(np.uint64)
    flags = np.concatenate([np.ones(a.size), np.zeros(20), np.ones(20), [0, 1],
                            np.zeros(a.size), np.ones(20), np.zeros(20), [1, 0]])
    add(WALK[5], _present(ids, flags))
    gone = m.absent()
    add(WALK[6], _present(rng.choice(gone, gone.size // 2, replace=False), 1))
    # a card update and a push on 40 absent and 40 present nodes; the absent ones stay absent
    gone, here = m.absent(), m.keep()
    a = rng.choice(gone, min(40, gone.size), replace=False)
    ids = rng.permutation(np.concatenate([a, rng.choice(here, 40, replace=False)]))
    free, healthy, fsum = cu._draw(rng, m, ids, pool)
    total = nd.total_memory_sum[ids]
    alloc = np.minimum((rng.random(ids.size) * (total.astype(np.float64) + 1)).astype(np.uint64),
                       total)
    cn = rng.integers(0, 9, ids.size).astype(np.uint64)
    add(WALK[7], cu._cards(ids, free, healthy, fsum), ("push", ids.astype(np.uint32), alloc, cn))
    add(WALK[8], _present(a, 1))
    add(WALK[9], _present(np.arange(n), 0))
    add(WALK[10], _present(np.arange(n), 1))
    return nd, pd, steps


def single_survivor(nodes=BASE_NODES, pods=BASE_PODS):
    """A pod whose Filter passes few nodes; one of them, the survivor, reports TotalMemorySum 0.
    As uploaded every pod that passes the survivor and another node ends in DIV_ZERO (Score would
    divide by it).  With every other node of that pod's feasible set absent, the pod -- and every
    pod at least as strict -- has ONE feasible node: it is returned without scoring, status OK.
    Returns (nodes, pods, steps, survivor, pod)."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    r = oracle.schedule(nd, pd, MODE_SCV, threads=8)
    cand = np.flatnonzero(r.n_feasible >= 4)
    p = int(cand[np.argmin(r.n_feasible[cand])])
    feas = np.flatnonzero(oracle.pod_detail(nd, pd, p, MODE_SCV)[1])
    s = int(feas[feas.size // 2])
    nd.total_memory_sum = nd.total_memory_sum.copy()
    nd.total_memory_sum[s] = 0
    others = feas[feas != s]
    steps = [("check", "as uploaded"), _present(others, 0), ("check", "one survivor"),
             _present(others, 1), ("check", "back")]
    return nd, pd, steps, s, p


def max_holders(nodes=BASE_NODES, pods=BASE_PODS):
    """Every node that holds a card of the snapshot's largest bandwidth leaves, then returns: the
    PreScore maxima of most pods and the G maxima (bandwidth, and with that GPU model the
    clock, core, power and TotalMemory) move down and back."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    ids = np.flatnonzero((nd.card_bandwidth == nd.card_bandwidth.max()).any(axis=1))
    steps = [("check", "as uploaded"), _present(ids, 0), ("check", "holders absent"),
             _present(ids, 1), ("check", "holders back")]
    return nd, pd, steps


def shard_absent(nodes=BASE_NODES, pods=BASE_PODS):
    """Every node of one shard absent: the middle shard of world 3, then (the middle one back)
    the first shard of world 2."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    n = nd.n_nodes
    mid = np.arange(int(SHARD_CUTS[3][0] * n), int(SHARD_CUTS[3][1] * n))
    first = np.arange(0, int(SHARD_CUTS[2][0] * n))
    steps = [_present(mid, 0), ("check", "world 3, shard 1 absent"),
             _present(mid, 1), _present(first, 0), ("check", "world 2, shard 0 absent"),
             _present(first, 1), ("check", "back")]
    return nd, pd, steps
