"""Node-state push scenarios as plain data (no fixtures): the snapshot as uploaded, the pods,
and a list of steps a long-lived handle would see between uploads.  tests/test_node_state_cases.py
checks with the oracle alone that every scenario moves enough picks to fail a wrong handle;
tests/test_gpu_node_state.py replays them on libyoda.

Each scenario returns (nodes, pods, steps); a step is one of
    ("push", ids u32, alloc u64, card_number u64)   yoda_set_node_state of that list (GLOBAL ids)
    ("update_alloc", alloc u64 [N])                 yoda_update_alloc
    ("check", tag)                                  compare the handle with the model here
Model applies the steps to numpy copies of alloc_memory / card_number and returns the NodeSoA
a fresh upload of that state would get."""
import functools

import numpy as np

from yoda_amd import synth

BASE_PODS, BASE_NODES = 2341, 4608  # grouped node order, >= 8 pod blocks, a partly live wave


class Model:
    """The state a handle holds after the steps applied so far."""

    def __init__(self, nodes):
        self.base = nodes
        self.alloc = nodes.alloc_memory.copy()
        self.card_number = nodes.card_number.copy()

    def apply(self, step):
        if step[0] == "push":
            _, ids, alloc, cn = step
            # ids outside the snapshot are ignored by contract; a repeated id keeps its last entry
            for i, a, c in zip(ids.tolist(), alloc.tolist(), cn.tolist()):
                if i < self.base.n_nodes:
                    self.alloc[i], self.card_number[i] = a, c
        elif step[0] == "update_alloc":
            self.alloc = np.array(step[1], np.uint64)
        elif step[0] != "check":
            raise ValueError(step[0])

    def nodes(self):
        m = self.base.slice(0, self.base.n_nodes)
        m.alloc_memory = self.alloc.copy()
        m.card_number = self.card_number.copy()
        return m


def states(nodes, steps):
    """[(tag, NodeSoA)] of every check, in order."""
    m, out = Model(nodes), []
    for s in steps:
        m.apply(s)
        if s[0] == "check":
            out.append((s[1], m.nodes()))
    return out


def _push(ids, alloc, cn):
    return ("push", np.asarray(ids, np.uint32), np.asarray(alloc, np.uint64),
            np.asarray(cn, np.uint64))


def _base(pods, nodes):
    return synth.make_config(3, pods=pods, nodes=nodes)


def wake(pods=BASE_PODS, nodes=BASE_NODES, woken=150):
    """(a) Scores rise: every node fully allocated at upload, then `woken` random nodes are
    pushed to alloc 0 in one list."""
    nd, pd = _base(pods, nodes)
    nd.alloc_memory = nd.total_memory_sum.copy()
    rng = np.random.default_rng(5)
    sel = np.sort(rng.choice(nd.n_nodes, woken, replace=False))
    steps = [("check", "asleep"),
             _push(sel, np.zeros(sel.size), nd.card_number[sel]),
             ("check", "woken")]
    return nd, pd, steps


def _static(nd, alloc):
    """The static part of the score (Allocate + Actual, algorithm.go:96) per node."""
    t = nd.total_memory_sum
    one, c = np.uint64(1), np.uint64(100)
    a = (t - np.minimum(alloc, t)) * c // np.maximum(t, one) * np.uint64(3)
    return a + nd.free_memory_sum * c // np.maximum(t, one) * np.uint64(2)


def sleep_wake(pods=BASE_PODS, nodes=BASE_NODES, moved=150):
    """(b) Round trip: fall, run, rise back, run; then a fall and a rise in one gap.  With
    every node's alloc 0 the picks sit on the few nodes with the highest static score, so the
    nodes that move are taken from there: `sel` is every second of the top `moved` (plus as
    many random others), `other` the ones between them, uploaded half allocated."""
    nd, pd = _base(pods, nodes)
    rng = np.random.default_rng(5)
    zero = np.zeros(nd.n_nodes, np.uint64)
    top = np.argsort(-_static(nd, zero).astype(np.int64), kind="stable")
    half, other = top[0:moved:2], top[1:moved:2]
    sel = np.concatenate([half, rng.choice(top[moved:], moved - half.size, replace=False)])
    nd.alloc_memory = zero
    nd.alloc_memory[other] = nd.total_memory_sum[other] // np.uint64(2)
    total, cn = nd.total_memory_sum, nd.card_number
    steps = [("check", "awake"),
             _push(sel, total[sel], cn[sel]), ("check", "asleep"),
             _push(sel, np.zeros(sel.size), cn[sel]), ("check", "awake again"),
             _push(half, total[half], cn[half]),                # falls: the bounds go loose
             _push(other, np.zeros(other.size), cn[other]),     # rises: ... and dirty
             ("check", "fall and rise in one gap")]
    return nd, pd, steps


def cards(pods=BASE_PODS, nodes=BASE_NODES):
    """(c) CardNumber: 80 % of the nodes uploaded with CardNumber 1; half of those rise to 8,
    then the other 20 % fall to 0."""
    nd, pd = _base(pods, nodes)
    rng = np.random.default_rng(6)
    n = nd.n_nodes
    T = rng.random(n) < 0.8
    up = T & (rng.random(n) < 0.5)
    nd.card_number = nd.card_number.copy()
    nd.card_number[T] = 1
    iu, iz = np.flatnonzero(up), np.flatnonzero(~T)
    steps = [("check", "one card"),
             _push(iu, nd.alloc_memory[iu], np.full(iu.size, 8)), ("check", "rise to 8"),
             _push(iz, nd.alloc_memory[iz], np.zeros(iz.size)), ("check", "fall to 0")]
    return nd, pd, steps


def card_blocks(pods=BASE_PODS, nodes=BASE_NODES):
    """CardNumber 1 on every node of each third 64-node block of the upload order (the order a
    greedy batch walks), so those blocks are summarised with maximum 1; then all of them rise
    to 8.  Unlike `cards`, whole blocks change: a block maximum that did not widen makes K1
    call the block infeasible for every pod that asks for more than one card."""
    nd, pd = _base(pods, nodes)
    low = np.flatnonzero((np.arange(nd.n_nodes) // 64) % 3 == 0)
    nd.card_number = nd.card_number.copy()
    nd.card_number[low] = 1
    steps = [("check", "one card in whole blocks"),
             _push(low, nd.alloc_memory[low], np.full(low.size, 8)), ("check", "rise to 8")]
    return nd, pd, steps


WALK_SIZES = (64, 1, 700, 0, 7, "all", 700, 64, 7, 700)
WALK_EMPTY = 3      # index of the check after the count == 0 push
WALK_OUTSIDE = 6    # this push's list also holds ids at or beyond n_nodes


def _most_picked(nd, pd):
    """Node ids by how many pods pick them in this state, most first."""
    import oracle
    r = oracle.schedule(nd, pd, 0, threads=8)
    ids, cnt = np.unique(r.pick[r.status == 0], return_counts=True)
    return ids[np.argsort(-cnt, kind="stable")]


@functools.lru_cache(maxsize=None)
def walk(pods=BASE_PODS, nodes=BASE_NODES, seed=12, in_bytes=False):
    """(d) A seeded walk of pushes of 1, 7, 64, 700 and all nodes (the last through
    yoda_update_alloc), one empty, one with ids outside the snapshot; alloc drawn in
    [0, total] per listed node and CardNumber in 0..8 on a third of them.  Up to half of every
    list (at least one node) are the nodes most pods pick when the push is made (the oracle's
    picks on the model's state), so even a one-node push moves picks; the rest are drawn from
    all nodes.  Cached: the arrays are shared, do not write to them."""
    nd, pd = _base(pods, nodes)
    if in_bytes:
        nd, pd = synth.memory_in_bytes(nd, pd)
    rng = np.random.default_rng(seed)
    n = nd.n_nodes
    m = Model(nd)
    steps = []
    for k, size in enumerate(WALK_SIZES):
        if size == "all":
            alloc = (rng.random(n) * (nd.total_memory_sum.astype(np.float64) + 1)).astype(np.uint64)
            step = ("update_alloc", np.minimum(alloc, nd.total_memory_sum))
        else:
            ids = _most_picked(m.nodes(), pd)[:(size + 1) // 2] if size else np.zeros(0, np.int64)
            rest = np.setdiff1d(np.arange(n), ids)
            ids = rng.permutation(np.concatenate([ids, rng.choice(rest, size - ids.size,
                                                                  replace=False)]))
            total = nd.total_memory_sum[ids]
            alloc = np.minimum((rng.random(ids.size) * (total.astype(np.float64) + 1))
                               .astype(np.uint64), total)
            cn = m.card_number[ids].copy()
            third = rng.random(ids.size) < 1 / 3
            cn[third] = rng.integers(0, 9, int(third.sum())).astype(np.uint64)
            if k == WALK_OUTSIDE:  # ignored by contract: n_nodes, beyond it, and u32 max
                out = np.array([n, n + 5, n + 100000, 0xFFFFFFFF], np.uint64)
                at = rng.choice(ids.size, out.size, replace=False)
                ids = np.insert(ids.astype(np.uint64), at, out)
                alloc = np.insert(alloc, at, 0)
                cn = np.insert(cn, at, 8)
            step = _push(ids, alloc, cn)
        m.apply(step)
        steps += [step, ("check", f"walk {k}")]
    return nd, pd, steps


def mixed_fleet(pods=32768 + 37, nodes=BASE_NODES):
    """Half the nodes hold mixed GPU models; a wake push, a CardNumber rise and a fall.  The
    card data decide most picks on such a fleet, so half the woken nodes are the ones the first
    3000 pods pick while asleep (their scores rise above what any table built at upload holds),
    the other half random."""
    nd, pd = _base(pods, nodes)
    nd = synth.mixed_models(nd, 0.5)
    nd.alloc_memory = nd.total_memory_sum.copy()
    rng = np.random.default_rng(7)
    n = nd.n_nodes
    one = rng.random(n) < 0.6
    nd.card_number = nd.card_number.copy()
    nd.card_number[one] = 1
    sel = _most_picked(nd, pd.slice(0, min(3000, pd.n_pods)))[:75]
    sel = np.sort(np.concatenate([sel, rng.choice(np.setdiff1d(np.arange(n), sel),
                                                  150 - sel.size, replace=False)]))
    up = np.flatnonzero(one & (rng.random(n) < 0.5))
    down = np.flatnonzero(~one)
    steps = [_push(sel, np.zeros(sel.size), nd.card_number[sel]), ("check", "woken"),
             _push(up, _alloc_after(nd, sel, up), np.full(up.size, 8)), ("check", "rise to 8"),
             _push(down, _alloc_after(nd, sel, down), np.zeros(down.size)), ("check", "fall to 0")]
    return nd, pd, steps


def _alloc_after(nd, woken, ids):
    """The allocated memory of `ids` after the wake push (pushes carry both values)."""
    a = nd.alloc_memory.copy()
    a[woken] = 0
    return a[ids]
