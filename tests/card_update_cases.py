"""Card-metric update scenarios as plain data (no fixtures): the snapshot as uploaded, the pods,
and the steps a long-lived handle would see between uploads.  tests/test_card_update_cases.py
checks with the oracle alone that every scenario moves enough picks or feasible counts to fail a
wrong handle; tests/test_gpu_card_update.py replays them on libyoda.

Each scenario returns (nodes, pods, steps); a step is one of
    ("cards", ids u32, free u64 [n, K], healthy u8 [n, K], free_sum u64 [n])
                                                    yoda_update_node_cards of that list (GLOBAL ids)
    ("push", ids u32, alloc u64, card_number u64)   yoda_set_node_state of that list
    ("check", tag)                                  compare the handle with the model here
Model applies the steps to numpy copies of the dynamic fields and returns the NodeSoA a fresh
upload of that state would get."""
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
        self.free = nodes.card_free_memory.copy()
        self.healthy = nodes.card_healthy.copy()
        self.free_sum = nodes.free_memory_sum.copy()

    def apply(self, step):
        n = self.base.n_nodes
        if step[0] == "cards":
            _, ids, free, healthy, fsum = step
            k = self.base.max_cards
            free, healthy = np.asarray(free).reshape(-1, k), np.asarray(healthy).reshape(-1, k)
            # ids outside the snapshot are ignored by contract; a repeated id keeps its last
            # entry; slots at or beyond the node's card count are ignored
            for t, i in enumerate(np.asarray(ids).tolist()):
                if i < n:
                    real = np.arange(k) < self.base.card_count[i]
                    self.free[i] = np.where(real, free[t], 0)
                    self.healthy[i] = np.where(real, healthy[t] != 0, 0)
                    self.free_sum[i] = fsum[t]
        elif step[0] == "push":
            _, ids, alloc, cn = step
            for i, a, c in zip(ids.tolist(), alloc.tolist(), cn.tolist()):
                if i < n:
                    self.alloc[i], self.card_number[i] = a, c
        elif step[0] != "check":
            raise ValueError(step[0])

    def nodes(self):
        m = self.base.slice(0, self.base.n_nodes)
        m.alloc_memory = self.alloc.copy()
        m.card_number = self.card_number.copy()
        m.card_free_memory = self.free.copy()
        m.card_healthy = self.healthy.copy()
        m.free_memory_sum = self.free_sum.copy()
        return m


def states(nodes, steps):
    """[(tag, NodeSoA)] of every check, in order."""
    m, out = Model(nodes), []
    for s in steps:
        m.apply(s)
        if s[0] == "check":
            out.append((s[1], m.nodes()))
    return out


def _cards(ids, free, healthy, fsum):
    return ("cards", np.asarray(ids, np.uint32), np.ascontiguousarray(free, np.uint64),
            np.ascontiguousarray(healthy, np.uint8), np.asarray(fsum, np.uint64))


def _most_picked(nd, pd):
    """Node ids by how many pods pick them in this state, most first."""
    import oracle
    r = oracle.schedule(nd, pd, 0, threads=8)
    ids, cnt = np.unique(r.pick[r.status == 0], return_counts=True)
    return ids[np.argsort(-cnt, kind="stable")]


def _real(nd, ids):
    return np.arange(nd.max_cards)[None, :] < nd.card_count[ids][:, None]


def _free_pool(nd):
    """The snapshot's distinct card-free values (what a rank table can hold)."""
    real = np.arange(nd.max_cards)[None, :] < nd.card_count[:, None]
    return np.unique(nd.card_free_memory[real])


def _draw(rng, m, ids, pool=None, flip=0.2):
    """New dynamic metrics of `ids`: every real card's free in [0, total] (from `pool` when
    given), health flipped on a share `flip` of the real cards, the sum of the frees."""
    nd = m.base
    real = _real(nd, ids)
    total = nd.card_total_memory[ids]
    if pool is None:
        free = np.minimum((rng.random(total.shape) * (total.astype(np.float64) + 1))
                          .astype(np.uint64), total)
    else:  # a pool value at most the total where there is one, else the smallest
        hi = np.maximum(np.searchsorted(pool, total, side="right"), 1)
        free = pool[(rng.random(total.shape) * hi).astype(np.int64)]
    free = np.where(real, free, 0).astype(np.uint64)
    healthy = (m.healthy[ids] != 0) ^ ((rng.random(total.shape) < flip) & real)
    return free, (healthy & real).astype(np.uint8), free.sum(axis=1, dtype=np.uint64)


SHAPES = ("base", "small", "mixed", "c4", "ranks", "f64", "u64")
UPLOAD_KW = {"f64": {"force_f64": True}, "u64": {"force_generic": True}}


def shape_workload(shape, mixed_pods=32768 + 37):
    """(nodes, pods) of a walk shape.  mixed: half the nodes hold mixed GPU models; the grouped
    node order needs >= 32768 pods there (the oracle-only tests pass fewer)."""
    if shape == "base" or shape == "ranks":
        nd, pd = synth.make_config(3, pods=BASE_PODS, nodes=BASE_NODES)
        if shape == "ranks":
            nd, pd = synth.memory_in_bytes(nd, pd)
    elif shape == "small":
        nd, pd = synth.make_config(3, pods=700, nodes=900)
    elif shape == "mixed":
        nd, pd = synth.make_config(3, pods=mixed_pods, nodes=BASE_NODES)
        nd = synth.mixed_models(nd, 0.5)
    elif shape == "c4":  # K = 16, empty CardLists, CardNumber != len(CardList)
        nd, pd = synth.make_config(4, pods=1500, nodes=BASE_NODES)
    elif shape in ("f64", "u64"):
        nd, pd = synth.make_config(3, pods=600, nodes=1500)
    else:
        raise ValueError(shape)
    return nd, pd


WALK_SIZES = (64, 1, 700, 0, 7, "push", 64, 700)
WALK_EMPTY = 3     # index of the check after the count == 0 list
WALK_PUSH = 5      # a push of alloc and CardNumber; the card list after it names the same nodes
WALK_OUTSIDE = 7   # this list also holds ids at or beyond n_nodes and repeated ids


@functools.lru_cache(maxsize=None)
def walk(shape="base", seed=21, mixed_pods=32768 + 37):
    """(a) A seeded walk of card updates of 1, 7, 64 and 700 nodes, one empty, one with ids
    outside the snapshot and repeated ids, and one push of alloc and CardNumber on the nodes of
    the card list after it.  Half of every list (at least one node) are the nodes most pods pick
    when the update is made (the oracle's picks on a sample of the pods), the rest random.
    ranks: the new frees are values the snapshot's cards already hold.  Cached: the arrays are
    shared, do not write to them."""
    nd, pd = shape_workload(shape, mixed_pods)
    rng = np.random.default_rng(seed)
    n = nd.n_nodes
    pool = _free_pool(nd) if shape == "ranks" else None
    sample = pd.slice(0, min(pd.n_pods, 3000))
    m = Model(nd)
    steps = []

    def choose(size):
        ids = _most_picked(m.nodes(), sample)[:(size + 1) // 2] if size else np.zeros(0, np.int64)
        rest = np.setdiff1d(np.arange(n), ids)
        return rng.permutation(np.concatenate([ids, rng.choice(rest, size - ids.size,
                                                               replace=False)]))

    for k, size in enumerate(WALK_SIZES):
        if size == "push":
            ids = pushed = choose(WALK_SIZES[k + 1])
            total = nd.total_memory_sum[ids]
            alloc = np.minimum((rng.random(ids.size) * (total.astype(np.float64) + 1))
                               .astype(np.uint64), total)
            cn = rng.integers(0, 9, ids.size).astype(np.uint64)
            step = ("push", ids.astype(np.uint32), alloc, cn)
        else:
            ids = pushed if k == WALK_PUSH + 1 else choose(size)
            free, healthy, fsum = _draw(rng, m, ids, pool)
            if k == WALK_OUTSIDE:
                # ignored by contract: n_nodes, beyond it, and u32 max; and 40 ids listed twice,
                # first with other values (another listed node's frees, every card unhealthy,
                # sum 0), their real entry last
                out = np.array([n, n + 5, n + 100000, 0xFFFFFFFF], np.uint64)
                at = rng.choice(ids.size, out.size, replace=False)
                ids2 = np.insert(ids.astype(np.uint64), at, out)
                free2 = np.insert(free, at, 7, axis=0)
                healthy2 = np.insert(healthy, at, 1, axis=0)
                fsum2 = np.insert(fsum, at, 7)
                rep = rng.choice(ids.size, 40, replace=False)
                other = np.where(_real(nd, ids[rep]), free[(rep + 1) % free.shape[0]], 0)
                ids = np.concatenate([ids[rep].astype(np.uint64), ids2])
                free = np.concatenate([other.astype(np.uint64), free2])
                healthy = np.concatenate([np.zeros_like(healthy[rep]), healthy2])
                fsum = np.concatenate([np.zeros_like(fsum[rep]), fsum2])
            step = _cards(ids, free, healthy, fsum)
        m.apply(step)
        steps += [step, ("check", f"walk {k}")]
    return nd, pd, steps


def block_drain(nodes=BASE_NODES, pods=BASE_PODS):
    """(b) Every 64-node block with block % 3 == 1 starts with every free 0; it is filled to its
    totals with every card healthy, then drained again.  Whole blocks change: a block summary
    that did not follow makes K1 rule the block out (or in) for a whole wave."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    ids = np.flatnonzero((np.arange(nd.n_nodes) // 64) % 3 == 1)
    nd.card_free_memory = nd.card_free_memory.copy()
    nd.free_memory_sum = nd.free_memory_sum.copy()
    nd.card_free_memory[ids] = 0
    nd.free_memory_sum[ids] = 0
    real = _real(nd, ids)
    total = np.where(real, nd.card_total_memory[ids], 0).astype(np.uint64)
    zero = np.zeros_like(total)
    steps = [("check", "drained at upload"),
             _cards(ids, total, real, total.sum(axis=1, dtype=np.uint64)), ("check", "filled"),
             _cards(ids, zero, real, zero.sum(axis=1, dtype=np.uint64)), ("check", "drained")]
    return nd, pd, steps


def free_maximum(nodes=BASE_NODES, pods=BASE_PODS):
    """(c) One card of one node -- the node most pods pick -- rises 1,000 above the largest
    card free of the fleet, then returns: the G maximum of FreeMemory moves up and back."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    i = int(_most_picked(nd, pd)[0])
    top = nd.card_free_memory.max() + np.uint64(1000)
    free = nd.card_free_memory[[i]].copy()
    j = int(np.argmax(nd.card_healthy[i] != 0))
    free[0, j] = top
    steps = [("check", "as uploaded"),
             _cards([i], free, nd.card_healthy[[i]], free.sum(axis=1, dtype=np.uint64)),
             ("check", "raised"),
             _cards([i], nd.card_free_memory[[i]], nd.card_healthy[[i]], nd.free_memory_sum[[i]]),
             ("check", "restored")]
    return nd, pd, steps


def health_only(nodes=BASE_NODES, pods=BASE_PODS, listed=700, share=0.5):
    """(d) Health flipped on a share of the real cards of `listed` nodes (half of them the most
    picked ones), frees and sums unchanged."""
    nd, pd = synth.make_config(3, pods=pods, nodes=nodes)
    rng = np.random.default_rng(31)
    ids = _most_picked(nd, pd)[:listed // 2]
    ids = np.concatenate([ids, rng.choice(np.setdiff1d(np.arange(nd.n_nodes), ids),
                                          listed - ids.size, replace=False)])
    real = _real(nd, ids)
    healthy = ((nd.card_healthy[ids] != 0) ^ ((rng.random(real.shape) < share) & real)) & real
    steps = [("check", "as uploaded"),
             _cards(ids, nd.card_free_memory[ids], healthy, nd.free_memory_sum[ids]),
             ("check", "health flipped")]
    return nd, pd, steps


def rejected():
    """(e) The ranks shape and a five-node list whose LAST entry holds a free value that no card
    of the snapshot has: the rank table cannot hold it."""
    nd, pd = shape_workload("ranks")
    pool = _free_pool(nd)
    ids = np.array([5, 70, 900, 2000, 4000], np.uint32)
    free = nd.card_free_memory[ids][:, ::-1].copy()  # the first four: the nodes' own values
    real = _real(nd, ids)
    free = np.where(real, free, 0).astype(np.uint64)
    alien = np.uint64(pool[len(pool) // 2]) + np.uint64(1)
    while alien in pool:
        alien += np.uint64(1)
    free[-1, 0] = alien
    return nd, pd, _cards(ids, free, nd.card_healthy[ids], free.sum(axis=1, dtype=np.uint64))
