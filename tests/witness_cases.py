"""Inputs and the reference for the PreScore maxima witnesses of a capacity greedy window
(yoda_shard_phase1_witness, include/yoda.h) as plain data (no fixtures).
tests/test_witness_cases.py checks the reference against the oracle and a brute-force loop, and
that every input can fail a wrong kernel; tests/test_gpu_witness.py compares libyoda with it.

A witness of a MaxValue field (collection.go:14-21) is a feasible node (filter.go:11-58) with a
qualifying card (collection.go:46: FreeMemory >= scv/memory and Clock >= scv/clock, no health
check) whose largest value of the field over its qualifying cards equals the pod's maximum."""
import functools

import numpy as np

from yoda_amd import synth

NONE = 0xFFFFFFFF  # wit_node of a field no node contributes to
FREE = 3           # the FreeMemory row (MaxValue order: bandwidth, clock, core, free, power, total)
SMALL = (0, 1, 2, 4)  # the per-model fields: bandwidth, clock, core, power


def _fields(nodes):
    return (nodes.card_bandwidth, nodes.card_clock, nodes.card_core, nodes.card_free_memory,
            nodes.card_power, nodes.card_total_memory)  # MaxValue order


def reference(nodes, pods, lo=0, hi=None):
    """For the nodes [lo, hi) of the snapshot, GLOBAL ids: a dict of n_feasible [P],
    n_zero_total [P] (feasible nodes with TotalMemorySum == 0), maxima [6, P] (floor 1),
    wit_count [6, P] and wit_node [6, P] (the lowest witness; NONE without one).  Plain numpy
    over the card arrays; pods with the same request are evaluated once."""
    hi = nodes.n_nodes if hi is None else hi
    P, n = pods.n_pods, hi - lo
    K = nodes.card_free_memory.shape[1]
    out = {"n_feasible": np.zeros(P, np.uint32), "n_zero_total": np.zeros(P, np.uint32),
           "maxima": np.ones((6, P), np.uint64), "wit_count": np.zeros((6, P), np.uint32),
           "wit_node": np.full((6, P), NONE, np.uint32)}
    if P == 0 or n <= 0:
        return out
    real = np.arange(K)[None, :] < np.asarray(nodes.card_count[lo:hi], np.int64)[:, None]
    healthy = real & (np.asarray(nodes.card_healthy[lo:hi]) != 0)
    free = np.asarray(nodes.card_free_memory[lo:hi], np.uint64)
    clock = np.asarray(nodes.card_clock[lo:hi], np.uint64)
    cn = np.asarray(nodes.card_number[lo:hi], np.uint64)
    zero_total = np.asarray(nodes.total_memory_sum[lo:hi], np.uint64) == 0
    fields = [np.asarray(a[lo:hi], np.uint64) for a in _fields(nodes)]
    ids = np.arange(lo, hi, dtype=np.int64)
    seen = {}
    for p in range(P):
        key = (int(pods.has_number[p]), int(pods.number[p]) if pods.has_number[p] else 0,
               int(pods.has_memory[p]), int(pods.memory[p]) if pods.has_memory[p] else 0,
               int(pods.has_clock[p]), int(pods.clock[p]) if pods.has_clock[p] else 0)
        if key not in seen:
            hn, number, hm, m, hc, c = key
            m64, c64 = np.uint64(m), np.uint64(c)
            # filter.go:11-16: without scv/number CardNumber > 0, and one card is needed
            feas = (np.uint64(number) <= cn) if hn else (cn > 0)
            need = number if hn else 1
            if hm:  # filter.go:18-33, 52-54: healthy cards with FreeMemory >= scv/memory
                feas = feas & ((healthy & (free >= m64)).sum(axis=1) >= need)
            if hc:  # filter.go:35-50, 56-58: healthy cards with Clock == scv/clock
                feas = feas & ((healthy & (clock == c64)).sum(axis=1) >= need)
            q = real & (free >= m64) & (clock >= c64) & feas[:, None]  # collection.go:41-46
            anyq = q.any(axis=1)
            mx, wc, wn = [1] * 6, [0] * 6, [NONE] * 6
            for f, arr in enumerate(fields):
                contrib = np.where(q, arr, np.uint64(0)).max(axis=1)
                mx[f] = max(1, int(contrib.max()))
                hit = anyq & (contrib == np.uint64(mx[f]))
                wc[f] = int(hit.sum())
                if wc[f]:
                    wn[f] = int(ids[hit].min())
            seen[key] = (int(feas.sum()), int((feas & zero_total).sum()), mx, wc, wn)
        nf, nz, mx, wc, wn = seen[key]
        out["n_feasible"][p], out["n_zero_total"][p] = nf, nz
        out["maxima"][:, p], out["wit_count"][:, p], out["wit_node"][:, p] = mx, wc, wn
    return out


def merged(parts):
    """The shards' references merged as dist.merge_witness merges the device buffers: maxima
    MAX, counts SUM, and of the shards that reach a field's global maximum the witness counts
    SUM and the lowest nodes MIN."""
    mx = np.maximum.reduce([r["maxima"] for r in parts])
    wc = sum(np.where(r["maxima"] == mx, r["wit_count"], 0).astype(np.uint32) for r in parts)
    wn = np.minimum.reduce([np.where(r["maxima"] == mx, r["wit_node"], NONE).astype(np.uint32)
                            for r in parts])
    return {"n_feasible": sum(r["n_feasible"] for r in parts),
            "n_zero_total": sum(r["n_zero_total"] for r in parts),
            "maxima": mx, "wit_count": wc, "wit_node": wn}


# ---- inputs (seeded; cached: the arrays are shared, do not write to them) -------------------
@functools.lru_cache(maxsize=None)
def base(P, N):
    return synth.make_config(2, pods=P, nodes=N)


def tied_ids(N):
    """The nodes tied_free makes identical: they straddle lanes, 64-node blocks and chunks."""
    ids = {0, 63, 64, 127, N // 2, N - 65, N - 64, N - 1}
    return np.array(sorted(i for i in ids if 0 <= i < N), np.int64)


_NODE_FIELDS = ("card_number", "card_count", "free_memory_sum", "total_memory_sum",
                "alloc_memory", "card_free_memory", "card_total_memory", "card_clock",
                "card_bandwidth", "card_core", "card_power", "card_healthy", "cpu", "disk_io")


@functools.lru_cache(maxsize=None)
def tied_free(P, N):
    """base with the nodes tied_ids(N) made copies of one node of the largest TotalMemory model,
    every card healthy and FreeMemory = TotalMemory, so the FreeMemory maximum is tied between
    them; CardNumber 1, 2, 4, 8 in turn, so the tie has another size for every scv/number."""
    nodes, pods = base(P, N)
    nodes = synth._copy(nodes)
    donor = int(np.argmax(nodes.card_total_memory[:, 0]))  # the first node of the largest model
    row = {f: np.array(getattr(nodes, f)[donor]) for f in _NODE_FIELDS}
    ids = tied_ids(N)
    for k, i in enumerate(ids):
        for f in _NODE_FIELDS:
            getattr(nodes, f)[i] = row[f]
        real = np.arange(nodes.max_cards) < nodes.card_count[i]
        nodes.card_healthy[i] = real.astype(np.uint8)
        nodes.card_free_memory[i] = nodes.card_total_memory[i]
        nodes.card_number[i] = (1, 2, 4, 8)[k % 4]
        nodes.free_memory_sum[i] = nodes.card_free_memory[i].sum(dtype=np.uint64)
    return nodes.normalized(), pods


@functools.lru_cache(maxsize=None)
def wide_chunks(P, N, requests=300):
    """A batch of many pod blocks (P pods repeating `requests` distinct requests), for which the
    witness K1 takes node chunks of several 64-node blocks, over base nodes where node 1 and
    the whole block 64..127 are copies of the tied_free donor.  For most waves block 1 is
    decided as a whole and node 1 one by one, inside an undecided block: the lowest FreeMemory
    witness is a single node folded AFTER a block of higher ids that ties with it."""
    nodes, pods = base(requests, N)
    tied, _ = tied_free(requests, N)
    nodes = synth._copy(nodes)
    donor = int(tied_ids(N)[0])
    for i in [1] + list(range(64, 128)):
        for f in _NODE_FIELDS:
            getattr(nodes, f)[i] = getattr(tied, f)[donor]
        nodes.card_number[i] = 8
    return nodes.normalized(), pods.take(np.resize(np.arange(requests), P))


@functools.lru_cache(maxsize=None)
def tied_top(P, N, copies=128):
    """tied_free with its first `copies` nodes (two 64-node chunks) all copies of the donor,
    CardNumber 8: for every pod they fit they are the best nodes and tie, so a chunk's list
    leaves tied nodes out and a deep list must end where such a node could enter; the pods they
    do not fit (another scv/clock) keep lists as long as their feasible sets."""
    nodes, pods = tied_free(P, N)
    nodes = synth._copy(nodes)
    donor = int(tied_ids(N)[0])
    for i in range(min(copies, N)):
        for f in _NODE_FIELDS:
            getattr(nodes, f)[i] = getattr(nodes, f)[donor]
        nodes.card_number[i] = 8
    return nodes.normalized(), pods


@functools.lru_cache(maxsize=None)
def mixed(P, N):
    """tied_free with half the nodes holding mixed GPU models: not every node is one model, so
    the witness phase 1 runs the per-node k1_witness<N32>, both of its branches."""
    nodes, pods = tied_free(P, N)
    return synth.mixed_models(nodes, 0.5), pods


@functools.lru_cache(maxsize=None)
def het(P, N):
    """Config 4: K = 16, card_count != CardNumber on 1 % of the nodes, nodes without cards, and
    requests most nodes fail."""
    return synth.make_config(4, pods=P, nodes=N)


@functools.lru_cache(maxsize=None)
def no_qualifying(P, N):
    """base plus nodes without any card (feasible for a pod without scv/memory and scv/clock,
    contributing nothing), half of them with TotalMemorySum 0, and pods with neither label and
    scv/number absent, 1, 8 and 9.  The cardless nodes hold CardNumber 9, one more than every
    other node: a pod asking for 9 is feasible on them alone, so each of its maxima stays 1."""
    nodes, pods = base(P, N)
    nodes, pods = synth._copy(nodes), synth._copy(pods)
    rng = np.random.default_rng(21)
    empty = np.sort(rng.choice(N, min(N, max(1, min(12, N // 8))), replace=False))
    nodes.card_count[empty] = 0
    nodes.card_number[empty] = 9
    nodes.free_memory_sum[empty] = 0
    nodes.total_memory_sum[empty[::2]] = 0
    plain = rng.choice(P, min(P, 9), replace=False)
    pods.has_memory[plain] = 0
    pods.memory[plain] = 0
    pods.has_clock[plain] = 0
    pods.clock[plain] = 0
    for k, p in enumerate(plain):
        kind = k % 4  # absent, 1, 8, and 9: only the cardless nodes hold 9
        pods.has_number[p] = 0 if kind == 0 else 1
        pods.number[p] = (0, 1, 8, 9)[kind]
    return nodes.normalized(), pods.normalized()


def decrement(nodes, seed, count=100, always=None):
    """A yoda_set_node_state push that lowers CardNumber of about `count` nodes -- every node of
    `always` (default: the tied nodes) and random others with CardNumber > 0 -- to a value
    drawn from below the old one, 0 included; the allocation stays.  Returns (ids u32, alloc
    u64, card_number u64, the snapshot after the push)."""
    rng = np.random.default_rng(seed)
    N = nodes.n_nodes
    always = tied_ids(N) if always is None else np.asarray(always, np.int64)
    rest = np.setdiff1d(np.flatnonzero(nodes.card_number > 0), always)
    more = rng.choice(rest, min(rest.size, max(0, count - always.size)), replace=False)
    ids = np.concatenate([always, more]).astype(np.int64)
    ids = rng.permutation(ids[nodes.card_number[ids] > 0])
    old = nodes.card_number[ids].astype(np.int64)
    new = (rng.random(ids.size) * old).astype(np.int64)  # uniform in [0, old)
    after = synth._copy(nodes)
    after.card_number[ids] = new.astype(np.uint64)
    return (ids.astype(np.uint32), np.array(nodes.alloc_memory[ids], np.uint64),
            new.astype(np.uint64), after.normalized())
