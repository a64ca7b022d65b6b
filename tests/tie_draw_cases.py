"""Shared by test_tie_hash.py and test_gpu_tie_draw.py: the selectHost draw word of
include/yoda.h (yoda_set_tie_draw) restated in numpy, and the picks it implies, computed from
the oracle alone -- the tie set of a pod is read from oracle.pod_detail, never from libyoda."""
import numpy as np

import oracle

U64 = np.uint64
U32 = np.uint32
I64_MAX = (1 << 63) - 1


def mix64(x):
    """splitmix64 finalizer over uint64 arrays (mod 2^64)."""
    x = np.asarray(x, U64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(0xBF58476D1CE4E5B9)
        x ^= x >> U64(27)
        x *= U64(0x94D049BB133111EB)
        x ^= x >> U64(31)
    return x


def fmix32(h):
    """murmur3 32-bit finalizer over uint32 arrays (mod 2^32)."""
    h = np.asarray(h, U32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> U32(16)
        h *= U32(0x85EBCA6B)
        h ^= h >> U32(13)
        h *= U32(0xC2B2AE35)
        h ^= h >> U32(16)
    return h


def tie_hash(seed, pod, node):
    """yoda_tie_hash(seed, pod, node); pod and node broadcast against each other."""
    with np.errstate(over="ignore"):
        s = mix64(U64(seed & (2**64 - 1)) +
                  U64(0x9E3779B97F4A7C15) * (np.asarray(pod, U64) + U64(1)))
        lo = (s & U64(0xFFFFFFFF)).astype(U32)
        hi = (s >> U64(32)).astype(U32)
        return fmix32(fmix32(np.asarray(node, U32) ^ lo) + hi)


def draw(seed, pod, ids):
    """The member of the GLOBAL node ids `ids` that pod `pod` draws: argmin of hash << 32 | id."""
    ids = np.asarray(ids, U64)
    key = (tie_hash(seed, pod, ids.astype(U32)).astype(U64) << U64(32)) | ids
    return int(ids[np.argmin(key)])


def tie_set(nodes, pods, p, mode, n_ties):
    """Local indices of pod p's tie set from the oracle's per-node detail: the feasible nodes of
    the maximal raw score or, where NormalizeScore's (highest - lowest) * 100 overflows int64
    (scheduler.go:178), of the maximal normalized score.  Its size must be the oracle's n_ties."""
    _, feas, raw, norm = oracle.pod_detail(nodes, pods, p, mode)
    idx = np.flatnonzero(feas)
    r = [int(v) for v in raw[idx]]
    hi, lo = max(max(r), 0), min(r)  # highest starts at 0 (scheduler.go:160)
    if hi == lo:
        lo -= 1
    if hi - lo > I64_MAX // 100:
        v = norm[idx]
    else:
        v = raw[idx]
    members = idx[v == v.max()]
    assert members.size == n_ties, (p, members.size, n_ties)
    return members


def expected(nodes, pods, mode, seed, pod_base=0, node_offset=0, want=None):
    """(oracle result with GLOBAL picks and the draw-off rule, picks with the draw, tied pods)."""
    if want is None:
        want = oracle.schedule(nodes, pods, mode, threads=8)
    off = want.pick.copy()
    off[off >= 0] += node_offset
    on = off.copy()
    tied = np.flatnonzero((want.status == 0) & (want.n_ties >= 2))
    for p in tied:
        members = tie_set(nodes, pods, int(p), mode, int(want.n_ties[p]))
        on[p] = draw(seed, pod_base + int(p), members.astype(np.int64) + node_offset)
    return want, off, on, tied
