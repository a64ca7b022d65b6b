"""Many-model fleets for the score quotients x*100/M of CalculateCardScore (bandwidth, clock /
MaxBandwidth, core, power, total memory), as plain seeded data: no fixtures, no GPU.
tests/test_quotient_cases.py shows with the oracle alone that these fleets fail a wrong kernel;
tests/test_gpu_quotients.py runs them through every entry point of libyoda.

Construction.  A tier has, per field, an ascending list of maxima M_0 < M_1 < ... (its "levels"):
a divisor chain M_i | M_j, most members multiples of 100 with an odd factor, plus the tier's own
edge values (55738; 55739, 65535 and five small bandwidths; 78599 and 0xFFFFFFFE).  Nodes fall into clock groups; a group
sits on one level l, three of its nodes hold that level's maxima (x = M_l, every card healthy and
as free as the level allows) and the others, on l or any level below, take x <= M_l around an
integer quotient of a maximum M_j, j in l .. l + 3: floor((k*M - 1)/100) (x*100 % M >= M - 100:
a reciprocal rounded up too far gives k), k*M/100 where that is an integer (a reciprocal rounded
down gives k - 1), the values next to both, k spread over 1..100, and 0, 1.  Along the chain such
an x sits on the same edge of every M_i below M_j too, so it meets several of the maxima it is
scored against.  The higher a level, the less free memory its cards have: a pod's scv/memory
decides which level is the highest still feasible (a staircase of maxima), its scv/clock selects
one group with that group's maxima.  The clocks come from a search over 0..cap for values that
are exact or near-integer quotients of many bandwidth levels at once (clock*100/MaxBandwidth is
not bounded by 100: k goes far beyond 100 against the small bandwidth levels).  Total memory has
a level of its own per group.  Pods: scv/clock at the groups' clocks (a few one off), scv/memory
at card frees and frees +-1, a tenth without any label.  ~5 % unhealthy cards, short and empty
CardLists, CardNumber 0 and off the list's length.

predict_format restates choose_format (csrc/yoda_capi.cpp) so that a tier's declared record path
is checked on the CPU as well as on the device.  Where it corrects what one might expect: memory
fields of 2^44 alone keep N32 (memory ranks), so `field44` holds a two-model node with a 17-bit
bandwidth to reach the F64 kernels with fields of exactly 2^44; an empty CardList is not "one
model", so the tiers that need one-model snapshots (pack16, wide, score32) have short lists but
no empty ones; and in `score32` no sum can reach 2^32 (16 * (800 + 268,434,600) = 4,294,966,400
is the largest the bound admits), it is its twin with one more clock whose sums pass 2^32.

Figures of the CPU run (tests/test_quotient_cases.py -s): per tier and field the distinct scored
(x, M) pairs (exact quotients / near-integer quotients / f32 quotient wrong):
    q32          bandwidth 5236 (749/835/0)  clock 2637 (752/894/0)  core 5914 (777/855/0)
                 power 4942 (717/858/0)  total 1422 (383/349)
    q32_grouped  bandwidth 5635 (727/865/0)  clock 602 (203/224/0)  core 5936 (751/810/0)
                 power 4979 (690/820/0)  total 1857 (544/566)
    q32_mixed    bandwidth 4806 (717/772/0)  clock 3272 (936/1322/0)  core 5452 (733/824/0)
                 power 4473 (695/765/0)  total 962 (246/203)
    ranks        bandwidth 5236 (749/835/0)  clock 2637 (752/894/0)  core 5913 (777/855/0)
                 power 4942 (717/858/0)  total 1457 (385/332)
    pack16       bandwidth 5130 (548/878/0)  clock 2606 (481/705/37)  core 5199 (636/718/0)
                 power 5764 (760/848/0)  total 1174 (364/307)
    wide         bandwidth 5516 (583/700/680)  clock 635 (149/183/230)  core 5406 (622/711/745)
                 power 4982 (584/695/679)  total 1318 (501/443)
wide: 2334 scored pairs with a wrong f32 quotient; 10 of the first 48 scheduled pods change their
pick or top score under f32 quotients.  pack16: for x <= M <= 65535 no f32 quotient is wrong, but
clock / MaxBandwidth has x > M: a search over every M <= 65535 and every x in 55739..65535 finds
96 values of M with failing x (47: 84 of them, 49: 26, 367: 15, 369: 14, 193: 11, ...).  The tier
holds those five as bandwidth levels with failing clocks on them: 37 scored pairs with a wrong
f32 quotient, and all 55 scheduled pods that ask for such a clock change their top score."""
import functools
from collections import namedtuple

import numpy as np

from yoda_amd.soa import NodeSoA, PodSoA

F32_SMALL_MAX = 55738          # kF32SmallMax
PACK16_MAX = 0xFFFF            # kPack16Max
N32_FIELD_MAX = 0xFFFFFFFE     # kN32FieldMax
FAST_FIELD_MAX = 1 << 44       # kFastFieldMax
FAST_SCORE_MAX = 1 << 52       # kFastScoreMax
SMALL = ("bandwidth", "clock", "core", "power")
FIELDS = ("bandwidth", "clock", "core", "power", "total")   # the five x*100/M quotients
MAXIMA_COL = {"bandwidth": 0, "clock": 0, "core": 2, "power": 4, "total": 5}  # clock / MaxBandwidth

Tier = namedtuple("Tier", "name nodes pods path flags")
BIG_N, BIG_P = 4700, 600
SMALL_N, SMALL_P = 65, 130


# ---- the f32 quotient of the block K2, emulated ------------------------------------------------
def ru32(M):
    """The smallest float32 >= 100/M (exact test of r*M < 100 in long double: 24 + 32 bits)."""
    M = np.asarray(M, np.uint64)
    r = (np.float64(100.0) / M.astype(np.float64)).astype(np.float32)
    low = r.astype(np.longdouble) * M.astype(np.longdouble) < np.longdouble(100.0)
    return np.where(low, np.nextafter(r, np.float32(np.inf)), r).astype(np.float32)


def rn32(M):
    """100/M rounded to the nearest float32: the wrong reciprocal."""
    return (np.float64(100.0) / np.asarray(M, np.uint64).astype(np.float64)).astype(np.float32)


def quot32(x, M, recip=ru32):
    """floor(fl32(fl32(x) * recip(M)))."""
    x = np.asarray(x, np.uint64)
    return np.floor(x.astype(np.float32) * recip(M)).astype(np.uint64)


def quot64_nearest(x, M):
    """floor(fl64(x * RN64(100/M))): the wrong reciprocal of the f64 quotients."""
    x, M = np.asarray(x, np.uint64), np.asarray(M, np.uint64)
    return np.floor(x.astype(np.float64) * (np.float64(100.0) / M.astype(np.float64))).astype(
        np.uint64)


def near_values(M, k):
    """The six values around the k-th integer quotient of M."""
    a, b = (k * M - 1) // 100, -((-k * M) // 100)
    return [a - 1, a, a + 1, b - 1, b, b + 1]


def f32_failing(M, xmax=None):
    """The x <= xmax (default M) around integer quotients of M whose f32 quotient is wrong."""
    xmax = M if xmax is None else xmax
    kmax = max(1, min(100 * xmax // max(M, 1) + 1, 400))
    ks = np.arange(1, kmax + 1, dtype=object)
    cand = set()
    for k in ks:
        cand.update(v for v in near_values(M, int(k)) if 0 <= v <= xmax)
    x = np.array(sorted(cand), np.uint64)
    if x.size == 0:
        return x
    bad = quot32(x, np.full(x.size, M, np.uint64)) != x * np.uint64(100) // np.uint64(M)
    return x[bad]


# ---- choose_format, restated -------------------------------------------------------------------
def predict_format(nodes, force_f64=False, force_generic=False, no_uniform=False,
                   mem_ranks=False, f64_quotients=False, per_node_k1=False, per_node_k2=False,
                   no_gtab=False):
    """(path, small_field_max, memory_ranks, node_order_grouped) as choose_format and
    grouped_node_order (csrc/yoda_capi.cpp) decide them, in Python integers."""
    nd = nodes.normalized()
    K = 1
    while K < max(int(nd.card_count.max()) if nd.n_nodes else 1, 1):
        K *= 2                                   # card slots: 1, 2, 4, 8 or 16
    real = np.arange(nd.max_cards)[None, :] < nd.card_count[:, None]
    small = [getattr(nd, "card_" + f) for f in SMALL]
    mem = [nd.card_free_memory, nd.card_total_memory]
    mx = lambda arrs: max([int(a[real].max()) for a in arrs if real.any()] + [0])  # noqa: E731
    max_small, max_mem = mx(small), mx(mem)
    max_field, max_clock = max(max_small, max_mem), mx([nd.card_clock])
    ck = nd.card_clock[real].astype(object)
    bw = np.maximum(nd.card_bandwidth[real], 1).astype(object)
    max_ckq = max([int(c) * 100 // int(b) for c, b in zip(ck, bw) if c <= N32_FIELD_MAX] + [0])
    one = nd.card_count > 0
    for a in small + [nd.card_total_memory]:
        one &= (np.where(real, a, a[:, :1]) == a[:, :1]).all(axis=1)
    all_one = bool(one.all()) and not no_uniform
    tot, fre, alloc = (a.astype(object) for a in
                       (nd.total_memory_sum, nd.free_memory_sum, nd.alloc_memory))
    stat = [(0 if t < a else (t - a) * 100 // t * 3) + f * 100 // t * 2 if t else 0
            for t, f, a in zip(tot, fre, alloc)]
    score_bound = K * (800 + 100 * max_clock) + max(stat + [0])
    f64_ok = max_field <= FAST_FIELD_MAX and score_bound < FAST_SCORE_MAX
    q32 = max_small <= F32_SMALL_MAX and not f64_quotients
    n32_ok = (f64_ok and max_small <= N32_FIELD_MAX and (q32 or all_one) and
              K * (800 + max_ckq) < (1 << 32))
    path = "n32" if n32_ok else ("f64" if f64_ok else "u64")
    if force_f64 and path == "n32":
        path = "f64"
    if force_generic:
        path = "u64"
    ranks = path == "n32" and (max_mem > N32_FIELD_MAX or mem_ranks)
    uni4 = nd.card_count > 0
    for a in small:
        uni4 &= (np.where(real, a, a[:, :1]) == a[:, :1]).all(axis=1)
    keys = set(nd.card_clock[uni4, 0].tolist()) | ({-1} if (~uni4).any() else set())
    grouped = (path == "n32" and nd.n_nodes >= 4096 and len(keys) <= 64 and
               not (per_node_k1 or per_node_k2))
    return path, max_small, ranks, grouped


# ---- the generator -----------------------------------------------------------------------------
def _chain(base, factors, extra=()):
    """An ascending divisor chain base, base*f0, base*f0*f1, ... plus the maxima `extra`.  Along
    a chain M_i | M_j a value x that is an exact or a near-integer quotient of M_j (100 x % M_j
    == 0, or >= M_j - 100) is one of every M_i below it too, so one node's x sits on the
    rounding edge of several of the maxima that pods see it scored against."""
    out, v = [base], base
    for f in factors:
        v *= f
        out.append(v)
    return sorted(set(out) | set(extra))


def _draw_x(rng, levels, lev, size, fail=None, top_share=0.0, fail_share=0.35, exact_share=0.4):
    """`size` values <= levels[lev] around integer quotients of a level j in lev .. lev + 3:
    a share exact_share k M/100 exact, 40 % floor((k M - 1)/100), the rest the values next to
    them; 3 % are 0 or 1.  top_share: the share aimed at the last level instead.  `fail`: per
    level the f32-failing values, taken with probability fail_share where there are any."""
    L, cap = len(levels), levels[lev]
    out = np.zeros(size, np.uint64)
    for t in range(size):
        j = min(L - 1, lev + int(rng.choice(4, p=(0.15, 0.2, 0.3, 0.35))))
        if rng.random() < top_share and 100 * cap // levels[-1] >= 2:
            j = L - 1
        M = levels[j]
        u = rng.random()
        if fail is not None and u < fail_share:
            pool = fail[j][fail[j] <= cap]
            if pool.size:
                out[t] = pool[int(rng.integers(pool.size))]
                continue
        if u > 0.97:
            out[t] = int(rng.integers(0, 2))
            continue
        kmax = max(1, min(100, 100 * cap // M))
        k = int(rng.integers(1, kmax + 1))
        v = rng.random()
        if v < exact_share:
            step = 100 // int(np.gcd(M, 100))
            k = min(max(step, k - k % step), 100)
            x = k * M // 100
        elif v < exact_share + 0.40:
            x = (k * M - 1) // 100
        else:
            x = near_values(M, k)[int(rng.integers(6))]
        out[t] = min(max(x, 0), cap)
    return out


def _choose_clocks(rng, bw_levels, cap, count, keep):
    """`count` distinct clocks <= cap: `keep`, then values that are an exact (100 c % M == 0) or a
    near-integer (100 c % M >= M - 100) quotient of many bandwidth levels at once (a search over
    0..cap, or over quotient candidates beyond 2^20), then values around single quotients."""
    if cap <= (1 << 20):
        c = np.arange(cap + 1, dtype=np.uint64)
    else:
        cand = {cap}
        for M in bw_levels:
            for k in range(1, 2000, 7):
                cand.update(v for v in near_values(M, k) if 0 <= v <= cap)
        c = np.array(sorted(cand), np.uint64)
    exact = np.zeros(c.size, np.int64)
    near = np.zeros(c.size, np.int64)
    for M in bw_levels:
        r = c * np.uint64(100) % np.uint64(M)
        exact += r == 0
        near += (r + np.uint64(100) >= np.uint64(M)) & (r != 0)
    chosen = list(dict.fromkeys(int(v) for v in keep))
    for score in (near, exact, near + exact):
        order = np.argsort(-score, kind="stable")[:max(4 * count, 64)]
        pick = rng.permutation(order)[:count // 4]
        chosen += [int(c[i]) for i in pick]
    chosen = list(dict.fromkeys(chosen))[:count]
    while len(chosen) < count:
        M = bw_levels[int(rng.integers(len(bw_levels)))]
        k = int(rng.integers(1, max(2, 100 * cap // M)))
        v = min(max(near_values(M, k)[int(rng.integers(6))], 0), cap)
        if v not in chosen:
            chosen.append(int(v))
    return np.array(chosen, np.uint64)


HOLDERS = 3   # nodes per clock group that hold its level's maxima


def make_fleet(seed, n, K, levels, clocks, free_caps, mixed=0.0, empty=0.02, short=0.05,
               fail=None, mixed_total=0.08, min_bw_per_clock=0, fail_share=0.35, high_levels=0.0,
               group_levels=None, exact_share=0.45):
    """The fleet of the module docstring.  levels: {field: ascending maxima} for bandwidth, core,
    power, total (one length L); clocks: the groups' clocks; free_caps: the free-memory ceiling
    of each level.  mixed: share of nodes whose cards each draw a
    model of their own; mixed_total: share of one-model nodes with two TotalMemory values.
    min_bw_per_clock: bandwidth >= clock // that + 1 (bounds clock*100/bandwidth), 0: off.
    fail_share: how often a value comes from `fail`; high_levels: share of the clock groups put
    on the upper half of the levels; group_levels: the levels of the last clock groups;
    exact_share: the share of values on exact quotients."""
    rng = np.random.default_rng(seed)
    L = len(levels["bandwidth"])
    G = len(clocks)
    assert G >= L and n >= HOLDERS * G
    glev = rng.integers(0, L, size=G)            # a clock group sits on one level ...
    up = rng.random(G) < high_levels
    glev[up] = rng.integers(L // 2, L, size=int(up.sum()))
    glev[:L] = rng.permutation(L)
    if group_levels is not None:                 # (the caller puts these groups on these levels)
        glev[-len(group_levels):] = group_levels
    grp = rng.integers(0, G, size=n)
    grp[:HOLDERS * G] = np.arange(HOLDERS * G) // HOLDERS
    lev = glev[grp]
    below = (rng.random(n) < 0.6) & (np.arange(n) >= HOLDERS * G)   # most others: any lower level
    lev = np.where(below, (rng.random(n) * (lev + 1)).astype(np.int64), lev)
    # ... and its first nodes hold the level's four maxima with every card healthy and as free
    # as the level allows: a pod that asks for the group's clock sees these maxima
    group_holder = np.arange(n) < HOLDERS * G
    cols = {f: np.zeros((n, K), np.uint64) for f in FIELDS}
    holder = (rng.random((n, 4)) < 0.1) | group_holder[:, None]
    # total memory has a level of its own per clock group, mostly a high one (the free-memory
    # ceilings follow the small fields' level), and half its values aim at the ladder's top,
    # the maximum a pod without scv/clock sees
    tlev = rng.integers(max(0, L - 6), L, size=G)
    tlev[:L] = rng.permutation(L)
    tlev = tlev[grp]
    for l in range(L):
        for fi, f in enumerate(("bandwidth", "core", "power", "total")):
            at = np.flatnonzero((tlev if f == "total" else lev) == l)
            x = _draw_x(rng, levels[f], l, at.size, None if fail is None else fail[f],
                        top_share=0.5 if f == "total" else 0.0, fail_share=fail_share,
                        exact_share=exact_share)
            x = np.where(holder[at, fi], np.uint64(levels[f][l]), x)
            cols[f][at] = x[:, None]
    cols["clock"][:] = clocks[grp][:, None]
    is_mixed = (rng.random(n) < mixed) & ~group_holder
    for i in np.flatnonzero(is_mixed):           # every card the model of some node of its level
        src = rng.choice(np.flatnonzero((lev == lev[i]) & ~is_mixed), K)
        for f in ("bandwidth", "core", "power", "clock"):
            cols[f][i] = cols[f][src, 0]
        cols["total"][i] = levels["total"][tlev[i]]   # (its group's largest card)
    two_totals = ~is_mixed & ~group_holder & (rng.random(n) < mixed_total)
    for i in np.flatnonzero(two_totals):
        cols["total"][i, rng.random(K) < 0.5] = _draw_x(rng, levels["total"], int(tlev[i]), 1)[0]
    if min_bw_per_clock:
        cols["bandwidth"] = np.maximum(cols["bandwidth"],
                                       cols["clock"] // np.uint64(min_bw_per_clock) + np.uint64(1))
    counts = np.full(n, K, np.uint32)
    u = rng.random(n)
    counts[u < short + empty] = rng.integers(1, K + 1, size=int((u < short + empty).sum()))
    counts[u < empty] = 0
    counts[group_holder] = K
    card_number = counts.astype(np.uint64)
    v = rng.random(n)
    card_number[v < 0.05] = 0
    card_number[(v >= 0.05) & (v < 0.08)] = rng.integers(0, K + 2, size=int(
        ((v >= 0.05) & (v < 0.08)).sum()))
    card_number[group_holder] = K
    cap = np.array(free_caps, np.uint64)[lev][:, None]
    top = np.minimum(cols["total"], cap)
    free = np.minimum((rng.random((n, K)) * (top.astype(np.float64) + 1)).astype(np.uint64), top)
    at_top = rng.random((n, K)) < 0.1            # some cards full: free == total or the ceiling
    free = np.where(at_top | group_holder[:, None], top, free)
    healthy = ((rng.random((n, K)) >= 0.05) | group_holder[:, None]).astype(np.uint8)
    used = np.arange(K)[None, :] < counts[:, None]
    for a in list(cols.values()) + [free, healthy]:
        a[~used] = 0
    total_sum = np.maximum(cols["total"].sum(axis=1, dtype=np.uint64), np.uint64(1))
    total_sum[counts == 0] = np.uint64(max(levels["total"][-1], 1)) * np.uint64(K)
    alloc = (rng.random(n) * (total_sum.astype(np.float64) / 2)).astype(np.uint64)
    return NodeSoA(card_number=card_number, card_count=counts,
                   free_memory_sum=free.sum(axis=1, dtype=np.uint64), total_memory_sum=total_sum,
                   alloc_memory=alloc, card_free_memory=free, card_total_memory=cols["total"],
                   card_clock=cols["clock"], card_bandwidth=cols["bandwidth"],
                   card_core=cols["core"], card_power=cols["power"], card_healthy=healthy,
                   cpu=rng.random(n) * 100.0, disk_io=rng.random(n) * 100.0).normalized()


def make_pods(seed, p, nodes, clock_share=0.55, clocks=None, priorities=False):
    """Pods over `nodes`: scv/clock at the fleet's clocks (a few one off: feasible nowhere),
    scv/memory at card frees and frees +-1, scv/number in {absent, 1, 2, 4, 8} and a
    tenth of the pods without any label."""
    rng = np.random.default_rng(seed)
    real = np.arange(nodes.max_cards)[None, :] < nodes.card_count[:, None]
    frees = np.sort(nodes.card_free_memory[real])
    ck = np.unique(nodes.card_clock[real]) if clocks is None else np.asarray(clocks, np.uint64)
    choice = rng.choice(5, size=p, p=[0.25, 0.35, 0.2, 0.12, 0.08])
    has_number = (choice > 0).astype(np.uint8)
    number = np.array([0, 1, 2, 4, 8], np.uint64)[choice]
    has_memory = (rng.random(p) < 0.75).astype(np.uint8)
    q = rng.random(p)
    m = frees[(q * (frees.size - 1)).astype(np.int64)].astype(object) + rng.integers(-1, 2, size=p)
    memory = np.where(has_memory == 1, np.maximum(m, 0), 0).astype(np.uint64)
    has_clock = (rng.random(p) < clock_share).astype(np.uint8)
    c = ck[rng.integers(0, ck.size, size=p)].astype(object)
    c = np.where(rng.random(p) < 0.04, c + 1, c)
    clock = np.where(has_clock == 1, c, 0).astype(np.uint64)
    bare = rng.random(p) < 0.1
    for a in (has_number, has_memory, has_clock, number, memory, clock):
        a[bare] = 0
    priority = (rng.integers(0, 10, size=p) if priorities else np.zeros(p)).astype(np.int64)
    return PodSoA(has_number=has_number, number=number, has_memory=has_memory, memory=memory,
                  has_clock=has_clock, clock=clock, priority=priority, rio=np.full(p, 10.0),
                  rcpu=np.full(p, 100, np.int64)).normalized()


def _copy(soa):
    return type(soa)(**{f: np.array(getattr(soa, f)) for f in soa.__dataclass_fields__})


# ---- the tiers ---------------------------------------------------------------------------------
# Most chain members are multiples of 100 with an odd factor: k*M/100 is then an integer for
# every k (a hundred exact quotients per maximum) while 100/M is no power of two.
MEMORY_LEVELS = _chain(15, (5,) + (2,) * 11)                                # 15 .. 153600 (MiB)


MEMORY_LEVELS_16 = sorted(MEMORY_LEVELS + [3, 45, 115200])


def _q32_levels():
    """16 maxima per field: a divisor chain, a few maxima that are 3 or 5 times a member of it
    (what sits on a rounding edge of theirs does so for that member and those below it) and 55738
    (kF32SmallMax) on top."""
    top = F32_SMALL_MAX
    return {"bandwidth": _chain(3, (2, 2, 5, 5) + (2,) * 7, (top, 48000, 28800, 7200)),
            "core": _chain(7, (2, 2, 5, 5) + (2,) * 6, (top, 50400, 33600, 16800, 4200)),
            "power": _chain(3, (3, 2, 2, 5, 5) + (2,) * 5, (top, 43200, 21600, 10800, 5400)),
            "total": MEMORY_LEVELS_16}


def _free_caps(total_levels):
    """The free-memory ceiling of each level of the small fields: the memory ladder reversed, so
    a rising scv/memory takes the high levels out first: a staircase of maxima."""
    return list(reversed(total_levels))


def _q32(seed, n, p, n_clocks, mixed=0.0, k=8, memory_scale=1):
    """memory_scale 2^20: every memory quantity in bytes (memory ranks), the ladder and the values
    around its quotients included."""
    rng = np.random.default_rng(seed)
    levels = _q32_levels()
    levels["total"] = [M * memory_scale for M in levels["total"]]
    clocks = _choose_clocks(rng, levels["bandwidth"], F32_SMALL_MAX, min(n_clocks, n // 3),
                            keep=(F32_SMALL_MAX, 0, 1))
    nodes = make_fleet(seed + 1, n, k, levels, clocks, _free_caps(levels["total"]), mixed=mixed)
    return nodes, make_pods(seed + 2, p, nodes)


# Bandwidth maxima against which a clock in 55739..65535 has a wrong f32 quotient (x > M: the
# clock quotient is not bounded by 100).  A search over every M <= 65535 and every x in that range
# finds 96 such M; these five have 150 failing clocks between them.
PACK16_BANDWIDTHS = (47, 49, 193, 367, 369)
PACK16_GROUPS = (16, 8, 5, 7, 7)      # clock groups that hold such a bandwidth and a failing clock


def f32_failing_range(M, lo, hi):
    """Every x in lo..hi whose f32 quotient by M is wrong."""
    x = np.arange(lo, hi + 1, dtype=np.uint64)
    Ma = np.full(x.size, M, np.uint64)
    return x[quot32(x, Ma) != x * np.uint64(100) // Ma]


def _pack16(seed, n, p):
    """Maxima up to 65535 with both ends of 55739..65535 among them; five low bandwidth
    levels are PACK16_BANDWIDTHS, and 64 clock groups sit on them with clocks whose f32 quotient
    by that bandwidth is wrong: a pod that asks for such a clock scores it against that
    MaxBandwidth, so f32 quotients on this tier (a misplaced kF32SmallMax) change scores."""
    rng = np.random.default_rng(seed)
    lo, hi = F32_SMALL_MAX + 1, PACK16_MAX
    levels = {"bandwidth": _chain(250, (2,) * 8, (lo, hi) + PACK16_BANDWIDTHS),  # .. 64000
              "core": _chain(3, (5, 5, 5, 5) + (2,) * 5, (lo, hi, 62000, 45000, 22500, 11250)),      # 3 .. 60000
              "power": _chain(9, (5, 5) + (2,) * 8, (lo, hi, 43200, 21600, 10800)),                  # 9 .. 57600
              "total": MEMORY_LEVELS_16}
    assert len({len(v) for v in levels.values()}) == 1, [len(v) for v in levels.values()]
    failing, group_levels = [], []
    for M, cnt in zip(PACK16_BANDWIDTHS, PACK16_GROUPS):
        l = levels["bandwidth"].index(M)
        failing += [int(c) for c in rng.choice(f32_failing_range(M, lo, hi), cnt, replace=False)]
        group_levels += [l] * cnt
    clocks = _choose_clocks(rng, levels["bandwidth"], hi, 200 - len(failing), keep=(hi, lo, 0, 1))
    clocks = np.concatenate([clocks[~np.isin(clocks, failing)], np.array(failing, np.uint64)])
    nodes = make_fleet(seed + 1, n, 8, levels, clocks, _free_caps(levels["total"]), empty=0.0,
                       mixed_total=0.0, group_levels=group_levels, exact_share=0.55)
    return nodes, make_pods(seed + 2, p, nodes)


def _wide_chain(rng, base=None):
    """base * {1, 2, 4} (base in 70001 .. 83000), then * 50 and eight more doublings (multiples
    of 100 from 1.4e7 to 4e9: a hundred exact quotients each, all of them beyond the f32 lemma),
    and 0xFFFFFFFE on top; the base and every member beyond 2^24 have f32-failing quotients."""
    for _ in range(4000):
        b = int(rng.integers(70001, 83001)) if base is None else base
        ch = _chain(b, (2, 2, 50) + (2,) * 8, (N32_FIELD_MAX,))
        if all(f32_failing(M).size for M in ch if M == b or M > (1 << 24)):
            return ch
        assert base is None, [M for M in ch if not f32_failing(M).size]
    raise AssertionError("no chain")


def _wide(seed, n, p, n_clocks=60):
    """Small fields up to 0xFFFFFFFE whose maxima all break the f32 quotient; bandwidth's chain
    starts at 78599 (x = 77813: f32 gives 99, the integer quotient is 98)."""
    rng = np.random.default_rng(seed)
    levels = {"bandwidth": _wide_chain(rng, 78599), "core": _wide_chain(rng),
              "power": _wide_chain(rng), "total": MEMORY_LEVELS}
    assert 77813 in f32_failing(78599)
    fail = {f: [f32_failing(M) for M in levels[f]] for f in ("bandwidth", "core", "power")}
    fail["total"] = [np.zeros(0, np.uint64)] * len(MEMORY_LEVELS)
    # clock / MaxBandwidth: clocks that fail in f32 against a bandwidth level (x > M allowed)
    clocks = [N32_FIELD_MAX]
    for M in levels["bandwidth"]:
        bad = f32_failing(M, xmax=min(N32_FIELD_MAX, 3 * M))
        if bad.size:
            clocks += [int(v) for v in rng.choice(bad, min(2, bad.size), replace=False)]
    clocks = list(dict.fromkeys(clocks))[:n_clocks]
    more = _choose_clocks(rng, levels["bandwidth"], N32_FIELD_MAX, min(n_clocks, n // 3),
                          keep=clocks)
    # (bandwidth >= clock / 4e6: K * (800 + clock*100/bandwidth) stays below 2^32 at K = 8)
    nodes = make_fleet(seed + 1, n, 8, levels, more, _free_caps(levels["total"]), empty=0.0,
                       mixed_total=0.0, fail=fail, min_bw_per_clock=4_000_000, high_levels=0.85,
                       fail_share=0.1, exact_share=0.57)
    return nodes, make_pods(seed + 2, p, nodes)


SCORE32_K = 16
# the largest clock c for which K * (800 + c*100/1) < 2^32 (choose_format's u32 score guard)
SCORE32_CLOCK = (((1 << 32) - 1) // SCORE32_K - 800) // 100
assert SCORE32_K * (800 + SCORE32_CLOCK * 100) < (1 << 32) <= \
    SCORE32_K * (800 + (SCORE32_CLOCK + 1) * 100)


def _score32(seed, clock, n=1500, p=300):
    """K = 16 one-model nodes; 48 of them hold one model with bandwidth 1, `clock`, 16 healthy
    cards of the fleet's largest TotalMemory and frees within a tenth of it; a quarter of the pods
    ask for that clock, so all 16 cards score clock*100 against MaxBandwidth = 1 and close to 100
    in every other quotient.  With SCORE32_CLOCK the node's card scores sum to just below 2^32
    (at most 16 * (800 + 268,434,600) = 4,294,966,400: the bound rules a wrap out); with one more
    they pass 2^32, which is why the host must refuse N32 there."""
    rng = np.random.default_rng(seed)
    levels = _q32_levels()
    clocks = _choose_clocks(rng, levels["bandwidth"], F32_SMALL_MAX, 30, keep=(F32_SMALL_MAX,))
    nodes = make_fleet(seed + 1, n, SCORE32_K, levels, clocks, _free_caps(levels["total"]),
                       empty=0.0, mixed_total=0.0)
    hot = rng.choice(np.arange(HOLDERS * 30, n), 48, replace=False)
    top = np.uint64(levels["total"][-1])
    nodes.card_count[hot] = SCORE32_K
    nodes.card_number[hot] = SCORE32_K
    nodes.card_bandwidth[hot] = 1
    nodes.card_clock[hot] = clock
    nodes.card_core[hot] = nodes.card_core[hot[0], 0]
    nodes.card_power[hot] = nodes.card_power[hot[0], 0]
    nodes.card_total_memory[hot] = top
    nodes.card_free_memory[hot] = top - rng.integers(0, int(top) // 10, size=(48, SCORE32_K)
                                                     ).astype(np.uint64)
    nodes.card_healthy[hot] = 1
    nodes.free_memory_sum[hot] = nodes.card_free_memory[hot].sum(axis=1, dtype=np.uint64)
    nodes.total_memory_sum[hot] = top * np.uint64(SCORE32_K)
    nodes.alloc_memory[hot] = nodes.total_memory_sum[hot] // np.uint64(3)
    pods = make_pods(seed + 2, p, nodes, clocks=clocks)
    ask = rng.random(p) < 0.25
    pods.has_clock[ask] = 1
    pods.clock[ask] = clock
    pods.has_memory[ask & (rng.random(p) < 0.5)] = 0
    return nodes.normalized(), pods.normalized()


def _field44(seed, top, n=1500, p=300):
    """Memory fields up to `top` (2^44: the last value of the F64 records), the total-memory
    maxima 2^29 .. 2^44 with x around their integer quotients (k = 100: 300 x + M next to 2^53);
    node 7 holds two GPU models, one with a 17-bit bandwidth, so the snapshot is not N32."""
    rng = np.random.default_rng(seed)
    levels = _q32_levels()
    levels["total"] = _chain(1 << 29, (2,) * 15)
    clocks = _choose_clocks(rng, levels["bandwidth"], F32_SMALL_MAX, 30, keep=(F32_SMALL_MAX,))
    nodes = make_fleet(seed + 1, n, 8, levels, clocks, _free_caps(levels["total"]), empty=0.0)
    hi = np.flatnonzero(nodes.card_total_memory[:, 0] == np.uint64(1 << 44))[:6]
    assert hi.size >= 2
    used = np.arange(8)[None, :] < nodes.card_count[hi][:, None]
    nodes.card_total_memory[hi] = np.where(used, top, 0).astype(np.uint64)
    nodes.card_free_memory[hi[0]] = nodes.card_total_memory[hi[0]]   # free == total == top
    nodes.card_healthy[hi[0]] = used[0].astype(np.uint8)
    nodes.card_bandwidth[7, 0] = 70000
    nodes.free_memory_sum = nodes.card_free_memory.sum(axis=1, dtype=np.uint64)
    nodes.total_memory_sum = np.maximum(nodes.card_total_memory.sum(axis=1, dtype=np.uint64),
                                        np.uint64(1))
    nodes = nodes.normalized()
    return nodes, make_pods(seed + 2, p, nodes)


def _with_two_models(nodes, i=11):
    out = _copy(nodes)
    c = int(out.card_core[i, 0])
    out.card_core[i, 0] = c + 1 if c < 1000 else c - 1
    return out.normalized()


TIERS = ("q32", "q32_grouped", "pack16", "wide", "wide_mixed", "q32_mixed", "score32",
         "score32_plus1", "field44", "field44_plus1", "field32", "ranks")
BIG_TIERS = ("q32", "q32_grouped", "pack16", "wide", "q32_mixed", "ranks")   # 4,700 nodes
LEMMA_TIERS = ("q32", "q32_grouped", "q32_mixed", "ranks")    # f32 quotients: inside the lemma
N32_TIERS = ("q32", "q32_grouped", "pack16", "wide", "q32_mixed", "score32", "ranks")
SEEDS = {"q32": 100, "q32_grouped": 200, "pack16": 310, "wide": 400, "q32_mixed": 500,
         "score32": 600, "field44": 700, "field32": 800}


@functools.lru_cache(maxsize=None)
def tier(name, small=False):
    """Tier(name, nodes, pods, expected path, expected flags); flags: small_le
    (small_field_max <= 55738), ranks, grouped.  small: the 130 x 65 shape (q32 and wide).
    Cached: the arrays are shared, do not write to them."""
    n, p = (SMALL_N, SMALL_P) if small else (BIG_N, BIG_P)
    path, ranks = "n32", False
    if name in ("q32", "ranks"):
        nodes, pods = _q32(SEEDS["q32"], n, p, 200,
                           memory_scale=(1 << 20) if name == "ranks" else 1)
        ranks = name == "ranks"
    elif name == "q32_grouped":
        nodes, pods = _q32(SEEDS[name], n, p, 48)
    elif name == "q32_mixed":
        nodes, pods = _q32(SEEDS[name], n, p, 200, mixed=0.3)
    elif name == "pack16":
        nodes, pods = _pack16(SEEDS[name], n, p)
    elif name in ("wide", "wide_mixed"):
        nodes, pods = _wide(SEEDS["wide"], n, p)
        if name == "wide_mixed":
            nodes, path = _with_two_models(nodes), "f64"
    elif name in ("score32", "score32_plus1"):
        plus = name.endswith("plus1")
        nodes, pods = _score32(SEEDS["score32"], SCORE32_CLOCK + plus)
        path = "f64" if plus else "n32"
    elif name in ("field44", "field44_plus1"):
        plus = name.endswith("plus1")
        nodes, pods = _field44(SEEDS["field44"], (1 << 44) + plus)
        path = "u64" if plus else "f64"
    elif name == "field32":
        nodes, pods = _q32(SEEDS[name], 1500, 300, 30)
        nodes = _copy(nodes)
        i = int(np.flatnonzero(nodes.card_count == 8)[5])
        nodes.card_power[i] = np.uint64(N32_FIELD_MAX + 1)
        nodes, path = nodes.normalized(), "f64"
    else:
        raise ValueError(name)
    flags = {"small_le": name not in ("pack16", "wide", "wide_mixed", "score32",
                                      "score32_plus1", "field44", "field44_plus1", "field32"),
             "ranks": ranks, "grouped": name in ("q32_grouped", "wide") and not small}
    return Tier(name, nodes, pods, path, flags)


def row_pods(t, count=24):
    """The 24-pod row batch of a tier: evenly spread over its pods."""
    return t.pods.take(np.linspace(0, t.pods.n_pods - 1, count).astype(np.int64))


# ---- CalculateCardScore in integers, with the wrong readings -----------------------------------
def scored_cards(nodes, pods, p):
    """(feasible [N] bool, scored [N, K] bool) of pod p: Filter, and the cards CollectMaxValues /
    CalculateBasicScore take (free >= memory and clock >= scv/clock, health not asked)."""
    real = np.arange(nodes.max_cards)[None, :] < nodes.card_count[:, None]
    number = int(pods.number[p]) if pods.has_number[p] else 1
    fit = (nodes.card_number >= np.uint64(number)) if pods.has_number[p] else nodes.card_number > 0
    m = pods.memory[p] if pods.has_memory[p] else np.uint64(0)
    c = pods.clock[p] if pods.has_clock[p] else np.uint64(0)
    hl = real & (nodes.card_healthy != 0)
    if pods.has_memory[p]:
        fit = fit & ((hl & (nodes.card_free_memory >= m)).sum(axis=1) >= number)
    if pods.has_clock[p]:
        fit = fit & ((hl & (nodes.card_clock == c)).sum(axis=1) >= number)
    scored = real & (nodes.card_free_memory >= m) & (nodes.card_clock >= c) & fit[:, None]
    return fit, scored


def evaluate(nodes, pods, p, reading="exact", f32=True):
    """(pick, top_score, n_feasible, raw scores [N]) of pod p with the quotients read as
    `reading`: exact; nearest (the reciprocal rounded to nearest, f32 when `f32` else f64, on the
    four small fields); f32 (the kernels' f32 quotient, reciprocal rounded up); maxclock (clock /
    MaxClock); wrap32 / wrap31 (the node's card scores summed modulo 2^32 / 2^31)."""
    U = np.uint64
    fit, scored = scored_cards(nodes, pods, p)
    if not fit.any():
        return -1, 0, 0, np.zeros(nodes.n_nodes, np.int64)
    col = {"bandwidth": nodes.card_bandwidth, "clock": nodes.card_clock, "core": nodes.card_core,
           "power": nodes.card_power, "total": nodes.card_total_memory,
           "free": nodes.card_free_memory}
    mx = {f: max(int(a[scored].max()) if scored.any() else 1, 1) for f, a in col.items()}

    def q(f, M, small=True):
        x = col[f]
        Ma = np.full(x.shape, M, np.uint64)
        if small and reading == "f32":
            return quot32(x, Ma)
        if small and reading == "nearest":
            return quot32(x, Ma, rn32) if f32 else quot64_nearest(x, Ma)
        return x * U(100) // U(M)

    card = (q("bandwidth", mx["bandwidth"]) +
            q("clock", mx["clock"] if reading == "maxclock" else mx["bandwidth"]) +
            q("core", mx["core"]) * U(2) + q("power", mx["power"]) +
            q("free", mx["free"], False) * U(3) + q("total", mx["total"], False))
    basic = np.where(scored, card, U(0)).sum(axis=1, dtype=np.uint64)
    if reading in ("wrap32", "wrap31"):
        basic &= U(0xFFFFFFFF if reading == "wrap32" else 0x7FFFFFFF)
    tot, fre, alloc = nodes.total_memory_sum, nodes.free_memory_sum, nodes.alloc_memory
    safe = np.maximum(tot, U(1))
    allocate = np.where(tot < alloc, U(0), (safe - np.minimum(alloc, safe)) * U(100) // safe * U(3))
    raw = (basic + allocate + fre * U(100) // safe * U(2)).astype(np.int64)
    idx = np.flatnonzero(fit)
    r = [int(v) for v in raw[idx]]
    if len(r) == 1:
        return int(idx[0]), r[0], 1, raw
    hi, lo = max(max(r), 0), min(r)
    if hi == lo:
        lo -= 1
    norm = [(v - lo) * 100 // (hi - lo) for v in r]
    k = norm.index(max(norm))
    return int(idx[k]), r[k], len(r), raw


def pair_census(t, want):
    """Per field the distinct scored (x, M) pairs of a tier, M from the oracle's maxima, as a
    uint64 [n, 2] array each."""
    nodes, pods = t.nodes, t.pods
    col = {"bandwidth": nodes.card_bandwidth, "clock": nodes.card_clock, "core": nodes.card_core,
           "power": nodes.card_power, "total": nodes.card_total_memory}
    seen = {f: set() for f in FIELDS}
    for p in range(pods.n_pods):
        _, scored = scored_cards(nodes, pods, p)
        if not scored.any():
            continue
        for f in FIELDS:
            M = int(want.maxima[p, MAXIMA_COL[f]])
            seen[f].update((int(x), M) for x in np.unique(col[f][scored]))
    return {f: np.array(sorted(s), np.uint64).reshape(-1, 2) for f, s in seen.items()}
