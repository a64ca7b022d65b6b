// yoda_modeb.h — the Mode B batch path's per-lane accumulator, its settle and the merges of its
// partials, shared by the HIP kernels (yoda_kernels.hip k2b_*), the host side of libyoda (the
// pod-class builder) and a stand-alone host program (tools/check_modeb_elig.cpp); and the walk
// plan of Mode B under node sampling (the k2b_samp_plan / k2b_sampled / k2b_rows kernels, the
// rows' host-filled bitmask, tools/check_modeb_sampling.cpp).
// See DESIGN.md §4 (Mode B) and §5 (eligibility: absent nodes and candidate classes; Mode B under
// node sampling).
#pragma once
#include <stdint.h>

#include <vector>

#include "yoda_layout.h"

namespace yoda {

// The Mode B score (algorithm.go:109-111): |d| = |alpha*V - beta*U|, then uint64(10 - 10*|d|) on
// amd64 and Uint64ToInt64: trunc for a value >= 1, else 0 (NaN, negatives).  Go on amd64 fuses
// nothing, so neither function is FMA-contracted, whatever the flags of the file that includes
// them.  The one definition for the kernels, the host's level table (diskio_levels) and the
// stand-alone checks.
__host__ __device__ __forceinline__ double disk_absdiff(double alpha, double v, double beta,
                                                        double u) {
#pragma clang fp contract(off)
  const double a = alpha * v;
  const double b = beta * u;
  return __builtin_fabs(a - b);  // :110
}

__host__ __device__ __forceinline__ double disk_score(double l) {
#pragma clang fp contract(off)
  const double t = 10.0 * l;
  const double s = 10.0 - t;  // :111
  return (s >= 1.0) ? __builtin_trunc(s) : 0.0;
}

// A lane keeps, over nodes in increasing order, the best level seen, its node count and its
// first (lowest) node; level 0 counts nothing while running (every node is >= 0, NaN included)
// and is settled at the end.
struct DiskAcc {
  uint32_t lev, cnt, idx;
  double tc, tu;  // count threshold of the current level (-1 at level 0), the next level's
};

__host__ __device__ __forceinline__ void disk_init(DiskAcc& s, const double* lv) {
  s.lev = 0;
  s.cnt = 0;
  s.idx = 0xffffffffu;
  s.tc = -1.0;
  s.tu = lv[1];
}

__host__ __device__ __forceinline__ void disk_step(DiskAcc& s, double ad, uint32_t n,
                                                   const double* lv) {
  s.cnt += (ad <= s.tc) ? 1u : 0u;
  if (ad <= s.tu) {  // a higher level (rare once the first nodes are seen)
    uint32_t L = 1;  // the levels are nested: |d| <= t[k] for every k up to its level
#pragma unroll
    for (int k = 2; k <= 10; ++k) L += (ad <= lv[k]) ? 1u : 0u;
    s.lev = L;
    s.cnt = 1;
    s.idx = n;
    s.tc = lv[L];
    s.tu = lv[L + 1];
  }
}

// ---------------------------------------------------------------------------------------
// Eligibility (yoda_mode_b_follow): pod p's cycle runs over E(p) = the present nodes that are
// candidates of p's class.  One record per node: lo holds the node's candidate word (every bit
// set while candidates are off, 0 while the node is absent), bit 0 of hi its presence.  A pod
// class selects bit `sel` of the 128: its candidate class 0..63, or kDiskSelAny (presence
// alone: YODA_CAND_ANY, or candidates off).
struct alignas(16) DiskElig {
  uint64_t lo, hi;
};
constexpr uint32_t kDiskSelAny = 64;
constexpr uint32_t kDiskSelCount = 65;  // the count table: nodes of each class, present nodes

__host__ __device__ __forceinline__ uint32_t disk_sel(uint8_t cls_byte) {
  return cls_byte == 0xFFu ? kDiskSelAny : (uint32_t)cls_byte;
}

// (by value, and the select on the shifted words: a select between the two members' addresses
// would send the record through memory)
__host__ __device__ __forceinline__ bool disk_eligible(DiskElig e, uint32_t sel) {
  const uint32_t sh = sel & 63u;
  const uint64_t lo = e.lo >> sh, hi = e.hi >> sh;
  return (((sel & 64u) ? hi : lo) & 1ull) != 0ull;
}

// A selector as masks over the record's three live 32-bit words (lo low, lo high, hi low): fixed
// per lane over a whole chunk, so the per-pair test is two ANDs, an OR and a compare.
struct DiskSelMask {
  uint32_t lo0, lo1, hi0;
};

__host__ __device__ __forceinline__ DiskSelMask disk_sel_mask(uint32_t sel) {
  DiskSelMask m;
  m.lo0 = sel < 32u ? 1u << sel : 0u;
  m.lo1 = (sel >= 32u && sel < 64u) ? 1u << (sel - 32u) : 0u;
  m.hi0 = sel == kDiskSelAny ? 1u : 0u;
  return m;
}

__host__ __device__ __forceinline__ bool disk_eligible(DiskElig e, DiskSelMask m) {
  return (((uint32_t)e.lo & m.lo0) | ((uint32_t)(e.lo >> 32) & m.lo1) |
          ((uint32_t)e.hi & m.hi0)) != 0u;
}

__host__ __device__ __forceinline__ DiskElig disk_elig_of(bool present, uint64_t word) {
  return DiskElig{present ? word : 0ull, present ? 1ull : 0ull};
}

// What a run with eligibility hands the Mode B kernels and their launchers, by value; elig ==
// nullptr (the empty value) is an unrestricted run, whose kernel instances (ELIG = false) read
// none of it.
struct DiskEligArgs {
  const DiskElig* elig;  // [n_nodes] records
  const uint32_t* csel;  // batch kernels: the [n_cls] selectors of the pod classes
  const uint8_t* cls;    // rows, draw, n_feasible: the pods' class bytes (nullptr: every pod ANY)
  const uint32_t* cnt;   // [kDiskSelCount] nodes of each class, present nodes
};

// The eligible nodes a lane has stepped over and the first of them: what level 0 settles from
// (the unrestricted instances settle it from the chunk's bounds, which count every node).
struct DiskSeen {
  uint32_t n, first;
};

__host__ __device__ __forceinline__ void disk_seen_init(DiskSeen& e) {
  e.n = 0;
  e.first = 0xffffffffu;
}

// One ELIGIBLE (node, class) pair; nodes arrive in increasing order.
__host__ __device__ __forceinline__ void disk_step_elig(DiskAcc& s, DiskSeen& e, double ad,
                                                        uint32_t n, const double* lv) {
  e.first = e.n ? e.first : n;
  ++e.n;
  disk_step(s, ad, n, lv);
}

// The branch-free form of the lane = class kernel, whose lanes walk the same nodes with different
// selectors.  An ineligible pair steps with +inf, which reaches no level and counts nothing; the
// eligible nodes are not tracked while running, and a lane that ends at level 0 (rare: every
// eligible node of the chunk scores 0) walks the chunk's words again with disk_seen_add.
__host__ __device__ __forceinline__ void disk_step_masked(DiskAcc& s, bool el, double ad,
                                                          uint32_t n, const double* lv) {
  disk_step(s, el ? ad : __builtin_huge_val(), n, lv);
}

__host__ __device__ __forceinline__ void disk_seen_add(DiskSeen& e, bool el, uint32_t n) {
  const uint32_t at = el ? n : 0xffffffffu;
  e.first = at < e.first ? at : e.first;  // (nodes in increasing order: the minimum is the first)
  e.n += el ? 1u : 0u;
}

// The lane's (count, lowest node) at its level; count 0 (node 0xffffffff): no eligible node.
__host__ __device__ __forceinline__ void disk_settle(const DiskAcc& s, const DiskSeen& e,
                                                     uint32_t& cnt, uint32_t& idx) {
  cnt = s.lev == 0u ? e.n : s.cnt;
  idx = s.lev == 0u ? e.first : s.idx;
}

__host__ __device__ __forceinline__ uint32_t disk_pack(uint32_t lev, uint32_t cnt) {
  return (lev << kDiskCountBits) | cnt;
}

// The running best over parts: level, nodes at it, the lowest of them.  A part with count 0
// holds no eligible node and contributes nothing, whatever its level and node say.
struct DiskBest {
  int64_t lev;
  uint32_t cnt, idx;
};

__host__ __device__ __forceinline__ void disk_best_init(DiskBest& b) {
  b.lev = -1;
  b.cnt = 0;
  b.idx = 0xffffffffu;
}

// Parts in any order (the lanes of a wave, the waves of a workgroup): the lowest node wins.
__host__ __device__ __forceinline__ void disk_merge_any(DiskBest& b, uint32_t lev, uint32_t cnt,
                                                        uint32_t idx) {
  if (cnt == 0u) return;
  if ((int64_t)lev > b.lev) {
    b.lev = (int64_t)lev;
    b.cnt = cnt;
    b.idx = idx;
  } else if ((int64_t)lev == b.lev) {
    b.cnt += cnt;
    b.idx = idx < b.idx ? idx : b.idx;
  }
}

// Chunk partials in node order: the first chunk reaching the best level holds the lowest node.
// idx points at the partial's node, which is read only when the partial takes the lead (a
// kernel's merge loop then loads one word per chunk, not two).
__host__ __device__ __forceinline__ void disk_merge_chunk(DiskBest& b, uint32_t word,
                                                          const uint32_t* idx) {
  const uint32_t cnt = word & ((1u << kDiskCountBits) - 1u);
  if (cnt == 0u) return;
  const int64_t L = (int64_t)(word >> kDiskCountBits);
  if (L > b.lev) {
    b.lev = L;
    b.cnt = cnt;
    b.idx = *idx;
  } else if (L == b.lev) {
    b.cnt += cnt;
  }
}

// ---------------------------------------------------------------------------------------
// Node sampling in Mode B (yoda_mode_b_sampling): pod p scores S(p), the first
// min(M, |E|) nodes of E(p) in the walk order start, start + 1, ..., wrapping at the snapshot's
// end.  S is E cut to at most two ascending id segments, so a walk is three words: the nodes of
// [start, stop) (stop > start), or of [start, N) and [0, stop) after a wrap; full: every node of
// E (|E| <= M, or an empty E).  Local ids throughout.
struct DiskWalk {
  uint32_t start, stop, full;
};

__host__ __device__ __forceinline__ bool disk_in_walk(uint32_t n, DiskWalk w) {
  if (w.full) return true;
  const bool ge = n >= w.start, lt = n < w.stop;
  return w.stop > w.start ? (ge && lt) : (ge || lt);
}

// The position of the set bit of rank r (0-based, r < popcount(x)): six popcount steps.
__host__ __device__ __forceinline__ uint32_t disk_select64(uint64_t x, uint32_t r) {
  uint32_t t = 0;
#pragma unroll
  for (uint32_t s = 32u; s >= 1u; s >>= 1) {
    const uint32_t c = (uint32_t)__builtin_popcountll((x >> t) & ((1ull << s) - 1ull));
    if (r >= c) {
      r -= c;
      t += s;
    }
  }
  return t;
}

// The rank tables of the walk plan, selector-major over 64-node blocks: bits[sel][b] holds the
// eligibility of nodes 64 b .. 64 b + 63 under selector sel (tail bits past the last node clear),
// pfx[sel][b] the eligible nodes below block b.
struct DiskRank {
  const uint64_t* bits;  // [kDiskSelCount][n_blocks]
  const uint32_t* pfx;   // [kDiskSelCount][n_blocks]
  uint32_t n_blocks;
};

// A pod's plan: its walk, |E| (n_found), |S| and the node the next walk starts at -- the
// (M + 1)-th node of E in walk order when |E| > M, else start itself.
struct DiskWalkPlan {
  DiskWalk walk;
  uint32_t n_found, n_sample, next_start;
};

// Every E whole: E is the id range [0, n_nodes), so the plan is arithmetic.
__host__ __device__ __forceinline__ DiskWalkPlan disk_plan_whole(uint32_t n_nodes, uint32_t start,
                                                                 uint32_t m) {
  DiskWalkPlan pl;
  pl.n_found = n_nodes;
  if (n_nodes <= m) {
    pl.walk = DiskWalk{start, start, 1u};
    pl.n_sample = n_nodes;
    pl.next_start = start;
  } else {
    const uint32_t stop = (uint32_t)(((uint64_t)start + m) % n_nodes);
    pl.walk = DiskWalk{start, stop, 0u};
    pl.n_sample = m;
    pl.next_start = stop;
  }
  return pl;
}

// One selector's rows (bits, pfx: n_blocks words each) and its total: r0 = the eligible ids below
// start; the walk's (M + 1)-th node has rank (r0 + M) mod total -- the block by binary search in
// the prefix row (the last block whose prefix is <= the rank holds it: the next one's is above),
// the node by the in-word select.
__host__ __device__ __forceinline__ DiskWalkPlan disk_plan_walk(const uint64_t* bits,
                                                                const uint32_t* pfx,
                                                                uint32_t n_blocks, uint32_t total,
                                                                uint32_t start, uint32_t m) {
  DiskWalkPlan pl;
  pl.n_found = total;
  if (total <= m) {
    pl.walk = DiskWalk{start, start, 1u};
    pl.n_sample = total;
    pl.next_start = start;
    return pl;
  }
  const uint32_t sb = start >> 6;
  const uint64_t below = bits[sb] & ((1ull << (start & 63u)) - 1ull);
  const uint32_t r0 = pfx[sb] + (uint32_t)__builtin_popcountll(below);
  const uint32_t k = (uint32_t)(((uint64_t)r0 + m) % total);
  uint32_t lo = 0, hi = n_blocks;  // pfx[lo] <= k < pfx[hi] (pfx[n_blocks] = total)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (pfx[mid] <= k) lo = mid; else hi = mid;
  }
  const uint32_t stop = 64u * lo + disk_select64(bits[lo], k - pfx[lo]);
  pl.walk = DiskWalk{start, stop, 0u};
  pl.n_sample = m;
  pl.next_start = stop;
  return pl;
}

// What a sampled run hands its kernels, by value.  rank.bits == nullptr: every E whole (the ELIG =
// false instances, which read no table).
struct DiskSampArgs {
  DiskRank rank;
  const uint8_t* cls;     // the pods' class bytes (nullptr: every pod ANY)
  const uint32_t* cnt;    // [kDiskSelCount] |E| of each selector
  const uint32_t* start;  // [n_pods] local start ids (nullptr: every walk starts at node 0)
  uint32_t m, n_nodes, n_pods, node_offset;
  uint32_t* n_found;      // [n_pods] |E(p)|
  uint32_t* next_start;   // [n_pods] global ids
  DiskWalk* walk;         // [n_pods]
};

// The selectHost draw inside the sampled kernel (yoda_set_tie_draw).
struct DiskDrawArgs {
  uint64_t seed, pod_base;
};

// ---------------------------------------------------------------------------------------
// The batch's pod classes (host): pods with bit-identical (alpha, beta) and the same selector
// score every node alike and walk the same node set (algorithm.go:105-111).  cls_bytes: one
// candidate class byte per pod (0..63, or 0xFF = YODA_CAND_ANY), or nullptr: every pod
// kDiskSelAny.  Classes are numbered in order of first appearance, so with cls_bytes == nullptr
// they are the (alpha, beta) pairs alone.
struct DiskClasses {
  std::vector<uint64_t> alpha, beta;  // [D] bit patterns
  std::vector<uint32_t> sel;          // [D]
  std::vector<uint32_t> cls;          // [P] class of each pod
};

inline void disk_build_classes(const uint64_t* al, const uint64_t* be,
                               const uint8_t* cls_bytes, uint32_t n_pods, DiskClasses& out) {
  size_t cap = 64;
  while (cap < 2 * (size_t)n_pods) cap <<= 1;
  std::vector<uint32_t> slot(cap, 0xffffffffu);  // class id, or empty
  out.alpha.clear();
  out.beta.clear();
  out.sel.clear();
  out.cls.assign(n_pods, 0u);
  for (uint32_t p = 0; p < n_pods; ++p) {
    const uint64_t a = al[p], b = be[p];
    const uint32_t s = cls_bytes ? disk_sel(cls_bytes[p]) : kDiskSelAny;
    size_t i = (size_t)(((a * 0x9e3779b97f4a7c15ull ^ b * 0xc2b2ae3d27d4eb4full) >> 20) +
                        (uint64_t)(kDiskSelAny - s) * 0x85ebca6bull) & (cap - 1);
    while (slot[i] != 0xffffffffu &&
           !(out.alpha[slot[i]] == a && out.beta[slot[i]] == b && out.sel[slot[i]] == s))
      i = (i + 1) & (cap - 1);
    if (slot[i] == 0xffffffffu) {
      slot[i] = (uint32_t)out.alpha.size();
      out.alpha.push_back(a);
      out.beta.push_back(b);
      out.sel.push_back(s);
    }
    out.cls[p] = slot[i];
  }
}

}  // namespace yoda
