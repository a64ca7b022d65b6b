// yoda_modeb.h — the Mode B batch path's per-lane accumulator, its settle and the merges of its
// partials, shared by the HIP kernels (yoda_kernels.hip k2b_*), the host side of libyoda (the
// pod-class builder) and a stand-alone host program (tools/check_modeb_elig.cpp).
// See DESIGN.md §4 (Mode B) and §5 (eligibility: absent nodes and candidate classes).
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
