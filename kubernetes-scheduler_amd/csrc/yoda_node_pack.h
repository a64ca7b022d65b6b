// yoda_node_pack.h — one node of a snapshot packed into the device layout of yoda_layout.h:
// its record, its K1 and K2 summary rows, its per-card model row and its K1 mixed tile.  Host
// code without a HIP runtime call: yoda_upload_nodes packs every node with it,
// yoda_update_node_cards the nodes whose card metrics changed, yoda_set_node_present the nodes
// that left or returned, yoda_replace_nodes the nodes whose whole record is the caller's, and
// tools/check_node_pack.cpp
// runs it under AddressSanitizer.  One packer, so the sparse path cannot drift from the upload;
// what is derived from these rows (block summaries, G table) has one builder too, on the device
// (k_bsum_build, k_gtable), which both callers run.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/yoda.h"
#include "yoda_layout.h"

namespace yoda {

// One node as the caller holds it.  The card arrays have `cnt` entries (cnt <= K).  fcode /
// tcode: the u32 codes of FreeMemory / TotalMemory on the N32 path (the value, or 2 + its rank
// with memory ranks: yoda_layout.h MemTab), read on that path only.
struct NodePackIn {
  uint32_t cnt = 0;
  uint64_t card_number = 0;
  uint64_t stat = 0;        // static score (CalculateAllocateScore + CalculateActualScore)
  bool zero_total = false;  // TotalMemorySum == 0
  bool no_uniform = false;  // YODA_UPLOAD_NO_UNIFORM: never mark the node one-model
  bool absent = false;      // yoda_set_node_present: kNodeAbsent / kSumAbsent
  const uint64_t* free_memory = nullptr;
  const uint64_t* total_memory = nullptr;
  const uint64_t* clock = nullptr;
  const uint64_t* bandwidth = nullptr;
  const uint64_t* core = nullptr;
  const uint64_t* power = nullptr;
  const uint8_t* healthy = nullptr;
  const uint32_t* fcode = nullptr;
  const uint32_t* tcode = nullptr;
};

// Where the node's rows go, node-major (contiguous words): rec has n32_stride(K) (N32) or
// node_stride(K) bytes; sum / sum2 / mix / x1 (N32 only, else nullptr) have k1sum_stride(K) / 4,
// k2sum_stride(K) / 4, mix_stride(K) / 4, x1_stride(K) / 4 words.
struct NodePackOut {
  unsigned char* rec = nullptr;
  uint32_t* sum = nullptr;
  uint32_t* sum2 = nullptr;
  uint32_t* mix = nullptr;
  uint32_t* x1 = nullptr;
  // the rows are known to hold zeros (the upload's fresh vectors): pack_node skips clearing them
  bool zeroed = false;
};

// Packs the node; returns its record flags (kNodeUniform4 | kNodeUniformTotal | kNodeAbsent).  Every row is
// written WHOLE -- cleared first unless out.zeroed -- so that packing over an older row of the
// same node leaves what a fresh pack leaves (hfs past the healthy count, the ch entries, the
// change bits).
inline uint32_t pack_node(Path path, int K, const NodePackIn& in, const NodePackOut& out) {
  const uint32_t cnt = in.cnt;
  const size_t stride = path == Path::N32 ? n32_stride(K) : node_stride(K);
  unsigned char* r = out.rec;
  if (!out.zeroed) std::memset(r, 0, stride);
  uint32_t hm = 0;
  for (uint32_t j = 0; j < cnt; ++j)
    if (in.healthy[j]) hm |= 1u << j;
  NodeHdrG hd{};  // NodeHdrF has the same layout; static_score's bits set below
  hd.card_number = in.card_number;
  hd.healthy_mask = hm;
  hd.zero_total = in.zero_total;
  hd.real_mask = cnt >= 32 ? 0xffffffffu : ((1u << cnt) - 1u);
  bool uni = cnt > 0;
  for (uint32_t j = 1; j < cnt; ++j)
    uni = uni && in.clock[j] == in.clock[0] && in.bandwidth[j] == in.bandwidth[0] &&
          in.core[j] == in.core[0] && in.power[j] == in.power[0];
  bool uni_total = uni;
  for (uint32_t j = 1; j < cnt; ++j) uni_total = uni_total && in.total_memory[j] == in.total_memory[0];
  hd.flags = 0u;
  if (uni && !in.no_uniform) hd.flags = kNodeUniform4 | (uni_total ? kNodeUniformTotal : 0u);
  if (in.absent) hd.flags |= kNodeAbsent;
  if (path == Path::U64) {
    hd.static_score = in.stat;
  } else {
    const double sd = (double)in.stat;
    std::memcpy(&hd.static_score, &sd, 8);
  }
  std::memcpy(r, &hd, sizeof(hd));
  if (path == Path::N32 && out.sum) {
    uint32_t* s = out.sum;
    if (!out.zeroed) std::memset(s, 0, k1sum_stride(K));
    s[kSumCnLo] = (uint32_t)hd.card_number;
    s[kSumCnHi] = (uint32_t)(hd.card_number >> 32);
    s[kSumMeta] = ((hd.flags & kNodeUniform4) ? kSumUni4 : 0u) |
                  ((hd.flags & kNodeUniformTotal) ? kSumUniTotal : 0u) |
                  (in.zero_total ? kSumZeroTotal : 0u) | (in.absent ? kSumAbsent : 0u) |
                  ((uint32_t)__builtin_popcount(hm) << 8);
    if (cnt > 0) {  // the model values of card 0 (all cards under kSumUni4)
      s[kSumClock] = (uint32_t)in.clock[0];
      s[kSumTotal] = in.tcode[0];
      s[kSumBw] = (uint32_t)in.bandwidth[0];
      s[kSumCore] = (uint32_t)in.core[0];
      s[kSumPower] = (uint32_t)in.power[0];
    }
    uint32_t mrf1 = 0, nhf = 0;
    uint32_t hfs[YODA_MAX_CARDS];
    for (uint32_t j = 0; j < cnt; ++j) {  // N32: free <= 0xFFFFFFFE, so free + 1 fits
      const uint32_t f1 = in.fcode[j] + 1u;
      mrf1 = std::max(mrf1, f1);
      if (in.healthy[j]) hfs[nhf++] = f1;
    }
    std::sort(hfs, hfs + nhf, [](uint32_t x, uint32_t y) { return x > y; });
    s[kSumMrf1] = mrf1;
    for (uint32_t j = 0; j < nhf; ++j) s[kSumHfs + j] = hfs[j];
    // K2 summary: real cards in descending free order (stable: ties keep card order)
    uint32_t* s2 = out.sum2;
    if (!out.zeroed) std::memset(s2, 0, k2sum_stride(K));
    std::memcpy(s2 + kS2Static, &hd.static_score, 8);  // f64 bits (set above)
    s2[kS2Clock] = s[kSumClock];
    s2[kS2Meta] = ((hd.flags & kNodeUniform4) ? kSumUni4 : 0u) | (cnt << 8);
    s2[kS2Bw] = s[kSumBw];
    s2[kS2Core] = s[kSumCore];
    s2[kS2Power] = s[kSumPower];
    uint32_t ord[YODA_MAX_CARDS];
    for (uint32_t j = 0; j < cnt; ++j) ord[j] = j;
    std::stable_sort(ord, ord + cnt, [&](uint32_t x, uint32_t y) {
      return in.free_memory[x] > in.free_memory[y];
    });
    uint32_t* mx = out.mix;
    if (!out.zeroed) std::memset(mx, 0, mix_stride(K));
    uint32_t minclk = 0xffffffffu, hmf = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t b = ord[j];
      s2[kS2Fs + j] = in.fcode[b];
      s2[kS2Fs + K + j] = in.tcode[b];
      // the per-card models in the same order (nodes without kSumUni4 read them)
      mx[mix_word(kMixCk, (int)j, K)] = (uint32_t)in.clock[b];
      mx[mix_word(kMixBw, (int)j, K)] = (uint32_t)in.bandwidth[b];
      mx[mix_word(kMixCo, (int)j, K)] = (uint32_t)in.core[b];
      mx[mix_word(kMixPw, (int)j, K)] = (uint32_t)in.power[b];
      if (in.healthy[b]) hmf |= 1u << j;
      minclk = std::min(minclk, (uint32_t)in.clock[b]);
    }
    mx[mix_hm(K)] = hmf;
    s2[kS2MinClk] = minclk;
    // K1 tile (K1MixWord): prefix maxima per 16-bit half, their change bits, the cards
    // packed, the healthy-card counts per distinct clock
    uint32_t* x = out.x1;
    if (!out.zeroed) std::memset(x, 0, x1_stride(K));
    uint32_t pa = 0, pb = 0, pt = 0, chg = 0, nch = 0;
    auto hmax = [](uint32_t u, uint32_t v) {
      return std::max(u & 0xffffu, v & 0xffffu) | (std::max(u >> 16, v >> 16) << 16);
    };
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t b = ord[j];
      const uint32_t ca = (uint32_t)in.clock[b] | ((uint32_t)in.bandwidth[b] << 16);
      const uint32_t cb = (uint32_t)in.core[b] | ((uint32_t)in.power[b] << 16);
      const uint32_t na = hmax(pa, ca), nb2 = hmax(pb, cb);
      const uint32_t nt = std::max(pt, s2[kS2Fs + K + j]);
      if (j == 0 || na != pa || nb2 != pb || nt != pt) chg |= 1u << (j + 1);
      pa = na;
      pb = nb2;
      pt = nt;
      x[x1_pm((int)j, 0)] = pa;
      x[x1_pm((int)j, 1)] = pb;
      x[x1_pm((int)j, 2)] = pt;
      x[x1_cd((int)j, 0, K)] = ca;
      x[x1_cd((int)j, 1, K)] = cb;
      if (in.healthy[b]) {
        const uint32_t ck = (uint32_t)in.clock[b];
        uint32_t e = 0;
        while (e < nch && (x[kX1Ch + e] & 0xffffu) != ck) ++e;
        if (e == nch) {
          if (nch == 4) {
            chg |= kX1ChgMany;
            continue;
          }
          x[kX1Ch + nch++] = ck;
        }
        x[kX1Ch + e] += 1u << 16;
      }
    }
    x[kX1Chg] = chg;
  }
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint64_t v[6] = {in.free_memory[j], in.clock[j], in.total_memory[j], in.bandwidth[j],
                           in.core[j], in.power[j]};  // CardField order
    if (path == Path::N32) {
      uint32_t* u = reinterpret_cast<uint32_t*>(r + 32);
      for (int f = 0; f < kCardFields; ++f) u[f * K + j] = (uint32_t)v[f];
      u[kFree * K + j] = in.fcode[j];
      u[kTotal * K + j] = in.tcode[j];
      double* d = reinterpret_cast<double*>(r + n32_f64_off(0, K));
      d[kF64Free * K + j] = (double)v[kFree];
      d[kF64Total * K + j] = (double)v[kTotal];
    } else if (path == Path::F64) {
      double* d = reinterpret_cast<double*>(r + 32);
      for (int f = 0; f < kCardFields; ++f) d[f * K + j] = (double)v[f];
    } else {
      uint64_t* u = reinterpret_cast<uint64_t*>(r + 32);
      for (int f = 0; f < kCardFields; ++f) u[f * K + j] = v[f];
    }
  }
  return hd.flags;
}

}  // namespace yoda
