// check_modeb_elig: the Mode B batch path's accumulator, settle and merges with eligibility
// (yoda_modeb.h, as the k2b_*<ELIG = true> kernels and k_reduce2b use them) against a brute-force
// loop over E, for both launch forms' merge orders, the pod-class builder, and the shared score
// (disk_score, disk_absdiff) against the level table of the earlier host-only form.
//
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I<hip include dir>
//       -D__HIP_PLATFORM_AMD__ -o check_modeb_elig tools/check_modeb_elig.cpp && ./check_modeb_elig
//
// Records, eligibility words and partials live in heap buffers of exactly their size, so a walk
// past a chunk's or the snapshot's end is an AddressSanitizer error, not a pass.
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "../kubernetes-scheduler_amd/csrc/yoda_modeb.h"

namespace {

using namespace yoda;

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// trunc(10 - 10 |d|) when >= 1, else 0 (algorithm.go:110-111, then Uint64ToInt64); no FMA: the
// volatile form libyoda's level table was built with before disk_score, kept as the yardstick
double score_of(double l) {
  volatile double t = 10.0 * l;
  volatile double s = 10.0 - t;
  return s >= 1.0 ? std::trunc((double)s) : 0.0;
}

// t[k]: the largest |d| whose score is >= k, by bisection over the double bit patterns
DiskLevels levels(double (*score)(double) = score_of) {
  DiskLevels d{};
  d.t[0] = HUGE_VAL;
  d.t[11] = -1.0;
  for (int k = 1; k <= 10; ++k) {
    uint64_t lo = 0, hi = 0x7ff0000000000000ull;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      double x;
      std::memcpy(&x, &mid, 8);
      if (score(x) >= (double)k) lo = mid; else hi = mid;
    }
    std::memcpy(&d.t[k], &lo, 8);
  }
  return d;
}

struct Want {
  int64_t lev;
  uint32_t cnt, idx;
};

double abs_d(double al, double be, const NodeRecB& r) {
  volatile double a = al * r.v;
  volatile double b = be * r.u;
  return std::fabs((double)a - (double)b);
}

long checked = 0;

int fail(const char* what, uint32_t n_nodes, uint32_t chunk, uint32_t c, const Want& w,
         const DiskBest& g) {
  std::printf("check_modeb_elig: %s: N %u chunk %u class %u: want (%lld, %u, %u) got (%lld, %u, %u)\n",
              what, n_nodes, chunk, c, (long long)w.lev, w.cnt, w.idx, (long long)g.lev, g.cnt,
              g.idx);
  return 1;
}

// One snapshot: n_nodes records, words and presence, n_cls classes, chunks of `chunk` nodes.
// zero: every score 0 (V = 10).  hole: the nodes of [hole0, hole1) are ineligible for every class.
int trial(const DiskLevels& lv, uint32_t n_nodes, uint32_t chunk, uint32_t n_cls, bool zero,
          double p_absent, double p_bit, uint32_t hole0, uint32_t hole1) {
  std::unique_ptr<NodeRecB[]> nodes(new NodeRecB[n_nodes]);
  std::unique_ptr<DiskElig[]> elig(new DiskElig[n_nodes]);
  for (uint32_t n = 0; n < n_nodes; ++n) {
    nodes[n].v = zero ? 10.0 : unit();
    nodes[n].u = zero ? 0.0 : unit() * 2.0;
    uint64_t w = 0;
    for (int b = 0; b < 64; ++b) w |= (unit() < p_bit ? 1ull : 0ull) << b;
    const bool present = unit() >= p_absent;
    elig[n] = disk_elig_of(present, w);
    if (n >= hole0 && n < hole1) elig[n] = DiskElig{0ull, 0ull};
    if (!present && (elig[n].lo | elig[n].hi)) return std::printf("elig_of: absent node with bits\n"), 1;
  }
  std::vector<double> al(n_cls), be(n_cls);
  std::vector<uint32_t> sel(n_cls);
  const uint32_t sels[] = {0u, 1u, 31u, 32u, 62u, 63u, kDiskSelAny};
  for (uint32_t c = 0; c < n_cls; ++c) {
    al[c] = c == 1 ? std::nan("") : unit() * 1.5;  // a NaN pod: every node scores 0
    be[c] = zero ? 0.0 : unit();
    sel[c] = c < 7 ? sels[c] : (uint32_t)(rnd() % kDiskSelCount);
  }
  const uint32_t C = (n_nodes + chunk - 1) / chunk;
  std::unique_ptr<uint32_t[]> plc(new uint32_t[(size_t)C * n_cls]), pix(new uint32_t[(size_t)C * n_cls]);
  for (int form = 0; form < 2; ++form) {  // 0: lane = class, 1: lane = node
    for (uint32_t k = 0; k < C; ++k) {
      const uint32_t n0 = k * chunk, n1 = std::min(n0 + chunk, n_nodes);
      for (uint32_t c = 0; c < n_cls; ++c) {
        uint32_t word, idx;
        if (form == 0) {  // one lane walks the chunk in node order, branch-free; level 0 walks
          DiskAcc s;      // the words again (k2b_class_lanes<.., true>)
          DiskSeen sn;
          const DiskSelMask sm = disk_sel_mask(sel[c]);
          disk_init(s, lv.t);
          disk_seen_init(sn);
          for (uint32_t n = n0; n < n1; ++n) {
            if (disk_eligible(elig[n], sm) != disk_eligible(elig[n], sel[c]))
              return std::printf("check_modeb_elig: mask test differs, sel %u\n", sel[c]), 1;
            disk_step_masked(s, disk_eligible(elig[n], sm), abs_d(al[c], be[c], nodes[n]), n, lv.t);
          }
          if (s.lev == 0u)
            for (uint32_t n = n0; n < n1; ++n) disk_seen_add(sn, disk_eligible(elig[n], sm), n);
          uint32_t cnt;
          disk_settle(s, sn, cnt, idx);
          word = disk_pack(s.lev, cnt);
        } else {  // kBlock lanes stride over the chunk; lanes of a wave, then the waves
          DiskBest wg;
          disk_best_init(wg);
          for (int w = 0; w < kBlock / kWave; ++w) {
            DiskBest wave;
            disk_best_init(wave);
            for (int l = 0; l < kWave; ++l) {
              DiskAcc s;
              DiskSeen sn;
              disk_init(s, lv.t);
              disk_seen_init(sn);
              for (uint32_t n = n0 + (uint32_t)(w * kWave + l); n < n1; n += kBlock)
                if (disk_eligible(elig[n], sel[c])) disk_step_elig(s, sn, abs_d(al[c], be[c], nodes[n]), n, lv.t);
              uint32_t mc, mi;
              disk_settle(s, sn, mc, mi);
              disk_merge_any(wave, s.lev, mc, mi);
            }
            disk_merge_any(wg, wave.lev < 0 ? 0u : (uint32_t)wave.lev, wave.cnt, wave.idx);
          }
          word = wg.cnt ? disk_pack((uint32_t)wg.lev, wg.cnt) : 0u;
          idx = wg.idx;
        }
        plc[(size_t)k * n_cls + c] = word;
        pix[(size_t)k * n_cls + c] = idx;
      }
    }
    for (uint32_t c = 0; c < n_cls; ++c) {
      Want w{-1, 0, 0xffffffffu};
      for (uint32_t n = 0; n < n_nodes; ++n) {
        if (!disk_eligible(elig[n], sel[c])) continue;
        const int64_t L = (int64_t)score_of(abs_d(al[c], be[c], nodes[n]));
        if (L > w.lev) w = Want{L, 1, n};
        else if (L == w.lev) ++w.cnt;
      }
      DiskBest g;
      disk_best_init(g);
      for (uint32_t k = 0; k < C; ++k) disk_merge_chunk(g, plc[(size_t)k * n_cls + c], &pix[(size_t)k * n_cls + c]);
      if (g.lev != w.lev || g.cnt != w.cnt || g.idx != w.idx)
        return fail(form ? "lane = node" : "lane = class", n_nodes, chunk, c, w, g);
      ++checked;
    }
  }
  return 0;
}

// disk_build_classes: pods are in one class exactly when their (alpha, beta, selector) agree;
// classes are numbered by first appearance; without class bytes the selector is ANY for all.
int classes_trial(uint32_t n_pods, bool bytes) {
  std::unique_ptr<uint64_t[]> al(new uint64_t[n_pods]), be(new uint64_t[n_pods]);
  std::unique_ptr<uint8_t[]> cb(new uint8_t[n_pods]);
  const uint8_t choice[] = {0, 1, 5, 63, 0xFF};
  for (uint32_t p = 0; p < n_pods; ++p) {
    al[p] = rnd() % 4;
    be[p] = (rnd() % 3) << 40;
    cb[p] = choice[rnd() % 5];
  }
  DiskClasses dc;
  disk_build_classes(al.get(), be.get(), bytes ? cb.get() : nullptr, n_pods, dc);
  std::map<std::tuple<uint64_t, uint64_t, uint32_t>, uint32_t> seen;
  if (dc.cls.size() != n_pods) return std::printf("classes: cls size\n"), 1;
  for (uint32_t p = 0; p < n_pods; ++p) {
    const uint32_t s = bytes ? disk_sel(cb[p]) : kDiskSelAny;
    auto key = std::make_tuple(al[p], be[p], s);
    auto it = seen.find(key);
    if (it == seen.end()) it = seen.emplace(key, (uint32_t)seen.size()).first;
    const uint32_t c = dc.cls[p];
    if (c != it->second || c >= dc.alpha.size() || dc.alpha[c] != al[p] || dc.beta[c] != be[p] ||
        dc.sel[c] != s)
      return std::printf("classes: pod %u of %u (bytes %d): class %u, want %u\n", p, n_pods,
                         (int)bytes, c, it->second), 1;
  }
  if (seen.size() != dc.alpha.size() || dc.sel.size() != dc.alpha.size() ||
      dc.beta.size() != dc.alpha.size())
    return std::printf("classes: %zu classes, want %zu\n", dc.alpha.size(), seen.size()), 1;
  ++checked;
  return 0;
}

}  // namespace

int main() {
  const DiskLevels lv = levels();
  // the shared score (yoda_modeb.h disk_score, disk_absdiff; contraction off by their own pragma,
  // so this holds under -ffp-contract=fast too) gives the level table bit for bit, and the
  // volatile forms' values on random pairs
  {
    const DiskLevels shared = levels([](double l) { return disk_score(l); });
    if (std::memcmp(shared.t, lv.t, sizeof lv.t) != 0)
      return std::printf("check_modeb_elig: disk_score moves the level table\n"), 1;
    for (int i = 0; i < 200000; ++i) {
      const NodeRecB r{unit() * 3.0, unit() * 3.0};
      const double al = unit() * 2.0, be = unit() * 2.0;
      const double want = abs_d(al, be, r), got = disk_absdiff(al, r.v, be, r.u);
      if (std::memcmp(&want, &got, 8) != 0 || score_of(want) != disk_score(got))
        return std::printf("check_modeb_elig: disk_absdiff / disk_score differ at %d\n", i), 1;
    }
    for (int k = 0; k < 12; ++k) std::printf("t[%2d] = %a\n", k, lv.t[k]);
  }
  // the selector's bit: class 63 is bit 63 of lo, ANY is presence alone
  {
    const DiskElig e = disk_elig_of(true, 1ull << 63), a = disk_elig_of(false, ~0ull);
    const DiskElig z = disk_elig_of(true, 0ull);
    if (!disk_eligible(e, 63) || disk_eligible(e, 62) || disk_eligible(e, 0) ||
        !disk_eligible(e, kDiskSelAny) || disk_eligible(a, kDiskSelAny) || disk_eligible(a, 63) ||
        !disk_eligible(z, kDiskSelAny) || disk_eligible(z, 0))
      return std::printf("check_modeb_elig: disk_eligible\n"), 1;
    if (disk_sel(0xFF) != kDiskSelAny || disk_sel(63) != 63u || disk_sel(0) != 0u)
      return std::printf("check_modeb_elig: disk_sel\n"), 1;
  }
  const uint32_t chunks[] = {1, 7, 8, 9, 64, 255, 256, 257, 2048};
  const uint32_t sizes[] = {1, 2, 7, 8, 9, 63, 65, 300, 2047, 2049, 4500};
  for (uint32_t n : sizes)
    for (uint32_t ch : chunks) {
      if ((uint64_t)(n + ch - 1) / ch > 600) continue;  // (chunk 1 on the small sizes only)
      for (int rep = 0; rep < 3; ++rep) {
        const bool zero = rep == 2;
        const double pa = rep == 0 ? 0.3 : 0.05, pb = rep == 1 ? 0.1 : 0.6;
        // no hole; the first chunk (and the first node of the next) ineligible; a middle stretch
        const uint32_t holes[3][2] = {{0, 0}, {0, std::min(n, ch + 1)}, {n / 3, n / 3 + 2 * ch}};
        for (auto& hl : holes)
          if (trial(lv, n, ch, 9, zero, pa, pb, hl[0], std::min(hl[1], n))) return 1;
      }
      // nothing eligible at all; everything eligible
      if (trial(lv, n, ch, 8, false, 1.0, 0.5, 0, 0)) return 1;
      if (trial(lv, n, ch, 8, false, 0.0, 1.0, 0, 0)) return 1;
      if (trial(lv, n, ch, 8, true, 0.0, 1.0, 0, 0)) return 1;
    }
  for (uint32_t p : {0u, 1u, 2u, 31u, 64u, 700u, 5000u})
    for (int b = 0; b < 2; ++b)
      if (classes_trial(p, b != 0)) return 1;
  std::printf("check_modeb_elig ok: %ld checks\n", checked);
  return 0;
}
