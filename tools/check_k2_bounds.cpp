// check_k2_bounds: the block kernels' level indices (yoda_layout.h kb_level_lo / kb_level_hi: a
// popcount of one compare per level) against the sequential searches they replace.
//
//   c++ -std=c++17 -fsanitize=address,undefined -I<hip include dir> -D__HIP_PLATFORM_AMD__
//       -o check_k2_bounds tools/check_k2_bounds.cpp && ./check_k2_bounds
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../kubernetes-scheduler_amd/csrc/yoda_layout.h"

namespace {

uint64_t rng_state = 0x2545f4914f6cdd1dull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

long checked = 0;
[[noreturn]] void fail(const char* what, uint64_t a, uint64_t b, uint64_t c) {
  std::printf("check_k2_bounds FAILED: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a,
              (unsigned long long)b, (unsigned long long)c);
  std::exit(1);
}

// ---- the level indices --------------------------------------------------------------------
// the searches of the block kernels before the ballot form (K2: l_lo, K1: l_hi)
uint32_t seq_lo(const std::vector<uint32_t>& lv, uint32_t m_min) {
  uint32_t l_lo = 0;
  for (uint32_t l = 1; l < lv.size(); ++l) l_lo = lv[l] <= m_min ? l : l_lo;
  return l_lo;
}
uint32_t seq_hi(const std::vector<uint32_t>& lv, uint32_t m_max) {
  uint32_t l_hi = (uint32_t)lv.size() - 1u;
  for (uint32_t l = (uint32_t)lv.size() - 1u; l-- > 0u;) l_hi = lv[l] >= m_max ? l : l_hi;
  return l_hi;
}
// the kernels' form: lane l compares its level, the ballot is the mask (lanes past the table
// hold a copy of a level: their bits must not count)
void check_levels_at(const std::vector<uint32_t>& lv, uint32_t m) {
  const uint32_t L = (uint32_t)lv.size();
  uint64_t le = 0, lt = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t lev = lv[lane & (L - 1u)];
    if (lev <= m) le |= 1ull << lane;
    if (lev < m) lt |= 1ull << lane;
  }
  if (yoda::kb_level_lo(le, L) != seq_lo(lv, m)) fail("kb_level_lo", L, m, yoda::kb_level_lo(le, L));
  if (yoda::kb_level_hi(lt, L) != seq_hi(lv, m)) fail("kb_level_hi", L, m, yoda::kb_level_hi(lt, L));
  ++checked;
}
void check_table(const std::vector<uint32_t>& lv) {
  for (uint32_t t : lv) {  // at a level, one below, one above
    check_levels_at(lv, t);
    if (t > 0u) check_levels_at(lv, t - 1u);
    if (t < 0xffffffffu) check_levels_at(lv, t + 1u);
  }
  check_levels_at(lv, 0u);
  check_levels_at(lv, 0xffffffffu);
}
// L strictly increasing levels, first 0, last 0xFFFFFFFF; the interior ones below `top`
std::vector<uint32_t> random_table(uint32_t L, uint32_t top) {
  std::vector<uint32_t> lv(L);
  for (;;) {
    lv[0] = 0u;
    lv[L - 1] = 0xffffffffu;
    for (uint32_t l = 1; l + 1 < L; ++l) lv[l] = 1u + (uint32_t)(rnd() % (top - 1u));
    std::vector<uint32_t> in(lv.begin() + 1, lv.end() - 1);
    for (size_t i = 1; i < in.size(); ++i)  // insertion sort
      for (size_t j = i; j > 0 && in[j - 1] > in[j]; --j) std::swap(in[j - 1], in[j]);
    bool ok = true;
    for (size_t i = 1; i < in.size(); ++i) ok = ok && in[i - 1] < in[i];
    if (!ok) continue;
    for (uint32_t l = 1; l + 1 < L; ++l) lv[l] = in[l - 1];
    return lv;
  }
}

}  // namespace

int main() {
  // the level indices: small tables exhaustively (every m in a small range, every table of
  // 4 levels over it), then tables of 32 and 64 levels
  for (uint32_t a = 1; a < 12; ++a)
    for (uint32_t b = a + 1; b < 13; ++b) {
      const std::vector<uint32_t> lv = {0u, a, b, 0xffffffffu};
      for (uint32_t m = 0; m < 16; ++m) check_levels_at(lv, m);
      check_table(lv);
    }
  for (uint32_t L : {32u, 64u}) {
    {  // the densest table: consecutive levels
      std::vector<uint32_t> lv(L);
      for (uint32_t l = 0; l < L; ++l) lv[l] = l;
      lv[L - 1] = 0xffffffffu;
      check_table(lv);
      for (uint32_t m = 0; m < 2 * L; ++m) check_levels_at(lv, m);
    }
    {  // levels up to the top of the range
      std::vector<uint32_t> lv(L);
      for (uint32_t l = 0; l < L; ++l) lv[l] = 0xffffffffu - (L - 1u - l);
      lv[0] = 0u;
      check_table(lv);
    }
    for (int t = 0; t < 200; ++t) {
      const std::vector<uint32_t> lv = random_table(L, t % 2 ? 0xffffffffu : 100000u);
      check_table(lv);
      for (int i = 0; i < 2500; ++i)  // 2 x 200 x 2500 = 10^6 random bounds
        check_levels_at(lv, (uint32_t)(i % 2 ? rnd() : rnd() % 100001u));
    }
  }
  std::printf("check_k2_bounds ok: %ld cases\n", checked);
  return 0;
}
