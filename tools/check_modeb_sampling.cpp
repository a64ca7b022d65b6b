// check_modeb_sampling: the walk plan of Mode B under node sampling (yoda_modeb.h disk_plan_walk,
// disk_plan_whole, disk_select64, disk_in_walk -- as k2b_samp_plan, k2b_sampled, k2b_rows and the
// rows' host-filled bitmask use them) against a brute-force walk over E: start, start + 1, ...,
// wrapping at the snapshot's end, until M eligible nodes are taken.
//
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I<hip include dir>
//       -D__HIP_PLATFORM_AMD__ -o check_modeb_sampling tools/check_modeb_sampling.cpp
//       && ./check_modeb_sampling
//
// The rank rows live in heap buffers of exactly ceil(N / 64) words, so a read past a row (the
// binary search, the start's block) is an AddressSanitizer error, and a shift out of range in the
// select an UBSan one.
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../kubernetes-scheduler_amd/csrc/yoda_modeb.h"

namespace {

using namespace yoda;

uint64_t rng_state = 0x243f6a8885a308d3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

long n_checked = 0;

#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      std::fprintf(stderr, "FAIL %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, "\n");           \
      std::exit(1);                         \
    }                                       \
  } while (0)

// One selector's rows from its eligibility flags, as k_modeb_rank_build / _scan leave them: the
// tail bits of the last block clear, pfx the exclusive counts.
struct Rows {
  uint32_t nb, total;
  std::unique_ptr<uint64_t[]> bits;
  std::unique_ptr<uint32_t[]> pfx;
};

Rows rows_of(const std::vector<uint8_t>& el) {
  const uint32_t n = (uint32_t)el.size();
  Rows r;
  r.nb = (n + 63u) / 64u;
  r.bits.reset(new uint64_t[r.nb]());
  r.pfx.reset(new uint32_t[r.nb]());
  for (uint32_t i = 0; i < n; ++i)
    if (el[i]) r.bits[i >> 6] |= 1ull << (i & 63u);
  r.total = 0;
  for (uint32_t b = 0; b < r.nb; ++b) {
    r.pfx[b] = r.total;
    r.total += (uint32_t)__builtin_popcountll(r.bits[b]);
  }
  return r;
}

// The walk itself: the sample's flags, |S| and next_start (the (M + 1)-th eligible node met, or
// start when the walk comes full circle first).
struct Brute {
  std::vector<uint8_t> in;
  uint32_t n_sample, next_start;
};

Brute brute(const std::vector<uint8_t>& el, uint32_t start, uint32_t m) {
  const uint32_t n = (uint32_t)el.size();
  Brute b{std::vector<uint8_t>(n, 0), 0u, start};
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = (uint32_t)(((uint64_t)start + k) % n);
    if (!el[i]) continue;
    if (b.n_sample == m) {
      b.next_start = i;
      break;
    }
    b.in[i] = 1;
    ++b.n_sample;
  }
  return b;
}

void check_one(const std::vector<uint8_t>& el, const Rows& r, uint32_t start, uint32_t m,
               const char* tag) {
  const uint32_t n = (uint32_t)el.size();
  const Brute want = brute(el, start, m);
  const DiskWalkPlan pl = disk_plan_walk(r.bits.get(), r.pfx.get(), r.nb, r.total, start, m);
  CHECK(pl.n_found == r.total, "%s N %u start %u M %u", tag, n, start, m);
  CHECK(pl.n_sample == want.n_sample, "%s N %u start %u M %u: |S| %u, want %u", tag, n, start, m,
        pl.n_sample, want.n_sample);
  CHECK(pl.next_start == want.next_start, "%s N %u start %u M %u T %u: next_start %u, want %u",
        tag, n, start, m, r.total, pl.next_start, want.next_start);
  CHECK((pl.walk.full != 0u) == (r.total <= m), "%s N %u start %u M %u: full", tag, n, start, m);
  uint32_t got = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const bool in = el[i] && disk_in_walk(i, pl.walk);
    CHECK(in == (want.in[i] != 0), "%s N %u start %u M %u T %u: node %u in S %d, want %d", tag, n,
          start, m, r.total, i, (int)in, (int)want.in[i]);
    got += in ? 1u : 0u;
  }
  CHECK(got == pl.n_sample, "%s: count", tag);
  ++n_checked;
}

// Every E whole: the arithmetic plan against the same brute force over all-eligible flags.
void check_whole(uint32_t n, uint32_t start, uint32_t m) {
  const std::vector<uint8_t> el(n, 1);
  const Brute want = brute(el, start, m);
  const DiskWalkPlan pl = disk_plan_whole(n, start, m);
  CHECK(pl.n_found == n && pl.n_sample == want.n_sample && pl.next_start == want.next_start,
        "whole N %u start %u M %u: |S| %u / %u next %u / %u", n, start, m, pl.n_sample,
        want.n_sample, pl.next_start, want.next_start);
  for (uint32_t i = 0; i < n; ++i)
    CHECK(disk_in_walk(i, pl.walk) == (want.in[i] != 0), "whole N %u start %u M %u: node %u", n,
          start, m, i);
  ++n_checked;
}

void check_select() {
  for (int t = 0; t < 4000; ++t) {
    uint64_t x = rnd();
    if (t % 4 == 1) x &= rnd() & rnd();
    if (t % 4 == 2) x |= rnd() | rnd();
    if (t == 0) x = 1ull;
    if (t == 1) x = 1ull << 63;
    if (t == 2) x = ~0ull;
    uint32_t r = 0;
    for (uint32_t i = 0; i < 64; ++i)
      if ((x >> i) & 1ull) {
        CHECK(disk_select64(x, r) == i, "select64(%016llx, %u) = %u, want %u",
              (unsigned long long)x, r, disk_select64(x, r), i);
        ++r;
      }
  }
}

// Eligibility flags with exactly `total` set bits (total <= n), at random places.
std::vector<uint8_t> flags_with(uint32_t n, uint32_t total) {
  std::vector<uint8_t> el(n, 0);
  uint32_t left = total;
  for (uint32_t i = 0; i < n; ++i) {  // selection sampling: every subset of that size alike
    if (rnd() % (n - i) < left) {
      el[i] = 1;
      --left;
    }
  }
  return el;
}

void check_shape(uint32_t n) {
  // starts: both ends, the block boundaries, the last partial block, random ones
  std::vector<uint32_t> starts = {0u, n - 1u, n / 2u};
  for (uint32_t s : {63u, 64u, 65u, 127u, 128u}) if (s < n) starts.push_back(s);
  if (n > 64u) starts.push_back((n - 1u) / 64u * 64u);  // the first node of the last block
  for (int i = 0; i < 6; ++i) starts.push_back((uint32_t)(rnd() % n));
  const std::vector<uint32_t> ms = {1u, 7u, 63u, 64u, 100u, 500u, n, n + 3u};
  // the arithmetic plan
  for (uint32_t s : starts)
    for (uint32_t m : ms) check_whole(n, s, m);
  // random densities (presence and a candidate word's bit alike: flags), the whole and the
  // empty set, a single node
  for (double dens : {0.0, 0.02, 0.5, 0.97, 1.0}) {
    std::vector<uint8_t> el(n, 0);
    for (uint32_t i = 0; i < n; ++i) el[i] = (double)(rnd() >> 11) / 9007199254740992.0 < dens;
    const Rows r = rows_of(el);
    for (uint32_t s : starts)
      for (uint32_t m : ms) check_one(el, r, s, m, "random");
  }
  // whole blocks without an eligible node between eligible ones (equal prefix counts)
  {
    std::vector<uint8_t> el(n, 0);
    for (uint32_t i = 0; i < n; ++i) el[i] = ((i >> 6) % 3u == 1u) && (rnd() & 1ull);
    el[n - 1] = 1;
    const Rows r = rows_of(el);
    for (uint32_t s : starts)
      for (uint32_t m : ms) check_one(el, r, s, m, "sparse blocks");
  }
  // T of 0, 1, M and M + 1
  for (uint32_t m : {1u, 7u, 100u}) {
    for (uint32_t total : {0u, 1u, m, m + 1u}) {
      if (total > n) continue;
      const std::vector<uint8_t> el = flags_with(n, total);
      const Rows r = rows_of(el);
      CHECK(r.total == total, "flags_with");
      for (uint32_t s : starts) check_one(el, r, s, m, "T");
      // ... with the start on an eligible node, just before one and just after one
      for (uint32_t i = 0; i < n; ++i) {
        if (!el[i]) continue;
        check_one(el, r, i, m, "T at");
        check_one(el, r, (i + n - 1u) % n, m, "T before");
        check_one(el, r, (i + 1u) % n, m, "T after");
      }
    }
  }
}

}  // namespace

int main() {
  check_select();
  for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 900u, 5000u}) check_shape(n);
  // the walk predicate's three forms by hand
  CHECK(disk_in_walk(5, DiskWalk{9, 9, 1}) && disk_in_walk(0, DiskWalk{0, 0, 1}), "full");
  CHECK(disk_in_walk(3, DiskWalk{3, 7, 0}) && disk_in_walk(6, DiskWalk{3, 7, 0}) &&
            !disk_in_walk(7, DiskWalk{3, 7, 0}) && !disk_in_walk(2, DiskWalk{3, 7, 0}),
        "one segment");
  CHECK(disk_in_walk(8, DiskWalk{8, 2, 0}) && disk_in_walk(1, DiskWalk{8, 2, 0}) &&
            !disk_in_walk(2, DiskWalk{8, 2, 0}) && !disk_in_walk(7, DiskWalk{8, 2, 0}),
        "wrapped");
  std::printf("check_modeb_sampling ok: %ld plans\n", n_checked);
  return 0;
}
