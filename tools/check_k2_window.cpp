// check_k2_window: yoda::window_bits (yoda_layout.h; the block K2's 64-block window of a
// block-list row) against a bit-by-bit reference.
//
//   c++ -std=c++17 -fsanitize=address,undefined -I<hip include dir> -D__HIP_PLATFORM_AMD__
//       -o check_k2_window tools/check_k2_window.cpp && ./check_k2_window
//
// The row is heap-allocated with exactly row_words words, so that a helper reading the word
// after the row (another wave's, or the seeds) is an AddressSanitizer error, not a pass.
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../kubernetes-scheduler_amd/csrc/yoda_layout.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// bit j of the window: block wb + j is below b1, inside the row, and listed
uint64_t reference(const uint64_t* row, uint32_t row_words, uint32_t wb, uint32_t b1) {
  uint64_t out = 0;
  for (uint32_t j = 0; j < 64; ++j) {
    const uint32_t b = wb + j;
    if (b >= b1 || (b >> 6) >= row_words) continue;
    if ((row[b >> 6] >> (b & 63u)) & 1ull) out |= 1ull << j;
  }
  return out;
}

long checked = 0;

int check_chunk(const uint64_t* row, uint32_t row_words, uint32_t b0, uint32_t b1, const char* what) {
  // the walk of the block K2: windows wb = b0, b0 + 64, ... while wb < b1
  uint32_t seen = 0;
  for (uint32_t wb = b0; wb < b1; wb += 64) {
    const uint64_t got = yoda::window_bits(row, row_words, wb, b1);
    const uint64_t want = reference(row, row_words, wb, b1);
    ++checked;
    if (got != want) {
      std::fprintf(stderr, "window_bits(%s, row_words=%u, wb=%u, b1=%u) = %016llx, want %016llx\n",
                   what, row_words, wb, b1, (unsigned long long)got, (unsigned long long)want);
      return 1;
    }
    seen += (uint32_t)__builtin_popcountll(got);
  }
  // every listed block of [b0, b1) in exactly one window
  uint32_t listed = 0;
  for (uint32_t b = b0; b < b1; ++b) listed += (uint32_t)((row[b >> 6] >> (b & 63u)) & 1ull);
  if (seen != listed) {
    std::fprintf(stderr, "%s row_words=%u [%u, %u): %u blocks in the windows, %u listed\n", what,
                 row_words, b0, b1, seen, listed);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  const uint32_t shifts[] = {0, 1, 31, 49, 63};
  const uint32_t lens[] = {1, 15, 49, 63, 64, 65, 79, 128, 129};
  int bad = 0;
  for (uint32_t row_words = 1; row_words <= 3; ++row_words) {
    // exactly row_words words on the heap: the word after them is not the row's
    std::unique_ptr<uint64_t[]> row(new uint64_t[row_words]);
    for (int fill = 0; fill < 10; ++fill) {  // all-zeros, all-ones, 8 random rows
      for (uint32_t w = 0; w < row_words; ++w)
        row[w] = fill == 0 ? 0ull : fill == 1 ? ~0ull : (fill & 1) ? rnd() : rnd() & rnd();
      const char* what = fill == 0 ? "zeros" : fill == 1 ? "ones" : "random";
      for (uint32_t base = 0; base < row_words; ++base)  // the word the chunk starts in
        for (uint32_t sh : shifts)
          for (uint32_t len : lens) {
            const uint32_t b0 = 64 * base + sh, b1 = b0 + len;
            // a chunk lies inside the row's blocks (its end may be anywhere in the last word:
            // len = 64 - sh, 128 - sh ... end a chunk on the row's last bit)
            if (b1 > 64 * row_words) continue;
            bad |= check_chunk(row.get(), row_words, b0, b1, what);
          }
      // chunks that end on the last bit of the row (windows ending in the row's last word, and
      // shifted windows whose second word would be the one past the row)
      for (uint32_t sh : shifts)
        for (uint32_t base = 0; base < row_words; ++base) {
          const uint32_t b0 = 64 * base + sh, b1 = 64 * row_words;
          if (b0 < b1) bad |= check_chunk(row.get(), row_words, b0, b1, what);
          if (b0 + 1 < b1) bad |= check_chunk(row.get(), row_words, b0, b1 - 1, what);
          // an end past the row (no caller has one): a window that starts inside the row still
          // reads no word after it, and the blocks past the row are unlisted
          for (uint32_t over : {1u, 15u, 64u}) {
            if (b0 >= b1) continue;
            const uint64_t got = yoda::window_bits(row.get(), row_words, b0, b1 + over);
            ++checked;
            if (got != reference(row.get(), row_words, b0, b1 + over)) {
              std::fprintf(stderr, "window_bits(%s, row_words=%u, wb=%u, b1=%u past the row)\n", what,
                           row_words, b0, b1 + over);
              bad = 1;
            }
          }
        }
    }
  }
  if (bad) return 1;
  std::printf("check_k2_window ok: %ld windows\n", checked);
  return 0;
}
