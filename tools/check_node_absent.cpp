// check_node_absent: the presence bits of yoda::pack_node (yoda_node_pack.h NodePackIn::absent,
// yoda_set_node_present) on random nodes of every record path.
//
//   c++ -std=c++17 -fsanitize=address,undefined -I<hip include dir> -D__HIP_PLATFORM_AMD__
//       -o check_node_absent tools/check_node_absent.cpp && ./check_node_absent
//
// Packing a node absent and packing it present differ in exactly two words: kNodeAbsent in the
// record header's flags and, on the N32 path, kSumAbsent in the K1 summary's meta -- every other
// word of the record, both summaries, the model row and the K1 tile is the same, so a node that
// returns shows what it would have shown had it never left.  The new bits overlap no other field
// of their words (the uniform flags, the zero-total flag, the healthy count at << 8), and packing
// over a row of the other state leaves what a pack into zeroed rows leaves.  Every row sits in a
// heap buffer of exactly its size: a word written past it is an AddressSanitizer error.
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kubernetes-scheduler_amd/csrc/yoda_node_pack.h"

namespace {

using namespace yoda;

uint64_t rng_state = 0x13198a2e03707344ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

#define REQUIRE(c)                                                                        \
  do {                                                                                    \
    if (!(c)) {                                                                           \
      std::printf("check_node_absent FAILED: %s (line %d, path %d, K %d, cnt %u)\n", #c, \
                  __LINE__, (int)path, K, cnt);                                           \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)

// One node's rows, each in a heap buffer of exactly its size.
struct Rows {
  std::vector<unsigned char> rec;
  std::vector<uint32_t> sum, sum2, mix, x1;
  NodePackOut out;
  Rows(Path path, int K, int fill)
      : rec(path == Path::N32 ? n32_stride(K) : node_stride(K), (unsigned char)fill),
        sum(k1sum_stride(K) / 4, 0x01010101u * (uint32_t)fill),
        sum2(k2sum_stride(K) / 4, 0x01010101u * (uint32_t)fill),
        mix(mix_stride(K) / 4, 0x01010101u * (uint32_t)fill),
        x1(x1_stride(K) / 4, 0x01010101u * (uint32_t)fill) {
    out.rec = rec.data();
    out.zeroed = fill == 0;
    if (path == Path::N32) {
      out.sum = sum.data();
      out.sum2 = sum2.data();
      out.mix = mix.data();
      out.x1 = x1.data();
    }
  }
};

long checked = 0;

void check(Path path, int K, uint32_t cnt, int style) {
  uint64_t fr[16], tot[16], ck[16], bw[16], co[16], pw[16];
  uint8_t hl[16];
  uint32_t fc[16], tc[16];
  for (uint32_t j = 0; j < cnt; ++j) {
    const bool one = style == 0;  // one GPU model with one TotalMemory
    tot[j] = one ? 16384 : 8192 + 8192 * (rnd() % 3);
    fr[j] = rnd() % (tot[j] + 1);
    ck[j] = one ? 1500 : 1200 + 100 * (rnd() % 6);
    bw[j] = one ? 900 : 700 + 100 * (rnd() % 4);
    co[j] = one ? 108 : 80 + (rnd() % 40);
    pw[j] = one ? 400 : 250 + 50 * (rnd() % 5);
    hl[j] = rnd() % 4 != 0;
    fc[j] = (uint32_t)fr[j];
    tc[j] = (uint32_t)tot[j];
  }
  NodePackIn in;
  in.cnt = cnt;
  in.card_number = rnd() % 9;
  in.stat = rnd() % 500;
  in.zero_total = style == 2;
  in.no_uniform = style == 3;
  in.free_memory = fr;
  in.total_memory = tot;
  in.clock = ck;
  in.bandwidth = bw;
  in.core = co;
  in.power = pw;
  in.healthy = hl;
  in.fcode = fc;
  in.tcode = tc;
  Rows here(path, K, 0), gone(path, K, 0), over(path, K, 0xa5), back(path, K, 0xa5);
  in.absent = false;
  const uint32_t f0 = pack_node(path, K, in, here.out);
  in.absent = true;
  const uint32_t f1 = pack_node(path, K, in, gone.out);
  REQUIRE((f0 & kNodeAbsent) == 0u && f1 == (f0 | kNodeAbsent));
  // the record: only the header's flags word (offset 28) differs, by that bit
  NodeHdrG h0, h1;
  std::memcpy(&h0, here.rec.data(), sizeof(h0));
  std::memcpy(&h1, gone.rec.data(), sizeof(h1));
  REQUIRE(h0.flags == f0 && h1.flags == f1);
  REQUIRE((kNodeAbsent & (kNodeUniform4 | kNodeUniformTotal)) == 0u);
  h1.flags &= ~kNodeAbsent;
  std::memcpy(gone.rec.data(), &h1, sizeof(h1));
  REQUIRE(here.rec == gone.rec);
  if (path == Path::N32) {
    const uint32_t m0 = here.sum[kSumMeta], m1 = gone.sum[kSumMeta];
    REQUIRE((m0 & kSumAbsent) == 0u && m1 == (m0 | kSumAbsent));
    REQUIRE((kSumAbsent & (kSumUni4 | kSumUniTotal | kSumZeroTotal | 0xffffff00u)) == 0u);
    uint32_t nh = 0;
    for (uint32_t j = 0; j < cnt; ++j) nh += hl[j] ? 1u : 0u;
    REQUIRE(((m1 >> 8) & 0xffu) == nh);  // the healthy count is read past the new bit
    gone.sum[kSumMeta] = m0;
    REQUIRE(here.sum == gone.sum && here.sum2 == gone.sum2 && here.mix == gone.mix &&
            here.x1 == gone.x1);
  }
  // over a used row of the other state: what a pack into zeroed rows leaves
  in.absent = false;
  pack_node(path, K, in, over.out);
  in.absent = true;
  pack_node(path, K, in, over.out);
  pack_node(path, K, in, gone.out);
  REQUIRE(over.rec == gone.rec);
  in.absent = false;
  pack_node(path, K, in, over.out);
  pack_node(path, K, in, back.out);
  REQUIRE(over.rec == here.rec && back.rec == here.rec);
  if (path == Path::N32)
    REQUIRE(over.sum == here.sum && over.sum2 == here.sum2 && over.mix == here.mix &&
            over.x1 == here.x1);
  ++checked;
}

}  // namespace

int main() {
  const Path paths[3] = {Path::N32, Path::F64, Path::U64};
  for (Path path : paths)
    for (int K = 1; K <= 16; K *= 2)
      for (uint32_t cnt = 0; cnt <= (uint32_t)K; ++cnt)
        for (int style = 0; style < 4; ++style)
          for (int rep = 0; rep < 8; ++rep) check(path, K, cnt, style);
  static_assert(kBsAbsent == 8u && (kBsAbsent & (kBsOneModel | kBsUni4 | kBsHcTab)) == 0u,
                "kBsAbsent overlaps a block-summary flag");
  std::printf("check_node_absent ok: %ld nodes\n", checked);
  return 0;
}
