// check_node_replace: yoda::pack_node (yoda_node_pack.h) packing ANOTHER node over a node's rows,
// as yoda_replace_nodes does: another card count, other GPU models, another presence bit.
//
//   c++ -std=c++17 -fsanitize=address,undefined -I<hip include dir> -D__HIP_PLATFORM_AMD__
//       -o check_node_replace tools/check_node_replace.cpp && ./check_node_replace
//
// Every row sits in a heap buffer of exactly its size, so that a word written past a row is an
// AddressSanitizer error.  A node of a cards is packed, then a node of b cards (every pair
// 0..K x 0..K, one-model and mixed-model either way) into the SAME buffers: the rows must equal
// the second node's pack into zeroed buffers -- no card, hfs entry, model word, change bit or
// clock count of the larger, older node survives -- and its returned flags must be those of the
// fresh pack (the one-model counts of a handle are kept from them).
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
uint64_t below(uint64_t n) { return rnd() % n; }

struct Node {
  uint64_t fr[16], tot[16], ck[16], bw[16], co[16], pw[16];
  uint8_t hl[16];
  uint32_t fc[16], tc[16];
  NodePackIn in;
  Node(uint32_t cnt, bool mixed) {
    static const uint64_t clocks[6] = {1200, 1410, 1500, 1600, 1755, 1980};
    const uint64_t ck0 = clocks[below(6)], bw0 = 1 + below(3000), co0 = 1 + below(20000),
                   pw0 = 1 + below(700), tot0 = 1 + below(90000);
    for (uint32_t j = 0; j < cnt; ++j) {
      ck[j] = mixed ? clocks[below(6)] : ck0;
      bw[j] = mixed ? 1 + below(3000) : bw0;
      co[j] = mixed ? 1 + below(20000) : co0;
      pw[j] = mixed ? 1 + below(700) : pw0;
      tot[j] = mixed && below(2) ? 1 + below(90000) : tot0;
      fr[j] = below(tot[j] + 1);
      hl[j] = below(5) != 0;
      fc[j] = (uint32_t)fr[j];
      tc[j] = (uint32_t)tot[j];
    }
    in.cnt = cnt;
    in.card_number = below(3) ? cnt : below(20);
    in.stat = below(500);
    in.zero_total = cnt == 0 || below(16) == 0;
    in.absent = below(4) == 0;
    in.free_memory = fr;
    in.total_memory = tot;
    in.clock = ck;
    in.bandwidth = bw;
    in.core = co;
    in.power = pw;
    in.healthy = hl;
    in.fcode = fc;
    in.tcode = tc;
  }
};

// Rows of exactly their size on the heap (vectors: freed on every path).
struct Rows {
  std::vector<unsigned char> rec;
  std::vector<uint32_t> sum, sum2, mix, x1;
  NodePackOut out;
  Rows(Path path, int K, bool zero)
      : rec(path == Path::N32 ? n32_stride(K) : node_stride(K), zero ? 0 : 0xa5),
        sum(k1sum_stride(K) / 4, zero ? 0u : 0xa5a5a5a5u),
        sum2(k2sum_stride(K) / 4, zero ? 0u : 0xa5a5a5a5u),
        mix(mix_stride(K) / 4, zero ? 0u : 0xa5a5a5a5u),
        x1(x1_stride(K) / 4, zero ? 0u : 0xa5a5a5a5u) {
    out.rec = rec.data();
    out.zeroed = zero;
    if (path == Path::N32) {
      out.sum = sum.data();
      out.sum2 = sum2.data();
      out.mix = mix.data();
      out.x1 = x1.data();
    }
  }
  bool same(const Rows& o, Path path) const {
    if (rec != o.rec) return false;
    return path != Path::N32 || (sum == o.sum && sum2 == o.sum2 && mix == o.mix && x1 == o.x1);
  }
};

long checked = 0;

void one_case(Path path, int K, uint32_t a, uint32_t b, bool mixed_a, bool mixed_b) {
  Node old_node(a, mixed_a), new_node(b, mixed_b);
  Rows used(path, K, false);
  pack_node(path, K, old_node.in, used.out);
  const uint32_t f_used = pack_node(path, K, new_node.in, used.out);
  Rows fresh(path, K, true);
  const uint32_t f_fresh = pack_node(path, K, new_node.in, fresh.out);
  const bool one = b > 0 && !mixed_b;
  if (!used.same(fresh, path) || f_used != f_fresh ||
      ((f_used & kNodeAbsent) != 0u) != new_node.in.absent ||
      (one && (f_used & (kNodeUniform4 | kNodeUniformTotal)) !=
                  (kNodeUniform4 | kNodeUniformTotal)) ||
      (b == 0 && (f_used & kNodeUniform4))) {
    std::printf("check_node_replace FAILED: path %d K %d cards %u -> %u mixed %d -> %d\n",
                (int)path, K, a, b, (int)mixed_a, (int)mixed_b);
    std::exit(1);
  }
  ++checked;
}

}  // namespace

int main() {
  const int Ks[5] = {1, 2, 4, 8, 16};
  const Path paths[3] = {Path::N32, Path::F64, Path::U64};
  for (Path path : paths)
    for (int K : Ks)
      for (uint32_t a = 0; a <= (uint32_t)K; ++a)
        for (uint32_t b = 0; b <= (uint32_t)K; ++b)
          for (int m = 0; m < 4; ++m)
            for (int rep = 0; rep < (path == Path::N32 ? 6 : 2); ++rep)
              one_case(path, K, a, b, (m & 1) != 0, (m & 2) != 0);
  std::printf("check_node_replace ok: %ld replacements checked\n", checked);
  return 0;
}
