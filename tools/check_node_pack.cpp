// check_node_pack: yoda::pack_node (yoda_node_pack.h; the one per-node packer of
// yoda_upload_nodes and yoda_update_node_cards) on random nodes.
//
//   c++ -std=c++17 -fsanitize=address,undefined -I<hip include dir> -D__HIP_PLATFORM_AMD__
//       -o check_node_pack tools/check_node_pack.cpp && ./check_node_pack
//
// Every row sits in a heap buffer of exactly its size, so that a word written past a row is an
// AddressSanitizer error, not a pass.  Checked per node: hfs descending and zero past the healthy
// count; the K2 cards a stable descending-free order of the inputs; the model rows that
// permutation; the prefix maxima monotone and the change bits consistent with them; and packing
// a node, changing its frees and health, and packing it again into the SAME buffers equals
// packing the changed node into zeroed ones.
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../kubernetes-scheduler_amd/csrc/yoda_node_pack.h"

namespace {

using namespace yoda;

uint64_t rng_state = 0x243f6a8885a308d3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return rnd() % n; }

long checked = 0;

#define REQUIRE(c)                                                                    \
  do {                                                                                \
    if (!(c)) {                                                                       \
      std::printf("check_node_pack FAILED: %s (line %d, K %d, cnt %u)\n", #c, __LINE__, \
                  K, in.cnt);                                                         \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

struct Node {
  uint64_t fr[16], tot[16], ck[16], bw[16], co[16], pw[16];
  uint8_t hl[16];
  uint32_t fc[16], tc[16];
  NodePackIn in;
  void bind(uint32_t cnt) {
    in.cnt = cnt;
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
  void codes() {
    for (uint32_t j = 0; j < in.cnt; ++j) fc[j] = (uint32_t)fr[j], tc[j] = (uint32_t)tot[j];
  }
};

// Rows of exactly their size on the heap.
struct Rows {
  std::unique_ptr<unsigned char[]> rec;
  std::unique_ptr<uint32_t[]> sum, sum2, mix, x1;
  NodePackOut out;
  Rows(Path path, int K, bool zero) {
    const size_t rs = path == Path::N32 ? n32_stride(K) : node_stride(K);
    rec.reset(new unsigned char[rs]);
    sum.reset(new uint32_t[k1sum_stride(K) / 4]);
    sum2.reset(new uint32_t[k2sum_stride(K) / 4]);
    mix.reset(new uint32_t[mix_stride(K) / 4]);
    x1.reset(new uint32_t[x1_stride(K) / 4]);
    const int fill = zero ? 0 : 0xa5;  // a used buffer: whatever an older row left
    std::memset(rec.get(), fill, rs);
    std::memset(sum.get(), fill, k1sum_stride(K));
    std::memset(sum2.get(), fill, k2sum_stride(K));
    std::memset(mix.get(), fill, mix_stride(K));
    std::memset(x1.get(), fill, x1_stride(K));
    out.rec = rec.get();
    out.zeroed = zero;  // the upload's case: rows known to hold zeros are not cleared again
    if (path == Path::N32) {
      out.sum = sum.get();
      out.sum2 = sum2.get();
      out.mix = mix.get();
      out.x1 = x1.get();
    }
  }
};

bool same(const Rows& a, const Rows& b, Path path, int K) {
  const size_t rs = path == Path::N32 ? n32_stride(K) : node_stride(K);
  if (std::memcmp(a.rec.get(), b.rec.get(), rs)) return false;
  if (path != Path::N32) return true;
  return !std::memcmp(a.sum.get(), b.sum.get(), k1sum_stride(K)) &&
         !std::memcmp(a.sum2.get(), b.sum2.get(), k2sum_stride(K)) &&
         !std::memcmp(a.mix.get(), b.mix.get(), mix_stride(K)) &&
         !std::memcmp(a.x1.get(), b.x1.get(), x1_stride(K));
}

void random_node(Node& nd, int K, uint32_t cnt, int style) {
  static const uint64_t clocks[7] = {1200, 1300, 1410, 1500, 1600, 1755, 1980};
  nd.bind(cnt);
  nd.in.card_number = below(3) ? cnt : below(20);
  nd.in.stat = below(500);
  nd.in.zero_total = below(16) == 0;
  nd.in.no_uniform = below(8) == 0;
  const bool mixed = style & 1, many_clocks = style & 2, equal_frees = style & 4;
  const uint64_t ck0 = clocks[below(7)], bw0 = 1 + below(3000), co0 = 1 + below(20000),
                 pw0 = 1 + below(700), tot0 = 1 + below(90000);
  for (uint32_t j = 0; j < cnt; ++j) {
    nd.ck[j] = mixed ? clocks[below(many_clocks ? 7 : 3)] : ck0;
    nd.bw[j] = mixed ? 1 + below(3000) : bw0;
    nd.co[j] = mixed ? 1 + below(20000) : co0;
    nd.pw[j] = mixed ? 1 + below(700) : pw0;
    nd.tot[j] = below(4) == 0 ? 1 + below(90000) : tot0;
    nd.fr[j] = equal_frees ? 1000 * below(3) : below(nd.tot[j] + 1);
    nd.hl[j] = below(5) != 0;
  }
  nd.codes();
}

void check_rows(Path path, int K, const Node& nd, const Rows& r) {
  const NodePackIn& in = nd.in;
  const uint32_t cnt = in.cnt;
  NodeHdrG hd;
  std::memcpy(&hd, r.rec.get(), sizeof(hd));
  uint32_t hm = 0, nh = 0;
  for (uint32_t j = 0; j < cnt; ++j)
    if (in.healthy[j]) hm |= 1u << j, ++nh;
  REQUIRE(hd.healthy_mask == hm && hd.card_number == in.card_number);
  REQUIRE(hd.real_mask == (cnt >= 32 ? ~0u : (1u << cnt) - 1u));
  if (path != Path::N32) return;
  const uint32_t *s = r.sum.get(), *s2 = r.sum2.get(), *mx = r.mix.get(), *x = r.x1.get();
  REQUIRE(((s[kSumMeta] >> 8) & 0xffu) == nh);
  // hfs: descending, zero past the healthy count, the healthy frees + 1 as a multiset
  uint64_t want = 0, got = 0;
  for (uint32_t j = 0; j < cnt; ++j)
    if (in.healthy[j]) want += in.fcode[j] + 1u;
  for (int t = 0; t < K; ++t) {
    const uint32_t v = s[kSumHfs + t];
    if ((uint32_t)t >= nh) REQUIRE(v == 0);
    if (t > 0 && (uint32_t)t < nh) REQUIRE(v <= s[kSumHfs + t - 1]);
    if ((uint32_t)t < nh) REQUIRE(v > 0);
    got += v;
  }
  REQUIRE(got == want);
  // the K2 cards: a stable descending-free order of the inputs; the model rows that permutation
  bool used[16] = {};
  uint32_t hmf = 0, minclk = 0xffffffffu, last_src = 0;
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint32_t f = s2[kS2Fs + j];
    if (j > 0) REQUIRE(f <= s2[kS2Fs + j - 1]);
    // its source: the first unused input card with that free (stable: sources of equal frees rise)
    uint32_t src = 0;
    while (src < cnt && (used[src] || in.fcode[src] != f)) ++src;
    REQUIRE(src < cnt);
    if (j > 0 && f == s2[kS2Fs + j - 1]) REQUIRE(src > last_src);
    used[src] = true;
    last_src = src;
    REQUIRE(s2[kS2Fs + K + j] == in.tcode[src]);
    REQUIRE(mx[mix_word(kMixCk, (int)j, K)] == (uint32_t)in.clock[src]);
    REQUIRE(mx[mix_word(kMixBw, (int)j, K)] == (uint32_t)in.bandwidth[src]);
    REQUIRE(mx[mix_word(kMixCo, (int)j, K)] == (uint32_t)in.core[src]);
    REQUIRE(mx[mix_word(kMixPw, (int)j, K)] == (uint32_t)in.power[src]);
    REQUIRE(x[x1_cd((int)j, 0, K)] == ((uint32_t)in.clock[src] | ((uint32_t)in.bandwidth[src] << 16)));
    REQUIRE(x[x1_cd((int)j, 1, K)] == ((uint32_t)in.core[src] | ((uint32_t)in.power[src] << 16)));
    if (in.healthy[src]) hmf |= 1u << j;
    minclk = minclk < (uint32_t)in.clock[src] ? minclk : (uint32_t)in.clock[src];
  }
  for (int j = (int)cnt; j < K; ++j) REQUIRE(s2[kS2Fs + j] == 0 && s2[kS2Fs + K + j] == 0);
  REQUIRE(mx[mix_hm(K)] == hmf && s2[kS2MinClk] == minclk);
  REQUIRE(((s2[kS2Meta] >> 8) & 0xffu) == cnt);
  // prefix maxima: monotone per 16-bit half; change bit q set exactly where they move
  const uint32_t chg = x[kX1Chg];
  uint32_t pa = 0, pb = 0, pt = 0;
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint32_t a = x[x1_pm((int)j, 0)], b = x[x1_pm((int)j, 1)], t = x[x1_pm((int)j, 2)];
    REQUIRE((a & 0xffffu) >= (pa & 0xffffu) && (a >> 16) >= (pa >> 16));
    REQUIRE((b & 0xffffu) >= (pb & 0xffffu) && (b >> 16) >= (pb >> 16));
    REQUIRE(t >= pt);
    const bool moved = j == 0 || a != pa || b != pb || t != pt;
    REQUIRE(((chg >> (j + 1)) & 1u) == (moved ? 1u : 0u));
    pa = a, pb = b, pt = t;
  }
  REQUIRE((chg & 1u) == 0u);
  for (uint32_t q = cnt + 1; q <= 16; ++q) REQUIRE(((chg >> q) & 1u) == 0u);
  // healthy cards per distinct clock: the counts add up unless there were more than 4 clocks
  uint32_t per = 0;
  for (uint32_t e = 0; e < 4; ++e) per += x[kX1Ch + e] >> 16;
  if (!(chg & kX1ChgMany)) REQUIRE(per == nh);
  else REQUIRE(per < nh);
  ++checked;
}

void one_case(Path path, int K, uint32_t cnt, int style) {
  Node nd;
  random_node(nd, K, cnt, style);
  Rows used(path, K, false);
  pack_node(path, K, nd.in, used.out);
  check_rows(path, K, nd, used);
  // change the frees and the health, pack into the SAME buffers: as a pack into zeroed ones
  for (uint32_t j = 0; j < cnt; ++j) {
    nd.fr[j] = (style & 4) ? 1000 * below(3) : below(nd.tot[j] + 1);
    nd.hl[j] = below(3) != 0;  // (the healthy count often falls)
  }
  if (cnt && below(3) == 0)
    for (uint32_t j = 0; j < cnt; ++j) nd.hl[j] = 0;
  nd.codes();
  nd.in.stat = below(500);
  pack_node(path, K, nd.in, used.out);
  Rows fresh(path, K, true);
  pack_node(path, K, nd.in, fresh.out);
  const NodePackIn& in = nd.in;
  REQUIRE(same(used, fresh, path, K));
  check_rows(path, K, nd, used);
}

}  // namespace

int main() {
  const int Ks[5] = {1, 2, 4, 8, 16};
  for (int K : Ks)
    for (uint32_t cnt = 0; cnt <= (uint32_t)K; ++cnt)
      for (int style = 0; style < 8; ++style)
        for (int rep = 0; rep < 40; ++rep) {
          one_case(Path::N32, K, cnt, style);
          if (rep < 4) one_case(Path::F64, K, cnt, style), one_case(Path::U64, K, cnt, style);
        }
  std::printf("check_node_pack ok: %ld rows checked\n", checked);
  return 0;
}
