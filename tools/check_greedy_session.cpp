// check_greedy_session: the host-side greedy session (yoda_greedy_session.{h,cpp}), flags 0,
// driven the way the greedy drivers drive it, on random small clusters, against a plain
// sequential loop over the same model.
//
//   c++ -std=c++17 -fsanitize=address,undefined -o check_greedy_session
//       tools/check_greedy_session.cpp && ./check_greedy_session
//
// The model: pod p fits node n or not, fixed per pair (flags 0: a pick changes no feasibility),
// and scores it dyn(p, n) + static_score(n), dyn fixed per pair -- the shape of the real score,
// where only the node's Allocate + Actual part moves inside a batch.  Some nodes have
// TotalMemorySum == 0 (the Error outcome), some start a few hundred below 2^64 of allocated
// memory, so Allocate wraps mid-window and their score rises; pods have none, one or many
// feasible nodes.  A stand-in for the device holds the node state it was last pushed
// (yoda_gs_take_dirty) and answers from it: windows of top-k lists, k smaller than the feasible
// counts so that certificates do fail, refreshed lists (yoda_gs_uncertified / yoda_gs_refresh),
// and the exact answer for a pod the session cannot certify (yoda_gs_assign).  Every pick must
// be the sequential loop's (none / the only node / error / argmax by score desc, node asc), and
// yoda_gs_touched_original must return every touched node to its original state.  Every list
// buffer is a heap block of exactly its size: a read past a list is an AddressSanitizer error.
#include "../kubernetes-scheduler_amd/csrc/yoda_greedy_session.cpp"

#include <cstdio>
#include <cstring>

// the kernels' list depths (yoda_kernels.hip), which only the shard-list merge reads
namespace yoda {
int topk_k() { return 8; }
int topk_k_capacity() { return 16; }
}  // namespace yoda

namespace {

uint64_t rng_state = 0x243f6a8885a308d3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int seed_now = 0;
#define REQUIRE(c)                                                                           \
  do {                                                                                       \
    if (!(c)) {                                                                              \
      std::printf("check_greedy_session FAILED: %s (line %d, seed %d)\n", #c, __LINE__,      \
                  seed_now);                                                                 \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)

struct Model {
  uint32_t N, P;
  std::vector<uint64_t> free_sum, total_sum, alloc, card_number;
  std::vector<uint8_t> has_memory, has_number, feas;  // feas [P][N]
  std::vector<uint64_t> memory, number;
  std::vector<int64_t> prio;
  std::vector<double> dyn;  // [P][N]
  double score(uint32_t p, uint32_t n, const std::vector<uint64_t>& al) const {
    bool z;
    return dyn[(size_t)p * N + n] + (double)static_score(free_sum[n], total_sum[n], al[n], &z);
  }
  // one scheduling cycle of pod p against the node state `al` (k8s' outcome rules)
  int32_t cycle(uint32_t p, const std::vector<uint64_t>& al) const {
    uint32_t nf = 0, nz = 0, first = 0;
    double bs = -1.0;
    int32_t bi = YODA_PICK_NONE;
    for (uint32_t n = 0; n < N; ++n) {
      if (!feas[(size_t)p * N + n]) continue;
      if (nf++ == 0) first = n;
      nz += total_sum[n] == 0;
      const double s = score(p, n, al);
      if (s > bs) bs = s, bi = (int32_t)n;  // (ascending n: the lowest node of a tie stays)
    }
    if (nf == 0) return YODA_PICK_NONE;
    if (nf == 1) return (int32_t)first;
    return nz ? YODA_PICK_ERROR : bi;
  }
  void assume(uint32_t p, int32_t n, std::vector<uint64_t>& al) const {
    if (n >= 0 && has_memory[p]) al[n] += memory[p];  // uint64 wrap
  }
};

Model make_model() {
  Model m;
  m.N = 1 + (uint32_t)(rnd() % 40);
  m.P = 1 + (uint32_t)(rnd() % 300);
  const uint32_t N = m.N, P = m.P;
  m.free_sum.resize(N), m.total_sum.resize(N), m.alloc.resize(N), m.card_number.resize(N);
  for (uint32_t n = 0; n < N; ++n) {
    m.total_sum[n] = rnd() % 6 == 0 ? 0 : 4000 + rnd() % 60000;
    m.free_sum[n] = m.total_sum[n] ? rnd() % (m.total_sum[n] + 1) : 0;
    m.alloc[n] = rnd() % 4 == 0 ? 0ull - (1 + rnd() % 300) : rnd() % 3000;
    m.card_number[n] = rnd() % 9;
  }
  m.has_memory.resize(P), m.has_number.resize(P), m.memory.resize(P), m.number.resize(P);
  m.prio.resize(P), m.feas.assign((size_t)P * N, 0), m.dyn.resize((size_t)P * N);
  for (uint32_t p = 0; p < P; ++p) {
    m.has_memory[p] = rnd() % 8 != 0;
    m.memory[p] = 1 + rnd() % 400;
    m.has_number[p] = rnd() % 2;
    m.number[p] = rnd() % 4;
    m.prio[p] = (int64_t)(rnd() % 5) - 2;
    // none, one, a few or most of the nodes feasible
    const uint32_t kind = (uint32_t)(rnd() % 10);
    const uint32_t pct = kind == 0 ? 0 : kind == 1 ? 3 : kind < 5 ? 30 : 90;
    for (uint32_t n = 0; n < N; ++n) {
      m.feas[(size_t)p * N + n] = rnd() % 100 < pct;
      m.dyn[(size_t)p * N + n] = (double)(rnd() % 40);  // few values: ties, close races
    }
    if (kind == 1) {
      std::fill(m.feas.begin() + (size_t)p * N, m.feas.begin() + (size_t)(p + 1) * N, 0);
      m.feas[(size_t)p * N + rnd() % N] = 1;
    }
  }
  return m;
}

// The "device": its node state is what the session's dirty lists pushed.
struct Device {
  const Model& m;
  std::vector<uint64_t> alloc, card_number;
  explicit Device(const Model& x) : m(x), alloc(x.alloc), card_number(x.card_number) {}
  void set(uint32_t cnt, const uint32_t* nodes, const uint64_t* al, const uint64_t* cn) {
    for (uint32_t t = 0; t < cnt; ++t) {
      REQUIRE(nodes[t] < m.N);
      alloc[nodes[t]] = al[t];
      card_number[nodes[t]] = cn[t];
    }
  }
  // window pod p's top-k list, [k][wn] or (row_major) [wn][k], from the current state
  uint32_t list(uint32_t p, uint32_t i, uint32_t wn, uint32_t k, bool row_major, double* ts,
                uint32_t* ti, uint32_t* nz) const {
    std::vector<std::pair<double, uint32_t>> c;
    *nz = 0;
    for (uint32_t n = 0; n < m.N; ++n)
      if (m.feas[(size_t)p * m.N + n]) {
        c.push_back({m.score(p, n, alloc), n});
        *nz += m.total_sum[n] == 0;
      }
    std::sort(c.begin(), c.end(), [](const auto& a, const auto& b) {
      return a.first > b.first || (a.first == b.first && a.second < b.second);
    });
    for (uint32_t kk = 0; kk < k; ++kk) {
      const size_t o = row_major ? (size_t)i * k + kk : (size_t)kk * wn + i;
      ts[o] = kk < c.size() ? c[kk].first : -1.0;
      ti[o] = kk < c.size() ? c[kk].second : 0xffffffffu;
    }
    return (uint32_t)c.size();
  }
};

struct Totals {
  long pods = 0, certified = 0, exact = 0, refreshes = 0, wraps = 0, none = 0, only = 0,
       error = 0, windows = 0;
} tot;

void run(int seed) {
  seed_now = seed;
  const Model m = make_model();
  const uint32_t N = m.N, P = m.P;
  // the sequential loop
  std::vector<uint32_t> order;
  queue_order(m.prio.data(), P, order);
  std::vector<int32_t> want(P);
  {
    std::vector<uint64_t> al(m.alloc);
    for (uint32_t q = 0; q < P; ++q) {
      const uint32_t p = order[q];
      want[p] = m.cycle(p, al);
      const uint64_t before = want[p] >= 0 ? al[want[p]] : 0;
      m.assume(p, want[p], al);
      tot.wraps += want[p] >= 0 && al[want[p]] < before;
      tot.none += want[p] == YODA_PICK_NONE, tot.error += want[p] == YODA_PICK_ERROR;
    }
  }
  // the session
  yoda_node_soa nv{};
  nv.n_nodes = N, nv.max_cards = 1;
  nv.card_number = m.card_number.data();
  nv.free_memory_sum = m.free_sum.data();
  nv.total_memory_sum = m.total_sum.data();
  nv.alloc_memory = m.alloc.data();
  yoda_pod_soa pv{};
  pv.n_pods = P;
  pv.has_memory = m.has_memory.data(), pv.memory = m.memory.data();
  pv.has_number = m.has_number.data(), pv.number = m.number.data();
  pv.priority = m.prio.data();
  yoda_gs_t* g = nullptr;
  REQUIRE(yoda_gs_create(&nv, &pv, 0, &g) == YODA_OK);
  std::vector<uint32_t> gorder(P);
  REQUIRE(yoda_gs_queue_order(g, gorder.data()) == YODA_OK && gorder == order);
  Device dev(m);
  auto push = [&] {
    std::vector<uint32_t> ids(N);
    std::vector<uint64_t> al(N), cn(N);
    uint32_t got = 0;
    REQUIRE(yoda_gs_take_dirty(g, N, ids.data(), al.data(), cn.data(), &got) == YODA_OK);
    dev.set(got, ids.data(), al.data(), cn.data());
  };
  const uint32_t k = 1 + (uint32_t)(rnd() % 4);
  const bool borrow = seed % 2 == 1, row_major = borrow && seed % 4 == 1;
  const uint32_t every = 1 + (uint32_t)(rnd() % 3), scan = 4 + (uint32_t)(rnd() % 12), bar = 2;
  for (uint32_t ws = 0; ws < P;) {
    const uint32_t wn = std::min<uint32_t>(P - ws, 1 + (uint32_t)(rnd() % 90));
    push();
    // exactly sized heap blocks, alive until the window ends (the borrowed form reads them then)
    std::vector<uint32_t> counts(2 * (size_t)wn), ti((size_t)k * wn);
    std::vector<double> ts((size_t)k * wn);
    for (uint32_t i = 0; i < wn; ++i)
      counts[i] = dev.list(order[ws + i], i, wn, k, row_major, ts.data(), ti.data(),
                           &counts[(size_t)wn + i]);
    REQUIRE((borrow ? gs_begin_window_at(g, ws, wn, k, counts.data(), ts.data(), ti.data(), true,
                                         row_major)
                    : yoda_gs_begin_window(g, ws, wn, k, counts.data(), ts.data(), ti.data())) ==
            YODA_OK);
    ++tot.windows;
    uint32_t next = 0, since = 0;
    for (;;) {
      REQUIRE(yoda_gs_resolve(g, &next) == YODA_OK);
      if (next >= wn) break;
      if (++since >= every && wn - next >= 2) {
        since = 0;
        uint32_t unc = 0;
        REQUIRE(yoda_gs_uncertified(g, next + 1, scan, &unc) == YODA_OK);
        if (unc >= bar) {
          push();
          std::vector<uint32_t> ti2((size_t)k * wn, 0xffffffffu), nz(1);
          std::vector<double> ts2((size_t)k * wn, -1.0);
          for (uint32_t i = next; i < wn; ++i)
            dev.list(order[ws + i], i, wn, k, false, ts2.data(), ti2.data(), nz.data());
          REQUIRE(yoda_gs_refresh(g, next, ts2.data(), ti2.data()) == YODA_OK);
          ++tot.refreshes;
          const uint32_t stuck = next;
          REQUIRE(yoda_gs_resolve(g, &next) == YODA_OK);
          if (next != stuck) continue;
        }
      }
      push();
      REQUIRE(yoda_gs_assign(g, ws + next, m.cycle(order[ws + next], dev.alloc)) == YODA_OK);
    }
    ws += wn;
  }
  std::vector<int32_t> got(P);
  uint32_t resolved = 0, assigned = 0;
  REQUIRE(yoda_gs_picks(g, got.data(), &resolved, &assigned) == YODA_OK);
  REQUIRE(resolved + assigned == P);
  for (uint32_t p = 0; p < P; ++p) REQUIRE(got[p] == want[p]);
  tot.pods += P, tot.certified += resolved, tot.exact += assigned;
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t nf = 0;
    for (uint32_t n = 0; n < N; ++n) nf += m.feas[(size_t)p * N + n];
    tot.only += nf == 1;
  }
  // the device ends on the sequential loop's state, and the restore list undoes all of it
  push();
  {
    std::vector<uint64_t> al(m.alloc);
    for (uint32_t q = 0; q < P; ++q) m.assume(order[q], want[order[q]], al);
    REQUIRE(dev.alloc == al && dev.card_number == m.card_number);
  }
  std::vector<uint32_t> ids(N);
  std::vector<uint64_t> al(N), cn(N);
  uint32_t n_back = 0;
  REQUIRE(yoda_gs_touched_original(g, N, ids.data(), al.data(), cn.data(), &n_back) == YODA_OK);
  dev.set(n_back, ids.data(), al.data(), cn.data());
  REQUIRE(dev.alloc == m.alloc && dev.card_number == m.card_number);
  REQUIRE(yoda_gs_destroy(g) == YODA_OK);
}

}  // namespace

int main() {
  for (int seed = 0; seed < 400; ++seed) run(seed);
  // the inputs reached every branch the check is about
  seed_now = -1;
  REQUIRE(tot.certified > 0 && tot.exact > 0 && tot.refreshes > 0 && tot.wraps > 0);
  REQUIRE(tot.none > 0 && tot.only > 0 && tot.error > 0);
  std::printf("check_greedy_session ok: %ld pods in %ld windows, %ld certified, %ld exact, "
              "%ld refreshes, %ld wraps\n", tot.pods, tot.windows, tot.certified, tot.exact,
              tot.refreshes, tot.wraps);
  return 0;
}
