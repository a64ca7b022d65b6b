// check_gs_candidates: the capacity greedy session (yoda_greedy_session.{h,cpp}) with candidate
// classes (yoda_gs_set_candidates), on the hand-built windows of tests/greedy_candidate_cases.py.
//
//   c++ -std=c++17 -fsanitize=address,undefined -o check_gs_candidates
//       tools/check_gs_candidates.cpp && ./check_gs_candidates
//
// A capacity window of such a session carries counts and lists over F' = F and cand (the narrowed
// masks) and maxima with witnesses over F (Yoda's Filter alone).  The certificate mixes the two
// sets in one place, scan_lost: a lost node that passed Yoda's Filter at the window start leaves
// F' only if it is the pod's candidate (lf, lz), and leaves the witnesses either way (lw).
//
// Five nodes with one identical card each, lists of one entry, three pods in queue order: pod 0
// takes X's last two cards; pod 1 takes A with enough scv/memory that A's Allocate score falls
// below pod 2's list threshold; pod 2 (class 0, two cards) lists A alone.
//   base    F'(2) = {A, B}; X passed Yoda's Filter for pod 2 but is not its candidate.  Two nodes
//           remain and the unlisted B may outscore A: the resolve stops at pod 2.  (Counting X as
//           lost from F' would leave one node and return A without scoring.)
//   mirror  F'(2) = {A, X}: X is lost, the one node left is A: certified.
//   zero    X and Z zero-total, Z a candidate of class 0 and X not: F'(2) = {A, B, Z}.  Z stays:
//           YODA_PICK_ERROR, certified.  (Counting X in lz would clear the zero-total count.)
// Every array handed to the session is a heap block of exactly its size.
#include "../kubernetes-scheduler_amd/csrc/yoda_greedy_session.cpp"

#include <cstdio>
#include <cstring>

namespace yoda {
int topk_k() { return 8; }
int topk_k_capacity() { return 16; }
}  // namespace yoda

namespace {

#define REQUIRE(c)                                                                     \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      std::printf("check_gs_candidates FAILED: %s (line %d)\n", #c, __LINE__);         \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

enum { A = 0, B = 1, X = 2, Y = 3, Z = 4, N = 5, P = 3 };
enum Variant { kBase, kMirror, kZero };

// a heap copy of exactly n elements
template <class T>
std::vector<T> heap(std::initializer_list<T> v) {
  return std::vector<T>(v);
}

struct Run {
  uint32_t next = 0;
  int32_t pick[P] = {};
};

Run run(Variant v, bool with_candidates) {
  std::vector<uint64_t> cn = heap<uint64_t>({4, 4, 2, 4, 4});
  std::vector<uint64_t> free_sum(N, 500), total(N, 1000), alloc(N, 0);
  if (v == kZero) total[X] = total[Z] = 0;
  std::vector<uint32_t> ccount(N, 1);
  std::vector<uint64_t> c_free(N, 500), c_total(N, 1000), c_clock(N, 1500), c_bw(N, 100),
      c_core(N, 64), c_power(N, 300);
  std::vector<uint8_t> healthy(N, 1);
  yoda_node_soa nd{};
  nd.n_nodes = N, nd.max_cards = 1;
  nd.card_number = cn.data(), nd.card_count = ccount.data();
  nd.free_memory_sum = free_sum.data(), nd.total_memory_sum = total.data();
  nd.alloc_memory = alloc.data();
  nd.card_free_memory = c_free.data(), nd.card_total_memory = c_total.data();
  nd.card_clock = c_clock.data(), nd.card_bandwidth = c_bw.data();
  nd.card_core = c_core.data(), nd.card_power = c_power.data(), nd.card_healthy = healthy.data();

  std::vector<uint8_t> has_number = heap<uint8_t>({1, 1, 1}), has_memory = heap<uint8_t>({0, 1, 0}),
                       has_clock(P, 0);
  std::vector<uint64_t> number = heap<uint64_t>({2, 1, 2}), memory = heap<uint64_t>({0, 600, 0}),
                        clock(P, 0);
  std::vector<int64_t> prio(P, 0);
  yoda_pod_soa pd{};
  pd.n_pods = P;
  pd.has_number = has_number.data(), pd.number = number.data();
  pd.has_memory = has_memory.data(), pd.memory = memory.data();
  pd.has_clock = has_clock.data(), pd.clock = clock.data();
  pd.priority = prio.data();

  std::vector<uint64_t> words(N, 0);
  std::vector<uint8_t> cls;
  std::vector<uint32_t> counts;
  if (v == kBase) {
    words[A] = words[B] = 1;
    cls = heap<uint8_t>({YODA_CAND_ANY, YODA_CAND_ANY, 0});
    counts = heap<uint32_t>({5, 5, 2, 0, 0, 0});
  } else if (v == kMirror) {
    words[A] = words[X] = 1;
    cls = heap<uint8_t>({YODA_CAND_ANY, YODA_CAND_ANY, 0});
    counts = heap<uint32_t>({5, 5, 2, 0, 0, 0});
  } else {
    words[A] |= 1, words[B] |= 1, words[Z] |= 1;  // class 0: pod 2
    words[X] |= 2;                                // class 1: pod 0
    words[A] |= 4, words[Y] |= 4;                 // class 2: pod 1
    cls = heap<uint8_t>({1, 2, 0});
    counts = heap<uint32_t>({1, 2, 3, 1, 0, 1});
  }
  std::vector<double> ts(P, 600.0);
  std::vector<uint32_t> ti = heap<uint32_t>({X, A, A});
  std::vector<uint64_t> mx;
  for (uint64_t m : {100ull, 1500ull, 64ull, 500ull, 300ull, 1000ull})
    for (int i = 0; i < P; ++i) mx.push_back(m);
  std::vector<uint32_t> wc(6 * P, 5), wn(6 * P, 0);

  yoda_gs_t* g = nullptr;
  REQUIRE(yoda_gs_create(&nd, &pd, YODA_GREEDY_CARD_CAPACITY, &g) == YODA_OK);
  if (with_candidates)
    REQUIRE(yoda_gs_set_candidates(g, 3, words.data(), cls.data()) == YODA_OK);
  REQUIRE(yoda_gs_begin_window(g, 0, P, 1, counts.data(), ts.data(), ti.data()) == YODA_OK);
  REQUIRE(yoda_gs_set_witness(g, mx.data(), wc.data(), wn.data()) == YODA_OK);
  // (once a window began the candidates are fixed)
  REQUIRE(yoda_gs_set_candidates(g, 3, words.data(), cls.data()) == YODA_ERR_STATE);
  Run r;
  REQUIRE(yoda_gs_resolve(g, &r.next) == YODA_OK);
  REQUIRE(yoda_gs_picks(g, r.pick, nullptr, nullptr) == YODA_OK);
  REQUIRE(yoda_gs_destroy(g) == YODA_OK);
  return r;
}

void arguments() {
  std::vector<uint64_t> cn(2, 4), sums(2, 100), words(2, 1);
  std::vector<uint8_t> hn(2, 0), hm(2, 0), cls = heap<uint8_t>({0, 7});
  std::vector<uint64_t> num(2, 0), mem(2, 0);
  yoda_node_soa nd{};
  nd.n_nodes = 2, nd.max_cards = 1;
  nd.card_number = cn.data(), nd.free_memory_sum = sums.data(), nd.total_memory_sum = sums.data();
  yoda_pod_soa pd{};
  pd.n_pods = 2;
  pd.has_number = hn.data(), pd.number = num.data(), pd.has_memory = hm.data(),
  pd.memory = mem.data();
  for (uint32_t flags : {0u, (uint32_t)YODA_GREEDY_CARD_CAPACITY}) {
    yoda_gs_t* g = nullptr;
    REQUIRE(yoda_gs_create(&nd, &pd, flags, &g) == YODA_OK);
    REQUIRE(yoda_gs_set_candidates(nullptr, 1, words.data(), nullptr) == YODA_ERR_INVALID_ARG);
    REQUIRE(yoda_gs_set_candidates(g, 65, words.data(), nullptr) == YODA_ERR_INVALID_ARG);
    REQUIRE(yoda_gs_set_candidates(g, 1, nullptr, nullptr) == YODA_ERR_INVALID_ARG);
    REQUIRE(yoda_gs_set_candidates(g, 7, words.data(), cls.data()) == YODA_ERR_RANGE);  // 7 >= 7
    REQUIRE(yoda_gs_set_candidates(g, 8, words.data(), cls.data()) == YODA_OK);
    cls[1] = YODA_CAND_ANY;
    REQUIRE(yoda_gs_set_candidates(g, 1, words.data(), cls.data()) == YODA_OK);
    REQUIRE(yoda_gs_set_candidates(g, 1, words.data(), nullptr) == YODA_OK);  // every pod ANY
    REQUIRE(yoda_gs_set_candidates(g, 0, nullptr, nullptr) == YODA_OK);       // cleared
    REQUIRE(g->cand_words.empty() && g->cand_cls.empty());
    cls[1] = 7;
    REQUIRE(yoda_gs_destroy(g) == YODA_OK);
  }
}

}  // namespace

int main() {
  arguments();
  Run r = run(kBase, true);
  REQUIRE(r.next == 2 && r.pick[0] == X && r.pick[1] == A);
  r = run(kBase, false);  // what ignoring the words gives: the one node "left", unscored
  REQUIRE(r.next == 3 && r.pick[2] == A);
  r = run(kMirror, true);
  REQUIRE(r.next == 3 && r.pick[0] == X && r.pick[1] == A && r.pick[2] == A);
  r = run(kZero, true);
  REQUIRE(r.next == 3 && r.pick[0] == X && r.pick[1] == A && r.pick[2] == YODA_PICK_ERROR);
  r = run(kZero, false);  // X counted in lz: the zero-total node believed gone
  REQUIRE(r.next == 2);
  std::printf("check_gs_candidates ok\n");
  return 0;
}
