// check_k2_help: two host/device pieces of the block K2 (yoda_layout.h): the argmax fold that
// merges partial results (k_reduce2, k_reduce2_finalize), and the walk's next-block pick.  The
// pick is also run as the claim step of a protocol no kernel uses yet -- several threads sharing
// one window word through atomic ANDs -- which lives in this file only.
//
//   c++ -std=c++17 -pthread -fsanitize=address,undefined -I<hip include dir>
//       -D__HIP_PLATFORM_AMD__ -o check_k2_help tools/check_k2_help.cpp && ./check_k2_help
#include <hip/hip_runtime.h>  // __host__ / __device__, as the host side of libyoda has them

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
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
  std::printf("check_k2_help FAILED: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a,
              (unsigned long long)b, (unsigned long long)c);
  std::exit(1);
}

using yoda::ArgmaxState;
bool same(const ArgmaxState& a, const ArgmaxState& b) {
  // (an empty state is empty whatever its idx / ties hold: both stay at their initial values)
  return a.best == b.best && a.idx == b.idx && a.ties == b.ties;
}
ArgmaxState fold(ArgmaxState a, const ArgmaxState& b) {
  yoda::argmax_fold(a, b);
  return a;
}

// ---- the fold ------------------------------------------------------------------------------
struct Node {
  int64_t score;  // below 0: infeasible
  uint32_t idx;
};
// the sequential argmax of a node list in any order: ties counted, lowest index kept
ArgmaxState sequential(const std::vector<Node>& nodes) {
  ArgmaxState s;
  for (const Node& n : nodes) {
    if (n.score < 0) continue;
    if (n.score > s.best) {
      s.best = n.score;
      s.idx = n.idx;
      s.ties = 1;
    } else if (n.score == s.best) {
      ++s.ties;
      if (n.idx < s.idx) s.idx = n.idx;
    }
  }
  return s;
}

void check_algebra(const std::vector<ArgmaxState>& st) {
  const ArgmaxState empty;
  for (const ArgmaxState& a : st) {
    if (!same(fold(a, empty), a) || !same(fold(empty, a), a)) fail("identity", a.best, a.idx, a.ties);
    for (const ArgmaxState& b : st) {
      if (!same(fold(a, b), fold(b, a))) fail("commutative", a.best, b.best, a.idx);
      for (const ArgmaxState& c : st) {
        if (!same(fold(fold(a, b), c), fold(a, fold(b, c)))) fail("associative", a.best, b.best, c.best);
        ++checked;
      }
    }
  }
}

// every partition of a node list into `parts` sets (by a random assignment), folded in a random
// order, equals the sequential argmax of the whole list
void check_partitions(const std::vector<Node>& nodes, uint32_t parts) {
  const ArgmaxState want = sequential(nodes);
  for (int rep = 0; rep < 8; ++rep) {
    std::vector<std::vector<Node>> sets(parts);
    for (const Node& n : nodes) sets[rnd() % parts].push_back(n);
    std::vector<ArgmaxState> ps;
    for (const auto& s : sets) ps.push_back(sequential(s));
    for (size_t i = ps.size(); i > 1; --i) std::swap(ps[i - 1], ps[rnd() % i]);  // fold order
    ArgmaxState got;
    for (const ArgmaxState& p : ps) yoda::argmax_fold(got, p);
    if (!same(got, want)) fail("partition", (uint64_t)want.best, want.idx, want.ties);
    ++checked;
  }
}

// ---- the claim protocol ----------------------------------------------------------------------
// Four threads share one window word as an owner wave and its helpers would: each reads the word,
// picks a bit (k2_claim_pick), clears it with fetch_and and owns the block if the returned value
// still had the bit; between blocks it drops a random part of the pruned set.  The blocks of
// `prune` are dropped by somebody before the end, at a random time.
struct ClaimLog {
  std::vector<uint32_t> claimed;      // in claim order
  std::vector<uint64_t> dropped_seen; // the drops this thread had applied before each claim
};
void claim_worker(std::atomic<uint64_t>* word, uint64_t hot, uint64_t prune, uint64_t seed,
                  std::atomic<uint64_t>* dropped_all, ClaimLog* log) {
  uint64_t s = seed;
  auto r = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 17;
  };
  for (;;) {
    // a refresh: drop some of the pruned blocks (an AND with the candidate mask)
    const uint64_t drop = prune & r() & r();
    if (drop != 0ull) {
      // (the word first, then the record: a drop that a claimer finds recorded was complete
      // on the word before that claim's own fetch_and, so the claim cannot have the bit)
      word->fetch_and(~drop, std::memory_order_acq_rel);
      dropped_all->fetch_or(drop, std::memory_order_acq_rel);
    }
    const uint64_t seen = word->load(std::memory_order_acquire);
    if (seen == 0ull) break;
    const uint32_t j = yoda::k2_claim_pick(seen, hot);
    if (j >= 64u || ((seen >> j) & 1ull) == 0ull) fail("pick outside the word", seen, hot, j);
    const uint64_t before_drop = dropped_all->load(std::memory_order_acquire);
    const uint64_t old = word->fetch_and(~(1ull << j), std::memory_order_acq_rel);
    if ((old >> j) & 1ull) {
      log->claimed.push_back(j);
      log->dropped_seen.push_back(before_drop);
    }
  }
}

void check_claims(uint64_t list, uint64_t hot, uint64_t prune) {
  std::atomic<uint64_t> word(list), dropped_all(0ull);
  ClaimLog logs[4];
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back(claim_worker, &word, hot, prune, rnd(), &dropped_all, &logs[t]);
  for (auto& x : th) x.join();
  if (word.load() != 0ull) fail("word not drained", word.load(), list, prune);
  uint64_t got = 0ull;
  for (const ClaimLog& l : logs)
    for (size_t i = 0; i < l.claimed.size(); ++i) {
      const uint64_t bit = 1ull << l.claimed[i];
      if ((list & bit) == 0ull) fail("claim outside the list", list, l.claimed[i], 0);
      if (got & bit) fail("claimed twice", list, l.claimed[i], 0);
      // a bit whose drop was complete (recorded) before the claim began is never claimed
      if (l.dropped_seen[i] & bit) fail("claimed after its drop", list, l.claimed[i], prune);
      got |= bit;
    }
  // every listed block that nobody pruned is claimed exactly once; a pruned one at most once
  if ((list & ~prune) & ~got) fail("unpruned block never claimed", list, prune, got);
  if (got & ~list) fail("claims outside the list", list, prune, got);
  // every block is accounted for: claimed, or dropped
  if (list & ~(got | dropped_all.load())) fail("block lost", list, prune, got);
  ++checked;
}

}  // namespace

int main() {
  // the fold: states that include empty, a score of 0, equal scores with different indices and
  // scores near 2^52
  const int64_t big = (int64_t)1 << 52;
  std::vector<ArgmaxState> st;
  st.push_back(ArgmaxState{});
  for (int64_t b : {(int64_t)0, (int64_t)1, (int64_t)7, big - 2, big - 1, big})
    for (uint32_t ix : {0u, 5u, 63u, 64u, 0xfffffffeu})
      for (uint32_t tt : {1u, 2u, 1000u}) {
        ArgmaxState s;
        s.best = b;
        s.idx = ix;
        s.ties = tt;
        st.push_back(s);
      }
  check_algebra(st);
  // partitions of node lists: few distinct scores (many ties), zeros, infeasible nodes, 2^52
  for (int rep = 0; rep < 400; ++rep) {
    const uint32_t n = 1u + (uint32_t)(rnd() % 300u);
    const int kind = rep % 4;
    std::vector<Node> nodes(n);
    for (uint32_t i = 0; i < n; ++i) {
      int64_t s;
      if (kind == 0) s = (int64_t)(rnd() % 3u);                          // 0, 1, 2: ties, zeros
      else if (kind == 1) s = big - 1 - (int64_t)(rnd() % 4u);           // near 2^52
      else if (kind == 2) s = (rnd() % 4u) ? -1 : (int64_t)(rnd() % 2u);  // mostly infeasible
      else s = (int64_t)(rnd() >> 12);                                   // below 2^52, distinct
      nodes[i] = Node{s, i};
    }
    for (size_t i = nodes.size(); i > 1; --i) std::swap(nodes[i - 1], nodes[rnd() % i]);
    for (uint32_t parts : {1u, 2u, 4u, 7u}) check_partitions(nodes, parts);
  }
  {  // all infeasible, and the empty list
    std::vector<Node> none(10, Node{-1, 3});
    check_partitions(none, 4);
    check_partitions({}, 4);
  }
  // the claim protocol over random list, hot and prune masks (and the edge masks)
  check_claims(~0ull, 0ull, 0ull);
  check_claims(~0ull, ~0ull, ~0ull);
  check_claims(1ull << 63, 1ull, 0ull);
  check_claims(0ull, ~0ull, ~0ull);
  for (int rep = 0; rep < 1500; ++rep) {
    const uint64_t list = rep % 3 ? rnd() : rnd() & rnd();
    const uint64_t hot = rep % 5 ? rnd() & rnd() : 0ull;
    const uint64_t prune = rep % 2 ? rnd() & rnd() : rnd();
    check_claims(list, hot, prune);
  }
  std::printf("check_k2_help ok: %ld cases\n", checked);
  return 0;
}
