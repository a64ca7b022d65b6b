// The host-side greedy session: the sequential part of the greedy batch -- the
// certificate per pod, the assume step, the mid-window refresh, the dirty-node and restore
// lists -- and the list merge of the sharded drivers.  Host code only: no HIP header, no HIP
// call, so a host compiler alone builds it (tools/check_greedy_session.cpp does, under ASan +
// UBSan).  Every greedy driver resolves through it: yoda_greedy and yoda_comm_greedy inside
// libyoda (direct access to the struct), dist.sharded_greedy through the yoda_gs_* entry points.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/yoda.h"

// Tuning knobs of the A/B harness (tools/ab_lib.sh).  Only the A/B build reads them from
// the environment (`make ab` -> libyoda_ab.so, -DYODA_AB_KNOBS); in the release library
// YODA_KNOB(name, default) is the default itself and the name is not even in the binary, so
// a scheduler process's environment cannot change kernel choice, chunking or greedy policy.
#ifdef YODA_AB_KNOBS
static inline uint32_t knob_env(const char* name, uint32_t dflt) {
  const char* s = std::getenv(name);
  return (s && *s) ? (uint32_t)std::strtoul(s, nullptr, 10) : dflt;
}
#define YODA_KNOB(name, dflt) knob_env(name, dflt)
#else
#define YODA_KNOB(name, dflt) ((uint32_t)(dflt))
#endif

// The candidate lists' depths (defined beside the kernels that write them, yoda_kernels.hip).
namespace yoda {
int topk_k();
int topk_k_capacity();
}  // namespace yoda

// CalculateAllocateScore + CalculateActualScore (algorithm.go:293-310), uint64 wrap.
// zero_total: TotalMemorySum == 0, where the reference divides by zero.
uint64_t static_score(uint64_t free_sum, uint64_t total_sum, uint64_t alloc, bool* zero_total);

// Queue order (sort.go:8-10): scv/priority descending, then input index.
void queue_order(const int64_t* prio, uint32_t P, std::vector<uint32_t>& order);

// Mid-window list refresh (flags 0): a window whose lists went stale (similar pods took their
// shared top nodes) would otherwise send each of its remaining similar pods to an exact
// evaluation.  Every `every` such pods, and only with at least 2 * scan pods left, the next
// `scan` window pods are checked (yoda_gs_uncertified); if at least `min` of them are
// uncertified already (they stay so: scores only drop), the window's top-k runs again against
// the current state (yoda_gs_refresh).  One definition for every driver
// (YODA_GREEDY_REFRESH_EVERY / _MIN: A/B knobs for the period and the bar).
struct GreedyRefresh {
  uint32_t every, scan, min;
};
inline const GreedyRefresh& greedy_refresh() {
  static const GreedyRefresh r{std::max<uint32_t>(1, YODA_KNOB("YODA_GREEDY_REFRESH_EVERY", 8)),
                               256, YODA_KNOB("YODA_GREEDY_REFRESH_MIN", 16)};
  return r;
}

// The session, over the node ids of its snapshot (yoda_greedy: the handle's LOCAL ids; the
// sharded drivers: the GLOBAL node set), fed with candidate lists.  Identical on every rank.
struct yoda_greedy_session {
  static constexpr uint32_t kCrossQ = 64;  // capacity mode: per-q removal counts up to here
  uint32_t N = 0, P = 0, flags = 0;
  std::vector<uint64_t> free_sum, total_sum, alloc, card_number, alloc0, cn0, stat, stat_w;
  std::vector<uint64_t> cn_w;  // CardNumber of a window-touched node at the window start
  std::vector<uint8_t> touched_w, dirty, ever;
  // the pods' labels, [P]: the session's copies (own_*), or the caller's arrays where they
  // outlive the session (gs_create with borrow_pods)
  const uint8_t *has_memory = nullptr, *has_number = nullptr, *has_clock = nullptr;
  const uint64_t *memory = nullptr, *number = nullptr, *clock = nullptr;
  std::vector<uint8_t> own_u8[3];
  std::vector<uint64_t> own_u64[3];
  // capacity mode: the nodes' cards (when the snapshot passed them), [N][K] in CardField
  // order, to tell which lost nodes were witnesses of a pod's maxima
  uint32_t K = 0;
  std::vector<uint64_t> cards;  // [N][6][K]
  std::vector<uint32_t> hmask, rmask;  // healthy / real card bits per node
  std::vector<uint32_t> order, touched_list, dirty_list, ever_list;
  std::vector<int32_t> pick;
  // current window (queue positions [ws, ws + wn)), inputs in window order
  uint32_t ws = 0, wn = 0, k = 0, next = 0, resolved = 0, assigned = 0, refreshes = 0;
  bool in_window = false, wrapped = false;
  // some node's static score rose within the window (never, short of a wrap: Allocate only
  // grows): a listed node's current score may then exceed its window-start one
  bool stat_rose = false;
  std::vector<uint32_t> counts, ti_own;
  std::vector<double> ts_own;
  // the window's lists [k][wn]: the session's copies, or (yoda_greedy, gs_begin_window_at)
  // the caller's staging, valid until the window ends
  double* ts = nullptr;
  uint32_t* ti = nullptr;
  // entry kk of window pod i: [k][wn] (the API's layout), or [wn][k] (row_major: a pod's list
  // contiguous, as k_window_out writes yoda_greedy's staging)
  bool row_major = false;
  size_t at(uint32_t i, uint32_t kk) const {
    return row_major ? (size_t)i * k + kk : (size_t)kk * wn + i;
  }
  // each list's certificate threshold (flags 0): its last entry's window-start -- or, after a
  // mid-window refresh (yoda_gs_refresh), refresh-time -- score and node
  std::vector<double> Tw;
  // entries of each list before its first empty one (a deep merge stops where it is no longer
  // exact, k_topk_merge_deep): the list holds every feasible node only when that is nf
  std::vector<uint32_t> vlen;
  std::vector<uint32_t> Tix;
  // YODA_GREEDY_CARD_CAPACITY (greedy): cross[q] = window-touched nodes whose
  // CardNumber has dropped from >= q (window start) to < q, i.e. nodes a pod needing q cards
  // has lost since its candidate list was made; and the window's PreScore maxima with their
  // witnesses ([6][wn] each, window order), when the caller supplied them.
  uint32_t cross[kCrossQ + 1] = {};
  std::vector<uint32_t> cross_list[kCrossQ + 1];  // the nodes counted in cross[q]
  bool has_wit = false;
  std::vector<uint64_t> wmax;
  std::vector<uint32_t> wcnt, wnode;

  // yoda_gs_set_candidates (capacity sessions): the candidate words [N] and the pods' classes [P]
  // in input order (empty: every pod YODA_CAND_ANY); no words: candidates off.  The window's
  // counts and lists are then over F' = F and cand, its maxima and witnesses over F (Yoda's
  // Filter alone): scan_lost is the one place that tells the two apart.
  std::vector<uint64_t> cand_words;
  std::vector<uint8_t> cand_cls;
  bool cand(uint32_t p, uint32_t n) const {
    if (cand_words.empty() || cand_cls.empty() || cand_cls[p] == YODA_CAND_ANY) return true;
    return (cand_words[n] >> cand_cls[p]) & 1ull;
  }

  // the assume step: pod p takes node `node` (a pick < 0 changes nothing)
  void apply(uint32_t p, int32_t node);
  // PodFitsNumber operand of pod p (filter.go:11-16): the label, or 1 (CardNumber > 0)
  uint64_t need_cards(uint32_t p) const { return has_number[p] ? number[p] : 1; }
  // node n was feasible for a pod needing q cards at the window start and is not any more
  bool removed(uint32_t n, uint64_t q) const {
    return touched_w[n] && card_number[n] < q && cn_w[n] >= q;
  }
  // how many nodes a pod needing q cards has lost in this window (an upper bound on its
  // feasible nodes lost: a touched node may never have passed its other predicates)
  uint64_t lost(uint64_t q) const {
    if (q <= kCrossQ) return cross[q];
    uint64_t r = 0;
    for (uint32_t n : touched_list) r += removed(n, q) ? 1 : 0;
    return r;
  }
  // Node n passed pod p's Filter at the window start (it needs q cards; PodFitsNumber held
  // then, n being a lost node): PodFitsMemory / PodFitsClock (filter.go:18-50) on its cards.
  bool fit_ws(uint32_t n, uint32_t p, uint64_t q) const;
  // per node (MaxValue order) the largest value over its real cards: no pod's contrib() from
  // the node exceeds it (scan_lost skips nodes that cannot be a witness)
  std::vector<uint64_t> nodemax;
  // Node n's contribution to pod p's maxima (ProcessMaxValueWithCard over the cards with
  // FreeMemory >= m and Clock >= c, collection.go:46-76), MaxValue field order.
  bool contrib(uint32_t n, uint32_t p, uint64_t v[6]) const;
  // The nodes pod p (needing q cards, window pod i) has lost in this window, examined with
  // the cards at hand: how many had passed its Filter at the window start (lf), how many of
  // those had TotalMemorySum == 0 (lz), and how many were witnesses of each of its maxima
  // (lw).  False (nothing computed) without the cards or when too many nodes were lost.
  // With candidate classes lf / lz count the pod's candidates only (the nodes F' lost: counts
  // is over F'), lw every node that passed Yoda's Filter (the witnesses F lost: wcnt is over F).
  // witness_only: the caller needs lw only (nf0 >= 2 + lq and no zero-total node at the window
  // start: lf and lz cannot change its outcome) -- and only for the fields whose witnesses lq
  // lost nodes could all be (wcnt <= lq); a node below every such maximum is skipped unvisited
  // (lf / lz then count only the visited nodes)
  static constexpr uint64_t kExactLost = 512;
  bool scan_lost(uint32_t i, uint32_t p, uint64_t q, uint64_t lq, uint64_t* lf, uint64_t* lz,
                 uint64_t lw[6], bool witness_only = false) const;
  // CollectMaxValues over the remaining feasible nodes still gives window pod i's maxima:
  // every field keeps a witness.  A maximum of 1 is the floor and cannot drop
  // (collection.go:31-38).  Exact: a field keeps its maximum iff fewer of its witnesses were
  // lost than it had (lw from scan_lost).  Bounds only: more witnesses than lost nodes, or a
  // single witness that is not lost.
  bool maxima_kept(uint32_t i, uint64_t q, uint64_t lq, bool exact, const uint64_t lw[6]) const;
  // Capacity-mode resolve of window pod i (input pod p): true with *pk when certified.
  bool resolve_capacity(uint32_t i, uint32_t p, int32_t* pk);
  // flags 0: window pod i's best current candidate (window-start score - old static + new
  // static) and whether the list certifies it: every unlisted node scored <= T at the window
  // start or last refresh (ties: higher index) and its score can only have dropped since
  bool certify0(uint32_t i, uint32_t* best) const;
  // why capacity certificates failed: wrap, few feasible left, zero-total, maxima, list
  // exhausted, below the threshold
  uint64_t why[6] = {};
  // (diagnostics, YODA_GREEDY_DEBUG) capacity resolves, lost-node scans and nodes they visited
  mutable uint64_t n_resolve = 0, n_scan = 0, n_scan_nodes = 0;
};

// yoda_gs_create; borrow_pods: the session reads the pods' label arrays in place instead of
// copying them (yoda_greedy: its pods outlive the batch; 1M pods are ~30 MB of copies)
int gs_create(const yoda_node_soa* nodes, const yoda_pod_soa* pods, uint32_t flags,
              bool borrow_pods, yoda_gs_t** out);

// yoda_gs_begin_window without copying the lists (borrow): the session reads (and, on a
// refresh, writes) top_score / top_node in place until the window ends (yoda_greedy's staging,
// libyoda's own kernel output: ids not validated); row_major: [wn][k] instead of [k][wn]
int gs_begin_window_at(yoda_gs_t* g, uint32_t ws, uint32_t wn, uint32_t k, const uint32_t* counts,
                       double* top_score, uint32_t* top_node, bool borrow,
                       bool row_major = false);

// The sharded greedy's list merge (window exchange 2), shared by yoda_comm_greedy and the
// caller-driven protocol (yoda_merge_shard_lists, dist.sharded_greedy): shard rk's list of
// window pod p is (sc[rk][l*wn + p], nd[rk][l*wn + p]), l < kl, sorted score desc / node asc and
// ended by a 0xFFFFFFFF node.  ts/ti [kl][wn] receive the first kl of the union in that order
// (pods [from, wn) only).  Deep lists (exact down to their last entry only): every node a shard
// left out scores at most the shard's last entry, so the union is certain only above the latest
// of those -- and for its first topk_k(), which lie within their shards' exact prefixes.
void merge_shard_lists(int world, uint32_t wn, uint32_t kl, bool deep, uint32_t from,
                       const double* const* sc, const uint32_t* const* nd, double* ts,
                       uint32_t* ti);
