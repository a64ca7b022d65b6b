// The host-side greedy session and the sharded drivers' list merge (yoda_greedy_session.h).
#include "yoda_greedy_session.h"

#include <iterator>
#include <utility>

uint64_t static_score(uint64_t free_sum, uint64_t total_sum, uint64_t alloc, bool* zero_total) {
  *zero_total = total_sum == 0;
  if (total_sum == 0) return 0;
  const uint64_t allocate = total_sum < alloc ? 0 : (total_sum - alloc) * 100u / total_sum * 3u;
  const uint64_t actual = (free_sum * 100u / total_sum) * 2u;
  return allocate + actual;
}

// Queue order (sort.go:8-10): scv/priority descending, then input index.  A counting sort
// when the priorities span < 2^16 values (the usual small integers), else a stable sort.
void queue_order(const int64_t* prio, uint32_t P, std::vector<uint32_t>& order) {
  order.resize(P);
  if (!prio || P == 0) {
    for (uint32_t i = 0; i < P; ++i) order[i] = i;
    return;
  }
  int64_t lo = prio[0], hi = prio[0];
  for (uint32_t i = 1; i < P; ++i) {
    lo = std::min(lo, prio[i]);
    hi = std::max(hi, prio[i]);
  }
  if ((uint64_t)hi - (uint64_t)lo < (1u << 16)) {
    const uint32_t R = (uint32_t)((uint64_t)hi - (uint64_t)lo) + 1;
    std::vector<uint32_t> start(R + 1, 0);
    for (uint32_t i = 0; i < P; ++i) ++start[(uint32_t)((uint64_t)hi - (uint64_t)prio[i]) + 1];
    for (uint32_t r = 0; r < R; ++r) start[r + 1] += start[r];
    for (uint32_t i = 0; i < P; ++i) order[start[(uint32_t)((uint64_t)hi - (uint64_t)prio[i])]++] = i;
    return;
  }
  for (uint32_t i = 0; i < P; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [prio](uint32_t a, uint32_t b) { return prio[a] > prio[b]; });
}

void yoda_greedy_session::apply(uint32_t p, int32_t node) {
  if (node < 0) return;
  const uint32_t n = (uint32_t)node;
  if (!touched_w[n]) {
    touched_w[n] = 1;
    stat_w[n] = stat[n];
    cn_w[n] = card_number[n];
    touched_list.push_back(n);
  }
  if (!dirty[n]) {
    dirty[n] = 1;
    dirty_list.push_back(n);
  }
  if (!ever[n]) {
    ever[n] = 1;
    ever_list.push_back(n);
  }
  const uint64_t before = alloc[n];
  if (has_memory[p]) alloc[n] += memory[p];  // uint64 wrap (algorithm.go:301)
  if (alloc[n] < before) wrapped = true;     // Allocate may grow: stop certifying
  if (flags & YODA_GREEDY_CARD_CAPACITY) {
    const uint64_t num = has_number[p] ? number[p] : 1;
    const uint64_t a = card_number[n], b = a >= num ? a - num : 0;
    card_number[n] = b;
    // pods needing q in (b, a] cards have just lost this node
    for (uint64_t q = b + 1; q <= std::min<uint64_t>(a, kCrossQ); ++q) {
      ++cross[q];
      cross_list[q].push_back(n);
    }
  }
  bool z;
  const int64_t before_stat = stat[n];
  stat[n] = static_score(free_sum[n], total_sum[n], alloc[n], &z);
  if (stat[n] > before_stat) stat_rose = true;
}

bool yoda_greedy_session::fit_ws(uint32_t n, uint32_t p, uint64_t q) const {
  const uint64_t* c = cards.data() + (size_t)n * 6 * K;
  uint64_t cm = 0, cc = 0;
  for (uint32_t j = 0; j < K; ++j) {
    if (!((hmask[n] >> j) & 1u)) continue;
    cm += c[0 * K + j] >= memory[p];  // kFree
    cc += c[1 * K + j] == clock[p];   // kClock
  }
  return (!has_memory[p] || cm >= q) && (!has_clock[p] || cc >= q);
}

bool yoda_greedy_session::contrib(uint32_t n, uint32_t p, uint64_t v[6]) const {
  const uint64_t* c = cards.data() + (size_t)n * 6 * K;
  const uint64_t m = has_memory[p] ? memory[p] : 0, ck = has_clock[p] ? clock[p] : 0;
  bool any = false;
  for (int f = 0; f < 6; ++f) v[f] = 0;
  for (uint32_t j = 0; j < K; ++j) {
    if (!((rmask[n] >> j) & 1u) || c[0 * K + j] < m || c[1 * K + j] < ck) continue;
    any = true;
    // CardField (free, clock, total, bw, core, power) -> MaxValue (bw, clock, core, free,
    // power, total)
    v[0] = std::max(v[0], c[3 * K + j]);
    v[1] = std::max(v[1], c[1 * K + j]);
    v[2] = std::max(v[2], c[4 * K + j]);
    v[3] = std::max(v[3], c[0 * K + j]);
    v[4] = std::max(v[4], c[5 * K + j]);
    v[5] = std::max(v[5], c[2 * K + j]);
  }
  return any;
}

bool yoda_greedy_session::scan_lost(uint32_t i, uint32_t p, uint64_t q, uint64_t lq,
                                    uint64_t* lf, uint64_t* lz, uint64_t lw[6],
                                    bool witness_only) const {
  *lf = *lz = 0;
  for (int f = 0; f < 6; ++f) lw[f] = 0;
  if (lq == 0) return true;
  if (cards.empty() || lq > kExactLost) return false;
  ++n_scan;
  uint32_t fmask = 0x3fu;
  if (witness_only && has_wit) {
    fmask = 0;
    for (int f = 0; f < 6; ++f) {
      const size_t o = (size_t)f * wn + i;
      if (wmax[o] > 1 && wcnt[o] <= lq) fmask |= 1u << f;
    }
    if (fmask == 0) return true;
  }
  auto visit = [&](uint32_t x) {
    if (witness_only && has_wit) {
      const uint64_t* nm = nodemax.data() + (size_t)x * 6;
      bool maybe = false;
      for (int f = 0; f < 6 && !maybe; ++f)
        maybe = ((fmask >> f) & 1u) && nm[f] >= wmax[(size_t)f * wn + i];
      if (!maybe) return;
    }
    ++n_scan_nodes;
    if (!fit_ws(x, p, q)) return;
    // x passed Yoda's Filter at the window start: F lost it, and F' too if it is a candidate
    if (cand(p, x)) {
      ++*lf;
      *lz += total_sum[x] == 0 ? 1 : 0;
    }
    uint64_t v[6];
    if (has_wit && contrib(x, p, v))
      for (int f = 0; f < 6; ++f) lw[f] += v[f] == wmax[(size_t)f * wn + i] ? 1 : 0;
  };
  if (q <= kCrossQ) {
    for (uint32_t x : cross_list[q]) visit(x);
  } else {
    for (uint32_t x : touched_list)
      if (removed(x, q)) visit(x);
  }
  return true;
}

bool yoda_greedy_session::maxima_kept(uint32_t i, uint64_t q, uint64_t lq, bool exact,
                                      const uint64_t lw[6]) const {
  if (lq == 0) return true;
  if (!has_wit) return false;
  for (int f = 0; f < 6; ++f) {
    const size_t o = (size_t)f * wn + i;
    if (wmax[o] <= 1) continue;
    if (exact) {
      if (wcnt[o] > lw[f]) continue;
    } else {
      if (wcnt[o] > lq) continue;
      if (wcnt[o] == 1 && wnode[o] < N && !removed(wnode[o], q)) continue;
    }
    return false;
  }
  return true;
}

bool yoda_greedy_session::certify0(uint32_t i, uint32_t* best) const {
  const uint32_t nf = counts[i], len = std::min<uint32_t>(nf, vlen[i]);
  double bs = -1.0;
  uint32_t bi = 0xffffffffu;
  for (uint32_t kk = 0; kk < len; ++kk) {  // (the listed entries: none empty, every id < N)
    const uint32_t n = ti[at(i, kk)];
    double cur = ts[at(i, kk)];
    if (touched_w[n]) cur = cur - (double)stat_w[n] + (double)stat[n];
    if (cur > bs || (cur == bs && n < bi)) {
      bs = cur;
      bi = n;
    }
  }
  *best = bi;
  if (bi == 0xffffffffu) return false;  // nothing listed
  return (nf <= k && vlen[i] >= nf) || bs > Tw[i] || (bs == Tw[i] && bi <= Tix[i]);
}

bool yoda_greedy_session::resolve_capacity(uint32_t i, uint32_t p, int32_t* pk) {
  const uint32_t KT = k;
  const uint32_t nf0 = counts[i], nz0 = counts[(size_t)wn + i];
  ++n_resolve;
  if (nf0 == 0) {  // feasibility only shrinks: still no node
    *pk = YODA_PICK_NONE;
    return true;
  }
  if (wrapped) return ++why[0], false;
  const uint64_t q = need_cards(p);
  const uint32_t len = std::min<uint32_t>(nf0, KT);
  // the list holds every feasible node of the window start
  const bool whole = nf0 <= KT && vlen[i] >= nf0;
  const uint64_t lq = lost(q);
  uint32_t alive = 0, first = 0xffffffffu, alive_zero = 0;
  double bs = -1.0;
  uint32_t bi = 0xffffffffu;
  // the list's best current candidate; alive / first / alive_zero too on a full scan.  A
  // partial scan stops at the first entry whose window-start score is below the best so far:
  // the list is in descending window-start order and a score only falls in a window (deep
  // lists, k_topk_merge_deep, make the full scan the resolve's main cost)
  auto scan = [&](bool full) {
    alive = 0, first = 0xffffffffu, alive_zero = 0;
    bs = -1.0, bi = 0xffffffffu;
    for (uint32_t kk = 0; kk < len; ++kk) {
      const size_t o = at(i, kk);
      if (!full && ts[o] < bs) break;
      const uint32_t n = ti[o];
      if (n >= N || removed(n, q)) continue;
      ++alive;
      if (first == 0xffffffffu) first = n;
      alive_zero += total_sum[n] == 0 ? 1u : 0u;
      double cur = ts[o];
      if (touched_w[n]) cur = cur - (double)stat_w[n] + (double)stat[n];
      if (cur > bs || (cur == bs && n < bi)) {
        bs = cur;
        bi = n;
      }
    }
  };
  const bool full_scan = whole || stat_rose;
  scan(full_scan);
  uint64_t lf = 0, lz = 0, lw[6] = {};
  // The bounds-only certificate first (no card scan): whatever it certifies, the exact one
  // certifies with the same outcome (nf0 >= 2 + lq leaves >= 2 feasible nodes; a field with
  // more witnesses than lost nodes, or an unlost single witness, keeps its maximum since
  // lw[f] <= lq).  The lost nodes' cards are examined only when it fails.
  // Candidate classes leave it as it is: nf0 / nz0 count F', wcnt counts F, and lq = lost(q)
  // counts the lost nodes of the whole snapshot, so it bounds the loss within F' (nf0 >= 2 + lq
  // still leaves two nodes of F'; nz0 > 0 && lq > 0 still means a zero-total node of F' may be
  // gone) as well as the loss within F (the witnesses).
  bool exact = false;
  if (!whole && lq > 0 && nf0 >= 2 + lq && nz0 == 0 && bi != 0xffffffffu &&
      maxima_kept(i, q, lq, false, lw)) {
    // (falls through to the list certificate below with exact == false)
  } else {
    exact = scan_lost(i, p, q, lq, &lf, &lz, lw, nf0 >= 2 + lq && nz0 == 0);
  }
  if (whole) {
    if (alive == 0) {
      *pk = YODA_PICK_NONE;
      return true;
    }
    if (alive == 1) {  // k8s returns the only feasible node without scoring
      *pk = (int32_t)first;
      return true;
    }
    if (alive_zero > 0) {  // Score would divide by TotalMemorySum == 0
      *pk = YODA_PICK_ERROR;
      return true;
    }
  } else if (exact) {
    // the feasible set is the window start's minus the lost nodes that were in it
    const uint64_t nf = nf0 - std::min<uint64_t>(nf0, lf);
    if (nf == 0) {
      *pk = YODA_PICK_NONE;
      return true;
    }
    if (nf == 1) {  // the only feasible node: listed and alive, or somewhere unlisted
      if (!full_scan) scan(true);
      if (alive != 1) return ++why[1], false;
      *pk = (int32_t)first;
      return true;
    }
    if (nz0 > lz) {  // a feasible zero-total node remains
      *pk = YODA_PICK_ERROR;
      return true;
    }
  } else {
    if (nf0 < 2 + lq) return ++why[1], false;  // might be down to 0 or 1 feasible nodes
    if (nz0 > 0) {
      if (lq > 0) return ++why[2], false;      // a zero-total node may be among the lost ones
      *pk = YODA_PICK_ERROR;
      return true;
    }
  }
  if (!maxima_kept(i, q, lq, exact, lw)) return ++why[3], false;  // unlisted scores may move
  if (bi == 0xffffffffu) return ++why[4], false;       // every listed node lost
  if (!whole) {
    // every unlisted node scored <= T at the window start or the list's last refresh (ties:
    // higher index) and has only lost Allocate since, or feasibility
    if (!(bs > Tw[i] || (bs == Tw[i] && bi <= Tix[i]))) return ++why[5], false;
  }
  *pk = (int32_t)bi;
  return true;
}

int gs_create(const yoda_node_soa* nodes, const yoda_pod_soa* pods, uint32_t flags,
              bool borrow_pods, yoda_gs_t** out) {
  if (!out || !nodes || !pods) return YODA_ERR_INVALID_ARG;
  *out = nullptr;
  const uint32_t N = nodes->n_nodes, P = pods->n_pods;
  if (N && (!nodes->free_memory_sum || !nodes->total_memory_sum || !nodes->card_number))
    return YODA_ERR_INVALID_ARG;
  if (P && (!pods->has_memory || !pods->memory || !pods->has_number || !pods->number))
    return YODA_ERR_INVALID_ARG;
  if (N >= 0x7fffffffu) return YODA_ERR_RANGE;
  try {
    yoda_gs_t* g = new yoda_gs_t();
    g->N = N, g->P = P, g->flags = flags;
    g->free_sum.assign(nodes->free_memory_sum, nodes->free_memory_sum + N);
    g->total_sum.assign(nodes->total_memory_sum, nodes->total_memory_sum + N);
    g->card_number.assign(nodes->card_number, nodes->card_number + N);
    if (nodes->alloc_memory)
      g->alloc.assign(nodes->alloc_memory, nodes->alloc_memory + N);
    else
      g->alloc.assign(N, 0);
    g->alloc0 = g->alloc;
    g->cn0 = g->card_number;
    g->stat.resize(N);
    g->stat_w.resize(N);
    g->cn_w.resize(N);
    for (uint32_t n = 0; n < N; ++n) {
      bool z;
      g->stat[n] = static_score(g->free_sum[n], g->total_sum[n], g->alloc[n], &z);
    }
    g->touched_w.assign(N, 0);
    g->dirty.assign(N, 0);
    g->ever.assign(N, 0);
    const uint8_t* src8[3] = {pods->has_memory, pods->has_number, pods->has_clock};
    const uint64_t* src64[3] = {pods->memory, pods->number, pods->clock};
    const bool no_clock = !pods->has_clock || !pods->clock;
    for (int a = 0; a < 3; ++a) {
      if (a == 2 && no_clock) {  // no clock labels: zeros of the session's own
        g->own_u8[a].assign(P, 0);
        g->own_u64[a].assign(P, 0);
      } else if (!borrow_pods) {
        g->own_u8[a].assign(src8[a], src8[a] + P);
        g->own_u64[a].assign(src64[a], src64[a] + P);
      } else {
        continue;
      }
      src8[a] = g->own_u8[a].data();
      src64[a] = g->own_u64[a].data();
    }
    g->has_memory = src8[0], g->has_number = src8[1], g->has_clock = src8[2];
    g->memory = src64[0], g->number = src64[1], g->clock = src64[2];
    // capacity mode: keep the cards for the exact witness accounting (optional)
    if ((flags & YODA_GREEDY_CARD_CAPACITY) && N && nodes->max_cards >= 1 &&
        nodes->max_cards <= YODA_MAX_CARDS && nodes->card_count && nodes->card_free_memory &&
        nodes->card_total_memory && nodes->card_clock && nodes->card_bandwidth &&
        nodes->card_core && nodes->card_power && nodes->card_healthy) {
      const uint32_t K = nodes->max_cards;
      g->K = K;
      g->cards.assign((size_t)N * 6 * K, 0);
      g->hmask.assign(N, 0);
      g->rmask.assign(N, 0);
      const uint64_t* src[6] = {nodes->card_free_memory, nodes->card_clock,
                                nodes->card_total_memory, nodes->card_bandwidth,
                                nodes->card_core, nodes->card_power};  // CardField order
      for (uint32_t n = 0; n < N; ++n) {
        const uint32_t cnt = std::min<uint32_t>(nodes->card_count[n], K);
        for (uint32_t j = 0; j < cnt; ++j) {
          const size_t k = (size_t)n * K + j;
          for (int f = 0; f < 6; ++f) g->cards[((size_t)n * 6 + f) * K + j] = src[f][k];
          g->rmask[n] |= 1u << j;
          if (nodes->card_healthy[k]) g->hmask[n] |= 1u << j;
        }
      }
      // each node's largest contribution to any pod's maxima (contrib() over every real card)
      g->nodemax.assign((size_t)N * 6, 0);
      for (uint32_t n = 0; n < N; ++n) {
        uint64_t* v = g->nodemax.data() + (size_t)n * 6;
        const uint64_t* c = g->cards.data() + (size_t)n * 6 * K;
        for (uint32_t j = 0; j < K; ++j) {
          if (!((g->rmask[n] >> j) & 1u)) continue;
          v[0] = std::max(v[0], c[3 * K + j]);
          v[1] = std::max(v[1], c[1 * K + j]);
          v[2] = std::max(v[2], c[4 * K + j]);
          v[3] = std::max(v[3], c[0 * K + j]);
          v[4] = std::max(v[4], c[5 * K + j]);
          v[5] = std::max(v[5], c[2 * K + j]);
        }
      }
    }
    g->pick.assign(P, YODA_PICK_NONE);
    // queue order: sort.Less (sort.go:8-10), scv/priority descending, then input index
    queue_order(pods->priority, P, g->order);
    *out = g;
    return YODA_OK;
  } catch (...) {
    return YODA_ERR_INVALID_ARG;
  }
}

extern "C" {

int yoda_gs_create(const yoda_node_soa* nodes, const yoda_pod_soa* pods, uint32_t flags,
                   yoda_gs_t** out) {
  return gs_create(nodes, pods, flags, false, out);
}

int yoda_gs_destroy(yoda_gs_t* g) {
  if (!g) return YODA_ERR_INVALID_ARG;
  delete g;
  return YODA_OK;
}

int yoda_gs_queue_order(const yoda_gs_t* g, uint32_t* order) {
  if (!g || (!order && g->P)) return YODA_ERR_INVALID_ARG;
  std::copy(g->order.begin(), g->order.end(), order);
  return YODA_OK;
}

int yoda_gs_begin_window(yoda_gs_t* g, uint32_t ws, uint32_t wn, uint32_t k,
                         const uint32_t* counts, const double* top_score,
                         const uint32_t* top_node) {
  return gs_begin_window_at(g, ws, wn, k, counts, const_cast<double*>(top_score),
                            const_cast<uint32_t*>(top_node), false, false);
}

}  // extern "C"

int gs_begin_window_at(yoda_gs_t* g, uint32_t ws, uint32_t wn, uint32_t k,
                       const uint32_t* counts, double* top_score, uint32_t* top_node,
                       bool borrow, bool row_major) {
  if (row_major && !borrow) return YODA_ERR_INVALID_ARG;
  if (!g || ws > g->P || wn > g->P - ws || k == 0 || !counts || !top_score || !top_node)
    return YODA_ERR_INVALID_ARG;
  if (!borrow)  // (the borrowed lists are libyoda's own kernel output)
    for (uint32_t i = 0; i < (uint32_t)k * wn; ++i)
      if (top_node[i] != 0xffffffffu && top_node[i] >= g->N) return YODA_ERR_RANGE;
  try {
    for (uint32_t n : g->touched_list) g->touched_w[n] = 0;
    g->touched_list.clear();
    g->ws = ws, g->wn = wn, g->k = k, g->next = 0;
    g->row_major = row_major;
    g->in_window = true;
    g->wrapped = false;
    g->stat_rose = false;
    std::fill(std::begin(g->cross), std::end(g->cross), 0u);
    for (auto& l : g->cross_list) l.clear();
    g->has_wit = false;
    g->counts.assign(counts, counts + 2 * (size_t)wn);
    if (borrow) {
      g->ts = top_score;
      g->ti = top_node;
    } else {
      g->ts_own.assign(top_score, top_score + (size_t)k * wn);
      g->ti_own.assign(top_node, top_node + (size_t)k * wn);
      g->ts = g->ts_own.data();
      g->ti = g->ti_own.data();
    }
    g->Tw.resize(wn);
    g->Tix.resize(wn);
    g->vlen.resize(wn);
    for (uint32_t i = 0; i < wn; ++i) {
      const uint32_t cap = std::min<uint32_t>(counts[i], k);
      uint32_t v = 0;
      while (v < cap && top_node[g->at(i, v)] != 0xffffffffu) ++v;
      g->vlen[i] = v;
      const uint32_t len = std::max<uint32_t>(1, v);  // (threshold: the last entry listed)
      g->Tw[i] = top_score[g->at(i, len - 1)];
      g->Tix[i] = top_node[g->at(i, len - 1)];
    }
    return YODA_OK;
  } catch (...) {
    return YODA_ERR_INVALID_ARG;
  }
}

extern "C" {

int yoda_gs_set_candidates(yoda_gs_t* g, uint32_t n_classes, const uint64_t* words,
                           const uint8_t* cls) {
  if (!g || n_classes > YODA_MAX_CAND_CLASSES) return YODA_ERR_INVALID_ARG;
  if (g->in_window) return YODA_ERR_STATE;
  if (n_classes == 0) {
    g->cand_words.clear();
    g->cand_cls.clear();
    return YODA_OK;
  }
  if (g->N && !words) return YODA_ERR_INVALID_ARG;
  if (cls)
    for (uint32_t p = 0; p < g->P; ++p)
      if (cls[p] != YODA_CAND_ANY && cls[p] >= n_classes) return YODA_ERR_RANGE;
  if (!(g->flags & YODA_GREEDY_CARD_CAPACITY)) return YODA_OK;  // (flags 0 reads neither)
  try {
    std::vector<uint64_t> w(words, words + g->N);
    std::vector<uint8_t> c;
    if (cls) c.assign(cls, cls + g->P);
    g->cand_words.swap(w);
    g->cand_cls.swap(c);
    return YODA_OK;
  } catch (...) {
    return YODA_ERR_INVALID_ARG;
  }
}

int yoda_gs_set_witness(yoda_gs_t* g, const uint64_t* maxima, const uint32_t* wit_count,
                        const uint32_t* wit_node) {
  if (!g || !g->in_window || (g->wn && (!maxima || !wit_count || !wit_node)))
    return YODA_ERR_INVALID_ARG;
  try {
    const size_t n = 6 * (size_t)g->wn;
    g->wmax.assign(maxima, maxima + n);
    g->wcnt.assign(wit_count, wit_count + n);
    g->wnode.assign(wit_node, wit_node + n);
    g->has_wit = true;
    return YODA_OK;
  } catch (...) {
    return YODA_ERR_INVALID_ARG;
  }
}

// Resolve the window in queue order until a pod cannot be certified from its candidate list
// (greedy): *next = its window index, or wn when the window is done.
int yoda_gs_resolve(yoda_gs_t* g, uint32_t* next) {
  if (!g || !next || !g->in_window) return YODA_ERR_INVALID_ARG;
  const uint32_t wn = g->wn;
  const bool capacity = (g->flags & YODA_GREEDY_CARD_CAPACITY) != 0;
  while (g->next < wn) {
    const uint32_t i = g->next;
    const uint32_t p = g->order[g->ws + i];
    const uint32_t nf = g->counts[i], nz = g->counts[(size_t)wn + i];
    int32_t pk;
    if (capacity) {
      if (!g->resolve_capacity(i, p, &pk)) break;
    } else if (nf == 0) {
      pk = YODA_PICK_NONE;
    } else if (nf >= 2 && nz > 0) {
      pk = YODA_PICK_ERROR;  // Score would divide by TotalMemorySum == 0
    } else if (nf == 1) {
      if (g->vlen[i] == 0) break;  // (not listed: the caller evaluates it)
      pk = (int32_t)g->ti[g->at(i, 0)];  // the only feasible node, returned without scoring
    } else if (g->wrapped) {
      break;
    } else {
      uint32_t bi;
      if (!g->certify0(i, &bi)) break;
      pk = (int32_t)bi;
    }
    g->pick[p] = pk;
    g->apply(p, pk);
    ++g->next;
    ++g->resolved;
  }
  *next = g->next;
  return YODA_OK;
}

uint32_t yoda_greedy_next_window(uint32_t progress, uint32_t wmax) {
  // the next window holds 130 % of this one's progress, in whole waves: small windows cost
  // less (K1 / K2 time grows with the pods) and most restart near where the last one did;
  // profiles/r03/greedy_capacity/grow_ab.txt (1.81-1.91 s with the earlier power of two >=
  // twice the progress, 1.57-1.64 s at 130 %).  YODA_GREEDY_GROW_PCT: A/B knob
  static const uint32_t grow = YODA_KNOB("YODA_GREEDY_GROW_PCT", 130);
  wmax = std::max<uint32_t>(wmax, 1);
  const uint64_t t = (uint64_t)progress * grow / 100;
  return (uint32_t)std::min<uint64_t>(wmax, std::max<uint64_t>(64, (t + 63) / 64 * 64));
}

int yoda_gs_uncertified(const yoda_gs_t* g, uint32_t from, uint32_t scan, uint32_t* count) {
  if (!g || !count || !g->in_window) return YODA_ERR_INVALID_ARG;
  if (g->flags & YODA_GREEDY_CARD_CAPACITY) return YODA_ERR_STATE;
  uint32_t c = 0, bi;
  // once Allocate has wrapped (alloc < before) no list certifies any more: a refresh cannot
  // help, so report none (the one rule of yoda_greedy, yoda_comm_greedy and dist.sharded_greedy)
  if (g->wrapped) {
    *count = 0;
    return YODA_OK;
  }
  const uint32_t end = (uint32_t)std::min<uint64_t>(g->wn, (uint64_t)from + scan);
  for (uint32_t i = from; i < end; ++i)
    if (g->counts[i] >= 2 && g->counts[(size_t)g->wn + i] == 0 && !g->certify0(i, &bi)) ++c;
  *count = c;
  return YODA_OK;
}

int yoda_gs_refresh(yoda_gs_t* g, uint32_t from, const double* top_score,
                    const uint32_t* top_node) {
  if (!g || !g->in_window || !top_score || !top_node || from > g->wn) return YODA_ERR_INVALID_ARG;
  // capacity sessions judge feasibility and maxima against the window start and restart
  // instead of refreshing (as yoda_gs_uncertified)
  if (g->flags & YODA_GREEDY_CARD_CAPACITY) return YODA_ERR_STATE;
  const uint32_t wn = g->wn, k = g->k;
  // validate every listed node first: a bad id leaves the session unchanged
  for (uint32_t i = from; i < wn; ++i) {
    const uint32_t len = std::min<uint32_t>(g->counts[i], k);
    for (uint32_t kk = 0; kk < len; ++kk)
      if (top_node[(size_t)kk * wn + i] >= g->N) return YODA_ERR_RANGE;
  }
  for (uint32_t i = from; i < wn; ++i) {
    const uint32_t len = std::min<uint32_t>(g->counts[i], k);
    for (uint32_t kk = 0; kk < len; ++kk) {
      const size_t o = (size_t)kk * wn + i;
      const uint32_t n = top_node[o];
      // stored so that the certificate's  stored - old static + current static  is its
      // current score (the refresh scored it with the current static)
      g->ti[g->at(i, kk)] = n;
      g->ts[g->at(i, kk)] = g->touched_w[n] ? top_score[o] + (double)g->stat_w[n] - (double)g->stat[n]
                                 : top_score[o];
    }
    g->vlen[i] = len;  // (a refresh's lists are whole: every id validated above)
    if (len) {
      g->Tw[i] = top_score[(size_t)(len - 1) * wn + i];
      g->Tix[i] = top_node[(size_t)(len - 1) * wn + i];
    }
  }
  ++g->refreshes;
  return YODA_OK;
}

int yoda_gs_assign(yoda_gs_t* g, uint32_t queue_pos, int32_t pick) {
  if (!g || queue_pos >= g->P) return YODA_ERR_INVALID_ARG;
  if (pick >= 0 && (uint32_t)pick >= g->N) return YODA_ERR_RANGE;
  const uint32_t p = g->order[queue_pos];
  g->pick[p] = pick;
  g->apply(p, pick);
  ++g->assigned;
  if (g->in_window && queue_pos == g->ws + g->next) ++g->next;
  return YODA_OK;
}

int yoda_gs_take_dirty(yoda_gs_t* g, uint32_t cap, uint32_t* nodes, uint64_t* alloc,
                       uint64_t* card_number, uint32_t* count) {
  if (!g || !count || (cap && (!nodes || !alloc || !card_number))) return YODA_ERR_INVALID_ARG;
  const uint32_t n = std::min<uint32_t>(cap, (uint32_t)g->dirty_list.size());
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t v = g->dirty_list[t];
    nodes[t] = v;
    alloc[t] = g->alloc[v];
    card_number[t] = g->card_number[v];
    g->dirty[v] = 0;
  }
  g->dirty_list.erase(g->dirty_list.begin(), g->dirty_list.begin() + n);
  *count = n;
  return YODA_OK;
}

int yoda_gs_touched_original(const yoda_gs_t* g, uint32_t cap, uint32_t* nodes, uint64_t* alloc,
                             uint64_t* card_number, uint32_t* count) {
  if (!g || !count || (cap && (!nodes || !alloc || !card_number))) return YODA_ERR_INVALID_ARG;
  const uint32_t n = std::min<uint32_t>(cap, (uint32_t)g->ever_list.size());
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t v = g->ever_list[t];
    nodes[t] = v;
    alloc[t] = g->alloc0[v];
    card_number[t] = g->cn0[v];
  }
  *count = n;
  return YODA_OK;
}

int yoda_gs_picks(const yoda_gs_t* g, int32_t* pick, uint32_t* resolved, uint32_t* assigned) {
  if (!g) return YODA_ERR_INVALID_ARG;
  if (pick) std::copy(g->pick.begin(), g->pick.end(), pick);
  if (resolved) *resolved = g->resolved;
  if (assigned) *assigned = g->assigned;
  return YODA_OK;
}

}  // extern "C"

void merge_shard_lists(int world, uint32_t wn, uint32_t kl, bool deep, uint32_t from,
                       const double* const* sc, const uint32_t* const* nd, double* ts,
                       uint32_t* ti) {
  auto before = [](const std::pair<double, uint32_t>& a, const std::pair<double, uint32_t>& b) {
    return a.first > b.first || (a.first == b.first && a.second < b.second);
  };
  std::vector<uint32_t> head(world), len(world);
  for (uint32_t p = from; p < wn; ++p) {
    bool any_last = false;
    std::pair<double, uint32_t> last_max{-1.0, 0xffffffffu};
    for (int rk = 0; rk < world; ++rk) {
      uint32_t l = 0;
      while (l < kl && nd[rk][(size_t)l * wn + p] != 0xffffffffu) ++l;
      len[rk] = l;
      head[rk] = 0;
      if (deep && l > 0) {
        const std::pair<double, uint32_t> last{sc[rk][(size_t)(l - 1) * wn + p],
                                               nd[rk][(size_t)(l - 1) * wn + p]};
        if (!any_last || before(last_max, last)) last_max = last;
        any_last = true;
      }
    }
    for (uint32_t k = 0; k < kl; ++k) {
      int best = -1;
      std::pair<double, uint32_t> bv{-1.0, 0xffffffffu};
      for (int rk = 0; rk < world; ++rk) {
        if (head[rk] >= len[rk]) continue;
        const size_t o = (size_t)head[rk] * wn + p;
        const std::pair<double, uint32_t> v{sc[rk][o], nd[rk][o]};
        if (best < 0 || before(v, bv)) best = rk, bv = v;
      }
      if (best < 0) break;
      if (any_last && k >= (uint32_t)yoda::topk_k() && !before(bv, last_max)) break;
      ++head[best];
      ts[(size_t)k * wn + p] = bv.first;
      ti[(size_t)k * wn + p] = bv.second;
    }
  }
}

extern "C" {

int yoda_merge_shard_lists(uint32_t world, uint32_t wn, uint32_t kl, uint32_t from,
                           const double* scores, const uint32_t* nodes, double* out_score,
                           uint32_t* out_node) {
  if (world < 1 || kl < 1 || from > wn || !scores || !nodes || !out_score || !out_node)
    return YODA_ERR_INVALID_ARG;
  try {
    std::vector<const double*> sc(world);
    std::vector<const uint32_t*> nd(world);
    for (uint32_t rk = 0; rk < world; ++rk) {
      sc[rk] = scores + (size_t)rk * kl * wn;
      nd[rk] = nodes + (size_t)rk * kl * wn;
    }
    for (uint32_t k = 0; k < kl; ++k)
      for (uint32_t p = from; p < wn; ++p) {
        out_score[(size_t)k * wn + p] = -1.0;
        out_node[(size_t)k * wn + p] = 0xffffffffu;
      }
    merge_shard_lists((int)world, wn, kl, kl > (uint32_t)yoda::topk_k_capacity(), from, sc.data(),
                      nd.data(), out_score, out_node);
    return YODA_OK;
  } catch (...) {
    return YODA_ERR_INVALID_ARG;
  }
}

}  // extern "C"
