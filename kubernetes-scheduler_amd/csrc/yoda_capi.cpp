// yoda_capi.cpp — host side of libyoda: the C-ABI of include/yoda.h.
//
// Packs the node snapshot and pod requests into the device layout of yoda_layout.h, picks
// the exact-f64 fast path or the exact-u64 generic path, and sequences the kernels of
// yoda_kernels.hip on the handle's stream.  No exception crosses the C boundary.
#include <dlfcn.h>
#include <unistd.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: librccl is opened at yoda_comm_init (dlopen)

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include <thread>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <array>

#include "../../include/yoda.h"
#include "yoda_layout.h"
#include "yoda_launch.h"
#include "yoda_modeb.h"
#include "yoda_node_pack.h"
#include "yoda_greedy_session.h"


using namespace yoda;

namespace {

struct Status {
  int code;
  std::string msg;
};

// Grow-only device buffer; frees itself.  Not copyable: a handle's members, swapped in place.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    const size_t alloc = std::max<size_t>(n, 256);
    hipError_t e = hipMalloc(&p, alloc);
    if (e == hipSuccess) bytes = alloc;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Grow-only pinned host buffer (fast async H2D); frees itself, not copyable.
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void* dp = nullptr;  // the same pages as seen by kernels (hipHostMalloc maps them)
  unsigned flags = hipHostMallocDefault;  // hipHostMallocCoherent: polled by the host
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = dp = nullptr;
    bytes = 0;
    const size_t alloc = std::max<size_t>(n, 4096);
    hipError_t e = hipHostMalloc(&p, alloc, flags);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, p, 0);
    if (e == hipSuccess) bytes = alloc;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// RCCL entry points, resolved at the first yoda_comm_* call: libyoda itself does not link
// RCCL (a process that already loaded one -- e.g. PyTorch's, same SONAME -- shares it).
struct RcclApi {
  bool tried = false, ok = false;
  std::string err;
  ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
  ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                             hipStream_t) = nullptr;
  ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t,
                             hipStream_t) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
  bool load() {
    if (tried) return ok;
    tried = true;
    void* so = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!so) so = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!so) {
      err = std::string("librccl.so.1 not found: ") + dlerror();
      return false;
    }
    auto sym = [&](const char* name) {
      void* f = dlsym(so, name);
      if (!f) err = std::string("librccl: missing ") + name;
      return f;
    };
    get_unique_id = reinterpret_cast<decltype(get_unique_id)>(sym("ncclGetUniqueId"));
    comm_init_rank = reinterpret_cast<decltype(comm_init_rank)>(sym("ncclCommInitRank"));
    all_reduce = reinterpret_cast<decltype(all_reduce)>(sym("ncclAllReduce"));
    all_gather = reinterpret_cast<decltype(all_gather)>(sym("ncclAllGather"));
    comm_destroy = reinterpret_cast<decltype(comm_destroy)>(sym("ncclCommDestroy"));
    group_start = reinterpret_cast<decltype(group_start)>(sym("ncclGroupStart"));
    group_end = reinterpret_cast<decltype(group_end)>(sym("ncclGroupEnd"));
    error_string = reinterpret_cast<decltype(error_string)>(sym("ncclGetErrorString"));
    ok = get_unique_id && comm_init_rank && all_reduce && all_gather && comm_destroy &&
         group_start && group_end && error_string;
    return ok;
  }
};
RcclApi& rccl() {
  static RcclApi a;
  return a;
}

enum PodArray {
  kPodMF, kPodCF, kPodMU, kPodCU, kPodNumber, kPodAlpha, kPodBeta,
  kPodM32, kPodC32, kPodNeedMem, kPodNeedClk, kPodArrays
};
constexpr size_t kPodArrayBytes[kPodArrays] = {8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 4};
// Placement in the uploaded blob: first the arrays a private run on the block kernels reads (the
// counting order included), then the rest, whose copy waits for the first entry point that
// needs it (pods_complete) -- after the kernels of such a run.
constexpr int kPodCoreArrays = 5;
constexpr int kPodPlace[kPodArrays] = {kPodM32, kPodC32, kPodNumber, kPodNeedMem, kPodNeedClk,
                                       kPodMU, kPodCU, kPodMF, kPodCF, kPodAlpha, kPodBeta};

}  // namespace

struct yoda_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  std::string last_error;

  // node snapshot
  bool has_nodes = false;
  bool generic = false;  // path == Path::U64
  Path path = Path::N32;
  bool nodes_diskio = false;  // node cpu/disk_io present
  bool pods_diskio = false;   // pod rio/rcpu present
  int K = 1;
  uint32_t n_nodes = 0, node_offset = 0;
  DevBuf nodes;     // fast or generic records
  DevBuf nodes_b;   // Mode B records
  DevBuf k1sum;     // K1 node summaries (N32 path, yoda_layout.h K1SumWord)
  DevBuf k2sum;     // K2 node summaries (N32 path, yoda_layout.h K2SumWord)
  DevBuf kmix;      // per-card GPU models in free order (N32 path, yoda_layout.h MixWord)
  DevBuf kx1;       // K1's tile of the mixed-model nodes (N32 path, yoda_layout.h K1MixWord)
  // memory ranks (yoda_layout.h MemTab): the N32 memory fields are ranks; value tables
  bool mem_ranks = false;
  DevBuf memtab;
  std::vector<double> h_memtab;  // the host side of memtab's copy, until the next upload's
  MemTab mt = {};
  std::vector<uint64_t> h_frees;  // the distinct card frees, ascending (pod thresholds)
  std::vector<uint64_t> h_totals;  // ... and the distinct card totals (yoda_replace_nodes)
  // yoda_replace_nodes: the flags of the upload, and how many nodes are one-model with one
  // TotalMemory / one-model (all_one_model, all_uni4 below are these against n_nodes)
  uint32_t upload_flags = 0;
  uint32_t n_one_model = 0, n_uni4 = 0;
  DevBuf gtab, gtab_aux;  // the G table (yoda_layout.h GTab) + [G maxima | its reciprocals]
  GTab g = {};
  bool has_k1sum = false, has_k2sum = false;
  bool all_one_model = false;  // every node: one GPU model, one TotalMemory (kNodeUniform4|Total)
  // block-grouped node order of the private batch runs (node_perm at upload): copies of the
  // K1 / K2 summaries and the G table in that order, the local id of each position, and each
  // node's position (k_set_static keeps the copies current)
  bool perm_on = false;
  DevBuf k1sum_p, k2sum_p, gtab_p, perm_ids, perm_inv;
  DevBuf kx1_p, kmix_p;  // the mixed-model tiles in that order (immutable card data)
  DevBuf win_inv;        // capacity windows: each window slot's sorted position (k_window_out)
  // 64-node block summaries (yoda_layout.h BlockSumWord) of the snapshot order and of the
  // block-grouped copy's; loose: node-state pushes left their CardNumber bounds valid but not
  // tight (k_set_static's atomics), recomputed before the next private run
  DevBuf blksum, blksum_p;
  bool blksum_loose = false;
  bool greedy_active = false;  // inside a greedy batch (its pushes keep the bounds valid)
  // K2 block bounds (yoda_layout.h kbub_*) of both orders; dirty: static scores changed since
  DevBuf kbub, kbub_p;
  DevBuf kbdec, kbdec_p;     // the non-G block bounds (yoda_layout.h kbdec_*) of both orders
  DevBuf kb_levels;          // the free levels of kbub's lv[] bounds (kKbLevels u32)
  bool seeds_valid = false;  // this run's block K1 cleared and writes the K2 pruning seeds
  bool blk_fresh = false;    // this run cleared the whole block-list buffer (list, seeds, gbest)
  bool kb_levels_ok = false;  // built for the current snapshot
  bool kbub_dirty = true;   // a static score rose above the bounds' own: rebuild before use
  bool kbub_loose = false;  // static scores only fell since the build: valid, rebuilt for runs
  std::vector<uint64_t> ub_stat;  // each node's static score when the bounds were built
  // a pushed static score against the bounds: above -> dirty, else loose
  void note_static(uint32_t n, uint64_t s) {
    if (n < ub_stat.size() && s <= ub_stat[n]) kbub_loose = true; else kbub_dirty = true;
  }
  // the top tenth of the blocks by bound (lv[0]) at upload, per order: K2 visits them first
  DevBuf hot, hot_p;
  bool hot_ok = false;
  PermCopy perm_copy() const {
    PermCopy pc;
    if (perm_on) {
      pc.inv = perm_inv.as<uint32_t>();
      pc.sum = k1sum_p.as<unsigned char>();
      pc.sum2 = k2sum_p.as<unsigned char>();
      pc.mix = kmix_p.as<uint32_t>();
      pc.x1 = kx1_p.as<uint32_t>();
      pc.bsum_p = blksum_p.p ? blksum_p.as<uint32_t>() : nullptr;
    }
    pc.bsum = blksum.p && path == Path::N32 ? blksum.as<uint32_t>() : nullptr;
    pc.bsum_words = bsum_stride(K) / 4u;
    return pc;
  }
  // this run is block-grouped.  On a snapshot with mixed-model nodes (or per-card TotalMemory)
  // only a large batch takes the grouped order: grouping gathers the nodes that need the
  // per-card pass into a few blocks, so a few (wave, chunk) tasks carry all of it -- on a
  // small batch (config 4: 10k pods x 20k nodes, K1 88 -> 143 us, the last tasks alone)
  // that tail outweighs the whole-block decisions, which win from 32k pods on (the config-4
  // generator at 100k x 100k: K1 0.52 -> 0.20 ms)
  // (a sampled run reads the upload-order tables, so that a mask position is a node id)
  bool perm_run() const {
    return perm_on && count_order && samp_m == 0 &&
           (all_one_model || n_work >= kGroupedMixedMinPods);
  }
  // yoda_set_node_sampling: samp_m != 0: on (num_to_find).  The pods' start ids (LOCAL, caller
  // order; empty: every pod starts at node 0 of the shard) stay across pod uploads.  samp_scr:
  // the pass's scratch; samp_zt: the upload order's zero_total bits per block, rebuilt by every
  // sampled run; samp_out [2][n_pods]: n_found, next_start of the last sampled run (samp_ran).
  uint32_t samp_m = 0;
  std::vector<uint32_t> h_start;
  DevBuf samp_start, samp_scr, samp_zt, samp_out;
  bool samp_ran = false;
  static constexpr uint32_t kGroupedMixedMinPods = 32768;
  bool all_uni4 = false;       // every node: one GPU model (kNodeUniform4)
  std::vector<unsigned char> host_records;  // kept for alloc updates (greedy)
  std::vector<uint32_t> host_k2sum;         // idem (its static score words)
  std::vector<uint64_t> h_total_sum, h_free_sum, h_alloc, h_card_number;
  // bound on any raw score of this snapshot whatever the allocated memory (Basic + the
  // largest Allocate 300 + Actual): the packed top-k keys need score < 2^(64 - index bits)
  uint64_t score_bound = ~0ull;
  long double sb_cards = 0.0L;  // its card and Allocate terms; sb_actual: the largest Actual
  uint64_t sb_actual = 0;
  uint64_t h_gmax[6] = {1, 1, 1, 1, 1, 1};  // the G maxima on the device (gtab_aux; N32)
  // yoda_set_node_present: 1 per absent node (the records' kNodeAbsent), how many; an upload
  // makes every node present.  The G maxima above are those of the PRESENT nodes.
  std::vector<uint8_t> h_absent;
  uint32_t n_absent = 0;
  // yoda_set_candidates: other plugins' Filter results as candidate classes.  cand_classes != 0:
  // on.  One 64-bit word per node (bit c: a candidate of class c): the host mirror, the device
  // table in upload order with the AND and the zero_total bits of each 64-node block, and all
  // three again in the block-grouped order (perm_on).  The pods' class bytes (caller order; empty: every pod YODA_CAND_ANY) stay
  // across pod uploads; cls_top: the largest class in them, -1 none.
  uint32_t cand_classes = 0;
  std::vector<uint64_t> h_cand;
  DevBuf cand_w, cand_and, cand_zt, cand_w_p, cand_and_p, cand_zt_p;
  std::vector<uint8_t> h_cls;
  int cls_top = -1;
  DevBuf cand_cls;
  // yoda_greedy_candidates: yoda_greedy honours the classes.  Inside such a batch h_cls is the
  // slice of the uploaded window (GreedyClasses) and cand_cls the batch's classes in queue order,
  // of which the uploaded pods start at cls_off (0 outside a batch)
  bool greedy_cand = false;
  size_t cls_off = 0;
  // yoda_shard_candidates: the sharded evaluation step honours the classes.  cls_hash: a 64-bit
  // hash of the caller's class bytes (yoda_set_pod_classes), for the shards' agreement digest
  bool shard_cand = false;
  uint64_t cls_hash = 0;
  // yoda_diagnose: the selected pods (caller ids) and their number, the counts [P][4];
  // diag_done: they are the pending run's (cleared wherever a run completes; a run that is no
  // longer pending -- ran == false -- has no diagnosis either).  diag_rows: yoda_reason_rows'
  // padded rows on the device and their pinned copy
  bool diag_done = false;
  DevBuf diag_list, diag_n, diag_counts, diag_rows;
  PinnedBuf diag_stage;
  // yoda_update_node_cards / yoda_snapshot_check: the changed nodes' packed rows (host), the
  // block summaries k_bsum_build writes for the self-check
  std::vector<uint32_t> cu_rows;
  DevBuf bsum_chk;

  // pods: one device blob of per-pod arrays (PodArray order), staged through pinned memory
  bool has_pods = false;
  uint32_t n_pods = 0;
  DevBuf pod_blob;
  PinnedBuf pod_stage;
  hipEvent_t stage_event = nullptr;
  // the deferred pod arrays' copy of a private run goes on a copy stream of its own, alongside
  // the run's kernels (pods_complete_async); rest_event joins it back into `stream`
  hipStream_t copy_stream = nullptr;
  hipEvent_t core_event = nullptr, rest_event = nullptr;
  bool rest_join = false;
  // the staged f64 thresholds and Mode B weights of the last upload are still to be written
  // (pods_pack_rest: derived from the staged u64 ones, after a run's kernel launches)
  bool rest_lazy = false;
  hipEvent_t switch_event = nullptr;  // yoda_set_stream: the old stream's work, waited on
  bool stage_pending = false;
  size_t pod_off[kPodArrays] = {};
  size_t pod_rest_off = 0, pod_rest_bytes = 0;  // the blob's deferred part (pods_complete)
  bool fast_run = false;  // inside a private block-kernel run: the deferred part may wait
  // a deferred private run's kernels are in flight before the non-core pod arrays (m_f, c_f,
  // m_u, c_u, alpha, beta) reach the device: pod_params hands out null pointers for them, so a
  // kernel that read them there would fault instead of reading the last batch's values
  bool core_only = false;
  // batch ordering (yoda_order.hip): when `ordered`, the kernels of this run read the pods
  // from pod_sorted (sorted position i = original pod perm[i]); bitmask/rows stay in sorted
  // order and are un-permuted by their transposes, the per-pod outputs by finalize().
  bool order_enabled = true;
  bool order_pad = true;  // yoda_set_pod_order(h, 1): pad private runs' groups to waves
  bool ordered = false;
  DevBuf pod_sorted, perm, order_scratch;
  uint32_t key_bits[3] = {24, 8, 32};  // widths of the batch's sort-key fields (c, n, m)
  // Counting-sort order (yoda_order.hip, OrderMeta), built at upload: the batch's distinct
  // (clock, number, has-memory) groups ascending, their first sorted positions unpadded and
  // padded to a wave, and the padding slots (dst, src) -- one device blob, host copy kept
  // for the async upload.  n_work: the sorted positions of this run (n_pad when padded).
  bool og_ok = false;
  uint32_t og_groups = 0, og_nb_log2 = 0, og_m_shift = 0, og_n_pad_slots = 0;
  uint32_t n_pad = 0, n_work = 0;
  size_t og_off_start = 0, og_off_start_pad = 0, og_off_pad = 0;
  std::vector<unsigned char> og_host;
  DevBuf order_meta, order_hist, order_bstart, order_slot, order_bkt;
  size_t sorted_off[kPodArrays] = {};

  // state
  DevBuf maxima, counts, rcp, best, idx, ties, lowest, pick, status, ties_out, flagged, n_flagged;
  // scatter targets of unpermute_outputs, swapped with the buffers above after each scatter
  DevBuf pick_alt, status_alt, ties_out_alt, counts_alt, best_alt, maxima_alt;
  DevBuf win_dev;  // a capacity window's outputs on the device, then one DMA copy to win_stage
  DevBuf bitmask, bitmask_t, rows, rows_t, norm;
  DevBuf blk;               // [wave][node block / 64] u64: blocks with a feasible pod (K1 -> K2)
  bool blk_valid = false;   // the last K1 wrote blk (block-classified K1 on this batch)
  bool blk_zeroed = false;  // this run's order already cleared blk (no memset in phase 1)
  bool flagged_dirty = true;  // n_flagged may be nonzero (a generic run since the last clear)
  bool maxima_sorted = false;  // h->maxima still in the last run's sorted order (n_work rows)
  bool rcp_ready = false;      // phase 1 wrote the reciprocals of its (final) maxima
  // a private ordered run off the generic path (defer_merge2, set by run_private around its
  // phase 2): phase 2 leaves the merge of its K2 partials to finalize, which runs it inside its
  // own kernel (launch_reduce2_finalize); merge2 is that pending merge
  bool defer_merge2 = false;
  struct Merge2 {
    bool on = false;
    Partials part{};
    uint32_t C = 0;
    bool is_f64 = false;
    const uint64_t* cmask = nullptr;
    int64_t *best = nullptr, *low = nullptr;
    uint32_t *idx = nullptr, *ties = nullptr;
  } merge2;
  bool count_order = false;    // this run orders by the counting sort (private runs)
  DevBuf bsum;              // [wave][node block] BlockMask: the block K1's sparse masks
  bool bm_sparse = false;   // the last K1 wrote the sparse form (bsum + partial masks only)
  const BlockMask* bs_ptr() const { return bm_sparse ? bsum.as<BlockMask>() : nullptr; }
  // the sparse masks' block list: a block whose bit is clear has no feasible pod of the wave
  // and its BlockMask was not written this run
  const uint64_t* blk_ptr() const { return bm_sparse ? blk.as<uint64_t>() : nullptr; }
  // greedy
  DevBuf tk_s_part, tk_i_part, tk_s, tk_i, upd_node, upd_val, upd_cn;
  DevBuf g1_part, g1_done;  // k_greedy_one partials + block counter (zeroed once)
  DevBuf p_wit, wit;        // capacity greedy: witness partials [2][6][C][P], merged [2][6][P]
  DevBuf one_feas, one_part, one_done, one_out;  // k_one_*: a pod against the current state
  PinnedBuf upd_stage, pick_stage, win_stage;
  PinnedBuf poll_stage;  // coherent: the greedy fallback's pick, polled by the host
  uint32_t greedy_restarts = 0;
  uint32_t greedy_refreshes = 0;  // flags-0 mid-window list refreshes (last yoda_greedy)
  hipEvent_t upd_event = nullptr;
  bool upd_pending = false;
  std::vector<uint32_t> upd_slot;  // yoda_set_node_state: a node's entry in the list (~0u: none)
  std::vector<uint32_t> h_pos;  // yoda_shard_topk: caller pod index -> sorted position
  bool topk_ready = false;      // the bitmask / reciprocals of that batch are still valid
  uint32_t greedy_windows = 0, greedy_fallbacks = 0;
  double greedy_window_ms = 0, greedy_fallback_ms = 0, greedy_resolve_ms = 0;
  double greedy_prep_ms = 0;  // (YODA_GREEDY_DEBUG) the host part of the windows: state push,
                              // window gather + pod upload + order launches
  DevBuf p_max_u, p_cnt, p_best_f, p_best_i, p_idx, p_ties, p_low_f, p_low_i, p_err;
  uint32_t C1 = 1, chunk1 = 32;  // K1 node chunking (partial chunks; chunk1: nodes per K1 wave)
  bool pack16 = true;            // N32: the small card fields fit 16 bits (packed K1 partials)
  bool q32 = true;               // ... and <= kF32SmallMax (the block K2's f32 quotients)
  uint64_t small_max = 0;        // the largest bandwidth / clock / core / power (any path)
  // heaviest-first pod blocks for the argmax block K2 (k_lpt_order): this run uses them,
  // the per-wave weights K1 adds to (zero between runs), the order (valid once sorted)
  bool lpt_active = false, lpt_sorted = false;
  DevBuf lpt_w, lpt_order;
  // the block K1's own heaviest-first order (k1_probe's weights, ranked before the K1): valid
  // for this run once k1_sorted
  bool k1_sorted = false;
  bool k1_rec_ok = false;  // k1_rec holds this run's records (written with the order)
  DevBuf k1_w, k1_order, k1_rec;  // (k1_rec: the waves' K1WaveRec records, beside k1_w)
  uint32_t C2 = 1, chunk2 = 32;  // K2 / K3 node chunking
  // selectHost draw (yoda_set_tie_draw): yoda_run / yoda_eval draw each tied pod's pick after
  // finalize (draw_pass); the listed sorted positions, their MIN keys, the list's length
  bool tie_draw = false;
  uint64_t tie_seed = 0, tie_pod_base = 0;
  DevBuf draw_list, draw_keys, draw_n;
  // The draw of a node-sharded step (yoda_shard_tie_draw; it draws only beside tie_draw).
  // draw_stage: 0 no sharded outcome to draw on, 1 a sharded finalize completed (its exact
  // merge may still be pending: k3_pending), 2 yoda_shard_draw_keys emitted that step's keys.
  // xkeys: comm_step's key buffer [P]; norm_top: the exact merge's GLOBAL top normalized
  // scores by sorted position (k_merge3_top)
  bool shard_draw = false;
  int draw_stage = 0;
  DevBuf xkeys, norm_top;
  bool shard_draws() const { return shard_draw && tie_draw; }
  int cap[2][3][2] = {};        // resident workgroups per (kernel, path, mode), cached
  int last_mode = -1;
  bool ran = false;
  bool ran_bitmask = false;
  bool phase1_done = false;
  bool phase1_wit = false;  // the last shard phase 1 was the witness one (capacity windows)

  // class counters of the block kernels (yoda_class_stats_*): device [8] u64 + host totals
  bool class_stats = false;
  DevBuf stats_dev;
  uint64_t stats_pairs1 = 0, stats_pairs2 = 0;
  unsigned long long* stats_ptr() const {
    return class_stats ? stats_dev.as<unsigned long long>() : nullptr;
  }
  // yoda_comm_*: this rank's RCCL communicator and the two exchange buffers of a step
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  DevBuf ex1, rec, rec_all;  // [maxima 6P | count slots world x P] u64; ShardRec [P], [world][P]
  // Caller-order exchange (xo): a node-shard evaluation whose exchanged buffers are in the
  // caller's pod order, so that each shard runs its private order -- the padded counting sort
  // and the block-grouped node order of yoda_run -- instead of the reproducible radix order
  // every shard must otherwise share (5.7x slower at one shard of config 3: no node grouping,
  // no padded waves).  yoda_comm_run does it on the fast record paths; the yoda_shard_* calls
  // after yoda_shard_exchange_order(h, 1).  xcnt, xbest, ... : the caller-order copies.
  bool xo_enabled = false, xo = false;
  DevBuf xcnt, xbest, xidx, xties, xlow;
  DevBuf cg_max, cg_cnt, cg_wit, cg_gather;  // yoda_comm_greedy: exchange buffers
  uint32_t comm_greedy_stats[5] = {};          // yoda_comm_greedy_stats
  // sharded exact normalize (K3 over a shard): per-pod records of the flagged pods, pending
  // until the shards' records are merged (yoda_shard_exact_merge)
  DevBuf k3rec, k3all;
  bool k3_pending = false;
  // Mode B batch path: the batch's pod classes (distinct (alpha, beta) bit pairs), built on
  // the first Mode B run after an upload: device [2][D] f64 (alpha, beta) + [P] u32 class
  // of each pod; chunk partials [2][C][D] u32
  bool b_cls_ready = false;
  uint32_t b_ncls = 0;
  DevBuf b_cab, b_cls, b_part;
  // yoda_mode_b_follow: Mode B's batch path honours the absent nodes and the candidate classes.
  // The classes are then keyed by (alpha, beta, candidate class) -- b_cls_keyed: the ready ones
  // are -- with their selectors in b_csel [D].  b_elig [n_nodes] DiskElig and b_ecnt [65] are
  // rebuilt on the first Mode B run after the node set or the words changed (b_elig_dirty;
  // b_elig_builds: since the upload).  b_last_*: the last Mode B batch run (yoda_mode_b_info).
  bool b_follow = false;
  bool b_cls_keyed = false;
  bool b_elig_dirty = true;
  uint32_t b_elig_builds = 0;
  bool b_last_elig = false;
  uint32_t b_last_ncls = 0;
  DevBuf b_csel, b_elig, b_ecnt, b_pres;
  // yoda_mode_b_sampling: Mode B's batch path honours node sampling.  b_rbits / b_rpfx: the rank
  // tables [65][ceil(n_nodes / 64)] of the walk plan, built with the eligibility table
  // (b_rank_for: the b_elig_builds they were built at; b_rank_builds: since the upload); b_walk
  // [n_pods] DiskWalk: the plan's records (b_walk_ok: of this run's phase 1).  b_samp_last_*: the
  // last Mode B run (yoda_mode_b_sampling_info).  ev_bplan: the plan's profile events.
  bool b_samp = false;
  uint32_t b_rank_for = 0xffffffffu;
  uint32_t b_rank_builds = 0;
  bool b_walk_ok = false;
  bool b_samp_last = false, b_samp_last_elig = false;
  DevBuf b_rbits, b_rpfx, b_walk;
  uint32_t k3_nfl = 0;
  // profiling: event pairs around K1 / K2
  bool profiling = false;
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_k1, ev_k2;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_cand;  // around the narrowing pass
  double cand_ms = 0;  // ... summed by yoda_profile_read, handed out by yoda_candidates_profile
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_samp;  // around the sampling pass
  double samp_ms = 0;  // ... likewise, handed out by yoda_sampling_profile
  size_t ev_used = 0;

  hipEvent_t next_event() {
    if (ev_used == ev_pool.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      ev_pool.push_back(e);
    }
    return ev_pool[ev_used++];
  }

  ~yoda_handle() {
    if (comm && rccl().ok) (void)rccl().comm_destroy(comm);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (stage_event) (void)hipEventDestroy(stage_event);
    if (switch_event) (void)hipEventDestroy(switch_event);
    if (upd_event) (void)hipEventDestroy(upd_event);
    if (core_event) (void)hipEventDestroy(core_event);
    if (rest_event) (void)hipEventDestroy(rest_event);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

namespace {

int fail(yoda_t* h, int code, const std::string& msg) {
  if (h) h->last_error = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(h, YODA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

int pow2_cards(uint32_t kmax) {
  int k = 1;
  while ((uint32_t)k < kmax) k <<= 1;
  return k;
}

// Node chunking of one kernel: C chunks x ceil(P/256) pod blocks = B workgroups.  B is sized
// to ~8 full "rounds" of the kernel's resident capacity (occupancy API), so the last round is
// nearly full (efficiency >= 1 - pod_blocks / (8 cap)) and chunks stay small enough to
// balance data-dependent work (K2 skips infeasible nodes).
// Tuning knobs for A/B runs (tools/ab.sh): YODA_CHUNK_ROUNDS1 / 2 (K1 / K2; defaults 6 / 8;
// both at once, config 3: 3 1.92 ms, 4 1.87, 6 1.81, 8 1.78, 10 2.02 per step) and
// YODA_MIN_CHUNK_NODES (default 0 = no floor; a floor keeps the per-(wave, chunk) set-up of
// the block-classified kernels amortised when few pod blocks would otherwise mean many
// small chunks, e.g. one rank's pod shard).  Read once per process.
// Host worker pool for the packing loops (pod upload): threads created once per process and
// parked on a condition variable between calls -- spawning 15 threads per upload cost more
// than the packing itself.  run(n, fn) calls fn(0..n-1) once each, the caller taking part;
// calls are serialised (one batch at a time).
uint32_t pool_spin_us();  // (below, after the knobs)

// After a batch the workers spin for a short while before parking: a scheduler uploads its
// batches back to back, and a parked thread's wake-up is what a late range costs the pack.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool pool;
    return pool;
  }
  uint32_t size() const { return (uint32_t)threads_.size() + 1u; }
  void run(uint32_t n, const std::function<void(uint32_t)>& fn) {
    if (n == 0) return;
    if (n == 1 || threads_.empty()) {
      for (uint32_t i = 0; i < n; ++i) fn(i);
      return;
    }
    std::lock_guard<std::mutex> serial(call_mu_);
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn;
      n_ = n;
      last_n_.store(n, std::memory_order_relaxed);
      next_.store(0);
      left_ = n;
      gen_.fetch_add(1);  // (after the batch's fields: a spinning worker reads them next)
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return left_ == 0; });
    fn_ = nullptr;
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_.store(true);
      gen_.fetch_add(1);
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }

 private:
  HostPool() {
    const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    const uint32_t n = std::min(16u, hw) - 1u;  // + the calling thread
    for (uint32_t i = 0; i < n; ++i) threads_.emplace_back([this, i] { loop(i); });
  }
  void work() {
    for (;;) {
      const uint32_t i = next_.fetch_add(1);
      if (i >= n_) return;
      (*fn_)(i);
      std::lock_guard<std::mutex> lk(mu_);
      if (--left_ == 0) done_cv_.notify_one();
    }
  }
  void loop(uint32_t self) {
    uint64_t seen = 0;
    const uint32_t spin_us = pool_spin_us();
    for (;;) {
      // only the workers the last batch used spin (a small batch leaves the rest parked), and
      // they pause between polls so a sibling hyperthread keeps its issue slots
      if (spin_us && self + 1u < last_n_.load(std::memory_order_relaxed)) {
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t it = 0;
        while (gen_.load() == seen && !stop_.load()) {
          __builtin_ia32_pause();
          if ((++it & 63u) == 0u &&
              std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us))
            break;
        }
      }
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_.load() || gen_.load() != seen; });
        if (stop_.load()) return;
        seen = gen_.load();
      }
      work();
    }
  }
  std::vector<std::thread> threads_;
  std::mutex mu_, call_mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(uint32_t)>* fn_ = nullptr;
  uint32_t n_ = 0, left_ = 0;
  std::atomic<uint32_t> next_{0}, last_n_{0};
  std::atomic<uint64_t> gen_{0};
  std::atomic<bool> stop_{false};
};

uint32_t pool_spin_us() {
  // how long a HostPool worker spins for the next batch before parking (YODA_POOL_SPIN_US,
  // A/B knob; 0 parks at once).  1 ms covers a batch-to-batch gap of the e2e loop (~0.9 ms);
  // a scheduler that uploads less often parks its workers after that.
  static const uint32_t v = YODA_KNOB("YODA_POOL_SPIN_US", 1000);
  return v;
}
// Diagnostics (*_TRACE, *_DEBUG): counters, timings and traces only, never results or policy.
static uint32_t diag_env(const char* name, uint32_t dflt) {
  const char* s = std::getenv(name);
  return (s && *s) ? (uint32_t)std::strtoul(s, nullptr, 10) : dflt;
}

constexpr uint32_t kMinChunkNodes = 1536;
// the reduces read the chunk partials one thread per pod up to this many chunks (the chunk
// masks' limit too); beyond, one wave per pod (yoda_kernels.hip kWaveReduceChunks)
constexpr uint32_t kPlainReduceChunks = 48;

void plan_chunks_for(uint32_t cap, uint32_t rounds, uint32_t n_pods, uint32_t n_nodes,
                     uint32_t* C_out, uint32_t* chunk_out) {
  static const uint32_t min_chunk = YODA_KNOB("YODA_MIN_CHUNK_NODES", 0);
  const uint32_t pod_blocks = std::max<uint32_t>(1, (n_pods + kBlock - 1) / kBlock);
  const uint32_t max_chunks = std::max<uint32_t>(1, (n_nodes + kChunkAlign - 1) / kChunkAlign);
  if (cap == 0) cap = 2048;
  uint32_t C = std::max<uint32_t>(1, (uint32_t)(((uint64_t)rounds * cap) / pod_blocks));
  C = std::min(C, max_chunks);
  if (min_chunk) {
    C = std::min(C, std::max<uint32_t>(1, (n_nodes + min_chunk - 1) / min_chunk));
  } else if (pod_blocks >= 64) {
    // a large pod batch over few nodes (one rank of a node-sharded batch): chunks of at least
    // kMinChunkNodes amortise the per-(wave, chunk) set-up of the block kernels, as long as
    // the grid keeps two rounds of resident workgroups (A/B in profiles/r02/final/)
    const uint32_t c_nodes = (n_nodes + kMinChunkNodes - 1) / kMinChunkNodes;
    const uint32_t c_rounds = (uint32_t)((2ull * cap + pod_blocks - 1) / pod_blocks);
    C = std::min(C, std::max<uint32_t>({1u, c_nodes, c_rounds}));
  }
  // a multiple of 8 chunks lets the kernels give each XCD whole chunks (tile() in
  // yoda_kernels.hip); trailing chunks may then be empty (they write identity partials)
  const bool xcd = C >= 8;
  if (xcd) C = (C + 7) / 8 * 8;
  uint32_t chunk = (n_nodes + C - 1) / C;
  chunk = std::max<uint32_t>(kChunkAlign, (chunk + kChunkAlign - 1) / kChunkAlign * kChunkAlign);
  *chunk_out = chunk;
  *C_out = xcd ? C : std::max<uint32_t>(1, (n_nodes + chunk - 1) / chunk);
}

int capacity(yoda_t* h, int which, int mode) {
  int& c = h->cap[which - 1][(int)h->path][mode == YODA_MODE_DISKIO ? 1 : 0];
  if (c == 0) c = kernel_capacity(h->K, h->path, which, mode == YODA_MODE_DISKIO);
  return c;
}

void plan_chunks(yoda_t* h, int mode, uint32_t n_pods, uint32_t n_nodes) {
  // K1's partials are 24 B a (pod, chunk) and its reduce reads them all, but with the
  // heaviest-first pod blocks and the lane = block pass a K1 task is short and the tail is
  // set by the task size: 8 rounds while the chunks stay few enough for the chunk masks
  // (C1 <= kPlainReduceChunks; config 3 K1 0.199 -> 0.182 ms, mixed50 / bytes / greedy neutral
  // or better; 10: 0.185, 12: 0.201, 16: 0.241 ms), else 6 (a 50k / 25k / 12.5k-pod batch,
  // one pod-sharded rank: K1 0.137 / 0.139 / 0.138 ms at 6 against 0.155 / 0.140 / 0.157 at
  // 8); profiles/r06/rounds1/.  YODA_CHUNK_ROUNDS1 (A/B knob) fixes the rounds.
  static const uint32_t r1_knob = YODA_KNOB("YODA_CHUNK_ROUNDS1", YODA_KNOB("YODA_CHUNK_ROUNDS", 0));
  static const uint32_t r2 = std::max<uint32_t>(1, YODA_KNOB("YODA_CHUNK_ROUNDS2",
                                                           YODA_KNOB("YODA_CHUNK_ROUNDS", 8)));
  const uint32_t cap1 = (uint32_t)capacity(h, 1, mode);
  plan_chunks_for(cap1, r1_knob ? r1_knob : 8u, n_pods, n_nodes, &h->C1, &h->chunk1);
  if (!r1_knob && h->C1 > kPlainReduceChunks)
    plan_chunks_for(cap1, 6u, n_pods, n_nodes, &h->C1, &h->chunk1);
  // YODA_K1_MAX_CHUNKS (A/B knob, default off): at most that many K1 chunks, so that small
  // batches keep their partials (and k_reduce1's reads) few
  static const uint32_t c1_max = YODA_KNOB("YODA_K1_MAX_CHUNKS", 0);
  if (c1_max && h->C1 > c1_max) {
    h->chunk1 = ((n_nodes + c1_max - 1) / c1_max + kChunkAlign - 1) / kChunkAlign * kChunkAlign;
    h->C1 = std::max<uint32_t>(1, (n_nodes + h->chunk1 - 1) / h->chunk1);
    if (h->C1 >= 8) {  // keep a multiple of 8 (XCD tiling); trailing chunks may be empty
      h->C1 = (h->C1 + 7) / 8 * 8;
    }
  }
  plan_chunks_for((uint32_t)capacity(h, 2, mode), r2, n_pods, n_nodes, &h->C2, &h->chunk2);
}

// u64 words of the block-list buffer: the list, the seeds, the shared best (ensure_state)
size_t blk_words(const yoda_t* h, uint32_t P) {
  const size_t nw = (P + 63) / 64;
  return nw * (blk_row(h->n_nodes) + 1) + P + 2 * nw;  // + the two chunk masks per wave
}

int ensure_state(yoda_t* h, uint32_t P) {
  const size_t CP = (size_t)std::max(h->C1, h->C2) * P;
  HIP_TRY(h, h->maxima.ensure(6 * (size_t)P * 8));
  HIP_TRY(h, h->counts.ensure(2 * (size_t)P * 4));
  HIP_TRY(h, h->rcp.ensure(5 * (size_t)P * 8));
  HIP_TRY(h, h->best.ensure((size_t)P * 8));
  HIP_TRY(h, h->idx.ensure((size_t)P * 4));
  HIP_TRY(h, h->ties.ensure((size_t)P * 4));
  HIP_TRY(h, h->lowest.ensure((size_t)P * 8));
  HIP_TRY(h, h->pick.ensure((size_t)P * 4));
  HIP_TRY(h, h->status.ensure((size_t)P * 4));
  HIP_TRY(h, h->ties_out.ensure((size_t)P * 4));
  HIP_TRY(h, h->flagged.ensure((size_t)P * 4));
  HIP_TRY(h, h->n_flagged.ensure(16));
  // [wave][node] u64 masks (yoda_layout.h), +8 words: K2 reads masks in groups of 8
  HIP_TRY(h, h->bitmask.ensure(((size_t)(P + 63) / 64 * bm_row(h->n_nodes) + 8) * 8));
  // the block list [waves][blk_row], the K2 pruning seeds [waves] (PodParams::seed), the shared
  // per-pod best [P] (PodParams::gbest): blk_words(P) u64, all cleared before each block K1
  HIP_TRY(h, h->blk.ensure(blk_words(h, P) * 8));
  HIP_TRY(h, h->bsum.ensure((size_t)(P + 63) / 64 * bs_row(h->n_nodes) * sizeof(BlockMask)));
  HIP_TRY(h, h->p_max_u.ensure(6 * CP * 8));
  if (h->generic) {
    HIP_TRY(h, h->p_best_i.ensure(CP * 8));
    HIP_TRY(h, h->p_low_i.ensure(CP * 8));
    HIP_TRY(h, h->p_err.ensure(CP * 4));
  }
  HIP_TRY(h, h->p_best_f.ensure(CP * 8));
  HIP_TRY(h, h->p_low_f.ensure(CP * 8));
  HIP_TRY(h, h->p_cnt.ensure(2 * CP * 4));
  HIP_TRY(h, h->p_idx.ensure(CP * 4));
  HIP_TRY(h, h->p_ties.ensure(CP * 4));
  return YODA_OK;
}

// gtab_aux: [G maxima 6 x u64 | G reciprocals 5 x f64]
constexpr size_t kGTabAuxBytes = 48 + 40;

PodParams pod_params(yoda_t* h) {
  unsigned char* b = (h->ordered ? h->pod_sorted : h->pod_blob).as<unsigned char>();
  const size_t* off = h->ordered ? h->sorted_off : h->pod_off;
  PodParams pp;
  pp.m_f = reinterpret_cast<double*>(b + off[kPodMF]);
  pp.c_f = reinterpret_cast<double*>(b + off[kPodCF]);
  pp.m_u = reinterpret_cast<uint64_t*>(b + off[kPodMU]);
  pp.c_u = reinterpret_cast<uint64_t*>(b + off[kPodCU]);
  pp.m_32 = reinterpret_cast<uint32_t*>(b + off[kPodM32]);
  pp.c_32 = reinterpret_cast<uint32_t*>(b + off[kPodC32]);
  pp.number = reinterpret_cast<uint64_t*>(b + off[kPodNumber]);
  pp.need_mem = reinterpret_cast<uint32_t*>(b + off[kPodNeedMem]);
  pp.need_clk = reinterpret_cast<uint32_t*>(b + off[kPodNeedClk]);
  pp.alpha = reinterpret_cast<double*>(b + off[kPodAlpha]);
  pp.beta = reinterpret_cast<double*>(b + off[kPodBeta]);
  if (h->core_only) pp.m_f = pp.c_f = pp.alpha = pp.beta = nullptr, pp.m_u = pp.c_u = nullptr;
  pp.g = h->has_k2sum ? h->g : GTab{};
  pp.mix = h->path == Path::N32 ? h->kmix.as<uint32_t>() : nullptr;
  pp.x1 = h->path == Path::N32 ? h->kx1.as<uint32_t>() : nullptr;
  pp.one_model = h->path == Path::N32 && h->all_one_model;
  pp.all_uni4 = h->path == Path::N32 && h->all_uni4;
  if (h->path == Path::N32 && h->has_k1sum && h->blksum.p) pp.bsum = h->blksum.as<uint32_t>();
  const bool ub_ok = h->path == Path::N32 && pp.g.tab && !h->kbub_dirty && h->kbub.p;
  if (ub_ok) pp.kbub = h->kbub.as<uint32_t>();
  pp.kbub_exact = ub_ok && !h->kbub_loose;
  // (A/B knobs: YODA_KB_LEVELS=0 / YODA_SEEDS=0 turn the level bounds / the seeds off)
  static const bool lv_env = YODA_KNOB("YODA_KB_LEVELS", 1) != 0;
  static const bool seeds_env = YODA_KNOB("YODA_SEEDS", 1) != 0;
  if (ub_ok && h->kb_levels_ok && lv_env) pp.kb_levels = h->kb_levels.as<uint32_t>();
  // the K2 pruning seeds live after the block list (cleared with it); the block K1 of this run
  // writes them, the argmax K2 of the same run reads them
  // (A/B knob: YODA_GBEST=0 turns the shared best off)
  static const bool gbest_env = YODA_KNOB("YODA_GBEST", 1) != 0;
  // (the non-G bounds pay on one-model snapshots at K <= 8: config 3's K2 0.32 -> 0.21 ms;
  // on mixed-model nodes and at K = 16 their per-block cost exceeds what they prune -- mixed50
  // K2 1.52 vs 1.29 ms, the config-4 generator 0.64 vs 0.48 ms, profiles/r05/y/ab.txt)
  // (YODA_KB_DEC_GROUPED, A/B knob: 1 = also on mixed fleets in the block-grouped order, whose
  // one-model blocks are whole again; 2 = there at K = 16 too)
  static const uint32_t dec_grouped = YODA_KNOB("YODA_KB_DEC_GROUPED", 1);
  const bool dec_ok = h->all_one_model ? h->K <= 8
                                        : h->perm_run() && dec_grouped != 0 &&
                                              (h->K <= 8 || dec_grouped == 2);
  if (ub_ok && dec_ok && h->kbdec.p) pp.kbdec = h->kbdec.as<uint32_t>();
  {
    const size_t nw = (h->n_work + 63) / 64;
    uint64_t* sd = h->blk.as<uint64_t>() + nw * blk_row(h->n_nodes);
    if (seeds_env && ub_ok && h->seeds_valid && h->blk_valid && h->bm_sparse && pp.g.tab)
      pp.seed = sd;
    if (gbest_env && ub_ok && h->blk_fresh) pp.gbest = sd + nw;  // [n_work] after the seeds
    // the chunk masks after the shared best
    uint64_t* cm = sd + nw + h->n_work;
    if (h->blk_fresh && h->path == Path::N32) {
      if (h->has_k1sum && h->C1 <= kPlainReduceChunks) pp.cmask1 = cm;
      if (h->has_k2sum && h->C2 <= kPlainReduceChunks) pp.cmask2 = cm + nw;
    }
  }
  if (ub_ok && h->hot_ok) pp.hot = h->hot.as<uint64_t>();
  if (h->perm_run()) {
    pp.ids = h->perm_ids.as<uint32_t>();
    pp.mix = h->kmix_p.as<uint32_t>();
    pp.x1 = h->kx1_p.as<uint32_t>();
    if (pp.g.tab) pp.g.tab = h->gtab_p.as<uint32_t>();
    pp.bsum = h->blksum_p.p ? h->blksum_p.as<uint32_t>() : nullptr;
    pp.kbub = ub_ok && h->kbub_p.p ? h->kbub_p.as<uint32_t>() : nullptr;
    pp.kbdec = pp.kbub && dec_ok && h->kbdec_p.p ? h->kbdec_p.as<uint32_t>() : nullptr;
    pp.hot = pp.kbub && h->hot_ok ? h->hot_p.as<uint64_t>() : nullptr;
  }
  pp.mt = h->mem_ranks ? h->mt : MemTab{};
  pp.nwords = h->pack16 ? kNarrowWords : kWideWords;
  pp.q32 = h->q32;
  if (h->lpt_active) {
    pp.lpt_w = h->lpt_w.as<uint32_t>();
    if (h->lpt_sorted) pp.lpt_order = h->lpt_order.as<uint32_t>();
    if (h->k1_sorted) pp.k1_order = h->k1_order.as<uint32_t>();
    if (h->k1_sorted && h->k1_rec_ok) pp.k1_rec = h->k1_rec.as<K1WaveRec>();
  }
  return pp;
}

Partials partials(yoda_t* h) {
  Partials p;
  p.max_u = h->p_max_u.as<uint64_t>();
  p.cnt = h->p_cnt.as<uint32_t>();
  p.best_f = h->p_best_f.as<double>();
  p.best_i = h->p_best_i.as<int64_t>();
  p.idx = h->p_idx.as<uint32_t>();
  p.ties = h->p_ties.as<uint32_t>();
  p.low_f = h->p_low_f.as<double>();
  p.low_i = h->p_low_i.as<int64_t>();
  p.err = h->p_err.as<uint32_t>();
  return p;
}

// The deferred part of the last pod upload (the arrays past kPodCoreArrays) to the device, on
// the handle's stream, from the pinned staging copy (reused only after stage_event).
constexpr uint64_t kPodF64Clamp = 1ull << 53;  // > every F64-path card field (<= 2^44)

// The staged arrays an upload left for later (rest_lazy): mf / cf from the staged mu / cu,
// alpha = beta = 0 (a batch without Mode B inputs).  Host work on the pool; a private run
// does it after launching its kernels.
void pods_pack_rest(yoda_t* h) {
  if (!h->rest_lazy) return;
  h->rest_lazy = false;
  const uint32_t P = h->n_pods;
  unsigned char* st = static_cast<unsigned char*>(h->pod_stage.p);
  const uint64_t* mu = reinterpret_cast<const uint64_t*>(st + h->pod_off[kPodMU]);
  const uint64_t* cu = reinterpret_cast<const uint64_t*>(st + h->pod_off[kPodCU]);
  double* mf = reinterpret_cast<double*>(st + h->pod_off[kPodMF]);
  double* cf = reinterpret_cast<double*>(st + h->pod_off[kPodCF]);
  double* al = reinterpret_cast<double*>(st + h->pod_off[kPodAlpha]);
  double* be = reinterpret_cast<double*>(st + h->pod_off[kPodBeta]);
  const uint32_t n_thr = std::min<uint32_t>(HostPool::get().size(), std::max(1u, P / 4096));
  const uint32_t per = (P + n_thr - 1) / n_thr;
  auto range = [&](uint32_t t) {
    for (uint32_t p = std::min(P, t * per), e = std::min(P, (t + 1) * per); p < e; ++p) {
      mf[p] = (double)std::min(mu[p], kPodF64Clamp);
      cf[p] = (double)std::min(cu[p], kPodF64Clamp);
      al[p] = be[p] = 0.0;
    }
  };
  if (n_thr > 1) HostPool::get().run(n_thr, range); else range(0);
}

// Make `stream` wait for a copy pods_complete_async issued (every reader of the deferred
// arrays comes through pods_complete).
int pods_join(yoda_t* h) {
  if (!h->rest_join) return YODA_OK;
  h->rest_join = false;
  HIP_TRY(h, hipStreamWaitEvent(h->stream, h->rest_event, 0));
  return YODA_OK;
}

// The deferred part on the copy stream, after what `stream` holds so far (the core copy of
// the upload: the run's kernels do not wait for it); pods_join after the run's launches.
int ensure_copy_stream(yoda_t* h) {
  if (h->copy_stream) return YODA_OK;
  HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  HIP_TRY(h, hipEventCreateWithFlags(&h->core_event, hipEventDisableTiming));
  HIP_TRY(h, hipEventCreateWithFlags(&h->rest_event, hipEventDisableTiming));
  return YODA_OK;
}

int pods_complete_async(yoda_t* h) {
  if (h->pod_rest_bytes == 0) return YODA_OK;
  if (!h->copy_stream) return fail(h, YODA_ERR_STATE, "pods_complete_async: no copy stream");
  pods_pack_rest(h);
  unsigned char* st = static_cast<unsigned char*>(h->pod_stage.p);
  // (core_event: recorded after the upload's copy -- the run's kernels are queued since)
  HIP_TRY(h, hipStreamWaitEvent(h->copy_stream, h->core_event, 0));
  HIP_TRY(h, hipMemcpyAsync(h->pod_blob.as<unsigned char>() + h->pod_rest_off, st + h->pod_rest_off,
                            h->pod_rest_bytes, hipMemcpyHostToDevice, h->copy_stream));
  HIP_TRY(h, hipEventRecord(h->stage_event, h->copy_stream));
  HIP_TRY(h, hipEventRecord(h->rest_event, h->copy_stream));
  h->stage_pending = true;
  h->rest_join = true;
  h->pod_rest_bytes = 0;
  return YODA_OK;
}

int pods_complete(yoda_t* h) {
  if (int rc = pods_join(h)) return rc;
  if (h->pod_rest_bytes == 0) return YODA_OK;
  pods_pack_rest(h);
  unsigned char* st = static_cast<unsigned char*>(h->pod_stage.p);
  HIP_TRY(h, hipMemcpyAsync(h->pod_blob.as<unsigned char>() + h->pod_rest_off, st + h->pod_rest_off,
                            h->pod_rest_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->stage_event, h->stream));
  h->stage_pending = true;
  h->pod_rest_bytes = 0;
  return YODA_OK;
}

// Mode B has no Filter and kernels of its own, none of which reads the presence bits
// (yoda_set_node_present): while a node is absent its entry points refuse to run.
// batch: the single-handle batch path (yoda_run, yoda_eval, the row calls, yoda_greedy), which
// follows both once yoda_mode_b_follow is on; the shard and communicator calls keep refusing.
// Node sampling cuts the batch path only (yoda_run, yoda_eval, the row calls) -- Mode A's, and
// Mode B's once yoda_mode_b_sampling is on: everything else that evaluates refuses while it is on.
int samp_refuse(yoda_t* h, const char* what) {
  if (!h->samp_m) return YODA_OK;
  return fail(h, YODA_ERR_STATE,
              std::string(what) + " does not honour node sampling (yoda_set_node_sampling): "
                                  "turn it off (num_to_find 0)");
}

int mode_b_absent(yoda_t* h, int mode, bool batch = false) {
  if (mode != YODA_MODE_DISKIO) return YODA_OK;
  // (yoda_mode_b_sampling: yoda_run, yoda_eval and the row calls score each pod's sample;
  // yoda_greedy refuses sampling before it gets here)
  if (!(batch && h->b_samp))
    if (int rc = samp_refuse(h, "Mode B")) return rc;
  if (batch && h->b_follow) return YODA_OK;
  if (h->cand_classes)
    return fail(h, YODA_ERR_STATE,
                "Mode B does not honour candidate classes (yoda_set_candidates): turn them off");
  if (h->n_absent == 0) return YODA_OK;
  return fail(h, YODA_ERR_STATE,
              "Mode B does not honour absent nodes (yoda_set_node_present): return every node "
              "or upload the snapshot without them");
}

// Candidate classes narrow the batch path only (yoda_run, yoda_eval, the row calls): the greedy,
// shard and communicator entry points refuse to run while they are on, as Mode B does
// (yoda_greedy on one handle: until yoda_greedy_candidates is on).
// step: a call of the sharded Mode A evaluation step, which runs once yoda_shard_candidates is
// on (phase 1 narrows the masks and counts whichever entry point called it; Mode B on shards
// keeps refusing through mode_b_absent).
int cand_refuse(yoda_t* h, const char* what, bool step = false) {
  // (every caller is a greedy, shard or communicator entry point: none of them samples)
  if (int rc = samp_refuse(h, what)) return rc;
  if (!h->cand_classes || (step && h->shard_cand)) return YODA_OK;
  return fail(h, YODA_ERR_STATE,
              std::string(what) + " does not honour candidate classes (yoda_set_candidates): "
                                  "turn them off (n_classes 0)");
}

// A batch run with candidates on: the class array fits the uploaded batch and the class count.
int cand_ready(yoda_t* h) {
  if (!h->cand_classes) return YODA_OK;
  if (!h->h_cls.empty() && h->h_cls.size() != h->n_pods)
    return fail(h, YODA_ERR_STATE, "yoda_set_pod_classes: the class array's length is not n_pods");
  if (h->cls_top >= (int)h->cand_classes)
    return fail(h, YODA_ERR_STATE, "yoda_set_pod_classes: a class is not below n_classes");
  return YODA_OK;
}

// A batch run with sampling on: the start array is empty or fits the uploaded batch.
int samp_ready(yoda_t* h) {
  if (h->samp_m && !h->h_start.empty() && h->h_start.size() != h->n_pods)
    return fail(h, YODA_ERR_STATE, "yoda_set_node_sampling: the start array's length is not n_pods");
  return YODA_OK;
}

int check_ready(yoda_t* h, int mode, bool batch = false) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (mode != YODA_MODE_SCV && mode != YODA_MODE_DISKIO)
    return fail(h, YODA_ERR_INVALID_ARG, "mode must be YODA_MODE_SCV or YODA_MODE_DISKIO");
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (!h->has_pods) return fail(h, YODA_ERR_NO_PODS, "no pods uploaded");
  if (mode == YODA_MODE_DISKIO && !(h->nodes_diskio && h->pods_diskio))
    return fail(h, YODA_ERR_INVALID_ARG, "Mode B needs node cpu/disk_io and pod rio/rcpu");
  if (int rc = mode_b_absent(h, mode, batch)) return rc;
  if (int rc = cand_ready(h)) return rc;
  if (int rc = samp_ready(h)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  return h->fast_run ? YODA_OK : pods_complete(h);
}

// Batches above this size are sorted (below it a batch fills at most one wave).
constexpr uint32_t kOrderMinPods = 2 * kWave;
// Groups x memory buckets of the counting-sort order (its LDS histogram: 64 KiB); a batch
// with more (clock, number, has-memory) groups takes the radix sort without padding.
constexpr uint32_t kOrderMaxGroups = 16384;

// Sort the batch by its Filter inputs and gather the pod arrays (yoda_order.hip).  Runs on
// the device inside every run, so its cost is part of the measured step.  The counting
// sort (groups built at upload) fills h->n_work sorted positions: n_pad when the run pads
// its groups to whole waves (prepare_run), else n_pods; the radix sort is the fallback for
// batches with too many groups.
// shared: the exchange buffers are in the shards' common radix order (the capacity windows'
// witness phase 1), so a shard without nodes sorts too: it downloads the reduced buffers of
// the others through its own permutation.  Otherwise an empty snapshot runs nothing to order.
int order_pods(yoda_t* h, int mode, bool shared = false) {
  const uint32_t P = h->n_pods, W = h->n_work;
  h->ordered = false;
  h->blk_zeroed = false;
  h->maxima_sorted = false;
  if (!h->order_enabled || mode != YODA_MODE_SCV || P < kOrderMinPods ||
      (h->n_nodes == 0 && !shared))
    return YODA_OK;
  const unsigned char* b = h->pod_blob.as<unsigned char>();
  HIP_TRY(h, h->perm.ensure((size_t)W * 4));
  size_t total = 0;
  for (int a = 0; a < kPodArrays; ++a) {
    h->sorted_off[a] = total;
    total += ((size_t)W * kPodArrayBytes[a] + 255) / 256 * 256;
  }
  HIP_TRY(h, h->pod_sorted.ensure(total));
  PermTable t{};
  for (int a = 0; a < kPodArrays; ++a) {
    t.src[t.n] = b + h->pod_off[a];
    t.dst[t.n] = h->pod_sorted.as<unsigned char>() + h->sorted_off[a];
    t.bytes[t.n] = (uint32_t)kPodArrayBytes[a];
    ++t.n;
  }
  // The counting sort's order inside a bucket follows its atomics (not reproducible from
  // one run to the next): only the padded single-handle run uses it.  Every other entry
  // point takes the radix sort, whose order is a function of the batch alone -- shards of
  // one batch on several GPUs must agree on it.
  if (h->count_order) {
    const bool padded = W != P;
    // the block kernels (N32 with both summaries) read 5 of the pod arrays; the rest of the
    // sorted blob is left unwritten and unread
    if (h->path == Path::N32 && h->has_k1sum && h->has_k2sum) {
      const int fast[] = {kPodM32, kPodC32, kPodNumber, kPodNeedMem, kPodNeedClk};
      t.n = 0;
      for (int a : fast) {
        t.src[t.n] = b + h->pod_off[a];
        t.dst[t.n] = h->pod_sorted.as<unsigned char>() + h->sorted_off[a];
        t.bytes[t.n] = (uint32_t)kPodArrayBytes[a];
        ++t.n;
      }
    }
    // the K1 block list is cleared here rather than by a memset in phase 1
    const uint32_t n_zero = h->has_k1sum ? (uint32_t)blk_words(h, W) : 0u;
    h->blk_zeroed = n_zero != 0;
    HIP_TRY(h, h->order_slot.ensure((size_t)P * 4));
    HIP_TRY(h, h->order_bkt.ensure((size_t)P * 4));
    const unsigned char* meta = h->order_meta.as<unsigned char>();
    OrderMeta o;
    o.groups = reinterpret_cast<const uint64_t*>(meta);
    o.gstart = reinterpret_cast<const uint32_t*>(meta + (padded ? h->og_off_start_pad
                                                                : h->og_off_start));
    o.n_groups = h->og_groups;
    o.nb_log2 = h->og_nb_log2;
    o.m_shift = h->og_m_shift;
    if (h->mem_ranks) {  // bucket the rank thresholds (< nf + 3) instead of the values
      uint32_t bits = 0;
      while (bits < 32 && ((uint64_t)(h->mt.nf + 2) >> bits)) ++bits;
      o.m_shift = bits > h->og_nb_log2 ? bits - h->og_nb_log2 : 0;
      o.m32 = reinterpret_cast<const uint32_t*>(b + h->pod_off[kPodM32]);
    }
    HIP_TRY(h, launch_order_count(o, reinterpret_cast<const uint64_t*>(b + h->pod_off[kPodNumber]),
                                  reinterpret_cast<const uint32_t*>(b + h->pod_off[kPodM32]),
                                  reinterpret_cast<const uint32_t*>(b + h->pod_off[kPodC32]),
                                  reinterpret_cast<const uint32_t*>(b + h->pod_off[kPodNeedMem]),
                                  P, h->order_hist.as<uint32_t>(), h->order_bstart.as<uint32_t>(),
                                  h->order_slot.as<uint32_t>(), h->order_bkt.as<uint32_t>(), t,
                                  reinterpret_cast<const uint32_t*>(meta + h->og_off_pad),
                                  padded ? h->og_n_pad_slots : 0u, h->blk.as<uint64_t>(), n_zero,
                                  h->perm.as<uint32_t>(), h->stream));
    h->ordered = true;
    return YODA_OK;
  }
  if (W != P) return fail(h, YODA_ERR_STATE, "padded order without its groups");
  uint32_t kb[3] = {h->key_bits[0], h->key_bits[1], h->key_bits[2]};
  if (h->mem_ranks) {  // the rank thresholds' width (< nf + 3)
    kb[2] = 0;
    while (kb[2] < 32 && ((uint64_t)(h->mt.nf + 2) >> kb[2])) ++kb[2];
  }
  const size_t scratch = order_scratch_bytes(P);
  HIP_TRY(h, h->order_scratch.ensure(scratch));
  HIP_TRY(h, launch_order_pods(reinterpret_cast<const uint64_t*>(b + h->pod_off[kPodNumber]),
                               reinterpret_cast<const uint64_t*>(b + h->pod_off[kPodMU]),
                               reinterpret_cast<const uint64_t*>(b + h->pod_off[kPodCU]),
                               reinterpret_cast<const uint32_t*>(b + h->pod_off[kPodNeedMem]), P,
                               kb,
                               h->og_ok ? reinterpret_cast<const uint64_t*>(
                                              h->order_meta.as<unsigned char>())
                                        : nullptr,
                               h->og_ok ? h->og_groups : 0u, h->order_scratch.p,
                               h->order_scratch.bytes, h->perm.as<uint32_t>(),
                               h->mem_ranks ? reinterpret_cast<const uint32_t*>(
                                                  b + h->pod_off[kPodM32])
                                            : nullptr,
                               h->stream));
  HIP_TRY(h, launch_permute(t, h->perm.as<uint32_t>(), P, false, h->stream));
  h->ordered = true;
  return YODA_OK;
}

// Scatter the per-pod outputs of an ordered run back to the caller's pod order.
int unpermute_outputs(yoda_t* h) {
  const uint32_t P = h->n_pods, W = h->n_work;  // W sorted positions (copies: same values)
  if (!h->ordered || P == 0) return YODA_OK;
  // Scatter every row into a second buffer of the same shape, then swap the two: no copy
  // back (the swapped-out buffers become the next scatter's targets).
  struct Arr {
    DevBuf* buf;
    DevBuf* alt;
    uint32_t rows;
    uint32_t bytes;
  };
  const Arr arrs[] = {{&h->pick, &h->pick_alt, 1, 4},         {&h->status, &h->status_alt, 1, 4},
                      {&h->ties_out, &h->ties_out_alt, 1, 4}, {&h->counts, &h->counts_alt, 2, 4},
                      {&h->best, &h->best_alt, 1, 8},         {&h->maxima, &h->maxima_alt, 6, 8}};
  PermTable t{};
  for (const Arr& a : arrs) {
    // sized like the buffer it is swapped with (no reallocation from one run to the next)
    HIP_TRY(h, a.alt->ensure(std::max(a.buf->bytes, (size_t)a.rows * W * a.bytes)));
    for (uint32_t r = 0; r < a.rows; ++r) {
      t.src[t.n] = a.buf->as<unsigned char>() + (size_t)r * W * a.bytes;
      t.dst[t.n] = a.alt->as<unsigned char>() + (size_t)r * P * a.bytes;
      t.bytes[t.n] = a.bytes;
      ++t.n;
    }
  }
  HIP_TRY(h, launch_permute(t, h->perm.as<uint32_t>(), W, true, h->stream));
  for (const Arr& a : arrs) a.buf->swap(*a.alt);
  return YODA_OK;
}

// Caller-order exchange (yoda_t::xo): rows of a run's sorted-order arrays (n_work positions)
// to the caller's pod order (n_pods) or back.  A sorted position that pads a group is a copy
// of its pod (the same values), so the scatter writes some caller slots twice, identically.
// A run left unordered is already in caller order: plain copies.
struct XArr {
  void* sorted;  // [rows][n_work]
  void* caller;  // [rows][n_pods]
  uint32_t rows, bytes;
};
int xfer(yoda_t* h, bool to_caller, std::initializer_list<XArr> arrs) {
  const uint32_t P = h->n_pods, W = h->n_work;
  if (P == 0) return YODA_OK;
  PermTable t{};
  for (const XArr& a : arrs)
    for (uint32_t r = 0; r < a.rows; ++r) {
      unsigned char* sp = static_cast<unsigned char*>(a.sorted) + (size_t)r * W * a.bytes;
      unsigned char* cp = static_cast<unsigned char*>(a.caller) + (size_t)r * P * a.bytes;
      if (!h->ordered) {
        if (sp != cp)
          HIP_TRY(h, hipMemcpyAsync(to_caller ? cp : sp, to_caller ? sp : cp, (size_t)P * a.bytes,
                                    hipMemcpyDeviceToDevice, h->stream));
        continue;
      }
      if (t.n == kPermArrays) {
        HIP_TRY(h, launch_permute(t, h->perm.as<uint32_t>(), W, to_caller, h->stream));
        t = PermTable{};
      }
      t.src[t.n] = to_caller ? sp : cp;
      t.dst[t.n] = to_caller ? cp : sp;
      t.bytes[t.n] = a.bytes;
      ++t.n;
    }
  if (t.n) HIP_TRY(h, launch_permute(t, h->perm.as<uint32_t>(), W, to_caller, h->stream));
  return YODA_OK;
}

int xo_ensure(yoda_t* h) {
  if (!h->xo) return YODA_OK;
  const size_t P = std::max<uint32_t>(h->n_pods, 1);
  HIP_TRY(h, h->xcnt.ensure(2 * P * 4));
  HIP_TRY(h, h->xbest.ensure(P * 8));
  HIP_TRY(h, h->xidx.ensure(P * 4));
  HIP_TRY(h, h->xties.ensure(P * 4));
  HIP_TRY(h, h->xlow.ensure(P * 8));
  return YODA_OK;
}

// Mode B score levels (yoda_layout.h DiskLevels): t[k] = the largest |d| >= 0 whose score
// (yoda_modeb.h disk_score, the kernels' own: algorithm.go:110-111, never FMA-contracted) is
// >= k, by bisection over the bit patterns of the non-negative doubles (ordered like their
// values); the score is non-increasing in |d|, so the set is [0, t[k]].
static const DiskLevels& diskio_levels() {
  static const DiskLevels lv = [] {
    DiskLevels d{};
    d.t[0] = HUGE_VAL;
    d.t[11] = -1.0;
    for (int k = 1; k <= 10; ++k) {
      uint64_t lo = 0, hi = 0x7ff0000000000000ull;  // score(+0) = 10 >= k, score(inf) = 0 < k
      while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        double x;
        std::memcpy(&x, &mid, 8);
        if (disk_score(x) >= (double)k) lo = mid; else hi = mid;
      }
      std::memcpy(&d.t[k], &lo, 8);
    }
    return d;
  }();
  return lv;
}

// Mode B runs with eligibility (yoda_mode_b_follow on) when E(p) is not every node for some pod:
// a node is absent, or candidates are on and some pod names a class.  Otherwise the unrestricted
// kernels run, exactly as without the setting.
bool modeb_keyed(const yoda_t* h) {
  return h->b_follow && h->cand_classes && !h->h_cls.empty() && h->cls_top >= 0;
}
bool modeb_elig_on(const yoda_t* h) { return h->b_follow && (h->n_absent > 0 || modeb_keyed(h)); }
// The pods' class bytes on the device for the eligibility kernels (nullptr: every pod ANY).
const uint8_t* modeb_cls_bytes(const yoda_t* h) {
  return modeb_keyed(h) ? h->cand_cls.as<uint8_t>() + h->cls_off : nullptr;
}

// What the Mode B launches take for eligibility: empty (the unrestricted kernels) unless it is
// on; else the table and counts (ensure_modeb_elig), the pods' class bytes and the pod classes'
// selectors behind (alpha, beta) in b_cab (ensure_diskio_classes: the batch kernels read them).
static DiskEligArgs modeb_elig_args(const yoda_t* h) {
  if (!modeb_elig_on(h)) return DiskEligArgs{};
  const double* cab = h->b_cab.as<double>();
  return DiskEligArgs{h->b_elig.as<DiskElig>(),
                      cab ? reinterpret_cast<const uint32_t*>(cab + 2 * (size_t)h->b_ncls) : nullptr,
                      modeb_cls_bytes(h), h->b_ecnt.as<uint32_t>()};
}

// The batch's Mode B pod classes, from the staged (alpha, beta) of the last upload: pods with
// bit-identical (alpha, beta) score every node alike (algorithm.go:105-111); with eligibility
// the pod's candidate class is part of the key (yoda_modeb.h disk_build_classes).  The device
// copy: [2][D] f64 (alpha, beta), then the [D] u32 selectors.
int ensure_diskio_classes(yoda_t* h) {
  const bool keyed = modeb_keyed(h);
  if (h->b_cls_ready && h->b_cls_keyed == keyed) return YODA_OK;
  pods_pack_rest(h);
  const uint32_t P = h->n_pods;
  const unsigned char* st = static_cast<const unsigned char*>(h->pod_stage.p);
  const uint64_t* al = reinterpret_cast<const uint64_t*>(st + h->pod_off[kPodAlpha]);
  const uint64_t* be = reinterpret_cast<const uint64_t*>(st + h->pod_off[kPodBeta]);
  DiskClasses dc;
  disk_build_classes(al, be, keyed ? h->h_cls.data() : nullptr, P, dc);
  const uint32_t D = (uint32_t)dc.alpha.size();
  std::vector<uint64_t> cab(2 * (size_t)D + ((size_t)D + 1) / 2, 0);
  std::copy(dc.alpha.begin(), dc.alpha.end(), cab.begin());
  std::copy(dc.beta.begin(), dc.beta.end(), cab.begin() + D);
  if (D) std::memcpy(cab.data() + 2 * (size_t)D, dc.sel.data(), (size_t)D * 4);
  HIP_TRY(h, h->b_cab.ensure(std::max<size_t>(cab.size(), 1) * 8));
  HIP_TRY(h, h->b_cls.ensure(std::max<size_t>(P, 1) * 4));
  HIP_TRY(h, hipMemcpyAsync(h->b_cab.p, cab.data(), cab.size() * 8, hipMemcpyHostToDevice,
                            h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->b_cls.p, dc.cls.data(), (size_t)P * 4, hipMemcpyHostToDevice,
                            h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // the host vectors go out of scope
  h->b_ncls = D;
  h->b_cls_ready = true;
  h->b_cls_keyed = keyed;
  return YODA_OK;
}

// The eligibility table and its counts, rebuilt when the node set or the candidate words changed
// since the last build (b_elig_dirty), on the handle's stream ahead of the run's kernels.
int ensure_modeb_elig(yoda_t* h) {
  if (!h->b_elig_dirty) return YODA_OK;
  const uint32_t N = h->n_nodes;
  const size_t words = std::max<size_t>(((size_t)N + 63) / 64, 1);
  std::vector<uint64_t> pres(words, 0);
  for (uint32_t n = 0; n < N; ++n)
    if (n >= h->h_absent.size() || !h->h_absent[n]) pres[n >> 6] |= 1ull << (n & 63u);
  HIP_TRY(h, h->b_pres.ensure(words * 8));
  HIP_TRY(h, h->b_elig.ensure(std::max<size_t>(N, 1) * sizeof(DiskElig)));
  HIP_TRY(h, h->b_ecnt.ensure(kDiskSelCount * 4));
  HIP_TRY(h, hipMemcpyAsync(h->b_pres.p, pres.data(), words * 8, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, launch_modeb_elig_build(h->cand_classes ? h->cand_w.as<uint64_t>() : nullptr,
                                     h->b_pres.as<uint64_t>(), N, h->b_elig.as<DiskElig>(),
                                     h->b_ecnt.as<uint32_t>(), h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the copy's source is pageable)
  h->b_elig_dirty = false;
  ++h->b_elig_builds;
  return YODA_OK;
}

// A Mode B batch run under node sampling (yoda_mode_b_sampling on) takes the sampled kernels.
bool modeb_sampled(const yoda_t* h) { return h->b_samp && h->samp_m != 0; }

// The rank tables of the sampled walk, rebuilt with the eligibility table (whose build they
// follow on the handle's stream); only a sampled run with eligibility asks for them.
int ensure_modeb_rank(yoda_t* h) {
  if (int rc = ensure_modeb_elig(h)) return rc;
  if (h->b_rank_for == h->b_elig_builds) return YODA_OK;
  const size_t nb = std::max<size_t>(((size_t)h->n_nodes + 63) / 64, 1);
  HIP_TRY(h, h->b_rbits.ensure(kDiskSelCount * nb * 8));
  HIP_TRY(h, h->b_rpfx.ensure(kDiskSelCount * nb * 4));
  HIP_TRY(h, launch_modeb_rank_build(h->b_elig.as<DiskElig>(), h->n_nodes,
                                     h->b_rbits.as<uint64_t>(), h->b_rpfx.as<uint32_t>(),
                                     h->stream));
  h->b_rank_for = h->b_elig_builds;
  ++h->b_rank_builds;
  return YODA_OK;
}

// What a sampled Mode B run hands its kernels (after ensure_modeb_rank when eligibility is on).
static DiskSampArgs modeb_samp_args(yoda_t* h) {
  DiskSampArgs a{};
  if (modeb_elig_on(h)) {
    a.rank = DiskRank{h->b_rbits.as<uint64_t>(), h->b_rpfx.as<uint32_t>(),
                      std::max<uint32_t>((h->n_nodes + 63u) / 64u, 1u)};
    a.cls = modeb_cls_bytes(h);
    a.cnt = h->b_ecnt.as<uint32_t>();
  }
  a.start = h->h_start.empty() ? nullptr : h->samp_start.as<uint32_t>();
  a.m = h->samp_m;
  a.n_nodes = h->n_nodes;
  a.n_pods = h->n_pods;
  a.node_offset = h->node_offset;
  a.n_found = h->samp_out.as<uint32_t>();
  a.next_start = a.n_found + h->n_pods;
  a.walk = h->b_walk.as<DiskWalk>();
  return a;
}

// The free levels t_0 = 0 < ... < t_{L-1} = 0xFFFFFFFF of the kbub lv[] bounds (yoda_layout.h):
// the quantiles of the snapshot's real card frees (K2 summary words: values, or memory ranks),
// so that a wave's scv/memory range falls between close levels wherever the cards are.
hipError_t build_kb_levels(yoda_t* h) {
  const uint32_t N = h->n_nodes, K = (uint32_t)h->K, S2 = k2sum_stride(h->K);
  std::vector<uint32_t> f;
  f.reserve((size_t)N * K);
  for (uint32_t n = 0; n < N; ++n) {
    const uint32_t cnt = std::min<uint32_t>((h->host_k2sum[sum_index(n, kS2Meta, S2)] >> 8) & 0xffu, K);
    for (uint32_t t = 0; t < cnt; ++t) f.push_back(h->host_k2sum[sum_index(n, kS2Fs + t, S2)]);
  }
  std::vector<uint32_t> lv(kKbLevels, 0u);
  lv[kKbLevels - 1] = 0xffffffffu;
  if (!f.empty()) {
    for (uint32_t l = 1; l + 1 < kKbLevels; ++l) {  // interior levels: quantiles l / (L - 1)
      const size_t at = (size_t)((double)l / (kKbLevels - 1) * (double)(f.size() - 1));
      std::nth_element(f.begin(), f.begin() + at, f.end());
      lv[l] = f[at];
    }
    std::sort(lv.begin() + 1, lv.end() - 1);
    for (uint32_t l = 1; l + 1 < kKbLevels; ++l)  // strictly increasing above t_0 = 0
      lv[l] = std::max(lv[l], lv[l - 1] + 1u);
  }
  hipError_t e = h->kb_levels.ensure(kKbLevels * 4);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->kb_levels.p, lv.data(), kKbLevels * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (lv goes out of scope)
  if (e == hipSuccess) h->kb_levels_ok = true;
  return e;
}

// The K2 block bounds of both orders from the current K2 summaries and G tables.
hipError_t build_block_ub(yoda_t* h) {
  hipError_t e = hipSuccess;
  if (!(h->path == Path::N32 && h->has_k2sum && h->gtab.p)) return e;
  if (!h->kb_levels_ok && (e = build_kb_levels(h)) != hipSuccess) return e;
  const size_t bytes = sum_words(std::max<uint32_t>((h->n_nodes + 63) / 64, 1),
                                 kbub_stride(h->K)) * 4;  // tiles of 64 blocks
  const size_t dbytes = sum_words(std::max<uint32_t>((h->n_nodes + 63) / 64, 1),
                                  kbdec_stride()) * 4;
  const MemTab mt = h->mem_ranks ? h->mt : MemTab{};
  e = h->kbub.ensure(bytes);
  if (e == hipSuccess) e = h->kbdec.ensure(dbytes);
  if (e == hipSuccess)
    e = launch_block_ub(h->K, h->k2sum.as<uint32_t>(), h->gtab.as<uint32_t>(), h->n_nodes,
                        h->kbub.as<uint32_t>(), h->kb_levels.as<uint32_t>(), h->stream);
  if (e == hipSuccess)
    e = launch_block_dec(h->K, h->k2sum.as<uint32_t>(), h->kmix.as<uint32_t>(), h->n_nodes,
                         h->kbdec.as<uint32_t>(),
                         h->kb_levels.as<uint32_t>(), mt, h->stream);
  if (e == hipSuccess && h->perm_on) {
    e = h->kbub_p.ensure(bytes);
    if (e == hipSuccess) e = h->kbdec_p.ensure(dbytes);
    if (e == hipSuccess)
      e = launch_block_ub(h->K, h->k2sum_p.as<uint32_t>(), h->gtab_p.as<uint32_t>(), h->n_nodes,
                          h->kbub_p.as<uint32_t>(), h->kb_levels.as<uint32_t>(), h->stream);
    if (e == hipSuccess)
      e = launch_block_dec(h->K, h->k2sum_p.as<uint32_t>(), h->kmix_p.as<uint32_t>(), h->n_nodes,
                           h->kbdec_p.as<uint32_t>(),
                           h->kb_levels.as<uint32_t>(), mt, h->stream);
  }
  if (e == hipSuccess) {
    h->kbub_dirty = h->kbub_loose = false;
    // the static scores the bounds hold (the host copy of the K2 summaries' static words)
    const uint32_t N = h->n_nodes, S2 = k2sum_stride(h->K);
    h->ub_stat.resize(N);
    for (uint32_t n = 0; n < N; ++n) {
      const uint64_t b = (uint64_t)h->host_k2sum[sum_index(n, kS2Static, S2)] |
                         ((uint64_t)h->host_k2sum[sum_index(n, kS2Static + 1, S2)] << 32);
      double d;
      std::memcpy(&d, &b, 8);
      h->ub_stat[n] = (uint64_t)d;
    }
  }
  return e;
}

// Inside a greedy batch: its node-state pushes leave the block summaries' bounds valid (the
// atomics of k_set_static), so its windows do not tighten them; the next private run does.
struct GreedyScope {
  yoda_t* h;
  bool prev;
  explicit GreedyScope(yoda_t* x) : h(x), prev(x->greedy_active) { h->greedy_active = true; }
  ~GreedyScope() { h->greedy_active = prev; }
};

// The block summaries' CardNumber bounds, tight again after node-state pushes.
hipError_t tighten_block_sums(yoda_t* h) {
  hipError_t e = hipSuccess;
  const uint32_t bsw = bsum_stride(h->K) / 4u;
  if (h->path == Path::N32 && h->has_k1sum && h->blksum.p)
    e = launch_bsum_cn(h->k1sum.as<unsigned char>(), k1sum_stride(h->K), h->n_nodes,
                       h->blksum.as<uint32_t>(), bsw, h->stream);
  if (e == hipSuccess && h->perm_on && h->blksum_p.p)
    e = launch_bsum_cn(h->k1sum_p.as<unsigned char>(), k1sum_stride(h->K), h->n_nodes,
                       h->blksum_p.as<uint32_t>(), bsw, h->stream);
  if (e == hipSuccess) h->blksum_loose = false;
  return e;
}

// Whose PreScore maxima a phase 1 produces.  (The K2 pruning seeds are scores under this
// handle's G table, lower bounds only for pods whose maxima are at most G's: exchanged maxima
// can exceed a shard's G, so the argmax K2 checks each wave's reciprocals against G's before
// it takes a seed -- tests/test_gpu_shard_seeds.py.)
enum class Maxima {
  Exchanged,  // a node shard: the maxima are reduced across shards after this phase
  Own,        // this handle's maxima are the run's (score rows, greedy windows)
  OwnFinal,   // ... and the reduce writes the reciprocals too (yoda_run)
};

// The narrowing pass after a phase 1's reduce (candidates on): the masks this run's K1 wrote
// (h->bm_sparse: which form) and counts [2][P] from Yoda's Filter to every plugin's.  The maxima
// stay K1's, over F.  pr: the run reads the block-grouped node tables.
int cand_narrow(yoda_t* h, uint32_t* counts, uint32_t P, bool pr) {
  CandArgs a{};
  a.words = (pr ? h->cand_w_p : h->cand_w).as<uint64_t>();
  a.band = (pr ? h->cand_and_p : h->cand_and).as<uint64_t>();
  a.cls = h->h_cls.empty() ? nullptr : h->cand_cls.as<uint8_t>() + h->cls_off;
  a.perm = h->ordered ? h->perm.as<uint32_t>() : nullptr;
  a.zt = (pr ? h->cand_zt_p : h->cand_zt).as<uint64_t>();
  a.n_nodes = h->n_nodes;
  a.n_work = P;
  a.bm = h->bitmask.as<uint64_t>();
  a.bs = h->bm_sparse ? h->bsum.as<BlockMask>() : nullptr;
  a.blk = h->bm_sparse ? h->blk.as<uint64_t>() : nullptr;
  a.bm_stride = bm_row(h->n_nodes);
  a.bs_stride = bs_row(h->n_nodes);
  a.blk_stride = blk_row(h->n_nodes);
  a.counts = counts;
  hipEvent_t c0 = h->profiling ? h->next_event() : nullptr;
  hipEvent_t c1 = h->profiling ? h->next_event() : nullptr;
  if (c0) HIP_TRY(h, hipEventRecord(c0, h->stream));
  HIP_TRY(h, launch_cand_narrow(a, h->stream));
  if (c1) {
    HIP_TRY(h, hipEventRecord(c1, h->stream));
    h->ev_cand.emplace_back(c0, c1);
  }
  return YODA_OK;
}

// The sampling pass after a phase 1's reduce and narrowing (sampling on): the masks and counts
// [2][P] from F' to each pod's sample S, n_found and next_start into samp_out.  The run read the
// upload-order tables (perm_run() is false), so a mask position is a local node id.
int samp_pass(yoda_t* h, uint32_t* counts, uint32_t P) {
  const uint32_t N = h->n_nodes;
  SampArgs a{};
  a.start = h->h_start.empty() ? nullptr : h->samp_start.as<uint32_t>();
  a.perm = h->ordered ? h->perm.as<uint32_t>() : nullptr;
  a.num_to_find = h->samp_m;
  a.node_offset = h->node_offset;
  a.n_nodes = N;
  a.n_work = P;
  a.bm = h->bitmask.as<uint64_t>();
  a.bs = h->bm_sparse ? h->bsum.as<BlockMask>() : nullptr;
  a.blk = h->bm_sparse ? h->blk.as<uint64_t>() : nullptr;
  a.bm_stride = bm_row(N);
  a.bs_stride = bs_row(N);
  a.blk_stride = blk_row(N);
  a.counts = counts;
  HIP_TRY(h, h->samp_scr.ensure(samp_scratch_words(P, N) * 4));
  HIP_TRY(h, h->samp_zt.ensure(std::max<size_t>((N + 63u) / 64u, 1) * 8));
  HIP_TRY(h, h->samp_out.ensure(2 * (size_t)std::max<uint32_t>(h->n_pods, 1) * 4));
  samp_scratch(a, h->samp_scr.as<uint32_t>());
  a.zt = h->samp_zt.as<uint64_t>();
  a.n_found = h->samp_out.as<uint32_t>();
  a.next_start = a.n_found + h->n_pods;
  hipEvent_t c0 = h->profiling ? h->next_event() : nullptr;
  hipEvent_t c1 = h->profiling ? h->next_event() : nullptr;
  if (c0) HIP_TRY(h, hipEventRecord(c0, h->stream));
  // (the zero_total bits follow yoda_replace_nodes: read from the records by every sampled run)
  HIP_TRY(h, launch_samp_zt(h->nodes.as<unsigned char>(),
                            h->path == Path::N32 ? n32_stride(h->K) : node_stride(h->K), N,
                            h->samp_zt.as<uint64_t>(), h->stream));
  HIP_TRY(h, launch_samp_pass(a, h->stream));
  if (c1) {
    HIP_TRY(h, hipEventRecord(c1, h->stream));
    h->ev_samp.emplace_back(c0, c1);
  }
  h->samp_ran = true;
  return YODA_OK;
}

// Phase 1: Filter + PreScore maxima (Mode A), or the all-feasible state (Mode B).
int phase1(yoda_t* h, int mode, uint64_t* maxima, uint32_t* counts,
           Maxima whose = Maxima::Exchanged) {
  const bool final_maxima = whose == Maxima::OwnFinal;
  h->seeds_valid = false;  // (set again below when this run's block K1 writes them)
  h->rcp_ready = false;
  h->samp_ran = false;
  h->b_walk_ok = false;
  const uint32_t P = h->n_work;  // sorted positions of this run
  if (P == 0) return YODA_OK;
  if (mode == YODA_MODE_DISKIO && modeb_sampled(h)) {
    // the plan: n_feasible = |S(p)|, n_found, next_start and each pod's walk record
    if (modeb_elig_on(h))
      if (int rc = ensure_modeb_rank(h)) return rc;
    HIP_TRY(h, h->samp_out.ensure(2 * (size_t)P * 4));
    HIP_TRY(h, h->b_walk.ensure((size_t)P * sizeof(DiskWalk)));
    hipEvent_t c0 = h->profiling ? h->next_event() : nullptr;
    hipEvent_t c1 = h->profiling ? h->next_event() : nullptr;
    if (c0) HIP_TRY(h, hipEventRecord(c0, h->stream));
    HIP_TRY(h, launch_k2b_samp_plan(modeb_samp_args(h), maxima, counts, h->stream));
    if (c1) {  // (Mode B has no K1: the plan reports in its place, yoda_profile_read)
      HIP_TRY(h, hipEventRecord(c1, h->stream));
      h->ev_k1.emplace_back(c0, c1);
    }
    h->b_walk_ok = true;
    h->samp_ran = true;
    return YODA_OK;
  }
  if (mode == YODA_MODE_DISKIO) {
    if (modeb_elig_on(h))
      if (int rc = ensure_modeb_elig(h)) return rc;
    // n_feasible = every node, or with eligibility |E|: the count of the pod's class, or of the
    // present nodes
    HIP_TRY(h, launch_fill_diskio_state(P, h->n_nodes, maxima, counts, modeb_elig_args(h),
                                        h->stream));
    return YODA_OK;
  }
  if (h->n_nodes == 0) {
    HIP_TRY(h, hipMemsetAsync(counts, 0, 2 * (size_t)P * 4, h->stream));
    std::vector<uint64_t> ones(6 * (size_t)P, 1);
    HIP_TRY(h, hipMemcpyAsync(maxima, ones.data(), ones.size() * 8, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return h->samp_m ? samp_pass(h, counts, P) : YODA_OK;
  }
  Partials part = partials(h);
  hipEvent_t e0 = h->profiling ? h->next_event() : nullptr;
  hipEvent_t e1 = h->profiling ? h->next_event() : nullptr;
  h->blk_valid = h->has_k1sum;
  h->bm_sparse = h->has_k1sum;  // the block K1 writes the sparse form
  // (candidates on: no seed -- it is a best over every node of an ALL block, and may sit above
  // the best of a pod's candidates)
  // (sampling on: likewise -- the best of an ALL block may sit above the best of a pod's sample)
  h->seeds_valid = h->has_k1sum && mode == YODA_MODE_SCV && !h->cand_classes && !h->samp_m;
  h->blk_fresh = h->has_k1sum;  // (the memset below or the order scatter clears it whole)
  if (h->blk_valid && !h->blk_zeroed)  // (the list and the seeds after it)
    HIP_TRY(h, hipMemsetAsync(h->blk.p, 0, blk_words(h, P) * 8, h->stream));
  h->blk_zeroed = false;
  const bool pr = h->perm_run();  // block-grouped node order (upload's node_perm)
  // current block bounds for the K1's seeds (loose ones -- static scores fell since the build --
  // are upper bounds only): a private run (yoda_run) rebuilds them here rather than in phase 2;
  // the other entry points (shards, greedy windows) keep phase 2's rule
  if (mode == YODA_MODE_SCV && h->count_order && !h->greedy_active &&
      (h->kbub_dirty || h->kbub_loose) && h->path == Path::N32 && h->has_k2sum && h->g.tab)
    HIP_TRY(h, build_block_ub(h));
  if (h->blksum_loose && !h->greedy_active) HIP_TRY(h, tighten_block_sums(h));
  // the block K1 visits its pod blocks heaviest first too (k1_probe: the per-node work its
  // whole-block decisions leave each wave on a sample of blocks)
  h->k1_sorted = h->k1_rec_ok = false;
  if (h->lpt_active && mode == YODA_MODE_SCV) {
    const PodParams pp0 = pod_params(h);
    if (pp0.bsum != nullptr) {
      const uint32_t n_pb = (P + kBlock - 1) / kBlock;
      HIP_TRY(h, h->k1_w.ensure((size_t)((P + 63) / 64) * 4));
      HIP_TRY(h, h->k1_order.ensure((size_t)n_pb * 4));
      // (a private run -- yoda_run, the only caller with final maxima: the probe leaves each
      // wave's bounds for the block K1 of this run.  The row, shard and greedy entry points pass
      // no record, and their K1 computes its set-up per chunk task)
      const bool k1_rec_env = final_maxima;
      if (k1_rec_env) HIP_TRY(h, h->k1_rec.ensure((size_t)((P + 63) / 64) * sizeof(K1WaveRec)));
      HIP_TRY(h, launch_k1_order(h->K, pp0, P, h->n_nodes, h->k1_w.as<uint32_t>(),
                                 h->k1_order.as<uint32_t>(),
                                 k1_rec_env ? h->k1_rec.as<K1WaveRec>() : nullptr, h->stream));
      h->k1_sorted = true;
      h->k1_rec_ok = k1_rec_env;
    }
  }
  // (the K1 profile events bracket the K1 launch alone, as rocprofv3's kernel trace does)
  if (e0) HIP_TRY(h, hipEventRecord(e0, h->stream));
  HIP_TRY(h, launch_k1(h->K, h->path, h->nodes.as<unsigned char>(),
                       h->has_k1sum ? (pr ? h->k1sum_p : h->k1sum).as<unsigned char>() : nullptr,
                       (pr ? h->k2sum_p : h->k2sum).as<unsigned char>(),
                       (pr ? h->kmix_p : h->kmix).as<unsigned char>(), h->n_nodes,
                       h->chunk1, h->C1, pod_params(h), P, part, h->bitmask.as<uint64_t>(),
                       bm_row(h->n_nodes), h->bsum.as<BlockMask>(), bs_row(h->n_nodes),
                       h->blk.as<uint64_t>(), blk_row(h->n_nodes), h->stats_ptr(), h->stream));
  if (h->class_stats && h->has_k1sum) h->stats_pairs1 += (uint64_t)(P + 63) / 64 * h->n_nodes;
  if (e1) {
    HIP_TRY(h, hipEventRecord(e1, h->stream));
    h->ev_k1.emplace_back(e0, e1);
  }
  // the block-classified K1 (N32) writes u32 maxima partials; a single-handle run's maxima
  // are final, so the reduce writes the reciprocals too (phase 2 then skips k_prep2)
  const bool rcp = final_maxima && !h->generic;
  HIP_TRY(h, launch_reduce1(part, h->C1, P, h->has_k1sum ? pod_params(h).nwords : 0u, maxima,
                            counts,
                            rcp ? h->rcp.as<double>() : nullptr, pod_params(h).mt, h->stream,
                            h->lpt_active ? h->lpt_w.as<uint32_t>() : nullptr,
                            h->lpt_active ? h->lpt_order.as<uint32_t>() : nullptr,
                            h->has_k1sum ? pod_params(h).cmask1 : nullptr));
  h->lpt_sorted = h->lpt_active;  // (the order of this run's pod blocks, for phase 2)
  h->rcp_ready = rcp;
  // the masks and counts from Yoda's Filter to every plugin's
  if (h->cand_classes)
    if (int rc = cand_narrow(h, counts, P, pr)) return rc;
  // ... and from F' to the sample of each pod's walk
  if (h->samp_m) return samp_pass(h, counts, P);
  return YODA_OK;
}

// Phase 1 of a capacity-decrement greedy window: Filter + PreScore maxima with their
// witnesses (k1_witness), dense masks.  Outputs maxima [6][P], counts [2][P] and
// wit [2][6][P] (witness count, lowest witness node + node_offset), in the run's pod order.
// With candidates on (yoda_greedy with yoda_greedy_candidates; the shard call refuses) the masks
// -- sparse from the block-witness kernel, dense from k1_witness -- and counts are then narrowed
// to F' through the upload-order tables, as phase 1's; maxima and wit stay over F, which is what
// the session's maxima certificate needs.
int phase1_witness(yoda_t* h, uint64_t* maxima, uint32_t* counts, uint32_t* wit,
                   uint32_t node_offset) {
  const uint32_t P = h->n_pods, N = h->n_nodes;
  if (P == 0) return YODA_OK;
  h->bm_sparse = false;
  h->blk_valid = false;
  h->seeds_valid = false;
  h->blk_fresh = false;
  if (N == 0) {
    HIP_TRY(h, hipMemsetAsync(counts, 0, 2 * (size_t)P * 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(wit, 0, 6 * (size_t)P * 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(wit + 6 * (size_t)P, 0xff, 6 * (size_t)P * 4, h->stream));
    std::vector<uint64_t> ones(6 * (size_t)P, 1);
    HIP_TRY(h, hipMemcpyAsync(maxima, ones.data(), ones.size() * 8, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return YODA_OK;
  }
  uint32_t C = h->C1;
  HIP_TRY(h, h->p_wit.ensure(12 * (size_t)C * P * 4));
  Partials part = partials(h);
  if (h->path == Path::N32 && h->has_k1sum && h->has_k2sum && h->all_one_model) {
    // block-classified, like phase 1's K1: sparse masks and the block list for the window's K2.
    // Its per-(wave, chunk) epilogue (18 wave reductions, 104 B of partials a pod) is the
    // cost that grows with the chunk count: chunks of >= YODA_WIT_CHUNK_NODES nodes
    static const uint32_t wit_chunk = std::max<uint32_t>(
        kChunkAlign, YODA_KNOB("YODA_WIT_CHUNK_NODES", 64) / kChunkAlign * kChunkAlign);
    uint32_t chunk = h->chunk1;
    if (chunk < wit_chunk) {
      chunk = wit_chunk;
      C = std::max<uint32_t>(1, (N + chunk - 1) / chunk);
      if (C >= 8) C = (C + 7) / 8 * 8;  // XCD tiling; trailing chunks may be empty
    }
    h->bm_sparse = true;
    h->blk_valid = true;
    h->blk_fresh = true;
    HIP_TRY(h, hipMemsetAsync(h->blk.p, 0, blk_words(h, P) * 8, h->stream));
    HIP_TRY(h, launch_k1_block_witness(h->K, h->nodes.as<unsigned char>(),
                                       h->k1sum.as<unsigned char>(), h->k2sum.as<unsigned char>(),
                                       h->kmix.as<unsigned char>(), N, chunk, C,
                                       pod_params(h), P, part.max_u, h->p_wit.as<uint32_t>(),
                                       part.cnt, h->bitmask.as<uint64_t>(), bm_row(N),
                                       h->bsum.as<BlockMask>(), bs_row(N), h->blk.as<uint64_t>(),
                                       blk_row(N), h->stream));
  } else {
    HIP_TRY(h, launch_k1_witness(h->K, h->path, h->nodes.as<unsigned char>(), N, h->chunk1, C,
                                 pod_params(h), P, part.max_u, h->p_wit.as<uint32_t>(), part.cnt,
                                 h->bitmask.as<uint64_t>(), bm_row(N), h->stream));
  }
  HIP_TRY(h, launch_reduce_wit(part.max_u, h->p_wit.as<uint32_t>(), part.cnt, C, P,
                               node_offset, maxima, counts, wit, wit + 6 * (size_t)P, pod_params(h).mt, h->stream));
  if (h->cand_classes) return cand_narrow(h, counts, P, false);
  return YODA_OK;
}

// Phase 2: Score over the feasible nodes with the (globally reduced) maxima.
// counts: the pods' feasible-node counts ([P] prefix of phase 1's [2][P], local or reduced;
// NULL: unknown): a pod with none takes no part in the block K2's wave bounds.
// draw: a private run with the selectHost draw on -- a sampled Mode B run draws inside its kernel.
int phase2(yoda_t* h, int mode, const uint64_t* maxima, const uint32_t* counts, int64_t* best,
           uint32_t* idx, uint32_t* ties, int64_t* low, int64_t* rows = nullptr,
           bool draw = false) {
  const uint32_t P = h->n_work;  // sorted positions of this run
  h->merge2.on = false;
  if (P == 0) return YODA_OK;
  const uint64_t* cmask2 = nullptr;
  if (h->n_nodes == 0) {
    std::vector<int64_t> neg(P, -1), big(P, INT64_MAX);
    std::vector<uint32_t> none(P, 0xffffffffu);
    HIP_TRY(h, hipMemcpyAsync(best, neg.data(), (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(low, big.data(), (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(idx, none.data(), (size_t)P * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(ties, 0, (size_t)P * 4, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return YODA_OK;
  }
  Partials part = partials(h);
  bool is_f64 = true;
  hipEvent_t e0 = h->profiling ? h->next_event() : nullptr;
  hipEvent_t e1 = h->profiling ? h->next_event() : nullptr;
  if (mode == YODA_MODE_SCV && !h->generic && !h->rcp_ready)
    HIP_TRY(h, launch_prep2(maxima, P, h->rcp.as<double>(),  h->stream));
  h->rcp_ready = false;
  // (under node sampling this run's phase 1 planned each pod's walk: yoda_mode_b_sampling)
  const bool sampled = mode == YODA_MODE_DISKIO && h->b_walk_ok && modeb_sampled(h);
  if (mode == YODA_MODE_DISKIO) {
    h->b_samp_last = sampled;
    h->b_samp_last_elig = sampled && modeb_elig_on(h);
  }
  if (mode == YODA_MODE_DISKIO && !rows) {
    // batch path: over the batch's pod classes, then each pod takes its class's outcome
    // (Mode B runs are never reordered: P == n_pods, caller order)
    if (sampled) {
      // under node sampling: one wave per pod over its walk, the outcome straight into the
      // pod's slot; with the draw on, the pick is drawn inside the same kernel
      if ((uint64_t)h->n_nodes >> kDiskCountBits)
        return fail(h, YODA_ERR_INVALID_ARG, "Mode B batch: more than 2^28 nodes");
      const DiskDrawArgs dr{h->tie_seed, h->tie_pod_base};
      if (e0) HIP_TRY(h, hipEventRecord(e0, h->stream));
      HIP_TRY(h, launch_k2b_sampled(h->nodes_b.as<NodeRecB>(), pod_params(h), diskio_levels(),
                                    modeb_samp_args(h), draw ? &dr : nullptr, best, idx,
                                    ties, low, h->stream));
      if (e1) {
        HIP_TRY(h, hipEventRecord(e1, h->stream));
        h->ev_k2.emplace_back(e0, e1);
      }
      return YODA_OK;
    }
    int rc = ensure_diskio_classes(h);
    if (rc) return rc;
    if ((uint64_t)h->n_nodes >> kDiskCountBits)
      return fail(h, YODA_ERR_INVALID_ARG, "Mode B batch: more than 2^28 nodes");
    const uint32_t D = h->b_ncls;
    const DiskPlan pl = diskio_plan(h->n_nodes, D);
    HIP_TRY(h, h->b_part.ensure(2 * (size_t)pl.C * D * 4));
    uint32_t* plc = h->b_part.as<uint32_t>();
    uint32_t* pix = plc + (size_t)pl.C * D;
    h->b_last_elig = modeb_elig_on(h);  // (its table: phase 1 of this run built it)
    h->b_last_ncls = D;
    if (e0) HIP_TRY(h, hipEventRecord(e0, h->stream));
    HIP_TRY(h, launch_k2b(h->nodes_b.as<NodeRecB>(), h->n_nodes, h->b_cab.as<double>(), D,
                          diskio_levels(), pl, plc, pix, modeb_elig_args(h), h->stream));
    if (e1) {
      HIP_TRY(h, hipEventRecord(e1, h->stream));
      h->ev_k2.emplace_back(e0, e1);
    }
    HIP_TRY(h, launch_reduce2b(plc, pix, pl.C, D, h->b_cls.as<uint32_t>(), P, h->node_offset,
                               best, idx, ties, low, h->stream));
    return YODA_OK;
  }
  if (mode == YODA_MODE_SCV && !rows && (h->kbub_dirty || (h->kbub_loose && !h->greedy_active)) &&
      h->path == Path::N32 && h->has_k2sum && h->g.tab)
    HIP_TRY(h, build_block_ub(h));
  if (e0) HIP_TRY(h, hipEventRecord(e0, h->stream));
  uint32_t C2 = h->C2;
  if (mode == YODA_MODE_DISKIO) {
    // score rows (the plugin's row per cycle, small P): lane = node over 256-node chunks
    C2 = (h->n_nodes + kBlock - 1) / kBlock;
    const size_t cp = (size_t)C2 * P;
    HIP_TRY(h, h->p_best_f.ensure(cp * 8));
    HIP_TRY(h, h->p_low_f.ensure(cp * 8));
    HIP_TRY(h, h->p_idx.ensure(cp * 4));
    HIP_TRY(h, h->p_ties.ensure(cp * 4));
    part = partials(h);
    HIP_TRY(h, launch_k2b_rows(h->nodes_b.as<NodeRecB>(), h->n_nodes, pod_params(h), P, part,
                               rows, modeb_elig_args(h), h->stream,
                               // (under node sampling: the row covers the pod's walk alone)
                               sampled ? h->b_walk.as<DiskWalk>() : nullptr));
  } else {
    // the block argmax K2 (N32 with summaries) marks the chunks it wrote (PodParams::cmask2)
    if (h->path == Path::N32 && h->has_k2sum && !rows) cmask2 = pod_params(h).cmask2;
    HIP_TRY(h, launch_k2(h->K, h->path, h->nodes.as<unsigned char>(),
                         h->has_k2sum ? (h->perm_run() ? h->k2sum_p : h->k2sum)
                                            .as<unsigned char>()
                                      : nullptr,
                         h->blk_valid ? h->blk.as<uint64_t>() : nullptr, blk_row(h->n_nodes),
                         h->n_nodes,
                         h->chunk2, h->C2, pod_params(h), maxima, h->rcp.as<double>(),
                          P, h->bitmask.as<uint64_t>(), bm_row(h->n_nodes),
                         h->bs_ptr(), bs_row(h->n_nodes), part, rows, h->stats_ptr(), counts,
                         h->stream));
    if (h->class_stats && h->has_k2sum && !rows)
      h->stats_pairs2 += (uint64_t)(P + 63) / 64 * h->n_nodes;
    is_f64 = !h->generic;
    // the shared best and the chunk masks hold this K2's scores: a later phase 2 on the same
    // phase 1 (other maxima) must not read them
    if (!rows) h->blk_fresh = false;
  }
  if (e1) {
    HIP_TRY(h, hipEventRecord(e1, h->stream));
    h->ev_k2.emplace_back(e0, e1);
  }
  // the block K2 (N32 with summaries, argmax) writes no lowest scores: the
  // merge reports each pod's best in their place
  Partials pr = part;
  if (mode == YODA_MODE_SCV && h->path == Path::N32 && h->has_k2sum && !rows) pr.low_f = nullptr;
  if (h->defer_merge2) {  // (finalize merges them in its own kernel)
    h->merge2 = {true, pr, C2, is_f64, cmask2, best, low, idx, ties};
    return YODA_OK;
  }
  HIP_TRY(h, launch_reduce2(pr, C2, P, is_f64, h->node_offset, best, idx, ties, low,
                            h->stream, cmask2));
  return YODA_OK;
}

// Finalize into the handle's pick/status/ties; runs K3 for generic-path overflow pods.
int finalize(yoda_t* h, int mode, const uint32_t* counts, const int64_t* best,
             const uint32_t* idx, const uint32_t* ties, const int64_t* low, bool sharded) {
  const uint32_t P = h->n_work;  // sorted positions of this run
  h->k3_pending = false;
  const yoda_t::Merge2 m2 = h->merge2;  // phase 2's pending merge (a private ordered run)
  h->merge2.on = false;
  if (P == 0) return YODA_OK;
  const bool generic = h->generic && mode == YODA_MODE_SCV;
  if (m2.on && !(h->ordered && !generic))  // (not the fused kernel's case: the merge alone)
    HIP_TRY(h, launch_reduce2(m2.part, m2.C, P, m2.is_f64, h->node_offset, m2.best, m2.idx,
                              m2.ties, m2.low, h->stream, m2.cmask));
  // the overflow count is written by the generic path only: clear it for those runs, and
  // once after one (yoda_shard_overflow_count reads it)
  if (generic || h->flagged_dirty) HIP_TRY(h, hipMemsetAsync(h->n_flagged.p, 0, 4, h->stream));
  h->flagged_dirty = generic;
  if (h->ordered && !generic) {
    // one kernel: the outputs computed and scattered to the caller's pod order into the
    // *_alt buffers, then swapped in (as unpermute_outputs would)
    const uint32_t Pc = h->n_pods;
    // (the maxima -- 48 B a pod, read only by yoda_download -- stay in sorted order until a
    // download asks for them: h->maxima_sorted)
    DevBuf* pairs[][2] = {{&h->pick, &h->pick_alt},         {&h->status, &h->status_alt},
                          {&h->ties_out, &h->ties_out_alt}, {&h->counts, &h->counts_alt},
                          {&h->best, &h->best_alt}};
    for (auto& pr : pairs) HIP_TRY(h, pr[1]->ensure(pr[0]->bytes));
    FinalScatter sc{h->perm.as<uint32_t>(), Pc, h->counts_alt.as<uint32_t>(),
                    h->best_alt.as<int64_t>(), nullptr, nullptr};
    if (m2.on)
      HIP_TRY(h, launch_reduce2_finalize(m2.part, m2.C, P, m2.is_f64, h->node_offset, m2.cmask,
                                         counts, m2.best, m2.idx, m2.ties, m2.low,
                                         h->pick_alt.as<int32_t>(), h->status_alt.as<int32_t>(),
                                         h->ties_out_alt.as<uint32_t>(), sc, h->stream));
    else
      HIP_TRY(h, launch_finalize(counts, best, idx, ties, low, P, false,
                                 h->pick_alt.as<int32_t>(), h->status_alt.as<int32_t>(),
                                 h->ties_out_alt.as<uint32_t>(), h->flagged.as<uint32_t>(),
                                 h->n_flagged.as<uint32_t>(), sc, h->stream));
    for (auto& pr : pairs) pr[0]->swap(*pr[1]);
    h->maxima_sorted = true;
    return YODA_OK;
  }
  const FinalScatter none{};
  HIP_TRY(h, launch_finalize(counts, best, idx, ties, low, P, generic, h->pick.as<int32_t>(),
                             h->status.as<int32_t>(), h->ties_out.as<uint32_t>(),
                             h->flagged.as<uint32_t>(), h->n_flagged.as<uint32_t>(), none,
                             h->stream));
  if (generic) {
    uint32_t nfl = 0;
    HIP_TRY(h, hipMemcpyAsync(&nfl, h->n_flagged.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (nfl > 0) {
      Partials part = partials(h);
      HIP_TRY(h, launch_k3(h->K, h->nodes.as<unsigned char>(), h->n_nodes, h->chunk2, h->C2,
                           pod_params(h), h->maxima.as<uint64_t>(), P, h->bitmask.as<uint64_t>(),
                           bm_row(h->n_nodes),
                           h->flagged.as<uint32_t>(), h->n_flagged.as<uint32_t>(), best, low,
                           part, nfl, h->stream));
      if (sharded) {
        // over this shard's nodes only: per-pod records, merged across the shards by
        // yoda_shard_exact_merge (the flagged set is the same on every shard: it depends on
        // the reduced counts, best and lowest only)
        HIP_TRY(h, h->k3rec.ensure((size_t)P * sizeof(ShardRec)));
        HIP_TRY(h, launch_reduce3_rec(part, h->C2, h->flagged.as<uint32_t>(),
                                      h->n_flagged.as<uint32_t>(), nfl, h->node_offset,
                                      h->k3rec.as<ShardRec>(), h->stream));
        h->k3_pending = true;
        h->k3_nfl = nfl;
        return YODA_OK;  // outputs stay in sorted order until the merge
      }
      HIP_TRY(h, launch_reduce3(part, h->C2, h->flagged.as<uint32_t>(), h->n_flagged.as<uint32_t>(),
                                nfl, h->node_offset, h->pick.as<int32_t>(), h->status.as<int32_t>(),
                                h->ties_out.as<uint32_t>(), h->stream));
    }
  }
  return unpermute_outputs(h);
}

// Top-k candidate lists of the run's P sorted pods (greedy windows, yoda_shard_topk) into
// h->tk_s / h->tk_i ([KT][P], scores and global node ids, (score desc, node asc)), after
// phase 1 and the reciprocals.  The block-classified K2 with packed keys whenever the record
// path and the score bound allow it (its own chunking: one round of workgroups, so that the
// [C][P][KT] lists stay small); else the per-pair K2 (k2_score OUT_TOPK).
// YODA_TOPK_PER_PAIR=1 forces the per-pair kernels (A/B, tests).
// The block-classified top-k K2 with packed keys serves this snapshot (else the per-pair one).
bool topk_block_ok(const yoda_t* h) {
  static const bool per_pair = YODA_KNOB("YODA_TOPK_PER_PAIR", 0) == 1;
  uint32_t ib = 1;
  while ((1ull << ib) <= h->n_nodes) ++ib;
  return !per_pair && h->path == Path::N32 && h->has_k2sum && h->K <= 8 && ib <= 40 &&
         h->score_bound < (1ull << (64 - ib));
}

// deep > KT (the capacity windows, block kernels only): the chunks' KT-deep lists merged into
// `deep`-deep lists exact as far as they reach (k_topk_merge_deep; entries past that empty);
// *depth_out: the depth written (deep, or KT where the block kernels do not run).
int topk_lists(yoda_t* h, uint32_t P, uint32_t KT, const uint32_t* d_counts, uint32_t deep = 0,
               uint32_t* depth_out = nullptr) {
  const uint32_t N = h->n_nodes;
  if (depth_out) *depth_out = KT;
  const uint32_t KD = std::max(KT, deep);
  HIP_TRY(h, h->tk_s.ensure((size_t)KD * P * 8));
  HIP_TRY(h, h->tk_i.ensure((size_t)KD * P * 4));
  if (P == 0 || N == 0) return YODA_OK;
  uint32_t ib = 1;
  while ((1ull << ib) <= N) ++ib;  // node ids < 2^ib - 1: a real key is never 0
  const bool block = topk_block_ok(h);
  if (block) {
    uint32_t Ct = 1, cht = 64;
    // rounds of resident workgroups: 4 for window-sized batches (more, shorter per-(wave,
    // chunk) lists balance better), 1 below 2048 pods (the capacity windows, where the merge's
    // reads dominate); A/B in profiles/r02/greedy_topk/
    static const uint32_t rt_env = YODA_KNOB("YODA_TOPK_ROUNDS", 0);
    const uint32_t rt = rt_env ? rt_env : (P >= 2048 ? 4u : 1u);
    plan_chunks_for((uint32_t)capacity(h, 2, YODA_MODE_SCV), rt, P, N, &Ct, &cht);
    // YODA_TOPK_MIN_CHUNK (A/B knob): chunks of at least that many nodes -- fewer per-(wave,
    // chunk) lists to write and merge in small windows
    static const uint32_t tk_min = YODA_KNOB("YODA_TOPK_MIN_CHUNK", 0);
    if (tk_min && cht < tk_min) {
      cht = (tk_min + kChunkAlign - 1) / kChunkAlign * kChunkAlign;
      Ct = std::max<uint32_t>(1, (N + cht - 1) / cht);
      if (Ct >= 8) Ct = (Ct + 7) / 8 * 8;
    }
    HIP_TRY(h, h->tk_s_part.ensure((size_t)Ct * P * KT * 8));
    PodParams pp = pod_params(h);
    // the list passes take neither the shared k-th keys nor the non-G bounds (the capacity
    // windows ran 1.51 s without them, 1.58 s with them, profiles/r05/g)
    pp.gbest = nullptr;
    pp.kbdec = nullptr;
    HIP_TRY(h, launch_k2_topk_block(h->K, h->nodes.as<unsigned char>(),
                                    h->k2sum.as<unsigned char>(),
                                    h->blk_valid ? h->blk.as<uint64_t>() : nullptr, blk_row(N), N,
                                    cht, Ct, pp, h->rcp.as<double>(),
                                     P, h->bitmask.as<uint64_t>(), bm_row(N),
                                    h->bs_ptr(), bs_row(N), d_counts,
                                    h->tk_s_part.as<uint64_t>(), ib, (int)KT, h->stream));
    if (deep > KT) {
      HIP_TRY(h, launch_topk_merge_deep(h->tk_s_part.as<uint64_t>(), Ct, P, ib, h->node_offset,
                                        h->tk_s.as<double>(), h->tk_i.as<uint32_t>(), (int)KT,
                                        (int)deep, h->stream));
      if (depth_out) *depth_out = deep;
      return YODA_OK;
    }
    HIP_TRY(h, launch_topk_merge_keys(h->tk_s_part.as<uint64_t>(), Ct, P, ib, h->node_offset,
                                      h->tk_s.as<double>(), h->tk_i.as<uint32_t>(), (int)KT,
                                      h->stream));
    return YODA_OK;
  }
  const size_t CPk = (size_t)h->C2 * KT * P;
  HIP_TRY(h, h->tk_s_part.ensure(CPk * 8));
  HIP_TRY(h, h->tk_i_part.ensure(CPk * 4));
  HIP_TRY(h, launch_k2_topk(h->K, h->path, h->nodes.as<unsigned char>(), N, h->chunk2, h->C2,
                            pod_params(h), h->rcp.as<double>(),  P,
                            h->bitmask.as<uint64_t>(), bm_row(N), h->bs_ptr(), bs_row(N),
                            h->blk_ptr(), blk_row(N), partials(h), h->tk_s_part.as<double>(), h->tk_i_part.as<uint32_t>(),
                            (int)KT, h->stream));
  HIP_TRY(h, launch_topk_merge(h->tk_s_part.as<double>(), h->tk_i_part.as<uint32_t>(), h->C2, P,
                               h->node_offset, h->tk_s.as<double>(), h->tk_i.as<uint32_t>(),
                               (int)KT, h->stream));
  return YODA_OK;
}

// ---- the derived tables of an N32 snapshot: one builder each, for yoda_upload_nodes and for
// yoda_update_node_cards ----

// The tiled per-node tables: the row stride, the table in snapshot order, its copy in the
// block-grouped order, its yoda_snapshot_check digest slot.  The first kPackedTables hold the
// rows pack_node writes (PackedRows order); the G table is built on the device.
struct SumTable {
  uint32_t stride;
  DevBuf yoda_handle::*base;
  DevBuf yoda_handle::*grouped;
  int digest;
};
constexpr int kPackedTables = 4, kSumTables = 5;
std::array<SumTable, kSumTables> sum_tables(int K) {
  return {{{k1sum_stride(K), &yoda_handle::k1sum, &yoda_handle::k1sum_p, 1},
           {k2sum_stride(K), &yoda_handle::k2sum, &yoda_handle::k2sum_p, 2},
           {mix_stride(K), &yoda_handle::kmix, &yoda_handle::kmix_p, 3},
           {x1_stride(K), &yoda_handle::kx1, &yoda_handle::kx1_p, 4},
           {gtab_stride(K), &yoda_handle::gtab, &yoda_handle::gtab_p, 6}}};
}

// The G table of both orders from the current K2 summaries and the maxima in gtab_aux.
int relaunch_gtables(yoda_t* h) {
  uint32_t* rcp_dev = reinterpret_cast<uint32_t*>(h->gtab_aux.as<unsigned char>() + 48);
  const MemTab mt = h->mem_ranks ? h->mt : MemTab{};
  HIP_TRY(h, launch_gtable(h->K, h->k2sum.as<uint32_t>(), h->kmix.as<uint32_t>(), h->n_nodes,
                           h->gtab_aux.as<uint64_t>(), h->gtab.as<uint32_t>(), rcp_dev, mt,
                           h->stream));
  if (h->perm_on)
    HIP_TRY(h, launch_gtable(h->K, h->k2sum_p.as<uint32_t>(), h->kmix_p.as<uint32_t>(),
                             h->n_nodes, h->gtab_aux.as<uint64_t>(), h->gtab_p.as<uint32_t>(),
                             rcp_dev, mt, h->stream));
  return YODA_OK;
}

float ru32(double r) {  // the smallest float >= r (yoda_kernels.hip ru32_of)
  float f = (float)r;
  if ((double)f < r) f = std::nextafter(f, INFINITY);
  return f;
}

// The reciprocals of the G maxima as k_gtable left them (ten words at gtab_aux + 48), into
// h->g.  Synchronises the stream.
int read_g_reciprocals(yoda_t* h) {
  uint32_t g_rcp[10] = {};
  HIP_TRY(h, hipMemcpyAsync(g_rcp, h->gtab_aux.as<unsigned char>() + 48, sizeof(g_rcp),
                            hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  std::memcpy(&h->g.r_bw, &g_rcp[0], 8);
  std::memcpy(&h->g.r_core, &g_rcp[2], 8);
  std::memcpy(&h->g.r_pow, &g_rcp[4], 8);
  std::memcpy(&h->g.r_free, &g_rcp[6], 8);
  std::memcpy(&h->g.r_tot, &g_rcp[8], 8);
  h->g.f_bw = ru32(h->g.r_bw);
  h->g.f_core = ru32(h->g.r_core);
  h->g.f_pow = ru32(h->g.r_pow);
  return YODA_OK;
}

// The block summaries of both orders from the device summaries (k_bsum_build).
int rebuild_block_sums(yoda_t* h) {
  HIP_TRY(h, launch_bsum_build(h->K, h->k1sum.as<uint32_t>(), h->k2sum.as<uint32_t>(),
                               h->kx1.as<uint32_t>(), h->kmix.as<uint32_t>(), h->n_nodes,
                               h->blksum.as<uint32_t>(), h->stream));
  if (h->perm_on)
    HIP_TRY(h, launch_bsum_build(h->K, h->k1sum_p.as<uint32_t>(), h->k2sum_p.as<uint32_t>(),
                                 h->kx1_p.as<uint32_t>(), h->kmix_p.as<uint32_t>(), h->n_nodes,
                                 h->blksum_p.as<uint32_t>(), h->stream));
  h->blksum_loose = false;
  return YODA_OK;
}

// ---- yoda_upload_nodes, step by step ----

// The caller's arrays: present, within the limits; *kmax: the largest card count (at least 1).
int check_node_soa(yoda_t* h, const yoda_node_soa* nd, uint32_t node_offset, uint32_t* kmax) {
  if (!nd) return fail(h, YODA_ERR_INVALID_ARG, "nodes is NULL");
  const uint32_t N = nd->n_nodes, KS = nd->max_cards;
  if (KS < 1 || KS > YODA_MAX_CARDS)
    return fail(h, YODA_ERR_INVALID_ARG, "max_cards must be in 1..16");
  if (N > 0 && (!nd->card_number || !nd->card_count || !nd->free_memory_sum ||
                !nd->total_memory_sum || !nd->card_free_memory || !nd->card_total_memory ||
                !nd->card_clock || !nd->card_bandwidth || !nd->card_core || !nd->card_power ||
                !nd->card_healthy))
    return fail(h, YODA_ERR_INVALID_ARG, "a required node array is NULL");
  if ((uint64_t)node_offset + N > 0x7fffffffull)
    return fail(h, YODA_ERR_RANGE, "node index exceeds int32");
  *kmax = 1;
  for (uint32_t i = 0; i < N; ++i) {
    if (nd->card_count[i] > KS) return fail(h, YODA_ERR_INVALID_ARG, "card_count > max_cards");
    *kmax = std::max(*kmax, nd->card_count[i]);
  }
  return YODA_OK;
}

// What an upload decides about the snapshot before it packs a row.
struct UploadFormat {
  int K = 1;
  Path path = Path::N32;
  bool ranks = false;   // the N32 memory fields hold ranks (yoda_layout.h MemTab)
  bool pack16 = true, q32 = true;
  bool all_one = true;  // every node one GPU model with one TotalMemory
  uint64_t max_small = 0;
  uint64_t score_bound = ~0ull;  // yoda_handle::score_bound, sb_cards, sb_actual
  long double sb_cards = 0.0L;
  uint64_t sb_actual = 0;
  std::vector<uint64_t> stat;  // per node: the static score ...
  std::vector<uint8_t> zt;     // ... and TotalMemorySum == 0
};

// Record format: the narrowest exact one.
UploadFormat choose_format(const yoda_node_soa* nd, int K, uint32_t flags) {
  const uint32_t N = nd->n_nodes, KS = nd->max_cards;
  UploadFormat f;
  f.K = K;
  f.stat.resize(N);
  f.zt.resize(N);
  uint64_t max_field = 0, max_small = 0, max_clock = 0, max_static = 0, max_mem = 0;
  uint64_t max_ckq = 0;  // the largest clock quotient a card can score
  bool all_one = true;   // every node one GPU model with one TotalMemory
  for (uint32_t i = 0; i < N; ++i) {
    bool z = false;
    const uint64_t alloc = nd->alloc_memory ? nd->alloc_memory[i] : 0;
    f.stat[i] = static_score(nd->free_memory_sum[i], nd->total_memory_sum[i], alloc, &z);
    f.zt[i] = z;
    max_static = std::max(max_static, f.stat[i]);
    for (uint32_t j = 0; j < nd->card_count[i]; ++j) {
      const size_t k = (size_t)i * KS + j;
      max_field = std::max({max_field, nd->card_free_memory[k], nd->card_total_memory[k],
                            nd->card_clock[k], nd->card_bandwidth[k], nd->card_core[k],
                            nd->card_power[k]});
      max_small = std::max({max_small, nd->card_bandwidth[k], nd->card_core[k],
                            nd->card_power[k], nd->card_clock[k]});
      max_mem = std::max({max_mem, nd->card_free_memory[k], nd->card_total_memory[k]});
      max_clock = std::max(max_clock, nd->card_clock[k]);
      // clock / MaxBandwidth (algorithm.go:283): a scored card qualifies, so MaxBandwidth is
      // at least its own bandwidth (and 1)
      if (nd->card_clock[k] <= kN32FieldMax)
        max_ckq = std::max(max_ckq, nd->card_clock[k] * 100u /
                                        std::max<uint64_t>(1, nd->card_bandwidth[k]));
    }
    // one GPU model with one TotalMemory (the mixed-model K1 tiles pack small fields in 16 bits)
    const size_t a = (size_t)i * KS;
    bool one = nd->card_count[i] > 0 && !(flags & YODA_UPLOAD_NO_UNIFORM);
    for (uint32_t j = 1; j < nd->card_count[i] && one; ++j)
      one = nd->card_clock[a + j] == nd->card_clock[a] &&
            nd->card_bandwidth[a + j] == nd->card_bandwidth[a] &&
            nd->card_core[a + j] == nd->card_core[a] && nd->card_power[a + j] == nd->card_power[a] &&
            nd->card_total_memory[a + j] == nd->card_total_memory[a];
    all_one = all_one && one;
  }
  // per-card score <= 800 + 100*clock (five quotients <= 100, clock/MaxBandwidth <= 100*clock)
  const long double score_bound =
      (long double)K * (800.0L + 100.0L * (long double)max_clock) + (long double)max_static;
  const bool f64_ok = max_field <= kFastFieldMax && score_bound < (long double)kFastScoreMax;
  {
    uint64_t max_actual = 0;  // Actual does not depend on the allocated memory
    for (uint32_t i = 0; i < N; ++i)
      if (nd->total_memory_sum[i] != 0)
        max_actual = std::max(max_actual,
                              nd->free_memory_sum[i] * 100u / nd->total_memory_sum[i] * 2u);
    const long double b = (long double)K * (800.0L + 100.0L * (long double)max_clock) + 300.0L +
                          (long double)max_actual;
    f.score_bound = b < 9.0e18L ? (uint64_t)b + 1u : ~0ull;
    // (yoda_update_node_cards raises the Actual term with the nodes' new FreeMemorySum)
    f.sb_cards = (long double)K * (800.0L + 100.0L * (long double)max_clock) + 300.0L;
    f.sb_actual = max_actual;
  }
  // N32: every small card field in u32, every quotient exact in f64 (x, M < 2^32: 300 x + M
  // < 2^53) -- the block K2 keeps the small-field quotients in f32 while those fields are
  // <= kF32SmallMax (q32) -- the card score summed in u32: per card at most 800 + the clock
  // quotient.  Small fields beyond that need one-model nodes (the mixed-model K1 tiles pack
  // them in 16 bits, and the f64 block K2 is instantiated without the mixed-model rows); beyond
  // 16 bits the K1 writes unpacked partial words (kWideWords).  Memory fields beyond 32 bits (e.g.
  // bytes) keep the N32 path with memory RANKS in the u32 fields (yoda_layout.h MemTab):
  // every compare and max is unchanged, the values come back for the quotients and the
  // maxima (all <= 2^44: exact in f64).
  f.pack16 = max_small <= kPack16Max;
  f.q32 = max_small <= kF32SmallMax && !(flags & YODA_UPLOAD_F64_QUOTIENTS);
  const bool n32_ok = f64_ok && max_small <= kN32FieldMax && (f.q32 || all_one) &&
                      (uint64_t)K * (800u + max_ckq) < (1ull << 32);
  f.path = n32_ok ? Path::N32 : (f64_ok ? Path::F64 : Path::U64);
  if ((flags & YODA_UPLOAD_FORCE_F64) && f.path == Path::N32) f.path = Path::F64;
  if (flags & YODA_UPLOAD_FORCE_GENERIC) f.path = Path::U64;
  f.ranks = f.path == Path::N32 &&
            (max_mem > kN32FieldMax || (flags & YODA_UPLOAD_MEM_RANKS) != 0u);
  f.all_one = all_one;
  f.max_small = max_small;
  return f;
}

// Memory ranks: the distinct card FreeMemory / TotalMemory values, ascending (empty without
// ranks), and the u32 code of a value: the value itself, or 2 + its rank.
struct MemCodes {
  bool ranks = false;
  std::vector<uint64_t> frees, totals;
  static uint32_t code(bool ranks, const std::vector<uint64_t>& v, uint64_t x) {
    if (!ranks) return (uint32_t)x;
    return 2u + (uint32_t)(std::lower_bound(v.begin(), v.end(), x) - v.begin());
  }
  uint32_t code_f(uint64_t x) const { return code(ranks, frees, x); }
  uint32_t code_t(uint64_t x) const { return code(ranks, totals, x); }
};

MemCodes build_mem_codes(const yoda_node_soa* nd, bool ranks) {
  MemCodes mc;
  mc.ranks = ranks;
  if (!ranks) return mc;
  const uint32_t N = nd->n_nodes, KS = nd->max_cards;
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t j = 0; j < nd->card_count[i]; ++j) {
      mc.frees.push_back(nd->card_free_memory[(size_t)i * KS + j]);
      mc.totals.push_back(nd->card_total_memory[(size_t)i * KS + j]);
    }
  for (auto* v : {&mc.frees, &mc.totals}) {
    std::sort(v->begin(), v->end());
    v->erase(std::unique(v->begin(), v->end()), v->end());
  }
  return mc;
}

// Every node's rows, node-major as pack_node writes them (sum .. x1: the N32 path only).
struct PackedRows {
  std::vector<unsigned char> rec;
  std::vector<uint32_t> sum, sum2, mix, x1;
  uint32_t n_one_model = 0, n_uni4 = 0;
};

PackedRows pack_rows(const yoda_node_soa* nd, const UploadFormat& f, const MemCodes& mc,
                     uint32_t flags) {
  const uint32_t N = nd->n_nodes, KS = nd->max_cards;
  const int K = f.K;
  const Path path = f.path;
  PackedRows r;
  const size_t stride = path == Path::N32 ? n32_stride(K) : node_stride(K);
  r.rec.assign((size_t)std::max<uint32_t>(N, 1) * stride, 0);
  // K1 node summaries (N32 path): the facts the block-classified K1 reads per node
  const bool want_sum = path == Path::N32;
  const size_t rows = want_sum ? std::max<uint32_t>(N, 1) : 0;
  const size_t sstride = k1sum_stride(K), s2stride = k2sum_stride(K), mstride = mix_stride(K),
               xstride = x1_stride(K);
  r.sum.assign(rows * sstride / 4, 0);
  r.sum2.assign(rows * s2stride / 4, 0);
  r.mix.assign(rows * mstride / 4, 0);
  r.x1.assign(rows * xstride / 4, 0);
  for (uint32_t i = 0; i < N; ++i) {
    // the node's rows, packed by the one per-node packer (yoda_node_pack.h)
    const size_t a = (size_t)i * KS;
    const uint32_t cnt = nd->card_count[i];
    uint32_t fc[YODA_MAX_CARDS], tc[YODA_MAX_CARDS];
    if (path == Path::N32)
      for (uint32_t j = 0; j < cnt; ++j) {
        fc[j] = mc.code_f(nd->card_free_memory[a + j]);
        tc[j] = mc.code_t(nd->card_total_memory[a + j]);
      }
    NodePackIn in;
    in.cnt = cnt;
    in.card_number = nd->card_number[i];
    in.stat = f.stat[i];
    in.zero_total = f.zt[i] != 0;
    in.no_uniform = (flags & YODA_UPLOAD_NO_UNIFORM) != 0u;
    in.free_memory = nd->card_free_memory + a;
    in.total_memory = nd->card_total_memory + a;
    in.clock = nd->card_clock + a;
    in.bandwidth = nd->card_bandwidth + a;
    in.core = nd->card_core + a;
    in.power = nd->card_power + a;
    in.healthy = nd->card_healthy + a;
    in.fcode = fc;
    in.tcode = tc;
    NodePackOut out;
    out.zeroed = true;  // (the vectors above: value-initialised, each row packed once)
    out.rec = r.rec.data() + (size_t)i * stride;
    if (want_sum) {
      out.sum = r.sum.data() + (size_t)i * sstride / 4;
      out.sum2 = r.sum2.data() + (size_t)i * s2stride / 4;
      out.mix = r.mix.data() + (size_t)i * mstride / 4;
      out.x1 = r.x1.data() + (size_t)i * xstride / 4;
    }
    const uint32_t nf = pack_node(path, K, in, out);
    r.n_one_model += (nf & (kNodeUniform4 | kNodeUniformTotal)) ==
                     (kNodeUniform4 | kNodeUniformTotal);
    r.n_uni4 += (nf & kNodeUniform4) != 0u;
  }
  return r;
}

// Block-grouped node order for the private batch runs (node order): a
// snapshot of one-model nodes is dealt into 64-node blocks of one clock each (PodFitsClock
// then rules whole blocks out for a clock-labelled wave, and K2 skips them), whole blocks
// round-robin in proportion to each clock's block count so that every node chunk keeps
// the snapshot's mix, the groups' remainders last.  Copies of the K1 / K2 summaries in
// that order; the kernels compare the nodes' local ids (perm_ids) on score ties.
// `sum`: the node-major K1 summaries of an N32 snapshot.  Returns the node of each position,
// empty when the snapshot keeps its own order.
std::vector<uint32_t> grouped_node_order(const std::vector<uint32_t>& sum, uint32_t N, int K,
                                         bool ranks, uint32_t flags) {
  std::vector<uint32_t> nperm;
  // Mixed-model nodes (cards of several GPU models) form a group of their own, so that
  // the one-model nodes still fill one-model blocks, which the block summaries decide
  // whole (50 % mixed-model nodes: every block mixed without it).
  if (N < 4096 || (flags & YODA_UPLOAD_PER_NODE_K1) || (flags & YODA_UPLOAD_PER_NODE_K2))
    return nperm;
  const uint32_t SW = k1sum_stride(K) / 4u;
  std::vector<uint32_t> keys;
  std::vector<std::vector<uint32_t>> grp;
  bool ok = true;
  for (uint32_t i = 0; i < N && ok; ++i) {
    // (a mixed-model node's kSumClock is its first card's: the key of its group is ~0)
    const uint32_t ck = (sum[(size_t)i * SW + kSumMeta] & kSumUni4)
                            ? sum[(size_t)i * SW + kSumClock] : 0xffffffffu;
    size_t g = 0;
    while (g < keys.size() && keys[g] != ck) ++g;
    if (g == keys.size()) {
      if (keys.size() == 64) ok = false;  // too many clocks to group usefully
      keys.push_back(ck);
      grp.emplace_back();
    }
    if (ok) grp[g].push_back(i);
  }
  const size_t G = grp.size();
  // Inside a clock group the nodes go into blocks by their healthy frees: sorted on a
  // Z-order key of hfs[0], hfs[1], hfs[3], hfs[7] (the frees that PodFitsMemory compares
  // for 1, 2, 4, 8 GPUs; hfs[15] too at K = 16), so that a block's nodes are alike and its
  // bounds decide it for a whole wave (tools: 16 % of (wave, block)s undecided on config 3
  // with the blocks as uploaded, 4 % sorted); the sorted blocks are then taken in
  // bit-reversed order, so that any run of consecutive blocks -- a node chunk -- still
  // samples every free level (the chunks stay even).
  // Not with memory ranks: there the rank-space K2 ran slower on the sorted blocks
  // (memory in bytes: 1.91 vs 1.80 ms, profiles/r05/y/ab.txt).
  if (ok && !ranks) {
    std::vector<uint32_t> hix;
    for (uint32_t t = 1; t <= (uint32_t)K; t <<= 1) hix.push_back(t - 1);
    const uint32_t nc = (uint32_t)hix.size(), bits = 64 / nc > 16 ? 16 : 64 / nc;
    std::vector<std::pair<uint64_t, uint32_t>> zk;
    for (auto& g : grp) {
      uint32_t mx[8] = {};
      for (uint32_t i : g)
        for (uint32_t c = 0; c < nc; ++c)
          mx[c] = std::max(mx[c], sum[(size_t)i * SW + kSumHfs + hix[c]]);
      zk.clear();
      for (uint32_t i : g) {
        uint64_t z = 0;
        for (uint32_t c = 0; c < nc; ++c) {
          const uint64_t v = sum[(size_t)i * SW + kSumHfs + hix[c]];
          const uint64_t qv = mx[c] ? std::min<uint64_t>((v << bits) / ((uint64_t)mx[c] + 1),
                                                         (1ull << bits) - 1) : 0;
          for (uint32_t b = 0; b < bits; ++b) z |= ((qv >> b) & 1ull) << (b * nc + c);
        }
        zk.emplace_back(z, i);
      }
      std::stable_sort(zk.begin(), zk.end(), [](const std::pair<uint64_t, uint32_t>& a,
                                                const std::pair<uint64_t, uint32_t>& b) {
        return a.first < b.first;
      });
      const size_t nbg = g.size() / 64;
      size_t lg = 0;
      while (((size_t)1 << lg) < nbg) ++lg;
      std::vector<uint32_t> out;
      out.reserve(g.size());
      for (size_t j = 0; j < ((size_t)1 << lg); ++j) {  // bit-reversed block order
        size_t r = 0;
        for (size_t b = 0; b < lg; ++b) r |= ((j >> b) & 1u) << (lg - 1 - b);
        if (r < nbg)
          for (size_t k = 0; k < 64; ++k) out.push_back(zk[r * 64 + k].second);
      }
      for (size_t k = nbg * 64; k < g.size(); ++k) out.push_back(zk[k].second);
      g.swap(out);
    }
  }
  if (ok && G >= 1) {
    std::vector<size_t> nb(G), done(G, 0);
    size_t total = 0;
    for (size_t g = 0; g < G; ++g) total += (nb[g] = grp[g].size() / 64);
    nperm.reserve(N);
    for (size_t b = 0; b < total; ++b) {
      size_t best = G;
      double bt = 0.0;
      for (size_t g = 0; g < G; ++g) {
        if (done[g] == nb[g]) continue;
        const double t = (done[g] + 0.5) / (double)nb[g];
        if (best == G || t < bt) best = g, bt = t;
      }
      const size_t o = done[best]++ * 64;
      nperm.insert(nperm.end(), grp[best].begin() + o, grp[best].begin() + o + 64);
    }
    for (size_t g = 0; g < G; ++g)
      nperm.insert(nperm.end(), grp[g].begin() + done[g] * 64, grp[g].end());
    if (nperm.size() != N) nperm.clear();
  }
  return nperm;
}

// Node-major rows -> 64-node tiles (sum_index, yoda_layout.h); position q of the result holds
// the row of node order[q] (order == nullptr: of node q).
void tile_rows(const std::vector<uint32_t>& v, uint32_t stride, uint32_t N, const uint32_t* order,
               std::vector<uint32_t>& t) {
  t.assign(sum_words(std::max<uint32_t>(N, 1), stride), 0u);
  const uint32_t W = stride / 4u;
  for (uint32_t q = 0; q < N; ++q) {
    const uint32_t* r = v.data() + (size_t)(order ? order[q] : q) * W;
    for (uint32_t w = 0; w < W; ++w) t[sum_index(q, w, stride)] = r[w];
  }
}

// The packed tables tiled and copied to the device: in snapshot order, and with a grouped order
// (nperm not empty) in that order too, with the order itself (perm_ids) and its inverse.  The
// copies are asynchronous: `staged` holds their host sides and must outlive the caller's
// synchronisation.  The tiled K2 summaries of the snapshot order are the handle's host mirror.
int upload_sum_tables(yoda_t* h, const PackedRows& rows, const std::vector<uint32_t>& nperm,
                      std::vector<std::vector<uint32_t>>& staged) {
  const uint32_t N = h->n_nodes;
  auto put = [&](DevBuf& d, const std::vector<uint32_t>& v) -> int {
    HIP_TRY(h, d.ensure(v.size() * 4));
    HIP_TRY(h, hipMemcpyAsync(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, h->stream));
    return YODA_OK;
  };
  const std::vector<uint32_t>* src[kPackedTables] = {&rows.sum, &rows.sum2, &rows.mix, &rows.x1};
  const auto tabs = sum_tables(h->K);
  staged.assign(2 * kPackedTables + 1, {});
  for (int k = 0; k < kPackedTables; ++k) {
    std::vector<uint32_t>& t = tabs[k].base == &yoda_handle::k2sum ? h->host_k2sum : staged[2 * k];
    tile_rows(*src[k], tabs[k].stride, N, nullptr, t);
    if (int rc = put(h->*tabs[k].base, t)) return rc;
    if (nperm.empty()) continue;
    tile_rows(*src[k], tabs[k].stride, N, nperm.data(), staged[2 * k + 1]);
    if (int rc = put(h->*tabs[k].grouped, staged[2 * k + 1])) return rc;
  }
  if (!nperm.empty()) {
    std::vector<uint32_t>& inv = staged[2 * kPackedTables];
    inv.resize(N);
    for (uint32_t q = 0; q < N; ++q) inv[nperm[q]] = q;
    if (int rc = put(h->perm_ids, nperm)) return rc;
    if (int rc = put(h->perm_inv, inv)) return rc;
  }
  return YODA_OK;
}

// The block summaries of the snapshot order and of the block-grouped copy's (BlockSumWord),
// built from the tables already enqueued.  k_bsum_build writes the real blocks only and DevBuf
// is grow-only, so the tile padding is cleared first: it may hold an older, larger snapshot's
// words, which yoda_snapshot_check would compare.
int upload_block_sums(yoda_t* h) {
  const size_t bytes =
      sum_words(std::max<uint32_t>((h->n_nodes + 63) / 64, 1), bsum_stride(h->K)) * 4;
  HIP_TRY(h, h->blksum.ensure(bytes));
  HIP_TRY(h, hipMemsetAsync(h->blksum.p, 0, bytes, h->stream));
  if (h->perm_on) {
    HIP_TRY(h, h->blksum_p.ensure(bytes));
    HIP_TRY(h, hipMemsetAsync(h->blksum_p.p, 0, bytes, h->stream));
  }
  return rebuild_block_sums(h);
}

// The G table: per field the max over every real card (floor 1, collection.go:31-38),
// the CollectMaxValues result of any pod feasible on the maximal cards' nodes; with memory
// ranks the value tables the kernels read the memory fields through (h->mt).
int upload_gtables(yoda_t* h, const yoda_node_soa* nd, const MemCodes& mc) {
  const uint32_t N = nd->n_nodes, KS = nd->max_cards;
  uint64_t gmax[6] = {1, 1, 1, 1, 1, 1};
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t j = 0; j < nd->card_count[i]; ++j) {
      const size_t k = (size_t)i * KS + j;
      gmax[kMaxBw] = std::max(gmax[kMaxBw], nd->card_bandwidth[k]);
      gmax[kMaxClock] = std::max(gmax[kMaxClock], nd->card_clock[k]);
      gmax[kMaxCore] = std::max(gmax[kMaxCore], nd->card_core[k]);
      gmax[kMaxFree] = std::max(gmax[kMaxFree], nd->card_free_memory[k]);
      gmax[kMaxPower] = std::max(gmax[kMaxPower], nd->card_power[k]);
      gmax[kMaxTotal] = std::max(gmax[kMaxTotal], nd->card_total_memory[k]);
    }
  const size_t tab_bytes = sum_words(std::max<uint32_t>(N, 1), gtab_stride(h->K)) * 4;
  HIP_TRY(h, h->gtab.ensure(tab_bytes));
  if (h->perm_on) HIP_TRY(h, h->gtab_p.ensure(tab_bytes));  // (the same rows, reordered)
  std::memcpy(h->h_gmax, gmax, sizeof(gmax));
  HIP_TRY(h, h->gtab_aux.ensure(kGTabAuxBytes));
  HIP_TRY(h, hipMemcpyAsync(h->gtab_aux.p, h->h_gmax, sizeof(h->h_gmax), hipMemcpyHostToDevice,
                            h->stream));
  h->mt = MemTab{};
  if (mc.ranks) {  // value tables: v[0] = v[1] = 0, v[2 + i] = the i-th distinct value
    // (the previous upload ended in a synchronisation: its copy of h_memtab is done)
    std::vector<double>& vt = h->h_memtab;
    vt.assign(4 + mc.frees.size() + mc.totals.size(), 0.0);
    for (size_t i = 0; i < mc.frees.size(); ++i) vt[2 + i] = (double)mc.frees[i];
    for (size_t i = 0; i < mc.totals.size(); ++i) vt[4 + mc.frees.size() + i] = (double)mc.totals[i];
    HIP_TRY(h, h->memtab.ensure(vt.size() * 8));
    // on the handle's stream, as every table of the upload: a step still queued there reads the
    // previous snapshot's values (a copy on the null stream does not wait for a non-blocking one)
    HIP_TRY(h, hipMemcpyAsync(h->memtab.p, vt.data(), vt.size() * 8, hipMemcpyHostToDevice,
                              h->stream));
    h->mt.vf = h->memtab.as<double>();
    h->mt.vt = h->memtab.as<double>() + 2 + mc.frees.size();
    h->mt.nf = (uint32_t)mc.frees.size();
  }
  return relaunch_gtables(h);
}

// The blocks whose bound with every card qualifying (lv[0]) is in the top tenth, per order: a
// static visiting order hint for the argmax K2 (results do not depend on it).
int build_hot_masks(yoda_t* h) {
  const int K = h->K;
  const uint32_t nb = (h->n_nodes + 63) / 64, KST = kbub_stride(K);
  std::vector<uint32_t> ubw(sum_words(nb, KST));
  std::vector<uint64_t> words((nb + 63) / 64), words_p((nb + 63) / 64);
  auto hot_bits = [&](const DevBuf& src, std::vector<uint64_t>& out) -> int {
    HIP_TRY(h, hipMemcpyAsync(ubw.data(), src.p, ubw.size() * 4, hipMemcpyDeviceToHost,
                              h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<double> u(nb);
    for (uint32_t b = 0; b < nb; ++b) {
      const uint64_t bits = (uint64_t)ubw[sum_index(b, kbub_lvl(K), KST)] |
                            ((uint64_t)ubw[sum_index(b, kbub_lvl(K) + 1u, KST)] << 32);
      std::memcpy(&u[b], &bits, 8);
    }
    std::vector<double> srt(u);
    const size_t q = srt.size() - 1 - srt.size() / 10;
    std::nth_element(srt.begin(), srt.begin() + q, srt.end());
    const double thr = srt[q];
    std::fill(out.begin(), out.end(), 0ull);
    for (uint32_t b = 0; b < nb; ++b)
      if (u[b] >= thr) out[b >> 6] |= 1ull << (b & 63);
    return YODA_OK;
  };
  int hr = hot_bits(h->kbub, words);
  if (!hr && h->perm_on) hr = hot_bits(h->kbub_p, words_p);
  if (hr) return hr;
  HIP_TRY(h, h->hot.ensure(words.size() * 8));
  HIP_TRY(h, hipMemcpy(h->hot.p, words.data(), words.size() * 8, hipMemcpyHostToDevice));
  if (h->perm_on) {
    HIP_TRY(h, h->hot_p.ensure(words_p.size() * 8));
    HIP_TRY(h, hipMemcpy(h->hot_p.p, words_p.data(), words_p.size() * 8,
                         hipMemcpyHostToDevice));
  }
  h->hot_ok = true;
  return YODA_OK;
}

}  // namespace

// ======================================================================================
extern "C" {

int yoda_abi_version(void) { return YODA_ABI_VERSION; }

int yoda_create(int device, yoda_t** out) {
  if (!out) return YODA_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return YODA_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return YODA_ERR_NO_DEVICE;
  yoda_t* h = new (std::nothrow) yoda_t();
  if (!h) return YODA_ERR_INVALID_ARG;
  h->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return YODA_ERR_HIP;
  }
  h->stream = h->own_stream;
  if (hipEventCreateWithFlags(&h->stage_event, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->upd_event, hipEventDisableTiming) != hipSuccess) {
    delete h;
    return YODA_ERR_HIP;
  }
  *out = h;
  return YODA_OK;
}

int yoda_destroy(yoda_t* h) {
  if (!h) return YODA_ERR_INVALID_ARG;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return YODA_OK;
}

const char* yoda_last_error(const yoda_t* h) {
  return h ? h->last_error.c_str() : "null handle";
}

// Switch the handle's stream: work already queued on the old stream (an upload's copies and
// kernels) is ordered before anything queued on the new one (an event wait, no host sync).
static int switch_stream(yoda_t* h, hipStream_t ns) {
  if (ns == h->stream) return YODA_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if (!h->switch_event)
    HIP_TRY(h, hipEventCreateWithFlags(&h->switch_event, hipEventDisableTiming));
  HIP_TRY(h, hipEventRecord(h->switch_event, h->stream));
  HIP_TRY(h, hipStreamWaitEvent(ns, h->switch_event, 0));
  h->stream = ns;
  return YODA_OK;
}

int yoda_set_stream(yoda_t* h, void* hip_stream) {
  if (!h) return YODA_ERR_INVALID_ARG;
  return switch_stream(h, static_cast<hipStream_t>(hip_stream));
}

int yoda_use_own_stream(yoda_t* h) {
  if (!h) return YODA_ERR_INVALID_ARG;
  return switch_stream(h, h->own_stream);
}

int yoda_synchronize(yoda_t* h) {
  if (!h) return YODA_ERR_INVALID_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return YODA_OK;
}

int yoda_upload_nodes(yoda_t* h, const yoda_node_soa* nd, uint32_t node_offset, uint32_t flags) {
  if (!h) return YODA_ERR_INVALID_ARG;
  try {
    h->topk_ready = false;
    uint32_t kmax = 1;
    if (int rc = check_node_soa(h, nd, node_offset, &kmax)) return rc;
    const uint32_t N = nd->n_nodes;
    HIP_TRY(h, hipSetDevice(h->device));
    const int K = pow2_cards(kmax);  // 1, 2, 4, 8 or 16
    // Host side: the format, the memory codes, every node's rows.
    const UploadFormat fmt = choose_format(nd, K, flags);
    MemCodes mc = build_mem_codes(nd, fmt.ranks);
    PackedRows rows = pack_rows(nd, fmt, mc, flags);
    const Path path = fmt.path;
    const bool want_sum = path == Path::N32;
    // From here on the handle describes the new snapshot: the table builders below read K,
    // n_nodes, perm_on and the memory ranks from it.  A call that fails on the way leaves no
    // snapshot.
    h->has_nodes = false;
    h->score_bound = fmt.score_bound;
    h->sb_cards = fmt.sb_cards;
    h->sb_actual = fmt.sb_actual;
    if (h->K != K || h->path != path) std::memset(h->cap, 0, sizeof(h->cap));
    h->K = K;
    h->path = path;
    h->generic = path == Path::U64;
    h->n_nodes = N;
    h->node_offset = node_offset;
    h->mem_ranks = fmt.ranks;
    h->mt = MemTab{};
    h->pack16 = fmt.pack16;
    h->q32 = fmt.q32;
    h->small_max = fmt.max_small;
    h->perm_on = false;
    h->host_k2sum.clear();
    HIP_TRY(h, h->nodes.ensure(rows.rec.size()));
    HIP_TRY(h, hipMemcpyAsync(h->nodes.p, rows.rec.data(), rows.rec.size(), hipMemcpyHostToDevice,
                              h->stream));
    // N32: the summaries in both node orders, then what the device derives from them
    std::vector<uint32_t> nperm;
    std::vector<std::vector<uint32_t>> staged;  // (host sides of the copies in flight)
    if (want_sum) {
      nperm = grouped_node_order(rows.sum, N, K, fmt.ranks, flags);
      h->perm_on = !nperm.empty();
      int rc = upload_sum_tables(h, rows, nperm, staged);
      if (!rc) rc = upload_block_sums(h);
      if (!rc) rc = upload_gtables(h, nd, mc);
      if (rc) return rc;
    }
    const bool diskio = nd->cpu && nd->disk_io;
    std::vector<NodeRecB> rb;
    if (diskio && N > 0) {
      rb.resize(N);
      for (uint32_t i = 0; i < N; ++i) {
        rb[i].v = nd->cpu[i] / 100.0;     // algorithm.go:73
        rb[i].u = nd->disk_io[i] / 50.0;  // algorithm.go:71
      }
      HIP_TRY(h, h->nodes_b.ensure((size_t)N * sizeof(NodeRecB)));
      HIP_TRY(h, hipMemcpyAsync(h->nodes_b.p, rb.data(), (size_t)N * sizeof(NodeRecB),
                                hipMemcpyHostToDevice, h->stream));
    }
    h->has_k1sum = want_sum && !(flags & YODA_UPLOAD_PER_NODE_K1);
    h->has_k2sum = want_sum && !(flags & YODA_UPLOAD_PER_NODE_K2);
    // The upload's one wait, for every copy and table kernel above; with a G table in use its
    // reciprocals come back in the same wait.
    h->g = GTab{};
    if (h->has_k2sum && N > 0 && !(flags & YODA_UPLOAD_NO_GTAB)) {
      h->g.tab = h->gtab.as<uint32_t>();
      if (int rc = read_g_reciprocals(h)) return rc;
    } else {
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->host_records.swap(rows.rec);
    h->h_total_sum.assign(nd->total_memory_sum, nd->total_memory_sum + N);
    h->h_free_sum.assign(nd->free_memory_sum, nd->free_memory_sum + N);
    h->h_card_number.assign(nd->card_number, nd->card_number + N);
    h->h_alloc.assign(N, 0);
    if (nd->alloc_memory) h->h_alloc.assign(nd->alloc_memory, nd->alloc_memory + N);
    h->h_absent.assign(N, 0);  // every node of a fresh snapshot is present
    h->n_absent = 0;
    h->cand_classes = 0;  // ... and a candidate of every pod (yoda_set_candidates: off)
    h->h_cand.clear();
    h->samp_m = 0;  // ... and every feasible node is scored (yoda_set_node_sampling: off)
    h->h_start.clear();
    h->samp_ran = false;
    h->b_elig_dirty = true;  // (Mode B's eligibility table is the old snapshot's)
    h->b_elig_builds = 0;
    h->b_rank_for = 0xffffffffu;  // (... and so are the rank tables of yoda_mode_b_sampling)
    h->b_rank_builds = 0;
    h->nodes_diskio = diskio;
    h->upload_flags = flags;
    h->n_one_model = rows.n_one_model;
    h->n_uni4 = rows.n_uni4;
    h->all_one_model = rows.n_one_model == N;
    h->all_uni4 = rows.n_uni4 == N;
    h->kbub_dirty = true;
    h->kbub_loose = false;
    h->kb_levels_ok = false;
    h->hot_ok = false;
    if (h->has_k2sum && h->g.tab && N > 0) {
      HIP_TRY(h, build_block_ub(h));
      if (int rc = build_hot_masks(h)) return rc;
    }
    h->h_frees.swap(mc.frees);
    h->h_totals.swap(mc.totals);
    h->has_nodes = true;
    // the uploaded pods' N32 memory thresholds follow the snapshot (ranks or the clamp)
    if (h->has_pods && path == Path::N32) {
      int rc = pods_complete(h);  // (the rank kernel reads the 64-bit scv/memory)
      if (rc) return rc;
      unsigned char* b = h->pod_blob.as<unsigned char>();
      HIP_TRY(h, launch_mem_rank(reinterpret_cast<const uint64_t*>(b + h->pod_off[kPodMU]),
                                 h->n_pods, pod_params(h).mt,
                                 reinterpret_cast<uint32_t*>(b + h->pod_off[kPodM32]), h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->ran = false;
    h->phase1_done = false;
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_uses_generic_path(const yoda_t* h) { return h ? (h->generic ? 1 : 0) : -1; }

int yoda_record_path(const yoda_t* h) { return h ? (int)h->path : -1; }

int yoda_memory_ranks(const yoda_t* h) { return h ? (h->mem_ranks ? 1 : 0) : -1; }
uint64_t yoda_small_field_max(const yoda_t* h) { return h ? h->small_max : 0; }

uint64_t yoda_score_bound(const yoda_t* h) { return h && h->has_nodes ? h->score_bound : ~0ull; }

int yoda_update_alloc(yoda_t* h, const uint64_t* alloc) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (!alloc && h->n_nodes) return fail(h, YODA_ERR_INVALID_ARG, "alloc is NULL");
  try {
    // Every node through the sparse node-state push: the records, the K2 summaries, their
    // block-grouped copies (perm_on) and the host copies (h_alloc, host_records) all change
    // together -- k_set_static is the one writer of a node's static score.
    const uint32_t N = h->n_nodes;
    std::vector<uint32_t> ids(N);
    for (uint32_t i = 0; i < N; ++i) ids[i] = h->node_offset + i;
    const std::vector<uint64_t> cn(h->h_card_number);
    int rc = yoda_set_node_state(h, N, ids.data(), alloc, cn.data());
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_upload_pods(yoda_t* h, const yoda_pod_soa* pd) {
  if (!h) return YODA_ERR_INVALID_ARG;
  try {
    if (!pd) return fail(h, YODA_ERR_INVALID_ARG, "pods is NULL");
    const uint32_t P = pd->n_pods;
    if (P > 0 && (!pd->has_number || !pd->number || !pd->has_memory || !pd->memory ||
                  !pd->has_clock || !pd->clock))
      return fail(h, YODA_ERR_INVALID_ARG, "a required pod array is NULL");
    h->topk_ready = false;
    h->b_cls_ready = false;
    HIP_TRY(h, hipSetDevice(h->device));
    // One blob of per-pod arrays, staged in pinned memory; the arrays a private block-kernel
    // run reads go with one copy now, the rest (kPodPlace) when an entry point needs them.
    size_t off[kPodArrays], total = 0, core_bytes = 0;
    for (int i = 0; i < kPodArrays; ++i) {
      const int a = kPodPlace[i];
      off[a] = total;
      total += ((size_t)std::max<uint32_t>(P, 1) * kPodArrayBytes[a] + 255) / 256 * 256;
      if (i == kPodCoreArrays - 1) core_bytes = total;
    }
    h->pod_rest_bytes = 0;  // (a deferred part of the previous batch is dropped)
    h->rest_lazy = false;
    // (memory ranks: the rank kernel below reads the 64-bit scv/memory now)
    const bool defer = !(h->has_nodes && h->mem_ranks);
    // the f64 thresholds and the Mode B weights (zero without rio / rcpu) are written later,
    // off the upload's critical path (pods_pack_rest)
    const bool lazy = defer && !(pd->rio && pd->rcpu);
    static const bool dbg = std::getenv("YODA_UPLOAD_DEBUG") != nullptr;
    auto now_ms = [] {
      return std::chrono::duration<double, std::milli>(
                 std::chrono::steady_clock::now().time_since_epoch()).count();
    };
    const double t_start = dbg ? now_ms() : 0.0;
    if (h->stage_pending) HIP_TRY(h, hipEventSynchronize(h->stage_event));  // staging reuse
    HIP_TRY(h, h->pod_stage.ensure(total));
    HIP_TRY(h, h->pod_blob.ensure(total));
    unsigned char* st = static_cast<unsigned char*>(h->pod_stage.p);
    double* mf = reinterpret_cast<double*>(st + off[kPodMF]);
    double* cf = reinterpret_cast<double*>(st + off[kPodCF]);
    uint64_t* mu = reinterpret_cast<uint64_t*>(st + off[kPodMU]);
    uint64_t* cu = reinterpret_cast<uint64_t*>(st + off[kPodCU]);
    uint64_t* num = reinterpret_cast<uint64_t*>(st + off[kPodNumber]);
    double* al = reinterpret_cast<double*>(st + off[kPodAlpha]);
    double* be = reinterpret_cast<double*>(st + off[kPodBeta]);
    uint32_t* m32 = reinterpret_cast<uint32_t*>(st + off[kPodM32]);
    uint32_t* c32 = reinterpret_cast<uint32_t*>(st + off[kPodC32]);
    uint32_t* nm = reinterpret_cast<uint32_t*>(st + off[kPodNeedMem]);
    uint32_t* nc = reinterpret_cast<uint32_t*>(st + off[kPodNeedClk]);
    const uint64_t kClamp = kPodF64Clamp;
    uint64_t key_or[3] = {0, 0, 0};       // OR of the sort key's clamped fields (c, n, m)
    // distinct (clock, number, has-memory) groups with their pod counts and, per group, its
    // pods of the largest and of the smallest memory (the padding copies) as (m << 32 | pod)
    // extremes.  The pods are packed by up to 16 host threads over contiguous ranges, each
    // with its own group table (merged after: counts add, extremes max/min).
    struct GroupTable {
      std::vector<uint64_t> key = std::vector<uint64_t>(64, 0ull);  // key + 1 (0 = empty)
      std::vector<uint32_t> cnt = std::vector<uint32_t>(64, 0u);
      std::vector<uint64_t> mx = std::vector<uint64_t>(64, 0ull), mn = std::vector<uint64_t>(64, ~0ull);
      size_t n = 0;
      size_t slot(uint64_t k1) const {
        size_t i = (size_t)(k1 * 0x9e3779b97f4a7c15ull >> 40) & (key.size() - 1);
        while (key[i] != 0ull && key[i] != k1) i = (i + 1) & (key.size() - 1);
        return i;
      }
      void add(uint64_t g, uint32_t c, uint64_t vmax, uint64_t vmin) {
        size_t i = slot(g + 1);
        if (key[i] == 0ull) {
          if (2 * (n + 1) > key.size()) {  // grow and rehash
            GroupTable o;
            const size_t n2 = key.size() * 2;
            o.key.assign(n2, 0ull);
            o.cnt.assign(n2, 0u);
            o.mx.assign(n2, 0ull);
            o.mn.assign(n2, ~0ull);
            for (size_t j = 0; j < key.size(); ++j)
              if (key[j]) {
                const size_t t = o.slot(key[j]);
                o.key[t] = key[j];
                o.cnt[t] = cnt[j];
                o.mx[t] = mx[j];
                o.mn[t] = mn[j];
              }
            o.n = n;
            *this = std::move(o);
            i = slot(g + 1);
          }
          key[i] = g + 1;
          ++n;
        }
        cnt[i] += c;
        mx[i] = std::max(mx[i], vmax);
        mn[i] = std::min(mn[i], vmin);
      }
    };
    auto pack_range = [&](uint32_t p0, uint32_t p1, GroupTable& gt, uint64_t* kor_out) {
      // (ORs accumulated locally: the per-thread outputs share cache lines)
      uint64_t kor[3] = {0ull, 0ull, 0ull};
      uint64_t g_last = ~0ull;
      uint32_t g_run = 0;
      uint64_t r_max = 0, r_min = ~0ull;  // the current run's extremes
      for (uint32_t p = p0; p < p1; ++p) {
        const uint64_t number = pd->has_number[p] ? pd->number[p] : 1;  // filter.go:12-15
        const uint64_t m = pd->has_memory[p] ? pd->memory[p] : 0;       // filter.go:19,32
        const uint64_t c = pd->has_clock[p] ? pd->clock[p] : 0;         // filter.go:36,49
        const uint32_t need = number > 0xffffffffull ? 0xffffffffu : (uint32_t)number;
        num[p] = number;
        nm[p] = pd->has_memory[p] ? need : 0;
        nc[p] = pd->has_clock[p] ? need : 0;
        mu[p] = m;
        cu[p] = c;
        if (!lazy) {
          mf[p] = (double)std::min(m, kClamp);
          cf[p] = (double)std::min(c, kClamp);
        }
        m32[p] = (uint32_t)std::min<uint64_t>(m, 0xffffffffull);  // > every N32 field
        c32[p] = (uint32_t)std::min<uint64_t>(c, 0xffffffffull);
        kor[0] |= std::min<uint64_t>(c, 0xffffffull);  // the clamps of k_order_keys
        kor[1] |= std::min<uint64_t>(number, 0xffull);
        kor[2] |= std::min<uint64_t>(m, 0xffffffffull);
        const uint64_t g = (std::min<uint64_t>(c, 0xffffffull) << 9) |
                           (std::min<uint64_t>(number, 0xffull) << 1) | (nm[p] != 0u ? 1u : 0u);
        if (g != g_last) {  // consecutive pods of one group (the common case) skip the probe
          if (g_run) gt.add(g_last, g_run, r_max, r_min);
          g_last = g;
          g_run = 0;
          r_max = 0;
          r_min = ~0ull;
        }
        ++g_run;
        const uint64_t mp = (std::min<uint64_t>(m, 0xffffffffull) << 32) | p;
        r_max = std::max(r_max, mp);
        r_min = std::min(r_min, mp);
        if (!lazy) al[p] = be[p] = 0.0;
        if (pd->rio && pd->rcpu) {  // algorithm.go:105-106
          const double beta = 1.0 / (1.0 + (double)pd->rcpu[p] / pd->rio[p]);
          be[p] = beta;
          al[p] = 1 - beta;
        }
      }
      if (g_run) gt.add(g_last, g_run, r_max, r_min);
      for (int f = 0; f < 3; ++f) kor_out[f] = kor[f];
    };
    // ranges of >= YODA_UPLOAD_MIN_RANGE (default 4096) pods over the process's worker pool
    // (HostPool); A/B knob for the greedy windows' 6144-pod uploads
    static const uint32_t thr_cap = YODA_KNOB("YODA_UPLOAD_THREADS", 16);
    static const uint32_t min_range = std::max<uint32_t>(256, YODA_KNOB("YODA_UPLOAD_MIN_RANGE", 4096));
    const uint32_t n_thr = std::min<uint32_t>({HostPool::get().size(), std::max(1u, thr_cap),
                                               std::max(1u, P / min_range)});
    std::vector<GroupTable> tables(n_thr);
    std::vector<std::array<uint64_t, 3>> kors(n_thr, {0ull, 0ull, 0ull});
    {
      std::vector<uint8_t> thr_failed(n_thr, 0);  // a worker's exception (bad_alloc) -> rethrown
      const uint32_t per = (P + n_thr - 1) / n_thr;
      HostPool::get().run(n_thr, [&](uint32_t t) {
        try {
          pack_range(std::min(P, t * per), std::min(P, (t + 1) * per), tables[t], kors[t].data());
        } catch (...) {
          thr_failed[t] = 1;
        }
      });
      for (uint8_t f : thr_failed)
        if (f) throw std::bad_alloc();
    }
    const double t_packed = dbg ? now_ms() : 0.0;
    GroupTable all = std::move(tables[0]);
    for (uint32_t t = 1; t < n_thr; ++t)
      for (size_t j = 0; j < tables[t].key.size(); ++j)
        if (tables[t].key[j])
          all.add(tables[t].key[j] - 1, tables[t].cnt[j], tables[t].mx[j], tables[t].mn[j]);
    for (const auto& k : kors)
      for (int f = 0; f < 3; ++f) key_or[f] |= k[f];
    std::vector<uint64_t>& gkey = all.key;
    std::vector<uint32_t>& gcnt = all.cnt;
    std::vector<uint64_t>& gmax = all.mx;
    std::vector<uint64_t>& gmin = all.mn;
    const size_t g_n = all.n;
    const double t_merged = dbg ? now_ms() : 0.0;
    HIP_TRY(h, hipMemcpyAsync(h->pod_blob.p, st, defer ? core_bytes : total, hipMemcpyHostToDevice,
                              h->stream));
    if (defer) {  // (the deferred copy of a private run starts from here: pods_complete_async)
      if (int rc = ensure_copy_stream(h)) return rc;
      HIP_TRY(h, hipEventRecord(h->core_event, h->stream));
    }
    const double t_copied = dbg ? now_ms() : 0.0;
    if (h->has_nodes && h->mem_ranks)  // scv/memory -> its rank threshold, on the device
      HIP_TRY(h, launch_mem_rank(reinterpret_cast<const uint64_t*>(
                                     h->pod_blob.as<unsigned char>() + off[kPodMU]),
                                 P, h->mt,
                                 reinterpret_cast<uint32_t*>(h->pod_blob.as<unsigned char>() +
                                                             off[kPodM32]),
                                 h->stream));
    {  // the counting-sort order's groups (yoda_order.hip)
      struct Grp {
        uint64_t key;
        uint32_t count, pod_max, pod_min;  // pods of the largest / smallest memory
        bool operator<(const Grp& o) const { return key < o.key; }
      };
      std::vector<Grp> gs;
      gs.reserve(g_n);
      for (size_t i = 0; i < gkey.size(); ++i)
        if (gkey[i])
          gs.push_back({gkey[i] - 1, gcnt[i], (uint32_t)gmax[i], (uint32_t)gmin[i]});
      std::sort(gs.begin(), gs.end());
      const uint32_t G = (uint32_t)gs.size();
      h->og_ok = G > 0 && G <= kOrderMaxGroups;
      h->n_pad = P;
      if (h->og_ok) {
        uint32_t nbl = 10;  // buckets per group: G * NB <= kOrderMaxGroups entries (LDS)
        while (nbl > 0 && ((size_t)G << nbl) > kOrderMaxGroups) --nbl;
        uint32_t bm = 0;
        while (bm < 32 && (key_or[2] >> bm)) ++bm;
        h->og_groups = G;
        h->og_nb_log2 = nbl;
        h->og_m_shift = bm > nbl ? bm - nbl : 0;
        std::vector<uint32_t> st0(G), stp(G), pad;
        uint32_t a0 = 0, ap = 0;
        for (uint32_t g = 0; g < G; ++g) {
          st0[g] = a0;
          stp[g] = ap;
          a0 += gs[g].count;
          const uint32_t padded = (gs[g].count + kWave - 1) / kWave * kWave;
          // copies of the group's last pod in memory order (largest memory in an ascending
          // -- even -- group, smallest in a descending one): the tail wave's neighbour
          const uint32_t last = (g & 1u) ? gs[g].pod_min : gs[g].pod_max;
          for (uint32_t i = gs[g].count; i < padded; ++i) {
            pad.push_back(ap + i);
            pad.push_back(last);
          }
          ap += padded;
        }
        h->n_pad = ap;
        h->og_n_pad_slots = (uint32_t)(pad.size() / 2);
        h->og_off_start = (size_t)G * 8;
        h->og_off_start_pad = h->og_off_start + (size_t)G * 4;
        h->og_off_pad = h->og_off_start_pad + (size_t)G * 4;
        h->og_host.assign(h->og_off_pad + pad.size() * 4, 0);
        for (uint32_t g = 0; g < G; ++g)
          std::memcpy(h->og_host.data() + (size_t)g * 8, &gs[g].key, 8);
        std::memcpy(h->og_host.data() + h->og_off_start, st0.data(), (size_t)G * 4);
        std::memcpy(h->og_host.data() + h->og_off_start_pad, stp.data(), (size_t)G * 4);
        if (!pad.empty())
          std::memcpy(h->og_host.data() + h->og_off_pad, pad.data(), pad.size() * 4);
        HIP_TRY(h, h->order_meta.ensure(h->og_host.size()));
        HIP_TRY(h, hipMemcpyAsync(h->order_meta.p, h->og_host.data(), h->og_host.size(),
                                  hipMemcpyHostToDevice, h->stream));
        const size_t nbk = (size_t)G << nbl;
        if (h->order_hist.bytes < nbk * 4) {  // the scan clears it after each use
          HIP_TRY(h, h->order_hist.ensure(nbk * 4));
          HIP_TRY(h, hipMemsetAsync(h->order_hist.p, 0, h->order_hist.bytes, h->stream));
        }
        HIP_TRY(h, h->order_bstart.ensure(nbk * 4));
      }
    }
    HIP_TRY(h, hipEventRecord(h->stage_event, h->stream));
    h->stage_pending = true;
    for (int a = 0; a < kPodArrays; ++a) h->pod_off[a] = off[a];
    h->pod_rest_off = core_bytes;
    h->pod_rest_bytes = defer ? total - core_bytes : 0;
    h->rest_lazy = lazy;
    for (int f = 0; f < 3; ++f) {
      uint32_t bits = 0;
      while (bits < 64 && (key_or[f] >> bits)) ++bits;
      h->key_bits[f] = bits;
    }
    h->n_pods = P;
    h->n_work = P;
    h->has_pods = true;
    h->ran = false;
    h->phase1_done = false;
    h->ordered = false;
    h->pods_diskio = pd->rio != nullptr && pd->rcpu != nullptr;
    if (dbg)
      std::fprintf(stderr, "yoda_upload_pods: %u pods, %u threads: pack %.3f merge %.3f copy %.3f "
                   "groups %.3f ms\n", P, n_thr, t_packed - t_start, t_merged - t_packed,
                   t_copied - t_merged, now_ms() - t_copied);
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

// pad: a private run (yoda_run without the bitmask) -- it may take the counting sort and pad
// the order's groups to whole waves; every other entry point keeps the radix order, one
// sorted position per caller pod, reproducible across the shards of a batch.
// batch: a single-handle batch entry point (mode_b_absent).
static int prepare_run(yoda_t* h, int mode, bool pad = false, bool batch = false) {
  int rc = check_ready(h, mode, batch);
  if (rc) return rc;
  h->topk_ready = false;  // this run overwrites the bitmask and reciprocals
  h->draw_stage = 0;      // ... and the outcome a sharded draw would read
  const bool ordering = h->order_enabled && mode == YODA_MODE_SCV &&
                        h->n_pods >= kOrderMinPods && h->n_nodes > 0;
  // a private run takes the counting sort, padded when that adds at most 1/8 of the batch
  // (many small groups would otherwise multiply the work)
  h->count_order = pad && ordering && h->og_ok;
  const bool padded = h->count_order && h->order_pad &&
                      (uint64_t)h->n_pad * 8 <= (uint64_t)h->n_pods * 9;
  h->n_work = padded ? h->n_pad : h->n_pods;
  plan_chunks(h, mode, h->n_work, h->n_nodes);
  // a run on the block kernels (argmax, or the greedy windows' top-k) visits its pod blocks
  // heaviest first (a block's weight: its heaviest wave's PART nodes in K1)
  const uint32_t n_pb = (h->n_work + kBlock - 1) / kBlock;
  h->lpt_sorted = false;
  h->lpt_active = mode == YODA_MODE_SCV && h->path == Path::N32 &&
                  h->has_k1sum && h->has_k2sum && n_pb >= 8 && n_pb <= 4096;
  if (h->lpt_active) {
    const size_t had = h->lpt_w.bytes;
    HIP_TRY(h, h->lpt_w.ensure((size_t)((h->n_work + 63) / 64) * 4));
    HIP_TRY(h, h->lpt_order.ensure((size_t)n_pb * 4));
    if (h->lpt_w.bytes != had)  // fresh weights start at zero (k_lpt_order re-zeroes them)
      HIP_TRY(h, hipMemsetAsync(h->lpt_w.p, 0, h->lpt_w.bytes, h->stream));
  }
  return ensure_state(h, std::max<uint32_t>(h->n_work, 1));
}

// Diagnostic (YODA_SEED_DEBUG): how close the block K1's K2 pruning seeds came to each wave's
// smallest best score (sorted order, before finalize), on stderr.  Never results or policy.
static void seed_report(yoda_t* h) {
  const uint32_t W = h->n_work, nw = (W + 63) / 64;
  std::vector<uint64_t> sd(nw);
  std::vector<int64_t> best(W);
  std::vector<uint32_t> cnt(W);
  const PodParams pp = pod_params(h);
  if (hipMemcpyAsync(sd.data(), pp.seed, nw * 8ull, hipMemcpyDeviceToHost, h->stream) ||
      hipMemcpyAsync(best.data(), h->best.p, W * 8ull, hipMemcpyDeviceToHost, h->stream) ||
      hipMemcpyAsync(cnt.data(), h->counts.p, W * 4ull, hipMemcpyDeviceToHost, h->stream) ||
      hipStreamSynchronize(h->stream))
    return;
  uint32_t zero = 0, bad = 0, act_w = 0, hist[6] = {};
  double gap = 0;
  for (uint32_t w = 0; w < nw; ++w) {
    int64_t mb = INT64_MAX;
    for (uint32_t l = 64 * w; l < std::min(W, 64 * w + 64); ++l)
      if (cnt[l] && best[l] >= 0) mb = std::min(mb, best[l]);
    if (mb == INT64_MAX) continue;
    ++act_w;
    if (sd[w] == 0) { ++zero; continue; }
    if ((int64_t)sd[w] > mb) ++bad;
    const double r = (double)sd[w] / (double)std::max<int64_t>(mb, 1);
    hist[r >= 1.0 ? 5 : r >= 0.99 ? 4 : r >= 0.95 ? 3 : r >= 0.9 ? 2 : r >= 0.75 ? 1 : 0]++;
    gap += (double)(mb - (int64_t)sd[w]);
  }
  std::fprintf(stderr, "seeds: %u waves with a best, %u without a seed, %u ABOVE the best (bug); "
               "seed/best <.75 %u, <.9 %u, <.95 %u, <.99 %u, <1 %u, =1 %u; mean gap %.1f\n",
               act_w, zero, bad, hist[0], hist[1], hist[2], hist[3], hist[4], hist[5],
               gap / std::max<uint32_t>(1, act_w - zero));
}

// The selectHost draw of a private run (yoda_set_tie_draw), after finalize: every per-pod output
// is in the caller's order by now, while the pod arrays, the reciprocals, the masks and the
// lowest scores are still in the run's sorted order (n_work positions, h->perm).
static int draw_pass(yoda_t* h, int mode) {
  const uint32_t W = h->n_work;
  if (W == 0 || h->n_pods == 0 || h->n_nodes == 0) return YODA_OK;
  HIP_TRY(h, h->draw_list.ensure((size_t)W * 4));
  HIP_TRY(h, h->draw_keys.ensure((size_t)W * 8));
  HIP_TRY(h, h->draw_n.ensure(16));
  DrawArgs a{};
  a.perm = h->ordered ? h->perm.as<uint32_t>() : nullptr;
  a.n_work = W;
  a.n_pods = h->n_pods;
  a.status = h->status.as<int32_t>();
  a.ties = h->ties_out.as<uint32_t>();
  a.best = h->best.as<int64_t>();
  a.pick = h->pick.as<int32_t>();
  a.list = h->draw_list.as<uint32_t>();
  a.n_list = h->draw_n.as<uint32_t>();
  a.keys = h->draw_keys.as<unsigned long long>();
  a.seed = h->tie_seed;
  a.pod_base = h->tie_pod_base;
  a.node_offset = h->node_offset;
  const bool diskio = mode == YODA_MODE_DISKIO;
  // (the U64 path's finalize scattered the maxima to the caller's order: unpermute_outputs)
  if (!diskio && h->generic && h->maxima_sorted)
    return fail(h, YODA_ERR_STATE, "draw pass: generic maxima still in sorted order");
  HIP_TRY(h, launch_draw(h->K, h->path, diskio ? 1 : 0, h->nodes.as<unsigned char>(),
                         h->nodes_b.as<NodeRecB>(), h->n_nodes, pod_params(h),
                         h->rcp.as<double>(), h->maxima.as<uint64_t>(), h->lowest.as<int64_t>(),
                         h->bitmask.as<uint64_t>(), bm_row(h->n_nodes), h->bs_ptr(),
                         bs_row(h->n_nodes), h->blk_ptr(), blk_row(h->n_nodes), a,
                         // (Mode B with eligibility: the draw among the top-scored nodes of E)
                         diskio ? modeb_elig_args(h) : DiskEligArgs{}, h->stream));
  return YODA_OK;
}

// yoda_run; draw: the selectHost draw when the handle has it enabled (the greedy batch's own
// runs pass false: it keeps the lowest-node rule).
static int run_private(yoda_t* h, int mode, uint32_t flags, bool draw);

int yoda_run(yoda_t* h, int mode, uint32_t flags) { return run_private(h, mode, flags, true); }

static int run_private(yoda_t* h, int mode, uint32_t flags, bool draw) {
  if (!h) return YODA_ERR_INVALID_ARG;
  // a private run on the block kernels in the counting order reads only the pod arrays the
  // upload copied first; the rest of the batch goes to the device after its kernels
  const bool fast = mode == YODA_MODE_SCV && !(flags & YODA_RUN_BITMASK) &&
                    h->path == Path::N32 && h->has_k1sum && h->has_k2sum && !h->mem_ranks;
  h->fast_run = fast;
  int rc = prepare_run(h, mode, (flags & YODA_RUN_BITMASK) == 0, true);
  h->fast_run = false;
  if (rc) return rc;
  const bool defer = fast && h->count_order;
  if (!defer && (rc = pods_complete(h))) return rc;
  h->core_only = defer;
  try {
    struct Clear {
      bool& f;
      ~Clear() { f = false; }
    } clear{h->core_only}, clear_defer{h->defer_merge2}, clear_merge{h->merge2.on};
    if ((rc = order_pods(h, mode))) return rc;
    if ((rc = phase1(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(),
                     Maxima::OwnFinal)))
      return rc;
    // an ordered run off the generic path merges the K2 partials in finalize's kernel (the seed
    // report reads the merged best scores before finalize: with it on, the two kernels)
    const bool seed_dbg = diag_env("YODA_SEED_DEBUG", 0);
    h->defer_merge2 = mode == YODA_MODE_SCV && h->ordered && !h->generic && !seed_dbg;
    rc = phase2(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>(), nullptr,
                draw && h->tie_draw);
    h->defer_merge2 = false;
    if (rc) return rc;
    if (seed_dbg && pod_params(h).seed) seed_report(h);
    if ((rc = finalize(h, mode, h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                       h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>(),
                       false)))
      return rc;
    // the deferred arrays: packed on the host while the kernels run, copied on the side stream
    // (from the upload's core copy on, so alongside the kernels), joined into the stream
    h->core_only = false;
    if (defer && h->copy_stream && (rc = pods_complete_async(h))) return rc;
    if (defer && (rc = pods_complete(h))) return rc;
    // (a sampled Mode B run drew inside its kernel: the list pass would rescan every node)
    const bool drawn = mode == YODA_MODE_DISKIO && h->b_samp_last;
    if (draw && h->tie_draw && !drawn && (rc = draw_pass(h, mode))) return rc;
    h->ran = true;
    h->diag_done = false;
    h->ran_bitmask = mode == YODA_MODE_SCV && (flags & YODA_RUN_BITMASK);
    h->last_mode = mode;
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_download(yoda_t* h, yoda_eval_out* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  if (!h->ran) return fail(h, YODA_ERR_STATE, "yoda_download before yoda_run/finalize");
  if (h->k3_pending)  // picks of the flagged pods unresolved, outputs still in sorted order
    return fail(h, YODA_ERR_STATE,
                "exact normalize pending: run yoda_shard_exact_records / yoda_shard_exact_merge");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t P = h->n_pods;
    if (P == 0) return YODA_OK;
    hipStream_t s = h->stream;
    if (out->pick)
      HIP_TRY(h, hipMemcpyAsync(out->pick, h->pick.p, P * 4ull, hipMemcpyDeviceToHost, s));
    if (out->status)
      HIP_TRY(h, hipMemcpyAsync(out->status, h->status.p, P * 4ull, hipMemcpyDeviceToHost, s));
    if (out->n_feasible)
      HIP_TRY(h, hipMemcpyAsync(out->n_feasible, h->counts.p, P * 4ull, hipMemcpyDeviceToHost, s));
    if (out->n_ties)
      HIP_TRY(h, hipMemcpyAsync(out->n_ties, h->ties_out.p, P * 4ull, hipMemcpyDeviceToHost, s));
    std::vector<int64_t> top;
    std::vector<int32_t> st;
    if (out->top_score) {
      top.resize(P);
      st.resize(P);
      HIP_TRY(h, hipMemcpyAsync(top.data(), h->best.p, P * 8ull, hipMemcpyDeviceToHost, s));
      HIP_TRY(h, hipMemcpyAsync(st.data(), h->status.p, P * 4ull, hipMemcpyDeviceToHost, s));
    }
    std::vector<uint64_t> mx;
    if (out->maxima && h->maxima_sorted) {  // scatter the maxima to the caller's order now
      const uint32_t W = h->n_work;
      HIP_TRY(h, h->maxima_alt.ensure(h->maxima.bytes));
      PermTable t{};
      for (uint32_t r = 0; r < 6; ++r) {
        t.src[t.n] = h->maxima.as<unsigned char>() + (size_t)r * W * 8;
        t.dst[t.n] = h->maxima_alt.as<unsigned char>() + (size_t)r * P * 8;
        t.bytes[t.n] = 8;
        ++t.n;
      }
      HIP_TRY(h, launch_permute(t, h->perm.as<uint32_t>(), W, true, s));
      h->maxima.swap(h->maxima_alt);
      h->maxima_sorted = false;
    }
    if (out->maxima) {
      mx.resize(6 * (size_t)P);
      HIP_TRY(h, hipMemcpyAsync(mx.data(), h->maxima.p, mx.size() * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    if (out->top_score)
      for (uint32_t p = 0; p < P; ++p) out->top_score[p] = st[p] == YODA_STATUS_OK ? top[p] : 0;
    if (out->maxima)
      for (uint32_t p = 0; p < P; ++p)
        for (int f = 0; f < 6; ++f) out->maxima[(size_t)p * 6 + f] = mx[(size_t)f * P + p];
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_download_bitmask(yoda_t* h, uint32_t* words, uint64_t n_words) {
  if (!h || !words) return YODA_ERR_INVALID_ARG;
  if (!h->ran_bitmask)
    return fail(h, YODA_ERR_STATE, "no bitmask: run Mode A with YODA_RUN_BITMASK first");
  const uint32_t W = (h->n_nodes + 31) / 32;
  const uint64_t need = (uint64_t)W * h->n_pods;
  if (n_words < need) return fail(h, YODA_ERR_INVALID_ARG, "bitmask buffer too small");
  if (need == 0) return YODA_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, h->bitmask_t.ensure(need * 4));
  HIP_TRY(h, launch_bitmask_transpose(h->bitmask.as<uint64_t>(), bm_row(h->n_nodes), h->bs_ptr(),
                                      bs_row(h->n_nodes), h->blk_ptr(), blk_row(h->n_nodes),
                                      h->n_nodes,
                                      W, h->n_pods,
                                      h->ordered ? h->perm.as<uint32_t>() : nullptr,
                                      h->bitmask_t.as<uint32_t>(), h->stream));
  HIP_TRY(h, hipMemcpyAsync(words, h->bitmask_t.p, need * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return YODA_OK;
}

int yoda_score_rows(yoda_t* h, int mode, uint32_t* bitmask_out, uint64_t n_bitmask_words,
                    int64_t* scores_out, uint64_t n_scores) {
  return yoda_score_rows_norm(h, mode, bitmask_out, n_bitmask_words, scores_out, n_scores,
                              nullptr, 0);
}

int yoda_score_rows_norm(yoda_t* h, int mode, uint32_t* bitmask_out, uint64_t n_bitmask_words,
                         int64_t* scores_out, uint64_t n_scores, int64_t* norm_out,
                         uint64_t n_norm) {
  int rc = prepare_run(h, mode, false, true);
  if (rc) return rc;
  try {
    const uint32_t P = h->n_pods, N = h->n_nodes;
    const uint64_t W = (N + 31) / 32;
    if (bitmask_out && n_bitmask_words < W * P)
      return fail(h, YODA_ERR_INVALID_ARG, "bitmask buffer too small");
    if (scores_out && n_scores < (uint64_t)N * P)
      return fail(h, YODA_ERR_INVALID_ARG, "scores buffer too small");
    if (norm_out && n_norm < (uint64_t)N * P)
      return fail(h, YODA_ERR_INVALID_ARG, "norm buffer too small");
    if ((uint64_t)N * P > (1ull << 31))
      return fail(h, YODA_ERR_RANGE, "yoda_score_rows is for small pod batches (P*N <= 2^31)");
    int64_t* rows = nullptr;
    if ((scores_out || norm_out) && (uint64_t)N * P > 0) {
      HIP_TRY(h, h->rows.ensure((size_t)N * P * 8));
      HIP_TRY(h, h->rows_t.ensure((size_t)N * P * 8));
      HIP_TRY(h, hipMemsetAsync(h->rows.p, 0xff, (size_t)N * P * 8, h->stream));  // -1
      rows = h->rows.as<int64_t>();
    }
    if ((rc = order_pods(h, mode))) return rc;
    if ((rc = phase1(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(), Maxima::Own)))
      return rc;
    if ((rc = phase2(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                     h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>(),
                     rows)))
      return rc;
    if (norm_out && rows) {  // before finalize: best / lowest still in the rows' pod order
      HIP_TRY(h, h->norm.ensure((size_t)N * P * 8));
      HIP_TRY(h, launch_norm_rows(rows, N, P, h->best.as<int64_t>(), h->lowest.as<int64_t>(),
                                  h->norm.as<int64_t>(), h->stream));
    }
    if ((rc = finalize(h, mode, h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                       h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>(),
                       false)))
      return rc;
    h->ran = true;
    h->diag_done = false;
    h->ran_bitmask = mode == YODA_MODE_SCV;
    h->last_mode = mode;
    if (rows && scores_out) {
      HIP_TRY(h, launch_rows_transpose(rows, N, P, h->ordered ? h->perm.as<uint32_t>() : nullptr,
                                       h->rows_t.as<int64_t>(), h->stream));
      HIP_TRY(h, hipMemcpyAsync(scores_out, h->rows_t.p, (size_t)N * P * 8,
                                hipMemcpyDeviceToHost, h->stream));
      if (norm_out) HIP_TRY(h, hipStreamSynchronize(h->stream));  // rows_t is reused below
    }
    if (rows && norm_out) {
      HIP_TRY(h, launch_rows_transpose(h->norm.as<int64_t>(), N, P,
                                       h->ordered ? h->perm.as<uint32_t>() : nullptr,
                                       h->rows_t.as<int64_t>(), h->stream));
      HIP_TRY(h, hipMemcpyAsync(norm_out, h->rows_t.p, (size_t)N * P * 8, hipMemcpyDeviceToHost,
                                h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (bitmask_out && W * P > 0) {
      if (mode == YODA_MODE_DISKIO && modeb_sampled(h)) {
        // S: E from the host mirrors, cut by the plan's walk records
        const bool el = modeb_elig_on(h), keyed = modeb_keyed(h);
        std::vector<DiskWalk> wk(P);
        HIP_TRY(h, hipMemcpyAsync(wk.data(), h->b_walk.p, (size_t)P * sizeof(DiskWalk),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        std::memset(bitmask_out, 0, (size_t)(W * P) * 4);
        for (uint64_t p = 0; p < P; ++p) {
          const uint32_t sel = keyed ? disk_sel(h->h_cls[p]) : kDiskSelAny;
          for (uint32_t n = 0; n < N; ++n) {
            if (!disk_in_walk(n, wk[p])) continue;
            if (el) {
              const DiskElig e =
                  disk_elig_of(!h->h_absent[n], h->cand_classes ? h->h_cand[n] : ~0ull);
              if (!disk_eligible(e, sel)) continue;
            }
            bitmask_out[p * W + (n >> 5)] |= 1u << (n & 31u);
          }
        }
      } else if (mode == YODA_MODE_DISKIO && modeb_elig_on(h)) {  // E, from the host mirrors
        const bool keyed = modeb_keyed(h);
        std::memset(bitmask_out, 0, (size_t)(W * P) * 4);
        for (uint64_t p = 0; p < P; ++p) {
          const uint32_t sel = keyed ? disk_sel(h->h_cls[p]) : kDiskSelAny;
          for (uint32_t n = 0; n < N; ++n) {
            const DiskElig e = disk_elig_of(!h->h_absent[n], h->cand_classes ? h->h_cand[n] : ~0ull);
            if (disk_eligible(e, sel)) bitmask_out[p * W + (n >> 5)] |= 1u << (n & 31u);
          }
        }
      } else if (mode == YODA_MODE_DISKIO) {  // Filter is a pass-through: every node feasible
        for (uint64_t p = 0; p < P; ++p)
          for (uint64_t w = 0; w < W; ++w) {
            const uint32_t bits = (w + 1) * 32 <= N ? 0xffffffffu : ((1u << (N % 32)) - 1);
            bitmask_out[p * W + w] = bits;
          }
      } else if ((rc = yoda_download_bitmask(h, bitmask_out, n_bitmask_words))) {
        return rc;
      }
    }
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

// ---- Filter diagnosis ----------------------------------------------------------------------
static_assert(YODA_REASON_NONE == kReasonNone && YODA_REASON_NUMBER == kReasonNumber &&
                  YODA_REASON_MEMORY == kReasonMemory && YODA_REASON_CLOCK == kReasonClock &&
                  YODA_REASON_NOT_CANDIDATE == kReasonNotCandidate &&
                  YODA_REASON_ABSENT == kReasonAbsent,
              "the kernels' reason codes are the header's");

// The sweep's inputs: the pod arrays of the upload (caller order; the record path's thresholds,
// those K1 reads through the run's order), the base records, the candidate state.
static DiagArgs diag_args(yoda_t* h) {
  DiagArgs a{};
  const unsigned char* b = h->pod_blob.as<unsigned char>();
  const size_t* off = h->pod_off;
  a.nodes = h->nodes.as<unsigned char>();
  a.n_nodes = h->n_nodes;
  a.n_pods = h->n_pods;
  switch (h->path) {
    case Path::N32: a.m = b + off[kPodM32]; a.c = b + off[kPodC32]; break;
    case Path::F64: a.m = b + off[kPodMF]; a.c = b + off[kPodCF]; break;
    case Path::U64: a.m = b + off[kPodMU]; a.c = b + off[kPodCU]; break;
  }
  a.number = reinterpret_cast<const uint64_t*>(b + off[kPodNumber]);
  a.need_mem = reinterpret_cast<const uint32_t*>(b + off[kPodNeedMem]);
  a.need_clk = reinterpret_cast<const uint32_t*>(b + off[kPodNeedClk]);
  if (h->cand_classes) {
    a.cand_w = h->cand_w.as<uint64_t>();
    a.cls = h->h_cls.empty() ? nullptr : h->cand_cls.as<uint8_t>() + h->cls_off;
  }
  return a;
}

int yoda_diagnose(yoda_t* h, uint32_t flags) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (flags & ~YODA_DIAG_ALL) return fail(h, YODA_ERR_INVALID_ARG, "yoda_diagnose: unknown flag bits");
  // (the default selection -- the pods with no feasible node -- had every node visited)
  if (flags & YODA_DIAG_ALL)
    if (int rc = samp_refuse(h, "yoda_diagnose with YODA_DIAG_ALL")) return rc;
  if (!h->ran || !h->has_nodes || !h->has_pods)
    return fail(h, YODA_ERR_STATE, "yoda_diagnose: no completed run is pending");
  if (h->k3_pending)
    return fail(h, YODA_ERR_STATE,
                "exact normalize pending: run yoda_shard_exact_records / yoda_shard_exact_merge");
  if (h->last_mode != YODA_MODE_SCV)
    return fail(h, YODA_ERR_STATE, "yoda_diagnose: Mode B has no Filter (the rejected nodes are "
                                   "n_nodes - absent - n_feasible)");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = pods_complete(h);  // (the f64 / u64 thresholds of a deferred upload)
    if (rc) return rc;
    const uint32_t P = h->n_pods;
    h->diag_done = false;
    if (P == 0) {
      h->diag_done = true;
      return YODA_OK;
    }
    HIP_TRY(h, h->diag_list.ensure((size_t)P * 4));
    HIP_TRY(h, h->diag_n.ensure(16));
    HIP_TRY(h, h->diag_counts.ensure((size_t)P * 16));
    HIP_TRY(h, hipMemsetAsync(h->diag_n.p, 0, 16, h->stream));
    HIP_TRY(h, launch_diag_select(h->counts.as<uint32_t>(), P, (flags & YODA_DIAG_ALL) != 0,
                                  h->diag_list.as<uint32_t>(), h->diag_n.as<uint32_t>(),
                                  h->diag_counts.as<uint32_t>(), h->stream));
    DiagArgs a = diag_args(h);
    a.list = h->diag_list.as<uint32_t>();
    a.n_list = h->diag_n.as<uint32_t>();
    a.counts = h->diag_counts.as<uint32_t>();
    HIP_TRY(h, launch_diagnose(h->K, h->path, false, a, h->stream));
    h->diag_done = true;
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_download_diagnosis(yoda_t* h, uint32_t* counts, uint64_t n_counts) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!counts) return fail(h, YODA_ERR_INVALID_ARG, "NULL counts buffer");
  if (!h->ran || !h->diag_done || h->k3_pending || h->last_mode != YODA_MODE_SCV)
    return fail(h, YODA_ERR_STATE, "yoda_download_diagnosis before this run's yoda_diagnose");
  if (n_counts != 4ull * h->n_pods)
    return fail(h, YODA_ERR_INVALID_ARG, "yoda_download_diagnosis: n_counts is not 4 * n_pods");
  if (h->n_pods == 0) return YODA_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(counts, h->diag_counts.p, (size_t)h->n_pods * 16,
                            hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return YODA_OK;
}

int yoda_reason_rows(yoda_t* h, uint8_t* reasons, uint64_t n_reasons) {
  if (!h) return YODA_ERR_INVALID_ARG;
  // (a node past the cut was never visited: it has no Filter verdict to report)
  int rc = samp_refuse(h, "yoda_reason_rows");
  if (rc) return rc;
  if ((rc = check_ready(h, YODA_MODE_SCV, true))) return rc;
  if (!reasons) return fail(h, YODA_ERR_INVALID_ARG, "NULL reasons buffer");
  const uint32_t P = h->n_pods, N = h->n_nodes;
  if (n_reasons != (uint64_t)P * N)
    return fail(h, YODA_ERR_INVALID_ARG, "yoda_reason_rows: n_reasons is not n_pods * n_nodes");
  if ((uint64_t)N * P > (1ull << 31))
    return fail(h, YODA_ERR_RANGE, "yoda_reason_rows is for small pod batches (P*N <= 2^31)");
  // what yoda_score_rows invalidates: the pending run, phase-1, top-k and draw state
  h->ran = false;
  h->ran_bitmask = false;
  h->diag_done = false;
  h->phase1_done = false;
  h->k3_pending = false;
  h->topk_ready = false;
  h->draw_stage = 0;
  if ((uint64_t)N * P == 0) return YODA_OK;
  try {
    const size_t stride = ((size_t)N + 63) / 64 * 64;
    HIP_TRY(h, h->diag_rows.ensure(stride * P));
    HIP_TRY(h, h->diag_stage.ensure(stride * P));
    DiagArgs a = diag_args(h);
    a.rows = h->diag_rows.as<unsigned char>();
    a.row_stride = (uint32_t)stride;
    HIP_TRY(h, launch_diagnose(h->K, h->path, true, a, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->diag_stage.p, h->diag_rows.p, stride * P, hipMemcpyDeviceToHost,
                              h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const unsigned char* st = static_cast<const unsigned char*>(h->diag_stage.p);
    for (uint32_t p = 0; p < P; ++p) std::memcpy(reasons + (size_t)p * N, st + p * stride, N);
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_eval(yoda_t* h, const yoda_pod_soa* pods, int mode, yoda_eval_out* out) {
  if (!h) return YODA_ERR_INVALID_ARG;
  int rc = mode_b_absent(h, mode, true);  // (before the pods are replaced)
  if (rc) return rc;
  if ((rc = yoda_upload_pods(h, pods))) return rc;
  if ((rc = yoda_run(h, mode, 0))) return rc;
  return yoda_download(h, out);
}

int yoda_set_tie_draw(yoda_t* h, int enable, uint64_t seed, uint64_t pod_base) {
  if (!h) return YODA_ERR_INVALID_ARG;
  h->tie_draw = enable != 0;
  h->tie_seed = seed;
  h->tie_pod_base = pod_base;
  return YODA_OK;
}

uint32_t yoda_tie_hash(uint64_t seed, uint64_t pod, uint32_t node) {
  return tie_word(tie_pod_state(seed, pod), node);
}

// ---- the draw of a node-sharded step ----------------------------------------------------
int yoda_shard_tie_draw(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  h->shard_draw = enable != 0;
  return YODA_OK;
}

// The state both passes need: a completed sharded step of this mode, with the draw enabled.
static int shard_draw_ready(yoda_t* h, const char* what) {
  const std::string w(what);
  if (!h->shard_draws())
    return fail(h, YODA_ERR_STATE, w + ": the draw is disabled (yoda_set_tie_draw and "
                                       "yoda_shard_tie_draw enable it)");
  if (!h->has_nodes || !h->has_pods || !h->ran || h->draw_stage == 0)
    return fail(h, YODA_ERR_STATE, w + " needs a completed yoda_shard_finalize / yoda_comm_run "
                                       "of this batch");
  if (h->k3_pending)
    return fail(h, YODA_ERR_STATE,
                w + ": exact normalize pending: run yoda_shard_exact_records / "
                    "yoda_shard_exact_merge first");
  return YODA_OK;
}

// The finalized outcome is in the caller's order by now and GLOBAL; the pod arrays, reciprocals,
// masks and lowest scores are in the step's sorted order, as draw_pass finds them.
static DrawArgs shard_draw_args(yoda_t* h) {
  DrawArgs a{};
  a.perm = h->ordered ? h->perm.as<uint32_t>() : nullptr;
  a.n_work = h->n_work;
  a.n_pods = h->n_pods;
  a.status = h->status.as<int32_t>();
  a.ties = h->ties_out.as<uint32_t>();
  a.best = h->best.as<int64_t>();
  a.pick = h->pick.as<int32_t>();
  a.list = h->draw_list.as<uint32_t>();
  a.n_list = h->draw_n.as<uint32_t>();
  a.seed = h->tie_seed;
  a.pod_base = h->tie_pod_base;
  a.node_offset = h->node_offset;
  a.norm_top = h->norm_top.as<int64_t>();
  return a;
}

int yoda_shard_draw_keys(yoda_t* h, int mode, uint64_t* d_keys) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!d_keys) return fail(h, YODA_ERR_INVALID_ARG, "NULL key buffer");
  if (mode != YODA_MODE_SCV && mode != YODA_MODE_DISKIO)
    return fail(h, YODA_ERR_INVALID_ARG, "mode must be YODA_MODE_SCV or YODA_MODE_DISKIO");
  int rc = cand_refuse(h, "yoda_shard_draw_keys", true);
  if (rc) return rc;
  if ((rc = mode_b_absent(h, mode))) return rc;
  if ((rc = shard_draw_ready(h, "yoda_shard_draw_keys"))) return rc;
  if (mode != h->last_mode)
    return fail(h, YODA_ERR_STATE, "yoda_shard_draw_keys: the step ran in the other mode");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t W = h->n_work;
    if (W == 0 || h->n_pods == 0) {
      h->draw_stage = 2;
      return YODA_OK;
    }
    const bool diskio = mode == YODA_MODE_DISKIO;
    if (!diskio && h->generic && h->maxima_sorted)
      return fail(h, YODA_ERR_STATE, "draw keys: generic maxima still in sorted order");
    HIP_TRY(h, h->draw_list.ensure((size_t)W * 4));
    HIP_TRY(h, h->draw_n.ensure(16));
    // (k_merge3_top filled it for the pods the exact merge handled; the key kernel reads no
    // other entry)
    if (!diskio && h->generic) HIP_TRY(h, h->norm_top.ensure((size_t)W * 8));
    DrawArgs a = shard_draw_args(h);
    a.keys = reinterpret_cast<unsigned long long*>(d_keys);
    HIP_TRY(h, launch_shard_draw_keys(
                   h->K, h->path, diskio ? 1 : 0, h->nodes.as<unsigned char>(),
                   h->nodes_b.as<NodeRecB>(), h->n_nodes, pod_params(h), h->rcp.as<double>(),
                   h->maxima.as<uint64_t>(), h->lowest.as<int64_t>(), h->bitmask.as<uint64_t>(),
                   bm_row(h->n_nodes), h->bs_ptr(), bs_row(h->n_nodes), h->blk_ptr(),
                   blk_row(h->n_nodes), a, h->stream));
    h->draw_stage = 2;
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_draw_apply(yoda_t* h, const uint64_t* d_keys) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!d_keys) return fail(h, YODA_ERR_INVALID_ARG, "NULL key buffer");
  int rc = cand_refuse(h, "yoda_shard_draw_apply", true);
  if (rc) return rc;
  if ((rc = shard_draw_ready(h, "yoda_shard_draw_apply"))) return rc;
  if (h->draw_stage != 2)
    return fail(h, YODA_ERR_STATE, "yoda_shard_draw_apply before this step's yoda_shard_draw_keys");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, launch_shard_draw_apply(shard_draw_args(h), d_keys, h->stream));
  h->draw_stage = 1;  // applied: another apply needs another key pass
  return YODA_OK;
}

// ---- sharded entry points -------------------------------------------------------------
int yoda_shard_exchange_order(yoda_t* h, int caller_order) {
  if (!h || (caller_order != 0 && caller_order != 1)) return YODA_ERR_INVALID_ARG;
  h->xo_enabled = caller_order == 1;
  return YODA_OK;
}

int yoda_shard_phase1(yoda_t* h, int mode, uint64_t* d_maxima, uint32_t* d_counts) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_phase1", true)) return rc;
  // caller-order exchange (yoda_shard_exchange_order): each shard its private order; not on the
  // U64 path (its exact-normalize records are per sorted position)
  h->xo = h->xo_enabled && !h->generic;
  int rc = prepare_run(h, mode, h->xo);
  if (rc) return rc;
  if (!d_maxima || !d_counts) return fail(h, YODA_ERR_INVALID_ARG, "NULL exchange buffer");
  try {
    if ((rc = order_pods(h, mode))) return rc;
    if (h->xo) {
      if ((rc = phase1(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>()))) return rc;
      if ((rc = xfer(h, true, {{h->maxima.p, d_maxima, 6, 8}, {h->counts.p, d_counts, 2, 4}})))
        return rc;
    } else if ((rc = phase1(h, mode, d_maxima, d_counts))) {
      return rc;
    }
    h->phase1_done = true;
    h->phase1_wit = false;
    h->ran = false;
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_phase2(yoda_t* h, int mode, const uint64_t* d_maxima, const uint32_t* d_counts,
                      int64_t* d_best, uint32_t* d_idx, uint32_t* d_ties, int64_t* d_lowest) {
  if (!h) return YODA_ERR_INVALID_ARG;
  int rc = cand_refuse(h, "yoda_shard_phase2", true);
  if (rc) return rc;
  if ((rc = check_ready(h, mode))) return rc;
  if (!h->phase1_done) return fail(h, YODA_ERR_STATE, "yoda_shard_phase2 before phase1");
  if (!d_maxima || !d_counts || !d_best || !d_idx || !d_ties || !d_lowest)
    return fail(h, YODA_ERR_INVALID_ARG, "NULL exchange buffer");
  try {
    const uint32_t P = h->n_pods;
    if (h->xo) {  // the reduced caller-order buffers into this run's order, and back
      int rc2 = xfer(h, false, {{h->maxima.p, const_cast<uint64_t*>(d_maxima), 6, 8},
                                {h->counts.p, const_cast<uint32_t*>(d_counts), 2, 4}});
      if (rc2) return rc2;
      if ((rc2 = phase2(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(),
                        h->best.as<int64_t>(), h->idx.as<uint32_t>(), h->ties.as<uint32_t>(),
                        h->lowest.as<int64_t>())))
        return rc2;
      return xfer(h, true, {{h->best.p, d_best, 1, 8}, {h->idx.p, d_idx, 1, 4},
                            {h->ties.p, d_ties, 1, 4}, {h->lowest.p, d_lowest, 1, 8}});
    }
    // keep the reduced maxima for download and the generic exact-normalize pass
    if (P) HIP_TRY(h, hipMemcpyAsync(h->maxima.p, d_maxima, 6ull * P * 8, hipMemcpyDeviceToDevice,
                                     h->stream));
    return phase2(h, mode, h->maxima.as<uint64_t>(), d_counts, d_best, d_idx, d_ties, d_lowest);
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_prepare_merge(yoda_t* h, const int64_t* d_best_global, const int64_t* d_best_local,
                             uint32_t* d_idx, uint32_t* d_ties) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_prepare_merge", true)) return rc;
  if (!d_best_global || !d_best_local || !d_idx || !d_ties)
    return fail(h, YODA_ERR_INVALID_ARG, "NULL exchange buffer");
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->n_pods == 0) return YODA_OK;
  HIP_TRY(h, launch_merge_prepare(d_best_global, d_best_local, h->n_pods, d_idx, d_ties,
                                  h->stream));
  return YODA_OK;
}

int yoda_shard_finalize(yoda_t* h, int mode, const uint32_t* d_counts, const int64_t* d_best,
                        const uint32_t* d_idx, const uint32_t* d_ties, const int64_t* d_lowest) {
  if (!h) return YODA_ERR_INVALID_ARG;
  int rc = cand_refuse(h, "yoda_shard_finalize", true);
  if (rc) return rc;
  if ((rc = check_ready(h, mode))) return rc;
  if (!d_counts || !d_best || !d_idx || !d_ties || !d_lowest)
    return fail(h, YODA_ERR_INVALID_ARG, "NULL exchange buffer");
  try {
    const uint32_t P = h->n_pods;
    if (h->xo) {  // the merged caller-order buffers into this run's order
      if ((rc = xfer(h, false, {{h->counts.p, const_cast<uint32_t*>(d_counts), 2, 4},
                                {h->best.p, const_cast<int64_t*>(d_best), 1, 8},
                                {h->idx.p, const_cast<uint32_t*>(d_idx), 1, 4},
                                {h->ties.p, const_cast<uint32_t*>(d_ties), 1, 4},
                                {h->lowest.p, const_cast<int64_t*>(d_lowest), 1, 8}})))
        return rc;
      if ((rc = finalize(h, mode, h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                         h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>(),
                         true)))
        return rc;
    } else {
      if (P) {
        HIP_TRY(h, hipMemcpyAsync(h->counts.p, d_counts, 2ull * P * 4, hipMemcpyDeviceToDevice,
                                  h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->best.p, d_best, P * 8ull, hipMemcpyDeviceToDevice, h->stream));
        // the sharded draw's U64 key pass repeats finalize's normalize test on the GLOBAL lowest
        if (h->shard_draws() && h->generic && d_lowest != h->lowest.p)
          HIP_TRY(h, hipMemcpyAsync(h->lowest.p, d_lowest, P * 8ull, hipMemcpyDeviceToDevice,
                                    h->stream));
      }
      if ((rc = finalize(h, mode, h->counts.as<uint32_t>(), h->best.as<int64_t>(), d_idx, d_ties,
                         d_lowest, true)))
        return rc;
    }
    h->ran = true;
    h->diag_done = false;
    h->ran_bitmask = false;
    h->last_mode = mode;
    h->draw_stage = 1;
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_exact_records(yoda_t* h, void* d_rec) {
  if (!h || !d_rec) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_exact_records", true)) return rc;
  if (!h->k3_pending) return fail(h, YODA_ERR_STATE, "no exact-normalize pods pending");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(d_rec, h->k3rec.p, (size_t)h->n_work * sizeof(ShardRec),
                            hipMemcpyDeviceToDevice, h->stream));
  return YODA_OK;
}

int yoda_shard_exact_merge(yoda_t* h, const void* d_all, int world) {
  if (!h || !d_all || world < 1) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_exact_merge", true)) return rc;
  if (!h->k3_pending) return fail(h, YODA_ERR_STATE, "no exact-normalize pods pending");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_merge3(static_cast<const ShardRec*>(d_all), h->n_work, (uint32_t)world,
                             h->flagged.as<uint32_t>(), h->n_flagged.as<uint32_t>(), h->k3_nfl,
                             h->pick.as<int32_t>(), h->status.as<int32_t>(),
                             h->ties_out.as<uint32_t>(), h->stream));
    if (h->shard_draws()) {  // the draw's key pass compares against the GLOBAL top normalized
      HIP_TRY(h, h->norm_top.ensure((size_t)h->n_work * 8));
      HIP_TRY(h, launch_merge3_top(static_cast<const ShardRec*>(d_all), h->n_work, (uint32_t)world,
                                   h->flagged.as<uint32_t>(), h->n_flagged.as<uint32_t>(),
                                   h->k3_nfl, h->norm_top.as<int64_t>(), h->stream));
    }
    h->k3_pending = false;
    return unpermute_outputs(h);
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_overflow_count(yoda_t* h, uint32_t* n_pods) {
  if (!h || !n_pods) return YODA_ERR_INVALID_ARG;
  *n_pods = 0;
  if (!h->generic || !h->n_flagged.p) return YODA_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(n_pods, h->n_flagged.p, 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return YODA_OK;
}

int yoda_order_info(const yoda_t* h, uint32_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  out[0] = h->og_ok ? h->og_groups : 0u;
  out[1] = h->n_pad;
  out[2] = h->n_work;
  out[3] = h->ordered ? (h->count_order ? 2u : 1u) : 0u;
  return YODA_OK;
}

int yoda_node_order(const yoda_t* h, uint32_t* grouped) {
  if (!h || !grouped) return YODA_ERR_INVALID_ARG;
  *grouped = h->perm_on ? 1u : 0u;
  return YODA_OK;
}

int yoda_set_pod_order(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (enable < 0 || enable > 2) return fail(h, YODA_ERR_INVALID_ARG, "enable must be 0, 1 or 2");
  h->order_enabled = enable != 0;
  h->order_pad = enable == 1;
  return YODA_OK;
}

int yoda_class_stats_enable(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  if (enable && !h->class_stats) {
    // YODA_K2_TRACE=<(wave, chunk) slots>: K2 also records per-(wave, chunk) timings
    const uint32_t tr = diag_env("YODA_K2_TRACE", 0);
    const size_t bytes = (16 + 4 * (size_t)tr) * 8;
    HIP_TRY(h, h->stats_dev.ensure(bytes));
    HIP_TRY(h, hipMemsetAsync(h->stats_dev.p, 0, bytes, h->stream));
    if (tr) {  // YODA_K1_TRACE set: the K1 records it instead of the K2
      // low byte: which kernel traces; above it the slot count (the kernels bound the index)
      const uint64_t one = (diag_env("YODA_K1_TRACE", 0) ? 2 : 1) | ((uint64_t)tr << 8);
      HIP_TRY(h, hipMemcpyAsync(h->stats_dev.as<uint64_t>() + 15, &one, 8,
                                hipMemcpyHostToDevice, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->stats_pairs1 = h->stats_pairs2 = 0;
  }
  h->class_stats = enable != 0;
  return YODA_OK;
}

int yoda_class_stats_read(yoda_t* h, uint64_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  for (int i = 0; i < 18; ++i) out[i] = 0;
  if (!h->stats_dev.p) return YODA_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  uint64_t d[16] = {};
  HIP_TRY(h, hipMemcpyAsync(d, h->stats_dev.p, 16 * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  out[0] = d[0];                                                   // K1 ALL
  out[1] = d[1];                                                   // K1 NONE
  out[2] = h->stats_pairs1 - std::min(h->stats_pairs1, d[0] + d[1]);  // K1 PART
  out[3] = d[2];                                                   // K2 U
  out[4] = d[3];                                                   // K2 FAST
  out[5] = d[4];                                                   // K2 EXACT
  out[6] = h->stats_pairs2 - std::min(h->stats_pairs2, d[2] + d[3] + d[4]);  // K2 skipped
  out[7] = d[5];                                                   // K2 (wave, chunk)s, uniform
  out[8] = d[6];                                                   // K2 (wave, chunk)s
  out[9] = h->stats_pairs1;
  out[10] = d[7];                                                  // K2 FAST via node records
  out[11] = d[8];                                                  // K2 per-pod, non-uniform
  out[12] = d[9];                                                  // max per-pod nodes/(w, c)
  out[13] = d[10];                                                 // K1 (w, block)s all NONE
  out[14] = d[11];                                                 // K1 (w, block)s all ALL
  out[15] = d[12];                                                 // K1 (w, block)s
  out[16] = d[13];                                                 // K2 (w, block)s pruned
  out[17] = d[14];                                                 // K2 (w, block)s worked
  HIP_TRY(h, hipMemsetAsync(h->stats_dev.p, 0, 15 * 8, h->stream));
  h->stats_pairs1 = h->stats_pairs2 = 0;
  return YODA_OK;
}

int yoda_k2_trace_read(yoda_t* h, uint64_t* out, uint64_t n_slots) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  if (!h->stats_dev.p || h->stats_dev.bytes < (16 + 4 * n_slots) * 8) return YODA_ERR_INVALID_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(out, h->stats_dev.as<uint64_t>() + 16, 4 * n_slots * 8,
                            hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return YODA_OK;
}

int yoda_profile(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  h->profiling = enable != 0;
  return YODA_OK;
}

int yoda_profile_read(yoda_t* h, double* k1_ms, double* k2_ms, uint32_t* n_launches) {
  if (!h) return YODA_ERR_INVALID_ARG;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  double t1 = 0, t2 = 0;
  for (auto& pr : h->ev_k1) {
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, pr.first, pr.second));
    t1 += ms;
  }
  for (auto& pr : h->ev_k2) {
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, pr.first, pr.second));
    t2 += ms;
  }
  for (auto& pr : h->ev_cand) {
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, pr.first, pr.second));
    h->cand_ms += ms;
  }
  for (auto& pr : h->ev_samp) {
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, pr.first, pr.second));
    h->samp_ms += ms;
  }
  if (k1_ms) *k1_ms = t1;
  if (k2_ms) *k2_ms = t2;
  if (n_launches) *n_launches = (uint32_t)h->ev_k2.size();
  h->ev_k1.clear();
  h->ev_k2.clear();
  h->ev_cand.clear();
  h->ev_samp.clear();
  h->ev_used = 0;
  return YODA_OK;
}

namespace {

// A static score as the record header holds it: f64 bits on the fast paths.
uint64_t stat_bits(const yoda_t* h, uint64_t s) {
  if (h->generic) return s;
  const double d = (double)s;
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

// The one node-state push: the static score (Allocate + Actual) and CardNumber of `cnt` LOCAL
// nodes (each at most once) go to the device (k_set_static).
// The host copies are the caller's business: yoda_set_node_state keeps them current, the greedy
// batch on one handle restores the device at its end instead.
// mapped: k_set_static reads the pinned staging pages itself, else a device copy of them.  The
// greedy batch's pushes are mapped: a few nodes, and the host waits for the kernel behind them,
// so the copy's own launch is what counts (config 5 with them copied: flags 0 0.248 -> 0.252 s,
// capacity 0.932 -> 0.943 s).  yoda_set_node_state's are copied: lists of any size, read over the
// link one entry per thread (14.6 vs 17.6 us a call at 256 entries, equal from 4096 on;
// profiles/greedy_session/ab.txt).
int push_node_state(yoda_t* h, uint32_t cnt, const uint32_t* loc, const uint64_t* stat,
                    const uint64_t* card_number, bool mapped) {
  if (cnt == 0) return YODA_OK;
  // one pinned staging copy: [node u32 x cnt | pad | static u64 x cnt | CardNumber u64 x cnt]
  const size_t o_val = ((size_t)cnt * 4 + 15) / 16 * 16, o_cn = o_val + (size_t)cnt * 8;
  const size_t bytes = o_cn + (size_t)cnt * 8;
  if (h->upd_pending) HIP_TRY(h, hipEventSynchronize(h->upd_event));
  HIP_TRY(h, h->upd_stage.ensure(bytes));
  unsigned char* st = static_cast<unsigned char*>(h->upd_stage.p);
  uint32_t* nd = reinterpret_cast<uint32_t*>(st);
  uint64_t* val = reinterpret_cast<uint64_t*>(st + o_val);
  uint64_t* cn = reinterpret_cast<uint64_t*>(st + o_cn);
  h->blksum_loose = true;  // (the atomics keep the block bounds valid, not tight)
  for (uint32_t t = 0; t < cnt; ++t) {
    nd[t] = loc[t];
    val[t] = stat_bits(h, stat[t]);
    cn[t] = card_number[t];
    h->note_static(loc[t], stat[t]);  // the K2 block bounds stay valid while scores only fall
  }
  // the event marks the end of the staging pages' read (by the copy, or by the kernel itself),
  // before which they are not rewritten
  const unsigned char* d = static_cast<const unsigned char*>(h->upd_stage.dp);
  if (!mapped) {
    HIP_TRY(h, h->upd_node.ensure(bytes));
    HIP_TRY(h, hipMemcpyAsync(h->upd_node.p, st, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->upd_event, h->stream));
    d = h->upd_node.as<unsigned char>();
  }
  const uint32_t stride = h->path == Path::N32 ? n32_stride(h->K) : node_stride(h->K);
  HIP_TRY(h, launch_set_static(h->nodes.as<unsigned char>(), stride,
                               reinterpret_cast<const uint32_t*>(d),
                               reinterpret_cast<const uint64_t*>(d + o_val),
                               reinterpret_cast<const uint64_t*>(d + o_cn), cnt,
                               h->has_k1sum ? h->k1sum.as<unsigned char>() : nullptr,
                               k1sum_stride(h->K),
                               h->has_k2sum ? h->k2sum.as<unsigned char>() : nullptr,
                               k2sum_stride(h->K), h->perm_copy(), h->stream));
  if (mapped) HIP_TRY(h, hipEventRecord(h->upd_event, h->stream));
  h->upd_pending = true;
  return YODA_OK;
}

// A pod SoA holding the pods `idx` of `src` (in that order).
struct PodGather {
  std::vector<uint8_t> hn, hm, hc;
  std::vector<uint64_t> n, m, c;
  std::vector<int64_t> prio, rcpu;
  std::vector<double> rio;
  yoda_pod_soa soa{};
  void build(const yoda_pod_soa* src, const uint32_t* idx, uint32_t cnt) {
    hn.resize(cnt), hm.resize(cnt), hc.resize(cnt), n.resize(cnt), m.resize(cnt), c.resize(cnt);
    prio.assign(cnt, 0), rcpu.assign(cnt, 0), rio.assign(cnt, 0.0);
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint32_t p = idx[i];
      hn[i] = src->has_number[p], n[i] = src->number[p];
      hm[i] = src->has_memory[p], m[i] = src->memory[p];
      hc[i] = src->has_clock[p], c[i] = src->clock[p];
      if (src->priority) prio[i] = src->priority[p];
      if (src->rio) rio[i] = src->rio[p];
      if (src->rcpu) rcpu[i] = src->rcpu[p];
    }
    soa.n_pods = cnt;
    soa.has_number = hn.data(), soa.number = n.data();
    soa.has_memory = hm.data(), soa.memory = m.data();
    soa.has_clock = hc.data(), soa.clock = c.data();
    soa.priority = prio.data();
    soa.rio = src->rio ? rio.data() : nullptr;
    soa.rcpu = src->rcpu ? rcpu.data() : nullptr;
  }
};

// 6144 pods: larger windows cost fewer, longer GPU windows but more exact fallbacks (touched
// nodes invalidate more candidate lists); profiles/r02/final/greedy_window_ab.txt
constexpr uint32_t kGreedyWindow = 6144;
// A/B knob: YODA_GREEDY_WINDOW overrides the window size (pods per GPU window).
uint32_t greedy_window() {
  static const uint32_t w = [] {
    const uint32_t v = YODA_KNOB("YODA_GREEDY_WINDOW", 0);
    return v >= 64 && v <= (1u << 20) ? v : kGreedyWindow;
  }();
  return w;
}

// Exact evaluation of ONE pod against the current device state (the caller has pushed the
// pending node updates).
int greedy_eval_one(yoda_t* h, const yoda_pod_soa* pods, uint32_t p, int mode,
                    int32_t* pick_out) {
  int rc;
  PodGather one;
  one.build(pods, &p, 1);
  if ((rc = yoda_upload_pods(h, &one.soa))) return rc;
  if ((rc = run_private(h, mode, 0, false))) return rc;
  HIP_TRY(h, h->pick_stage.ensure(16));
  HIP_TRY(h, hipMemcpyAsync(h->pick_stage.p, h->pick.p, 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  *pick_out = *static_cast<int32_t*>(h->pick_stage.p);
  return YODA_OK;
}

// Exact evaluation of the window pod at sorted position s against the current node state,
// reusing the window's feasibility bits and maxima (only static scores change inside a
// window, and the caller's push has made them current): one launch + an 4-byte copy.
int greedy_eval_fast(yoda_t* h, uint32_t s, int32_t* pick_out) {
  const uint32_t nb = greedy_one_blocks();
  if (h->g1_done.bytes == 0) {
    HIP_TRY(h, h->g1_done.ensure(16));
    HIP_TRY(h, hipMemsetAsync(h->g1_done.p, 0, 16, h->stream));
  }
  HIP_TRY(h, h->g1_part.ensure((size_t)nb * 12 + 16));
  double* ps = h->g1_part.as<double>();
  uint32_t* pi = reinterpret_cast<uint32_t*>(ps + nb);
  uint32_t* done = h->g1_done.as<uint32_t>();
  // the last block writes the pick straight into mapped (coherent) pinned memory: no copy,
  // and the host polls the node word instead of synchronising the stream (the next device
  // work is stream-ordered after this kernel anyway)
  h->poll_stage.flags = hipHostMallocCoherent;
  HIP_TRY(h, h->poll_stage.ensure(16));
  volatile uint32_t* res = static_cast<volatile uint32_t*>(h->poll_stage.p) + 1;
  constexpr uint32_t kPending = 0xfffffffeu;  // never a node index (N < 2^31)
  *res = kPending;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  HIP_TRY(h, launch_greedy_one(h->K, h->path, h->nodes.as<unsigned char>(),
                               h->has_k2sum ? h->k2sum.as<unsigned char>() : nullptr, h->n_nodes,
                               pod_params(h), h->rcp.as<double>(), 
                               h->n_pods, s, h->bitmask.as<uint64_t>(), bm_row(h->n_nodes),
                               h->bs_ptr(), bs_row(h->n_nodes), h->blk_ptr(),
                               blk_row(h->n_nodes), ps, pi, done,
                               static_cast<uint32_t*>(h->poll_stage.dp) + 1, h->stream));
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0; *res == kPending; ++spin) {
      // past a generous bound (a stalled device, or memory the device cannot reach coherently
      // on this system) the stream synchronisation decides
      if ((spin & 1023u) == 0u &&
          std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        break;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  // (word 1: the kernel's out[0]; its f64 score follows 8-byte aligned at word 2)
  const uint32_t n = *res;
  if (n == kPending) return fail(h, YODA_ERR_STATE, "greedy: the fallback's result never arrived");
  if (n == 0xffffffffu) return fail(h, YODA_ERR_INVALID_ARG, "greedy: no feasible node found");
  *pick_out = (int32_t)(n + h->node_offset);
  return YODA_OK;
}

}  // namespace

}  // extern "C"
static int greedy_batch(yoda_t* h, const yoda_pod_soa* pods, int mode, uint32_t flags,
                        int32_t* pick);
static int greedy_mode_b(yoda_t* h, const yoda_pod_soa* pods, int32_t* pick);
extern "C" {

int yoda_greedy(yoda_t* h, const yoda_pod_soa* pods, int mode, uint32_t flags, int32_t* pick) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!pods || !pick) return fail(h, YODA_ERR_INVALID_ARG, "NULL pods or pick");
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (int rc = samp_refuse(h, "yoda_greedy")) return rc;
  if (!h->greedy_cand)
    if (int rc = cand_refuse(h, "yoda_greedy")) return rc;
  if (int rc = mode_b_absent(h, mode, true)) return rc;
  // (candidates on: the class array is the batch's, in input order -- cand_ready's rule)
  if (h->cand_classes && !h->h_cls.empty() && h->h_cls.size() != pods->n_pods)
    return fail(h, YODA_ERR_STATE, "yoda_set_pod_classes: the class array's length is not n_pods");
  if (h->cand_classes && h->cls_top >= (int)h->cand_classes)
    return fail(h, YODA_ERR_STATE, "yoda_set_pod_classes: a class is not below n_classes");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    GreedyScope scope(h);
    const uint32_t P = pods->n_pods;
    h->greedy_windows = 0;
    h->greedy_fallbacks = 0;
    h->greedy_restarts = 0;
    h->greedy_refreshes = 0;
    h->greedy_window_ms = h->greedy_fallback_ms = h->greedy_resolve_ms = 0;
    h->greedy_prep_ms = 0;
    if (P == 0) return YODA_OK;
    if (mode != YODA_MODE_DISKIO) return greedy_batch(h, pods, mode, flags, pick);
    return greedy_mode_b(h, pods, pick);
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_greedy_restarts(const yoda_t* h, uint32_t* restarts) {
  if (!h || !restarts) return YODA_ERR_INVALID_ARG;
  *restarts = h->greedy_restarts;
  return YODA_OK;
}

int yoda_greedy_refreshes(const yoda_t* h, uint32_t* refreshes) {
  if (!h || !refreshes) return YODA_ERR_INVALID_ARG;
  *refreshes = h->greedy_refreshes;
  return YODA_OK;
}

int yoda_greedy_stats(const yoda_t* h, uint32_t* windows, uint32_t* fallbacks,
                      double* times_ms) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (windows) *windows = h->greedy_windows;
  if (fallbacks) *fallbacks = h->greedy_fallbacks;
  if (times_ms) {
    times_ms[0] = h->greedy_window_ms;
    times_ms[1] = h->greedy_resolve_ms;
    times_ms[2] = h->greedy_fallback_ms;
  }
  return YODA_OK;
}

// ---- sharded greedy (config 5 across GPUs) ---------------------------------------------
// Each rank's handle holds a node shard.  Per window: yoda_shard_phase1 (+ MAX/SUM
// all-reduce) -> yoda_shard_topk (local top-k with the global maxima) -> the caller merges
// the shards' lists -> the host session resolves the window in queue order; pods it cannot
// certify are scored exactly on every shard (yoda_shard_best_one) and merged by the caller.
// Between steps the caller pushes the nodes the session changed (yoda_gs_take_dirty ->
// yoda_set_node_state on every shard).

int yoda_topk_k(void) { return topk_k(); }
int yoda_topk_k_capacity(void) { return topk_k_capacity(); }

int yoda_set_node_state(yoda_t* h, uint32_t count, const uint32_t* nodes, const uint64_t* alloc,
                        const uint64_t* card_number) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (count && (!nodes || !alloc || !card_number))
    return fail(h, YODA_ERR_INVALID_ARG, "NULL node state array");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    // One entry per node, the last of a repeated id: k_set_static runs one thread per entry,
    // and two of them storing to one node's words would leave the device with either value
    // while the host copies keep the last.  upd_slot[i] = node i's entry in this list.
    if (h->upd_slot.size() != h->n_nodes) h->upd_slot.assign(h->n_nodes, ~0u);
    std::vector<uint32_t> loc;
    std::vector<uint64_t> al, st, cn;
    auto forget = [&] { for (uint32_t i : loc) h->upd_slot[i] = ~0u; };
    for (uint32_t t = 0; t < count; ++t) {
      if (nodes[t] < h->node_offset || nodes[t] - h->node_offset >= h->n_nodes) continue;
      const uint32_t i = nodes[t] - h->node_offset;
      bool z = false;
      const uint64_t s = static_score(h->h_free_sum[i], h->h_total_sum[i], alloc[t], &z);
      if (!h->generic && s >= (1ull << 51)) {
        forget();
        return fail(h, YODA_ERR_RANGE, "static score leaves the fast path; re-upload the nodes");
      }
      uint32_t& slot = h->upd_slot[i];
      if (slot == ~0u) {
        slot = (uint32_t)loc.size();
        loc.push_back(i);
        al.push_back(alloc[t]);
        st.push_back(s);
        cn.push_back(card_number[t]);
      } else {
        al[slot] = alloc[t];
        st[slot] = s;
        cn[slot] = card_number[t];
      }
    }
    forget();
    // keep the host copies current (yoda_update_alloc / yoda_greedy start from them)
    const size_t stride = h->path == Path::N32 ? n32_stride(h->K) : node_stride(h->K);
    for (size_t ti = 0; ti < loc.size(); ++ti) {
      const uint32_t i = loc[ti];
      h->h_alloc[i] = al[ti];
      h->h_card_number[i] = cn[ti];
      unsigned char* r = h->host_records.data() + (size_t)i * stride;
      const uint64_t bits = stat_bits(h, st[ti]);
      std::memcpy(r, &bits, 8);          // header word 0: static score
      std::memcpy(r + 8, &cn[ti], 8);    // header word 1: CardNumber
      if (h->has_k2sum) {
        h->host_k2sum[sum_index(i, kS2Static, k2sum_stride(h->K))] = (uint32_t)bits;
        h->host_k2sum[sum_index(i, kS2Static + 1, k2sum_stride(h->K))] = (uint32_t)(bits >> 32);
      }
    }
    return push_node_state(h, (uint32_t)loc.size(), loc.data(), st.data(), cn.data(), false);
  } catch (const std::bad_alloc&) {
    h->upd_slot.clear();  // (rebuilt empty by the next call)
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

namespace {

// One card of a host record (the formats of yoda_layout.h), back as the uint64 it was uploaded.
uint64_t rec_field(const yoda_t* h, const unsigned char* r, int field, uint32_t j) {
  const int K = h->K;
  if (h->path == Path::N32) {
    if (field == kFree || field == kTotal) {
      double d;
      std::memcpy(&d, r + n32_f64_off(field == kFree ? kF64Free : kF64Total, K) + 8u * j, 8);
      return (uint64_t)d;
    }
    uint32_t u;
    std::memcpy(&u, r + n32_u32_off(field, K) + 4u * j, 4);
    return u;
  }
  if (h->path == Path::F64) {
    double d;
    std::memcpy(&d, r + 32 + 8u * ((size_t)field * K + j), 8);
    return (uint64_t)d;
  }
  uint64_t u;
  std::memcpy(&u, r + 32 + 8u * ((size_t)field * K + j), 8);
  return u;
}

// Words of one packed node in h->cu_rows: its record, then on N32 its K1 summary, K2 summary,
// model row and K1 tile (pack_node's outputs, node-major).
uint32_t packed_row_words(const yoda_t* h) {
  const int K = h->K;
  if (h->path != Path::N32) return node_stride(K) / 4u;
  return (n32_stride(K) + k1sum_stride(K) + k2sum_stride(K) + mix_stride(K) + x1_stride(K)) / 4u;
}

// Where pack_node writes node ti of h->cu_rows.
void packed_row_out(yoda_t* h, uint32_t ti, uint32_t row_words, NodePackOut& out) {
  const int K = h->K;
  uint32_t* row = h->cu_rows.data() + (size_t)ti * row_words;
  out = NodePackOut{};
  out.rec = reinterpret_cast<unsigned char*>(row);
  if (h->path == Path::N32) {
    out.sum = row + n32_stride(K) / 4u;
    out.sum2 = out.sum + k1sum_stride(K) / 4u;
    out.mix = out.sum2 + k2sum_stride(K) / 4u;
    out.x1 = out.mix + mix_stride(K) / 4u;
  }
}

// The packed rows of the listed nodes (h->cu_rows, one row per entry of loc) onto the host
// mirrors and the device: the records, the tiled tables and their block-grouped copies
// (k_set_cards), then on N32 the block summaries of both orders again (k_bsum_build).  Ordered
// on the handle's stream; pending run, phase-1 and top-k state is invalidated.  The one sparse
// writer of whole rows: yoda_update_node_cards and yoda_set_node_present both end here.
int apply_packed_rows(yoda_t* h, const std::vector<uint32_t>& loc, uint32_t row_words) {
  const int K = h->K;
  const bool n32 = h->path == Path::N32;
  const size_t stride = n32 ? n32_stride(K) : node_stride(K);
  const uint32_t cnt = (uint32_t)loc.size();
  const uint32_t RW = (uint32_t)(stride / 4), SW = k1sum_stride(K) / 4u, S2W = k2sum_stride(K) / 4u;
  const size_t o_rows = ((size_t)cnt * 4 + 15) / 16 * 16;
  const size_t bytes = o_rows + (size_t)cnt * row_words * 4;
  if (h->upd_pending) HIP_TRY(h, hipEventSynchronize(h->upd_event));
  HIP_TRY(h, h->upd_stage.ensure(bytes));
  HIP_TRY(h, h->upd_node.ensure(bytes));
  unsigned char* st = static_cast<unsigned char*>(h->upd_stage.p);
  std::memcpy(st, loc.data(), (size_t)cnt * 4);
  std::memcpy(st + o_rows, h->cu_rows.data(), (size_t)cnt * row_words * 4);
  for (uint32_t ti = 0; ti < cnt; ++ti) {
    const uint32_t i = loc[ti];
    const uint32_t* row = h->cu_rows.data() + (size_t)ti * row_words;
    std::memcpy(h->host_records.data() + (size_t)i * stride, row, stride);
    if (n32)
      for (uint32_t w = 0; w < S2W; ++w)
        h->host_k2sum[sum_index(i, w, k2sum_stride(K))] = row[RW + SW + w];
  }
  h->ran = false;
  h->phase1_done = false;
  h->topk_ready = false;
  HIP_TRY(h, hipMemcpyAsync(h->upd_node.p, st, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->upd_event, h->stream));
  h->upd_pending = true;
  unsigned char* d = h->upd_node.as<unsigned char>();
  HIP_TRY(h, launch_set_cards(h->nodes.as<unsigned char>(), (uint32_t)stride,
                              reinterpret_cast<const uint32_t*>(d),
                              reinterpret_cast<const uint32_t*>(d + o_rows), row_words, cnt, K,
                              n32 ? h->k1sum.as<uint32_t>() : nullptr, h->k2sum.as<uint32_t>(),
                              h->kmix.as<uint32_t>(), h->kx1.as<uint32_t>(), h->perm_copy(),
                              h->stream));
  if (!n32) return YODA_OK;
  // the block summaries of both orders: the old ones are wrong now, not merely loose
  return rebuild_block_sums(h);
}

// After apply_packed_rows on N32: the G maxima become g (those of the PRESENT nodes), the G table
// of both orders is rebuilt from the new K2 summaries, the K2 block bounds are marked for a
// rebuild before their next reader, and when a maximum moved its reciprocals are read back as
// the upload reads them.
int apply_gmax(yoda_t* h, const uint64_t g[6]) {
  const bool g_moved = std::memcmp(g, h->h_gmax, sizeof(h->h_gmax)) != 0;
  if (g_moved) {
    std::memcpy(h->h_gmax, g, sizeof(h->h_gmax));
    HIP_TRY(h, hipMemcpyAsync(h->gtab_aux.p, h->h_gmax, sizeof(h->h_gmax), hipMemcpyHostToDevice,
                              h->stream));
  }
  int rc = relaunch_gtables(h);
  if (rc) return rc;
  h->kbub_dirty = true;
  h->kbub_loose = false;
  if (g_moved && h->g.tab && (rc = read_g_reciprocals(h))) return rc;
  return YODA_OK;
}

// MaxValue field -> the CardField it is taken over.
constexpr int kMaxToCard[6] = {kBandwidth, kClock, kCore, kFree, kPower, kTotal};

}  // namespace

int yoda_update_node_cards(yoda_t* h, uint32_t count, const uint32_t* nodes, uint32_t max_cards,
                           const uint64_t* card_free_memory, const uint8_t* card_healthy,
                           const uint64_t* free_memory_sum) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (count == 0) return YODA_OK;
  if (!nodes || !card_free_memory || !card_healthy || !free_memory_sum)
    return fail(h, YODA_ERR_INVALID_ARG, "NULL card update array");
  if (max_cards < 1 || max_cards > YODA_MAX_CARDS)
    return fail(h, YODA_ERR_INVALID_ARG, "max_cards must be in 1..16");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const int K = h->K;
    const bool n32 = h->path == Path::N32;
    const size_t stride = n32 ? n32_stride(K) : node_stride(K);
    const uint32_t row_words = packed_row_words(h);
    // one entry per node, the last of a repeated id (the upd_slot pattern of yoda_set_node_state)
    if (h->upd_slot.size() != h->n_nodes) h->upd_slot.assign(h->n_nodes, ~0u);
    std::vector<uint32_t> loc, ent;
    auto forget = [&] { for (uint32_t i : loc) h->upd_slot[i] = ~0u; };
    for (uint32_t t = 0; t < count; ++t) {
      if (nodes[t] < h->node_offset || nodes[t] - h->node_offset >= h->n_nodes) continue;
      const uint32_t i = nodes[t] - h->node_offset;
      uint32_t& slot = h->upd_slot[i];
      if (slot == ~0u) {
        slot = (uint32_t)loc.size();
        loc.push_back(i);
        ent.push_back(t);
      } else {
        ent[slot] = t;
      }
    }
    forget();
    const uint32_t cnt = (uint32_t)loc.size();
    if (cnt == 0) return YODA_OK;
    // Validate and pack every row into host scratch; nothing of the handle is written before
    // the whole list has passed.
    h->cu_rows.assign((size_t)cnt * row_words, 0u);
    std::vector<uint64_t> new_stat(cnt);
    uint64_t new_actual = h->sb_actual, new_free_max = 0;
    bool held_max = false;  // a changed node held the G maximum of FreeMemory
    for (uint32_t ti = 0; ti < cnt; ++ti) {
      const uint32_t i = loc[ti], t = ent[ti];
      const unsigned char* r = h->host_records.data() + (size_t)i * stride;
      NodeHdrG hd;
      std::memcpy(&hd, r, sizeof(hd));
      const uint32_t nc = (uint32_t)__builtin_popcount(hd.real_mask);
      // (an absent node takes its new values and stays absent: they count for G when it returns)
      const bool absent = (hd.flags & kNodeAbsent) != 0u;
      if (nc > max_cards)
        return fail(h, YODA_ERR_INVALID_ARG, "max_cards below a listed node's card count");
      uint64_t fr[YODA_MAX_CARDS], tot[YODA_MAX_CARDS], ck[YODA_MAX_CARDS], bw[YODA_MAX_CARDS],
          co[YODA_MAX_CARDS], pw[YODA_MAX_CARDS];
      uint8_t hl[YODA_MAX_CARDS];
      uint32_t fc[YODA_MAX_CARDS], tc[YODA_MAX_CARDS];
      for (uint32_t j = 0; j < nc; ++j) {
        const uint64_t f = card_free_memory[(size_t)t * max_cards + j];
        fr[j] = f;
        hl[j] = card_healthy[(size_t)t * max_cards + j] ? 1 : 0;
        tot[j] = rec_field(h, r, kTotal, j);
        ck[j] = rec_field(h, r, kClock, j);
        bw[j] = rec_field(h, r, kBandwidth, j);
        co[j] = rec_field(h, r, kCore, j);
        pw[j] = rec_field(h, r, kPower, j);
        if (n32) {
          std::memcpy(&tc[j], r + n32_u32_off(kTotal, K) + 4u * j, 4);
          if (h->mem_ranks) {
            const auto it = std::lower_bound(h->h_frees.begin(), h->h_frees.end(), f);
            if (it == h->h_frees.end() || *it != f)
              return fail(h, YODA_ERR_RANGE,
                          "FreeMemory value outside the snapshot's rank table; re-upload the nodes");
            fc[j] = 2u + (uint32_t)(it - h->h_frees.begin());
          } else {
            if (f > kN32FieldMax)
              return fail(h, YODA_ERR_RANGE, "FreeMemory leaves the 32-bit path; re-upload the nodes");
            fc[j] = (uint32_t)f;
          }
        } else if (h->path == Path::F64 && f > kFastFieldMax) {
          return fail(h, YODA_ERR_RANGE, "FreeMemory leaves the fast path; re-upload the nodes");
        }
        if (absent) continue;
        new_free_max = std::max(new_free_max, f);
        if (n32 && std::max<uint64_t>(rec_field(h, r, kFree, j), 1) == h->h_gmax[kMaxFree])
          held_max = true;
      }
      bool z = false;
      const uint64_t s = static_score(free_memory_sum[t], h->h_total_sum[i], h->h_alloc[i], &z);
      if (!h->generic && s >= (1ull << 51))
        return fail(h, YODA_ERR_RANGE, "static score leaves the fast path; re-upload the nodes");
      new_stat[ti] = s;
      if (h->h_total_sum[i] != 0)
        new_actual = std::max(new_actual, free_memory_sum[t] * 100u / h->h_total_sum[i] * 2u);
      NodePackIn in;
      in.cnt = nc;
      in.card_number = h->h_card_number[i];
      in.stat = s;
      in.zero_total = z;
      in.no_uniform = !(hd.flags & kNodeUniform4);  // (as uploaded: the card models are the same)
      in.absent = absent;
      in.free_memory = fr;
      in.total_memory = tot;
      in.clock = ck;
      in.bandwidth = bw;
      in.core = co;
      in.power = pw;
      in.healthy = hl;
      in.fcode = fc;
      in.tcode = tc;
      NodePackOut out;
      packed_row_out(h, ti, row_words, out);
      pack_node(h->path, K, in, out);
    }
    // ---- the list passed: the rows onto the mirrors and the device, then the host copies ----
    int rc = apply_packed_rows(h, loc, row_words);
    if (rc) return rc;
    for (uint32_t ti = 0; ti < cnt; ++ti) h->h_free_sum[loc[ti]] = free_memory_sum[ent[ti]];
    if (new_actual > h->sb_actual) {  // the score bound may only grow
      h->sb_actual = new_actual;
      const long double b = h->sb_cards + (long double)new_actual;
      h->score_bound =
          std::max<uint64_t>(h->score_bound, b < 9.0e18L ? (uint64_t)b + 1u : ~(uint64_t)0);
    }
    if (!n32) return YODA_OK;
    // The G maximum of FreeMemory over the present nodes, exact: it rises with a larger free; when
    // a changed node held it, recomputed from the host K2 summaries (word kS2Fs + 0: each node's
    // largest free).
    uint64_t gfree = std::max(h->h_gmax[kMaxFree], std::max<uint64_t>(new_free_max, 1));
    if (held_max) {
      gfree = 1;
      const uint32_t S2 = k2sum_stride(K);
      for (uint32_t n = 0; n < h->n_nodes; ++n) {
        if (h->h_absent[n]) continue;
        const uint32_t c = h->host_k2sum[sum_index(n, kS2Fs, S2)];
        uint64_t v = c;
        if (h->mem_ranks) v = c >= 2u && c - 2u < h->h_frees.size() ? h->h_frees[c - 2u] : 0;
        gfree = std::max(gfree, v);
      }
    }
    uint64_t g[6];
    std::memcpy(g, h->h_gmax, sizeof(g));
    g[kMaxFree] = gfree;
    return apply_gmax(h, g);
  } catch (const std::bad_alloc&) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_set_node_present(yoda_t* h, uint32_t count, const uint32_t* nodes,
                          const uint8_t* present) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (count == 0) return YODA_OK;
  if (!nodes || !present) return fail(h, YODA_ERR_INVALID_ARG, "NULL node presence array");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const int K = h->K;
    const bool n32 = h->path == Path::N32;
    const size_t stride = n32 ? n32_stride(K) : node_stride(K);
    const uint32_t row_words = packed_row_words(h);
    // one entry per node, the last of a repeated id (the upd_slot pattern of yoda_set_node_state)
    if (h->upd_slot.size() != h->n_nodes) h->upd_slot.assign(h->n_nodes, ~0u);
    if (h->h_absent.size() != h->n_nodes) h->h_absent.assign(h->n_nodes, 0);
    std::vector<uint32_t> seen, ent;
    for (uint32_t t = 0; t < count; ++t) {
      if (nodes[t] < h->node_offset || nodes[t] - h->node_offset >= h->n_nodes) continue;
      const uint32_t i = nodes[t] - h->node_offset;
      uint32_t& slot = h->upd_slot[i];
      if (slot == ~0u) {
        slot = (uint32_t)seen.size();
        seen.push_back(i);
        ent.push_back(t);
      } else {
        ent[slot] = t;
      }
    }
    for (uint32_t i : seen) h->upd_slot[i] = ~0u;
    // the pending outcomes are the old node set's, whether or not a listed node changes sides
    h->ran = false;
    h->phase1_done = false;
    h->topk_ready = false;
    h->draw_stage = 0;
    // the nodes whose presence changes, their rows repacked from the host records with the new bit
    std::vector<uint32_t> loc;
    std::vector<uint8_t> gone;
    for (size_t k = 0; k < seen.size(); ++k) {
      const uint8_t a = present[ent[k]] ? 0 : 1;
      if (a == h->h_absent[seen[k]]) continue;
      loc.push_back(seen[k]);
      gone.push_back(a);
    }
    const uint32_t cnt = (uint32_t)loc.size();
    if (cnt == 0) return YODA_OK;
    h->cu_rows.assign((size_t)cnt * row_words, 0u);
    uint64_t g[6];
    std::memcpy(g, h->h_gmax, sizeof(g));
    uint32_t lost = 0;  // bit f: a node that leaves holds the G maximum of MaxValue field f
    for (uint32_t ti = 0; ti < cnt; ++ti) {
      const uint32_t i = loc[ti];
      const unsigned char* r = h->host_records.data() + (size_t)i * stride;
      NodeHdrG hd;
      std::memcpy(&hd, r, sizeof(hd));
      const uint32_t nc = (uint32_t)__builtin_popcount(hd.real_mask);
      uint64_t v[kCardFields][YODA_MAX_CARDS];  // CardField order
      uint8_t hl[YODA_MAX_CARDS];
      uint32_t fc[YODA_MAX_CARDS] = {}, tc[YODA_MAX_CARDS] = {};
      for (uint32_t j = 0; j < nc; ++j) {
        for (int f = 0; f < kCardFields; ++f) v[f][j] = rec_field(h, r, f, j);
        hl[j] = (hd.healthy_mask >> j) & 1u;
        if (n32) {  // the memory codes as the record holds them (values, or ranks)
          std::memcpy(&fc[j], r + n32_u32_off(kFree, K) + 4u * j, 4);
          std::memcpy(&tc[j], r + n32_u32_off(kTotal, K) + 4u * j, 4);
        }
      }
      if (n32)
        for (int f = 0; f < 6; ++f) {
          uint64_t m = 1;
          for (uint32_t j = 0; j < nc; ++j) m = std::max(m, v[kMaxToCard[f]][j]);
          if (gone[ti])
            lost |= m == h->h_gmax[f] ? 1u << f : 0u;
          else
            g[f] = std::max(g[f], m);
        }
      NodePackIn in;
      in.cnt = nc;
      in.card_number = hd.card_number;
      if (h->generic) {
        in.stat = hd.static_score;
      } else {
        double sd;
        std::memcpy(&sd, &hd.static_score, 8);
        in.stat = (uint64_t)sd;
      }
      in.zero_total = hd.zero_total != 0u;
      in.no_uniform = !(hd.flags & kNodeUniform4);  // (as uploaded: the card models are the same)
      in.absent = gone[ti] != 0;
      in.free_memory = v[kFree];
      in.total_memory = v[kTotal];
      in.clock = v[kClock];
      in.bandwidth = v[kBandwidth];
      in.core = v[kCore];
      in.power = v[kPower];
      in.healthy = hl;
      in.fcode = fc;
      in.tcode = tc;
      NodePackOut out;
      packed_row_out(h, ti, row_words, out);
      pack_node(h->path, K, in, out);
    }
    int rc = apply_packed_rows(h, loc, row_words);
    if (rc) return rc;
    for (uint32_t ti = 0; ti < cnt; ++ti) {
      h->h_absent[loc[ti]] = gone[ti];
      if (gone[ti]) ++h->n_absent; else --h->n_absent;
    }
    h->b_elig_dirty = true;
    if (!n32) return YODA_OK;
    // The G maxima are those of the present nodes (a wave whose maxima are G's takes the G-table
    // K2; with a stale G none would).  A returning node can only raise them (above); a field
    // whose holder left is searched over the present nodes, stopping at the first that still
    // reaches the old maximum (one GPU model in the fleet: the first node).
    for (int f = 0; f < 6; ++f) {
      if (!((lost >> f) & 1u)) continue;
      const uint64_t old = h->h_gmax[f];
      uint64_t m = 1;
      for (uint32_t n = 0; n < h->n_nodes && m < old; ++n) {
        if (h->h_absent[n]) continue;
        const unsigned char* r = h->host_records.data() + (size_t)n * stride;
        NodeHdrG hd;
        std::memcpy(&hd, r, sizeof(hd));
        const uint32_t nc = (uint32_t)__builtin_popcount(hd.real_mask);
        for (uint32_t j = 0; j < nc; ++j) m = std::max(m, rec_field(h, r, kMaxToCard[f], j));
      }
      // (m < old: the scan was whole and m is the maximum; else g[f] holds the returning nodes')
      g[f] = m < old ? m : std::max(g[f], m);
    }
    return apply_gmax(h, g);
  } catch (const std::bad_alloc&) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_nodes_absent(const yoda_t* h, uint32_t* n_absent) {
  if (!h || !n_absent) return YODA_ERR_INVALID_ARG;
  *n_absent = h->has_nodes ? h->n_absent : 0u;
  return YODA_OK;
}

namespace {
// A change of the candidate state: the pending outcomes are the old candidates', a sharded
// step's pending exact merge included.
void cand_invalidate(yoda_t* h) {
  h->b_cls_ready = false;  // (Mode B's classes are keyed by the pods' candidate classes)
  h->k3_pending = false;
  h->ran = false;
  h->phase1_done = false;
  h->topk_ready = false;
  h->draw_stage = 0;
}

// The per-block ANDs of both node orders from the device tables (whole: one wave per block).
int cand_rebuild_sums(yoda_t* h, bool copy) {
  const unsigned char* rec = h->nodes.as<unsigned char>();
  const uint32_t stride = h->path == Path::N32 ? n32_stride(h->K) : node_stride(h->K);
  HIP_TRY(h, launch_cand_build(h->cand_w.as<uint64_t>(), nullptr, rec, stride, h->n_nodes, nullptr,
                               h->cand_and.as<uint64_t>(), h->cand_zt.as<uint64_t>(), h->stream));
  if (h->perm_on)  // (copy: the grouped table too; else it is current -- k_cand_update)
    HIP_TRY(h, launch_cand_build(h->cand_w.as<uint64_t>(), h->perm_ids.as<uint32_t>(), rec, stride,
                                 h->n_nodes, copy ? h->cand_w_p.as<uint64_t>() : nullptr,
                                 h->cand_and_p.as<uint64_t>(), h->cand_zt_p.as<uint64_t>(),
                                 h->stream));
  return YODA_OK;
}
}  // namespace

int yoda_set_candidates(yoda_t* h, uint32_t n_classes, const uint64_t* words) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (n_classes > YODA_MAX_CAND_CLASSES)
    return fail(h, YODA_ERR_INVALID_ARG, "n_classes above YODA_MAX_CAND_CLASSES");
  if (n_classes == 0) {
    if (h->cand_classes) {
      cand_invalidate(h);
      h->b_elig_dirty = true;
    }
    h->cand_classes = 0;
    h->h_cand.clear();
    return YODA_OK;
  }
  if (!words) return fail(h, YODA_ERR_INVALID_ARG, "NULL candidate words");
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t N = h->n_nodes;
    const size_t nb = std::max<size_t>((N + 63u) / 64u, 1);
    HIP_TRY(h, h->cand_w.ensure(std::max<size_t>(N, 1) * 8));
    HIP_TRY(h, h->cand_and.ensure(nb * 8));
    HIP_TRY(h, h->cand_zt.ensure(nb * 8));
    if (h->perm_on) {
      HIP_TRY(h, h->cand_w_p.ensure(std::max<size_t>(N, 1) * 8));
      HIP_TRY(h, h->cand_and_p.ensure(nb * 8));
      HIP_TRY(h, h->cand_zt_p.ensure(nb * 8));
    }
    cand_invalidate(h);
    h->b_elig_dirty = true;
    h->cand_classes = 0;  // (off until the tables are whole)
    h->h_cand.assign(words, words + N);
    if (N) {
      HIP_TRY(h, hipMemcpyAsync(h->cand_w.p, h->h_cand.data(), (size_t)N * 8,
                                hipMemcpyHostToDevice, h->stream));
      if (int rc = cand_rebuild_sums(h, true)) return rc;
      HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the copy's source is pageable)
    }
    h->cand_classes = n_classes;
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_update_candidates(yoda_t* h, uint32_t count, const uint32_t* nodes,
                           const uint64_t* words) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (!h->cand_classes)
    return fail(h, YODA_ERR_STATE, "yoda_update_candidates: candidates are off");
  if (count == 0) return YODA_OK;
  if (!nodes || !words) return fail(h, YODA_ERR_INVALID_ARG, "NULL candidate update array");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    // one entry per node, the last of a repeated id (the upd_slot pattern of yoda_set_node_state)
    if (h->upd_slot.size() != h->n_nodes) h->upd_slot.assign(h->n_nodes, ~0u);
    std::vector<uint32_t> loc;
    std::vector<uint64_t> val;
    for (uint32_t t = 0; t < count; ++t) {
      if (nodes[t] < h->node_offset || nodes[t] - h->node_offset >= h->n_nodes) continue;
      const uint32_t i = nodes[t] - h->node_offset;
      uint32_t& slot = h->upd_slot[i];
      if (slot == ~0u) {
        slot = (uint32_t)loc.size();
        loc.push_back(i);
        val.push_back(words[t]);
      } else {
        val[slot] = words[t];
      }
    }
    for (uint32_t i : loc) h->upd_slot[i] = ~0u;
    cand_invalidate(h);
    const uint32_t cnt = (uint32_t)loc.size();
    if (cnt == 0) return YODA_OK;
    const size_t o_val = ((size_t)cnt * 4 + 15) / 16 * 16;
    const size_t bytes = o_val + (size_t)cnt * 8;
    if (h->upd_pending) HIP_TRY(h, hipEventSynchronize(h->upd_event));
    HIP_TRY(h, h->upd_stage.ensure(bytes));
    HIP_TRY(h, h->upd_node.ensure(bytes));
    unsigned char* st = static_cast<unsigned char*>(h->upd_stage.p);
    std::memcpy(st, loc.data(), (size_t)cnt * 4);
    std::memcpy(st + o_val, val.data(), (size_t)cnt * 8);
    for (uint32_t t = 0; t < cnt; ++t) h->h_cand[loc[t]] = val[t];
    h->b_elig_dirty = true;
    HIP_TRY(h, hipMemcpyAsync(h->upd_node.p, st, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->upd_event, h->stream));
    h->upd_pending = true;
    const unsigned char* d = h->upd_node.as<unsigned char>();
    HIP_TRY(h, launch_cand_update(reinterpret_cast<const uint32_t*>(d),
                                  reinterpret_cast<const uint64_t*>(d + o_val), cnt,
                                  h->cand_w.as<uint64_t>(),
                                  h->perm_on ? h->perm_inv.as<uint32_t>() : nullptr,
                                  h->perm_on ? h->cand_w_p.as<uint64_t>() : nullptr, h->stream));
    // the block ANDs of both orders: whole, one wave a block (12 KB each at 100k nodes)
    return cand_rebuild_sums(h, false);
  } catch (const std::bad_alloc&) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

namespace {

// Mode B's records of cnt nodes onto the device (k_set_node_metrics): local node loc[k] -- node
// k when loc == nullptr, the dense form -- takes entry ent[k] (entry k when ent == nullptr) of
// cpu / disk_io.  The division is the upload's own expression, on the host: the stored records
// are bit-identical to a fresh upload's.  Staged as the other sparse writers stage (upd_stage /
// upd_node / upd_event), ordered on the handle's stream.
int push_node_metrics(yoda_t* h, uint32_t cnt, const uint32_t* loc, const uint32_t* ent,
                      const double* cpu, const double* disk_io) {
  if (cnt == 0) return YODA_OK;
  const size_t o_rec = loc ? ((size_t)cnt * 4 + 15) / 16 * 16 : 0;
  const size_t bytes = o_rec + (size_t)cnt * sizeof(NodeRecB);
  if (h->upd_pending) HIP_TRY(h, hipEventSynchronize(h->upd_event));
  HIP_TRY(h, h->upd_stage.ensure(bytes));
  HIP_TRY(h, h->upd_node.ensure(bytes));
  unsigned char* st = static_cast<unsigned char*>(h->upd_stage.p);
  if (loc) std::memcpy(st, loc, (size_t)cnt * 4);
  NodeRecB* rb = reinterpret_cast<NodeRecB*>(st + o_rec);
  for (uint32_t k = 0; k < cnt; ++k) {
    const uint32_t e = ent ? ent[k] : k;
    rb[k].v = cpu[e] / 100.0;     // algorithm.go:73
    rb[k].u = disk_io[e] / 50.0;  // algorithm.go:71
  }
  HIP_TRY(h, hipMemcpyAsync(h->upd_node.p, st, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->upd_event, h->stream));
  h->upd_pending = true;
  const unsigned char* d = h->upd_node.as<unsigned char>();
  HIP_TRY(h, launch_set_node_metrics(h->nodes_b.as<NodeRecB>(),
                                     loc ? reinterpret_cast<const uint32_t*>(d) : nullptr,
                                     reinterpret_cast<const NodeRecB*>(d + o_rec), cnt, h->n_nodes,
                                     h->stream));
  return YODA_OK;
}

// One card's largest value per MaxValue field (floor 1) of a host record.
void record_maxima(const yoda_t* h, const unsigned char* r, uint64_t m[6]) {
  NodeHdrG hd;
  std::memcpy(&hd, r, sizeof(hd));
  const uint32_t nc = (uint32_t)__builtin_popcount(hd.real_mask);
  for (int f = 0; f < 6; ++f) {
    m[f] = 1;
    for (uint32_t j = 0; j < nc; ++j) m[f] = std::max(m[f], rec_field(h, r, kMaxToCard[f], j));
  }
}

}  // namespace

int yoda_update_node_metrics(yoda_t* h, uint32_t count, const uint32_t* nodes, const double* cpu,
                             const double* disk_io) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (!h->nodes_diskio)
    return fail(h, YODA_ERR_STATE, "the snapshot was uploaded without cpu / disk_io");
  if (!nodes && count != h->n_nodes)
    return fail(h, YODA_ERR_INVALID_ARG, "the dense form takes n_nodes entries");
  if (count == 0) return YODA_OK;
  if (!cpu || !disk_io) return fail(h, YODA_ERR_INVALID_ARG, "NULL node metrics array");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<uint32_t> loc, ent;
    if (nodes) {
      // one entry per node, the last of a repeated id (the upd_slot pattern of yoda_set_node_state)
      if (h->upd_slot.size() != h->n_nodes) h->upd_slot.assign(h->n_nodes, ~0u);
      for (uint32_t t = 0; t < count; ++t) {
        if (nodes[t] < h->node_offset || nodes[t] - h->node_offset >= h->n_nodes) continue;
        const uint32_t i = nodes[t] - h->node_offset;
        uint32_t& slot = h->upd_slot[i];
        if (slot == ~0u) {
          slot = (uint32_t)loc.size();
          loc.push_back(i);
          ent.push_back(t);
        } else {
          ent[slot] = t;
        }
      }
      for (uint32_t i : loc) h->upd_slot[i] = ~0u;
      if (loc.empty()) return YODA_OK;
    }
    // the pending outcomes are the old metrics'; the eligibility table of yoda_mode_b_follow
    // reads the presence bits and the candidate words only and stays, as do the pods' classes
    h->ran = false;
    h->phase1_done = false;
    h->topk_ready = false;
    h->draw_stage = 0;
    h->diag_done = false;
    h->k3_pending = false;
    if (nodes) return push_node_metrics(h, (uint32_t)loc.size(), loc.data(), ent.data(), cpu, disk_io);
    return push_node_metrics(h, count, nullptr, nullptr, cpu, disk_io);
  } catch (const std::bad_alloc&) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_replace_nodes(yoda_t* h, uint32_t count, const uint32_t* nodes,
                       const yoda_node_soa* recs) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (count == 0) return YODA_OK;
  if (!nodes || !recs) return fail(h, YODA_ERR_INVALID_ARG, "NULL node replacement array");
  if (recs->n_nodes != count)
    return fail(h, YODA_ERR_INVALID_ARG, "recs->n_nodes differs from count");
  const uint32_t KS = recs->max_cards;
  if (KS < 1 || KS > YODA_MAX_CARDS)
    return fail(h, YODA_ERR_INVALID_ARG, "max_cards must be in 1..16");
  if (!recs->card_number || !recs->card_count || !recs->free_memory_sum ||
      !recs->total_memory_sum || !recs->card_free_memory || !recs->card_total_memory ||
      !recs->card_clock || !recs->card_bandwidth || !recs->card_core || !recs->card_power ||
      !recs->card_healthy)
    return fail(h, YODA_ERR_INVALID_ARG, "a required node array is NULL");
  if (h->nodes_diskio && !(recs->cpu && recs->disk_io))
    return fail(h, YODA_ERR_INVALID_ARG, "the snapshot holds cpu / disk_io: the records need them");
  for (uint32_t t = 0; t < count; ++t)
    if (recs->card_count[t] > KS) return fail(h, YODA_ERR_INVALID_ARG, "card_count > max_cards");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const int K = h->K;
    const bool n32 = h->path == Path::N32;
    const size_t stride = n32 ? n32_stride(K) : node_stride(K);
    const uint32_t row_words = packed_row_words(h);
    // one entry per node, the last of a repeated id (the upd_slot pattern of yoda_set_node_state)
    if (h->upd_slot.size() != h->n_nodes) h->upd_slot.assign(h->n_nodes, ~0u);
    if (h->h_absent.size() != h->n_nodes) h->h_absent.assign(h->n_nodes, 0);
    std::vector<uint32_t> loc, ent;
    for (uint32_t t = 0; t < count; ++t) {
      if (nodes[t] < h->node_offset || nodes[t] - h->node_offset >= h->n_nodes) continue;
      const uint32_t i = nodes[t] - h->node_offset;
      uint32_t& slot = h->upd_slot[i];
      if (slot == ~0u) {
        slot = (uint32_t)loc.size();
        loc.push_back(i);
        ent.push_back(t);
      } else {
        ent[slot] = t;
      }
    }
    for (uint32_t i : loc) h->upd_slot[i] = ~0u;
    const uint32_t cnt = (uint32_t)loc.size();
    if (cnt == 0) return YODA_OK;
    // Validate every record against the format the upload chose (choose_format's rules, one node
    // at a time) and pack it into host scratch; nothing of the handle is written before the whole
    // list has passed.
    const bool no_uniform = (h->upload_flags & YODA_UPLOAD_NO_UNIFORM) != 0u;
    h->cu_rows.assign((size_t)cnt * row_words, 0u);
    std::vector<uint64_t> stat(cnt);
    std::vector<uint32_t> new_flags(cnt);
    uint64_t g[6];
    std::memcpy(g, h->h_gmax, sizeof(g));
    uint32_t lost = 0;  // bit f: a replaced record held the G maximum of MaxValue field f
    uint64_t new_actual = h->sb_actual, new_small = h->small_max;
    long double new_cards = h->sb_cards;
    for (uint32_t ti = 0; ti < cnt; ++ti) {
      const uint32_t i = loc[ti], t = ent[ti];
      const size_t a = (size_t)t * KS;
      const uint32_t nc = recs->card_count[t];
      if (nc > (uint32_t)K)
        return fail(h, YODA_ERR_RANGE, "card count above the snapshot's; re-upload the nodes");
      const uint64_t* fr = recs->card_free_memory + a;
      const uint64_t* tot = recs->card_total_memory + a;
      const uint64_t* ck = recs->card_clock + a;
      const uint64_t* bw = recs->card_bandwidth + a;
      const uint64_t* co = recs->card_core + a;
      const uint64_t* pw = recs->card_power + a;
      uint8_t hl[YODA_MAX_CARDS];
      uint32_t fc[YODA_MAX_CARDS] = {}, tc[YODA_MAX_CARDS] = {};
      uint64_t max_clock = 0, max_small = 0, max_field = 0, max_ckq = 0;
      bool one = nc > 0 && !no_uniform;  // one GPU model with one TotalMemory
      for (uint32_t j = 0; j < nc; ++j) {
        hl[j] = recs->card_healthy[a + j] ? 1 : 0;
        max_clock = std::max(max_clock, ck[j]);
        max_small = std::max({max_small, ck[j], bw[j], co[j], pw[j]});
        max_field = std::max({max_field, fr[j], tot[j], ck[j], bw[j], co[j], pw[j]});
        if (ck[j] <= kN32FieldMax)
          max_ckq = std::max(max_ckq, ck[j] * 100u / std::max<uint64_t>(1, bw[j]));
        one = one && ck[j] == ck[0] && bw[j] == bw[0] && co[j] == co[0] && pw[j] == pw[0] &&
              tot[j] == tot[0];
      }
      if (n32) {
        if (max_small > kN32FieldMax)
          return fail(h, YODA_ERR_RANGE, "a card field leaves the 32-bit path; re-upload the nodes");
        if (h->pack16 && max_small > kPack16Max)
          return fail(h, YODA_ERR_RANGE,
                      "a card field leaves the snapshot's 16-bit packing; re-upload the nodes");
        if (h->q32 && max_small > kF32SmallMax)
          return fail(h, YODA_ERR_RANGE,
                      "a card field leaves the snapshot's f32 quotients; re-upload the nodes");
        if (!h->q32 && !one)
          return fail(h, YODA_ERR_RANGE,
                      "a mixed-model node in a snapshot of wide one-model nodes; re-upload the nodes");
        if ((uint64_t)K * (800u + max_ckq) >= (1ull << 32))
          return fail(h, YODA_ERR_RANGE, "a clock quotient leaves the 32-bit path; re-upload the nodes");
        for (uint32_t j = 0; j < nc; ++j) {
          if (h->mem_ranks) {
            const auto itf = std::lower_bound(h->h_frees.begin(), h->h_frees.end(), fr[j]);
            const auto itt = std::lower_bound(h->h_totals.begin(), h->h_totals.end(), tot[j]);
            if (itf == h->h_frees.end() || *itf != fr[j] || itt == h->h_totals.end() ||
                *itt != tot[j])
              return fail(h, YODA_ERR_RANGE,
                          "memory value outside the snapshot's rank tables; re-upload the nodes");
            fc[j] = 2u + (uint32_t)(itf - h->h_frees.begin());
            tc[j] = 2u + (uint32_t)(itt - h->h_totals.begin());
          } else {
            if (fr[j] > kN32FieldMax || tot[j] > kN32FieldMax)
              return fail(h, YODA_ERR_RANGE,
                          "a memory field leaves the 32-bit path; re-upload the nodes");
            fc[j] = (uint32_t)fr[j];
            tc[j] = (uint32_t)tot[j];
          }
        }
      } else if (h->path == Path::F64 && max_field > kFastFieldMax) {
        return fail(h, YODA_ERR_RANGE, "a card field leaves the fast path; re-upload the nodes");
      }
      bool z = false;
      const uint64_t alloc = recs->alloc_memory ? recs->alloc_memory[t] : 0;
      const uint64_t s =
          static_score(recs->free_memory_sum[t], recs->total_memory_sum[t], alloc, &z);
      const long double cards = (long double)K * (800.0L + 100.0L * (long double)max_clock);
      if (!h->generic && (s >= (1ull << 51) || cards + (long double)s >= (long double)kFastScoreMax))
        return fail(h, YODA_ERR_RANGE, "a score leaves the fast path; re-upload the nodes");
      stat[ti] = s;
      // the upper bounds only grow (yoda_score_bound, yoda_small_field_max)
      new_cards = std::max(new_cards, cards + 300.0L);
      new_small = std::max(new_small, max_small);
      if (recs->total_memory_sum[t] != 0)
        new_actual = std::max(new_actual, recs->free_memory_sum[t] * 100u /
                                              recs->total_memory_sum[t] * 2u);
      // old record out, new record in: the G maxima of the present nodes
      const bool absent = h->h_absent[i] != 0;
      if (n32 && !absent) {
        uint64_t m[6];
        record_maxima(h, h->host_records.data() + (size_t)i * stride, m);
        for (int f = 0; f < 6; ++f) lost |= m[f] == h->h_gmax[f] ? 1u << f : 0u;
        const uint64_t* src[6] = {bw, ck, co, fr, pw, tot};  // MaxValue field order
        for (int f = 0; f < 6; ++f)
          for (uint32_t j = 0; j < nc; ++j) g[f] = std::max(g[f], src[f][j]);
      }
      NodePackIn in;
      in.cnt = nc;
      in.card_number = recs->card_number[t];
      in.stat = s;
      in.zero_total = z;
      in.no_uniform = no_uniform;
      in.absent = absent;
      in.free_memory = fr;
      in.total_memory = tot;
      in.clock = ck;
      in.bandwidth = bw;
      in.core = co;
      in.power = pw;
      in.healthy = hl;
      in.fcode = fc;
      in.tcode = tc;
      NodePackOut out;
      packed_row_out(h, ti, row_words, out);
      new_flags[ti] = pack_node(h->path, K, in, out);
    }
    // ---- the list passed: the one-model counts (old flags out, new in), then the rows onto the
    // mirrors and the device, then the host copies ----
    constexpr uint32_t kOne = kNodeUniform4 | kNodeUniformTotal;
    for (uint32_t ti = 0; ti < cnt; ++ti) {
      NodeHdrG hd;
      std::memcpy(&hd, h->host_records.data() + (size_t)loc[ti] * stride, sizeof(hd));
      h->n_one_model -= (hd.flags & kOne) == kOne;
      h->n_uni4 -= (hd.flags & kNodeUniform4) != 0u;
      h->n_one_model += (new_flags[ti] & kOne) == kOne;
      h->n_uni4 += (new_flags[ti] & kNodeUniform4) != 0u;
    }
    h->all_one_model = h->n_one_model == h->n_nodes;
    h->all_uni4 = h->n_uni4 == h->n_nodes;
    h->draw_stage = 0;
    h->diag_done = false;
    h->k3_pending = false;
    int rc = apply_packed_rows(h, loc, row_words);
    if (rc) return rc;
    for (uint32_t ti = 0; ti < cnt; ++ti) {
      const uint32_t i = loc[ti], t = ent[ti];
      h->h_total_sum[i] = recs->total_memory_sum[t];
      h->h_free_sum[i] = recs->free_memory_sum[t];
      h->h_card_number[i] = recs->card_number[t];
      h->h_alloc[i] = recs->alloc_memory ? recs->alloc_memory[t] : 0;
    }
    h->small_max = new_small;
    if (new_cards > h->sb_cards || new_actual > h->sb_actual) {
      h->sb_cards = new_cards;
      h->sb_actual = new_actual;
      const long double b = new_cards + (long double)new_actual;
      h->score_bound =
          std::max<uint64_t>(h->score_bound, b < 9.0e18L ? (uint64_t)b + 1u : ~(uint64_t)0);
    }
    // the candidate tables' zero_total bits per block are read from the records
    if (h->cand_classes && (rc = cand_rebuild_sums(h, false))) return rc;
    if (h->nodes_diskio &&
        (rc = push_node_metrics(h, cnt, loc.data(), ent.data(), recs->cpu, recs->disk_io)))
      return rc;
    if (!n32) return YODA_OK;
    // A field whose holder was replaced is searched over the present nodes' new records, stopping
    // at the first that still reaches the old maximum (yoda_set_node_present's scan).
    for (int f = 0; f < 6; ++f) {
      if (!((lost >> f) & 1u) || g[f] > h->h_gmax[f]) continue;
      const uint64_t old = h->h_gmax[f];
      uint64_t m = 1;
      for (uint32_t n = 0; n < h->n_nodes && m < old; ++n) {
        if (h->h_absent[n]) continue;
        const unsigned char* r = h->host_records.data() + (size_t)n * stride;
        NodeHdrG hd;
        std::memcpy(&hd, r, sizeof(hd));
        const uint32_t nc = (uint32_t)__builtin_popcount(hd.real_mask);
        for (uint32_t j = 0; j < nc; ++j) m = std::max(m, rec_field(h, r, kMaxToCard[f], j));
      }
      g[f] = m;  // (m < old: the scan was whole; else a present node still reaches old)
    }
    return apply_gmax(h, g);
  } catch (const std::bad_alloc&) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    h->upd_slot.clear();
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_set_pod_classes(yoda_t* h, uint32_t n_pods, const uint8_t* cls) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!cls || n_pods == 0) {
    if (!h->h_cls.empty()) cand_invalidate(h);
    h->h_cls.clear();
    h->cls_top = -1;
    h->cls_hash = 0;
    return YODA_OK;
  }
  // (candidates off: any class a later yoda_set_candidates could name; the run checks again)
  const uint32_t lim = h->cand_classes ? h->cand_classes : (uint32_t)YODA_MAX_CAND_CLASSES;
  int top = -1;
  for (uint32_t p = 0; p < n_pods; ++p) {
    if (cls[p] == YODA_CAND_ANY) continue;
    if (cls[p] >= lim)
      return fail(h, YODA_ERR_INVALID_ARG, "a pod class is neither below n_classes nor YODA_CAND_ANY");
    top = std::max(top, (int)cls[p]);
  }
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->cand_cls.ensure(n_pods));
    std::vector<uint8_t> copy(cls, cls + n_pods);
    HIP_TRY(h, hipMemcpyAsync(h->cand_cls.p, copy.data(), n_pods, hipMemcpyHostToDevice,
                              h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the copy's source is pageable)
    cand_invalidate(h);
    h->h_cls.swap(copy);
    h->cls_top = top;
    uint64_t x = 0xcbf29ce484222325ull;  // (FNV-1a, once per array: the steps read the result)
    for (uint8_t c : h->h_cls) x = (x ^ c) * 0x100000001b3ull;
    h->cls_hash = x;
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_mode_b_follow(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  const bool on = enable != 0;
  if (on != h->b_follow) cand_invalidate(h);  // the pending outcomes are the other reading's
  h->b_follow = on;
  return YODA_OK;
}

int yoda_mode_b_sampling(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  const bool on = enable != 0;
  if (on != h->b_samp && h->samp_m) {  // the pending outcomes are the other reading's
    cand_invalidate(h);
    h->samp_ran = false;
  }
  h->b_samp = on;
  return YODA_OK;
}

int yoda_mode_b_sampling_info(const yoda_t* h, uint32_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  out[0] = h->b_samp ? 1u : 0u;
  out[1] = h->b_samp_last ? 1u : 0u;
  out[2] = h->b_rank_builds;
  out[3] = h->b_samp_last_elig ? 1u : 0u;
  return YODA_OK;
}

int yoda_greedy_candidates(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  h->greedy_cand = enable != 0;
  return YODA_OK;
}

int yoda_shard_candidates(yoda_t* h, int enable) {
  if (!h) return YODA_ERR_INVALID_ARG;
  const bool on = enable != 0;
  // (a step begun under the other setting does not continue under this one)
  if (on != h->shard_cand && h->cand_classes) cand_invalidate(h);
  h->shard_cand = on;
  return YODA_OK;
}

int yoda_mode_b_info(const yoda_t* h, uint32_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  out[0] = h->b_follow ? 1u : 0u;
  out[1] = h->b_last_ncls;
  out[2] = h->b_last_elig ? 1u : 0u;
  out[3] = h->b_elig_builds;
  return YODA_OK;
}

int yoda_candidates_profile(yoda_t* h, double* narrow_ms) {
  if (!h || !narrow_ms) return YODA_ERR_INVALID_ARG;
  *narrow_ms = h->cand_ms;
  h->cand_ms = 0;
  return YODA_OK;
}

int yoda_candidates_info(const yoda_t* h, uint32_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  out[0] = h->cand_classes;
  out[1] = (uint32_t)h->h_cls.size();
  out[2] = 0;
  if (h->cand_classes) {
    const uint64_t all = h->cand_classes == 64 ? ~0ull : (1ull << h->cand_classes) - 1ull;
    for (uint64_t w : h->h_cand) out[2] += (w & all) != all;
  }
  return YODA_OK;
}

uint32_t yoda_num_feasible_to_find(uint32_t n_nodes, int32_t percentage) {
  // numFeasibleNodesToFind (generic_scheduler.go, k8s v1.22.3): minFeasibleNodesToFind = 100,
  // minFeasibleNodesPercentageToFind = 5, the adaptive default 50 - n / 125
  const int64_t n = n_nodes;
  if (n < 100 || percentage >= 100) return n_nodes;
  int64_t a = percentage;
  if (a <= 0) a = std::max<int64_t>(5, 50 - n / 125);
  return (uint32_t)std::max<int64_t>(n * a / 100, 100);
}

int yoda_set_node_sampling(yoda_t* h, uint32_t num_to_find, uint32_t n_pods,
                           const uint32_t* start) {
  if (!h) return YODA_ERR_INVALID_ARG;
  auto invalidate = [&]() {
    cand_invalidate(h);
    h->diag_done = false;
    h->ran_bitmask = false;
    h->samp_ran = false;
  };
  if (num_to_find == 0) {
    if (h->samp_m) invalidate();
    h->samp_m = 0;
    h->h_start.clear();
    return YODA_OK;
  }
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (!start) n_pods = 0;
  for (uint32_t p = 0; p < n_pods; ++p)
    if (start[p] < h->node_offset || start[p] - h->node_offset >= h->n_nodes)
      return fail(h, YODA_ERR_RANGE, "yoda_set_node_sampling: a start id is outside the shard");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<uint32_t> loc(n_pods);
    for (uint32_t p = 0; p < n_pods; ++p) loc[p] = start[p] - h->node_offset;
    if (n_pods) {
      HIP_TRY(h, h->samp_start.ensure((size_t)n_pods * 4));
      HIP_TRY(h, hipMemcpyAsync(h->samp_start.p, loc.data(), (size_t)n_pods * 4,
                                hipMemcpyHostToDevice, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the copy's source is pageable)
    }
    invalidate();
    h->h_start.swap(loc);
    h->samp_m = num_to_find;
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_download_sampling(yoda_t* h, uint32_t* n_found, uint32_t* next_start) {
  if (!h) return YODA_ERR_INVALID_ARG;
  // (a Mode B run answers when it took the sampled kernels: yoda_mode_b_sampling)
  if (!h->ran || h->k3_pending || !h->samp_m ||
      (h->last_mode != YODA_MODE_SCV && !(h->b_samp_last || h->n_pods == 0)) ||
      !(h->samp_ran || h->n_pods == 0))
    return fail(h, YODA_ERR_STATE, "yoda_download_sampling before a sampled yoda_run");
  const uint32_t P = h->n_pods;
  if (P == 0) return YODA_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  const uint32_t* d = h->samp_out.as<uint32_t>();
  if (n_found)
    HIP_TRY(h, hipMemcpyAsync(n_found, d, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
  if (next_start)
    HIP_TRY(h, hipMemcpyAsync(next_start, d + P, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return YODA_OK;
}

int yoda_sampling_info(const yoda_t* h, uint32_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  out[0] = h->samp_m;
  out[1] = (uint32_t)h->h_start.size();
  out[2] = h->samp_ran ? 1u : 0u;
  return YODA_OK;
}

int yoda_sampling_profile(yoda_t* h, double* pass_ms) {
  if (!h || !pass_ms) return YODA_ERR_INVALID_ARG;
  *pass_ms = h->samp_ms;
  h->samp_ms = 0;
  return YODA_OK;
}

int yoda_snapshot_check(yoda_t* h, uint64_t* digest, uint32_t* mismatch) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->has_nodes) return fail(h, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  if (!digest || !mismatch) return fail(h, YODA_ERR_INVALID_ARG, "NULL buffer");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t N = h->n_nodes;
    const int K = h->K;
    const bool n32 = h->path == Path::N32;
    for (int k = 0; k < 8; ++k) digest[k] = 0;
    for (int k = 0; k < 4; ++k) mismatch[k] = 0;
    if (n32 && h->blksum_loose) HIP_TRY(h, tighten_block_sums(h));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    auto hash = [](const std::vector<uint32_t>& v) {
      uint64_t x = 0xcbf29ce484222325ull;
      for (uint32_t w : v) x = (x ^ w) * 0x100000001b3ull;
      return x;
    };
    auto fetch = [&](const DevBuf& b, size_t words, std::vector<uint32_t>& out) -> int {
      out.assign(words, 0u);
      if (words) HIP_TRY(h, hipMemcpy(out.data(), b.p, words * 4, hipMemcpyDeviceToHost));
      return YODA_OK;
    };
    int rc;
    const size_t stride = n32 ? n32_stride(K) : node_stride(K);
    std::vector<uint32_t> rec;
    if ((rc = fetch(h->nodes, (size_t)N * stride / 4, rec))) return rc;
    digest[0] = hash(rec);
    for (size_t w = 0; w < rec.size(); ++w) {
      uint32_t hw;
      std::memcpy(&hw, h->host_records.data() + 4 * w, 4);
      mismatch[3] += hw != rec[w];
    }
    if (!n32 || N == 0) return YODA_OK;
    std::vector<uint32_t> ids, a, b;
    if (h->perm_on && (rc = fetch(h->perm_ids, N, ids))) return rc;
    for (const SumTable& t : sum_tables(K)) {
      if ((rc = fetch(h->*t.base, sum_words(N, t.stride), a))) return rc;
      digest[t.digest] = hash(a);
      if (t.base == &yoda_handle::k2sum)
        for (size_t w = 0; w < a.size() && w < h->host_k2sum.size(); ++w)
          mismatch[3] += a[w] != h->host_k2sum[w];
      if (!h->perm_on) continue;
      if ((rc = fetch(h->*t.grouped, sum_words(N, t.stride), b))) return rc;
      for (uint32_t q = 0; q < N; ++q)
        for (uint32_t w = 0; w < t.stride / 4u; ++w)
          mismatch[0] += b[sum_index(q, w, t.stride)] != a[sum_index(ids[q], w, t.stride)];
    }
    // the stored block summaries of both orders against a fresh build (k_bsum_build run now)
    const size_t bw = sum_words((N + 63) / 64, bsum_stride(K));
    HIP_TRY(h, h->bsum_chk.ensure(bw * 4));
    for (int o = 0; o < (h->perm_on ? 2 : 1); ++o) {
      HIP_TRY(h, hipMemsetAsync(h->bsum_chk.p, 0, bw * 4, h->stream));
      HIP_TRY(h, launch_bsum_build(K, (o ? h->k1sum_p : h->k1sum).as<uint32_t>(),
                                   (o ? h->k2sum_p : h->k2sum).as<uint32_t>(),
                                   (o ? h->kx1_p : h->kx1).as<uint32_t>(),
                                   (o ? h->kmix_p : h->kmix).as<uint32_t>(), N,
                                   h->bsum_chk.as<uint32_t>(), h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      if ((rc = fetch(o ? h->blksum_p : h->blksum, bw, a))) return rc;
      if ((rc = fetch(h->bsum_chk, bw, b))) return rc;
      if (o == 0) digest[5] = hash(a);
      for (size_t w = 0; w < bw; ++w) mismatch[1 + o] += a[w] != b[w];
    }
    if ((rc = fetch(h->gtab_aux, kGTabAuxBytes / 4, a))) return rc;
    digest[7] = hash(a);
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_topk_depth(const yoda_t* h) {
  if (!h) return YODA_ERR_INVALID_ARG;
  // the capacity windows' deeper lists after the witness phase 1 (yoda_greedy's depths)
  return h->phase1_wit ? topk_k_capacity() : topk_k();
}

namespace {
int shard_topk_impl(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_counts, uint32_t k,
                    uint32_t deep, uint32_t* counts, double* top_score, uint32_t* top_node);
}  // namespace

int yoda_shard_topk(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_counts, uint32_t k,
                    uint32_t* counts, double* top_score, uint32_t* top_node) {
  return shard_topk_impl(h, d_maxima, d_counts, k, 0, counts, top_score, top_node);
}

namespace {
// deep > 0 (libyoda's sharded capacity windows): lists `deep` long, exact down to their last
// entry, at least min(k, n_feasible) entries, and empty past it -- the k-deep chunk lists merged
// deeper where the block kernels run (k_topk_merge_deep), else the k-deep lists padded --
// whatever this shard's kernels.
int shard_topk_impl(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_counts, uint32_t k,
                    uint32_t deep, uint32_t* counts, double* top_score, uint32_t* top_node) {
  if (!h) return YODA_ERR_INVALID_ARG;
  int rc = cand_refuse(h, "yoda_shard_topk");
  if (rc) return rc;
  if ((rc = check_ready(h, YODA_MODE_SCV))) return rc;
  if (h->xo)  // (the window top-k reads the shared radix order's buffers)
    return fail(h, YODA_ERR_STATE, "yoda_shard_topk after a caller-order phase 1: turn "
                                   "yoda_shard_exchange_order off for greedy windows");
  if (!h->phase1_done) return fail(h, YODA_ERR_STATE, "yoda_shard_topk before yoda_shard_phase1");
  if (h->generic)
    return fail(h, YODA_ERR_STATE, "top-k lists need a fast record path (N32 or F64)");
  if (!d_maxima || !d_counts || !counts || !top_score || !top_node)
    return fail(h, YODA_ERR_INVALID_ARG, "NULL buffer");
  const uint32_t KT = (uint32_t)yoda_shard_topk_depth(h);
  if (k != KT)
    return fail(h, YODA_ERR_INVALID_ARG,
                "yoda_shard_topk: k = " + std::to_string(k) + " but this phase 1 lists " +
                    std::to_string(KT) + " candidates per pod (yoda_shard_topk_depth)");
  try {
    const uint32_t P = h->n_pods, N = h->n_nodes;
    h->h_pos.resize(P);
    for (uint32_t i = 0; i < P; ++i) h->h_pos[i] = i;
    h->topk_ready = false;
    if (P == 0) return YODA_OK;
    const uint32_t KO = std::max(KT, deep);  // the depth written to the caller
    std::vector<uint32_t> cnt(2 * (size_t)P), ti((size_t)KO * P, 0xffffffffu), perm(P);
    std::vector<double> ts((size_t)KO * P, -1.0);
    uint32_t KD = KT;  // the depth the device lists hold
    HIP_TRY(h, hipMemcpyAsync(h->maxima.p, d_maxima, 6ull * P * 8, hipMemcpyDeviceToDevice,
                              h->stream));
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), d_counts, 2ull * P * 4, hipMemcpyDeviceToHost,
                              h->stream));
    if (N > 0) {
      HIP_TRY(h, launch_prep2(h->maxima.as<uint64_t>(), P, h->rcp.as<double>(),
                               h->stream));
      if (deep > KT && topk_block_ok(h)) {
        // (the chunks' lists at this phase 1's depth: a deep list is never shorter than the
        // KT-deep list yoda_shard_topk gives -- with 8-deep chunk lists after the witness phase
        // 1, pods whose best scores all tie came back with 8 entries of 300 feasible nodes)
        if ((rc = topk_lists(h, P, KT, d_counts, deep, &KD))) return rc;
      } else if ((rc = topk_lists(h, P, KT, d_counts))) {
        return rc;
      }
      HIP_TRY(h, hipMemcpyAsync(ts.data(), h->tk_s.p, (size_t)KD * P * 8, hipMemcpyDeviceToHost,
                                h->stream));
      HIP_TRY(h, hipMemcpyAsync(ti.data(), h->tk_i.p, (size_t)KD * P * 4, hipMemcpyDeviceToHost,
                                h->stream));
    }
    if (h->ordered)
      HIP_TRY(h, hipMemcpyAsync(perm.data(), h->perm.p, (size_t)P * 4, hipMemcpyDeviceToHost,
                                h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->ordered)
      for (uint32_t q = 0; q < P; ++q) h->h_pos[perm[q]] = q;  // perm[q]: pod at sorted q
    for (uint32_t i = 0; i < P; ++i) {
      const uint32_t q = h->h_pos[i];
      counts[i] = cnt[q];
      counts[(size_t)P + i] = cnt[(size_t)P + q];
      for (uint32_t k = 0; k < KO; ++k) {
        top_score[(size_t)k * P + i] = k < KD ? ts[(size_t)k * P + q] : -1.0;
        top_node[(size_t)k * P + i] = k < KD ? ti[(size_t)k * P + q] : 0xffffffffu;
      }
    }
    h->topk_ready = true;
    return YODA_OK;
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}
}  // namespace

int yoda_shard_phase1_witness(yoda_t* h, uint64_t* d_maxima, uint32_t* d_counts,
                              uint32_t* d_wit) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_phase1_witness")) return rc;
  h->xo = false;  // (greedy windows: the shared radix order)
  int rc = prepare_run(h, YODA_MODE_SCV);
  if (rc) return rc;
  if (h->generic)
    return fail(h, YODA_ERR_STATE, "witness phase 1 needs a fast record path (N32 or F64)");
  if (!d_maxima || !d_counts || !d_wit) return fail(h, YODA_ERR_INVALID_ARG, "NULL buffer");
  try {
    if ((rc = order_pods(h, YODA_MODE_SCV, true))) return rc;
    if ((rc = phase1_witness(h, d_maxima, d_counts, d_wit, h->node_offset))) return rc;
    h->phase1_done = true;
    h->phase1_wit = true;
    h->ran = false;
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_witness_prepare(yoda_t* h, const uint64_t* d_maxima_global,
                               const uint64_t* d_maxima_local, uint32_t* d_wit) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_witness_prepare")) return rc;
  if (!d_maxima_global || !d_maxima_local || !d_wit)
    return fail(h, YODA_ERR_INVALID_ARG, "NULL buffer");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, launch_wit_prepare(d_maxima_global, d_maxima_local, h->n_pods, d_wit, h->stream));
  return YODA_OK;
}

int yoda_shard_witness_download(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_wit,
                                uint64_t* maxima, uint32_t* wit) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_witness_download")) return rc;
  if (!d_maxima || !d_wit || !maxima || !wit) return fail(h, YODA_ERR_INVALID_ARG, "NULL buffer");
  if (!h->topk_ready)
    return fail(h, YODA_ERR_STATE, "yoda_shard_witness_download before yoda_shard_topk");
  try {
    const uint32_t P = h->n_pods;
    if (P == 0) return YODA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<uint64_t> mx(6 * (size_t)P);
    std::vector<uint32_t> wt(12 * (size_t)P);
    HIP_TRY(h, hipMemcpyAsync(mx.data(), d_maxima, mx.size() * 8, hipMemcpyDeviceToHost,
                              h->stream));
    HIP_TRY(h, hipMemcpyAsync(wt.data(), d_wit, wt.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < P; ++i) {
      const uint32_t q = h->h_pos[i];
      for (int f = 0; f < 6; ++f) maxima[(size_t)f * P + i] = mx[(size_t)f * P + q];
      for (int f = 0; f < 12; ++f) wit[(size_t)f * P + i] = wt[(size_t)f * P + q];
    }
    return YODA_OK;
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_shard_best_one(yoda_t* h, uint32_t pod, double* score, int32_t* node) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (int rc = cand_refuse(h, "yoda_shard_best_one")) return rc;
  if (!score || !node) return fail(h, YODA_ERR_INVALID_ARG, "NULL output");
  if (!h->topk_ready) return fail(h, YODA_ERR_STATE, "yoda_shard_best_one before yoda_shard_topk");
  if (pod >= h->n_pods) return fail(h, YODA_ERR_INVALID_ARG, "pod index out of range");
  *score = -1.0;
  *node = -1;
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->n_nodes == 0) return YODA_OK;
  const uint32_t s = h->h_pos[pod];
  const uint32_t nb = greedy_one_blocks();
  if (h->g1_done.bytes == 0) {
    HIP_TRY(h, h->g1_done.ensure(16));
    HIP_TRY(h, hipMemsetAsync(h->g1_done.p, 0, 16, h->stream));
  }
  HIP_TRY(h, h->g1_part.ensure((size_t)nb * 12 + 16));
  double* ps = h->g1_part.as<double>();
  uint32_t* pi = reinterpret_cast<uint32_t*>(ps + nb);
  uint32_t* done = h->g1_done.as<uint32_t>();
  HIP_TRY(h, launch_greedy_one(h->K, h->path, h->nodes.as<unsigned char>(),
                               h->has_k2sum ? h->k2sum.as<unsigned char>() : nullptr, h->n_nodes,
                               pod_params(h), h->rcp.as<double>(), 
                               h->n_pods, s, h->bitmask.as<uint64_t>(), bm_row(h->n_nodes),
                               h->bs_ptr(), bs_row(h->n_nodes), h->blk_ptr(),
                               blk_row(h->n_nodes), ps, pi, done, done + 1, h->stream));
  HIP_TRY(h, h->pick_stage.ensure(16));
  HIP_TRY(h, hipMemcpyAsync(h->pick_stage.p, done, 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const unsigned char* st = static_cast<const unsigned char*>(h->pick_stage.p);
  uint32_t n;
  double b;
  std::memcpy(&n, st + 4, 4);
  std::memcpy(&b, st + 8, 8);
  if (n != 0xffffffffu) {
    *node = (int32_t)(n + h->node_offset);
    *score = b;
  }
  return YODA_OK;
}

}  // extern "C"

// Pod p of `pods` scheduled exactly against the CURRENT device node state (k_one_*: Filter,
// CollectMaxValues, Score, then k8s' outcome rules as k_finalize applies them).  Local pick.
// cls: the pod's candidate class (YODA_CAND_ANY, or candidates off: the unrestricted kernels).
static int greedy_eval_exact(yoda_t* h, const yoda_pod_soa* pods, uint32_t p, uint8_t cls,
                             int32_t* pick) {
  const uint32_t N = h->n_nodes;
  *pick = YODA_PICK_NONE;
  if (N == 0) return YODA_OK;
  OnePod op{};
  const uint64_t number = pods->has_number[p] ? pods->number[p] : 1;  // filter.go:12-15
  const uint32_t need = number > 0xffffffffull ? 0xffffffffu : (uint32_t)number;
  const uint64_t m = pods->has_memory[p] ? pods->memory[p] : 0;
  const uint64_t c = pods->has_clock[p] ? pods->clock[p] : 0;
  op.number = number;
  op.need_mem = pods->has_memory[p] ? need : 0;
  op.need_clk = pods->has_clock[p] ? need : 0;
  op.m32 = (uint32_t)std::min<uint64_t>(m, 0xffffffffull);
  if (h->mem_ranks)  // the rank threshold (yoda_layout.h MemTab)
    op.m32 = 2u + (uint32_t)(std::lower_bound(h->h_frees.begin(), h->h_frees.end(), m) -
                             h->h_frees.begin());
  op.c32 = (uint32_t)std::min<uint64_t>(c, 0xffffffffull);
  op.mf = (double)std::min<uint64_t>(m, 1ull << 53);
  op.cf = (double)std::min<uint64_t>(c, 1ull << 53);
  HIP_TRY(h, h->one_feas.ensure(((size_t)N + 63) / 64 * 8 + 64));
  HIP_TRY(h, h->one_part.ensure((size_t)one_blocks() * 9 * 8));
  HIP_TRY(h, h->one_out.ensure(sizeof(OneOut)));
  if (h->one_done.bytes == 0) {
    HIP_TRY(h, h->one_done.ensure(16));
    HIP_TRY(h, hipMemsetAsync(h->one_done.p, 0, 16, h->stream));
  }
  HIP_TRY(h, launch_one(h->K, h->path, h->nodes.as<unsigned char>(), N, op,
                        h->one_feas.as<uint64_t>(), h->one_part.p, h->one_done.as<uint32_t>(),
                        h->one_out.as<OneOut>(), pod_params(h).mt, h->stream,
                        h->cand_classes && cls != YODA_CAND_ANY ? h->cand_w.as<uint64_t>() : nullptr,
                        cls));
  HIP_TRY(h, h->pick_stage.ensure(sizeof(OneOut)));
  HIP_TRY(h, hipMemcpyAsync(h->pick_stage.p, h->one_out.p, sizeof(OneOut), hipMemcpyDeviceToHost,
                            h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  OneOut o;
  std::memcpy(&o, h->pick_stage.p, sizeof(o));
  if (o.nf == 0)
    *pick = YODA_PICK_NONE;
  else if (o.nf == 1)  // k8s: the only feasible node is returned without scoring
    *pick = (int32_t)o.first;
  else if (o.nz > 0)   // Score would divide by TotalMemorySum == 0
    *pick = YODA_PICK_ERROR;
  else
    *pick = (int32_t)o.idx;
  return YODA_OK;
}

// ---- the greedy batch on one handle (yoda_greedy, Mode A) --------------------------------
// One driver for flags 0, YODA_GREEDY_CARD_CAPACITY and the exact sequence of the U64 record
// path (greedy).  The sequential part is the host session's
// (yoda_greedy_session.h), built from the handle's host copies over its LOCAL node ids; the
// driver evaluates windows of pods on the device against the state at the window start (K1 or
// k1_witness + top-k K2), hands the lists to the session in window order, answers the pods the
// session cannot certify, and pushes the nodes the session changed.  Inside the batch the
// handle's node_offset is 0, so every kernel writes local ids; the picks get the offset once,
// at the end, and the snapshot its original node state.
namespace {

// The handle's host copies as the session's snapshot; with_cards: the cards too, decoded from
// the host copy of the records, for the capacity certificate's exact witness accounting
// (CardField order: free, clock, total, bandwidth, core, power).
struct HostNodes {
  yoda_node_soa nv{};
  std::vector<uint32_t> ccount;
  std::vector<uint64_t> fld[6];
  std::vector<uint8_t> healthy;
  HostNodes(const yoda_t* h, bool with_cards) {
    const uint32_t N = h->n_nodes, K = (uint32_t)h->K;
    nv.n_nodes = N;
    nv.max_cards = 1;
    nv.card_number = h->h_card_number.data();
    nv.free_memory_sum = h->h_free_sum.data();
    nv.total_memory_sum = h->h_total_sum.data();
    nv.alloc_memory = h->h_alloc.data();
    if (!with_cards) return;
    const size_t stride = h->path == Path::N32 ? n32_stride(h->K) : node_stride(h->K);
    ccount.resize(N);
    healthy.resize((size_t)N * K);
    for (auto& v : fld) v.resize((size_t)N * K);
    for (uint32_t n = 0; n < N; ++n) {
      const unsigned char* r = h->host_records.data() + (size_t)n * stride;
      const NodeHdrG* hd = reinterpret_cast<const NodeHdrG*>(r);
      ccount[n] = (uint32_t)__builtin_popcount(hd->real_mask);
      for (uint32_t j = 0; j < K; ++j) {
        healthy[(size_t)n * K + j] = (hd->healthy_mask >> j) & 1u;
        for (int f = 0; f < 6; ++f)
          fld[f][(size_t)n * K + j] =
              h->path == Path::N32
                  ? reinterpret_cast<const uint32_t*>(r + n32_u32_off(f, h->K))[j]
                  : (uint64_t) reinterpret_cast<const double*>(r + 32 + 8 * (size_t)f * K)[j];
        if (h->path == Path::N32) {  // memory values from the f64 groups (the u32 ones may be ranks)
          fld[kFree][(size_t)n * K + j] =
              (uint64_t) reinterpret_cast<const double*>(r + n32_f64_off(kF64Free, h->K))[j];
          fld[kTotal][(size_t)n * K + j] =
              (uint64_t) reinterpret_cast<const double*>(r + n32_f64_off(kF64Total, h->K))[j];
        }
      }
    }
    nv.max_cards = K;
    nv.card_count = ccount.data();
    nv.card_free_memory = fld[kFree].data();
    nv.card_clock = fld[kClock].data();
    nv.card_total_memory = fld[kTotal].data();
    nv.card_bandwidth = fld[kBandwidth].data();
    nv.card_core = fld[kCore].data();
    nv.card_power = fld[kPower].data();
    nv.card_healthy = healthy.data();
  }
};

// The pod classes of a batch with candidates on (yoda_greedy_candidates).  The caller's array is
// in input order and as long as the batch; the batch uploads its pods window by window in queue
// order.  begin() takes the caller's array off the handle and puts the batch's own device copy
// in queue order (cls[order[q]]) in its place; window() points what phase 1, cand_ready and Mode
// B's class keys read -- h_cls and cls_off -- at the uploaded slice [ws, ws + wn), which
// k_cand_narrow reads through the window's sort permutation.  The destructor puts the caller's
// array back, host and device, on every exit path.
struct GreedyClasses {
  yoda_t* h;
  std::vector<uint8_t> caller, queue;
  DevBuf dev;
  bool on = false;
  explicit GreedyClasses(yoda_t* x) : h(x) {}
  GreedyClasses(const GreedyClasses&) = delete;
  GreedyClasses& operator=(const GreedyClasses&) = delete;
  int begin(const uint32_t* order, uint32_t P) {
    if (!h->cand_classes || h->h_cls.empty() || P == 0) return YODA_OK;
    queue.resize(P);
    for (uint32_t q = 0; q < P; ++q) queue[q] = h->h_cls[order[q]];
    HIP_TRY(h, dev.ensure(P));
    HIP_TRY(h, hipMemcpyAsync(dev.p, queue.data(), P, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the copy's source is pageable)
    caller.swap(h->h_cls);
    h->cand_cls.swap(dev);
    on = true;
    window(0, P);
    return YODA_OK;
  }
  void window(uint32_t ws, uint32_t wn) {
    if (!on) return;
    h->h_cls.assign(queue.begin() + ws, queue.begin() + ws + wn);
    h->cls_off = ws;
  }
  // the class of the pod at queue position q
  uint8_t at(uint32_t q) const { return on ? queue[q] : (uint8_t)YODA_CAND_ANY; }
  ~GreedyClasses() {
    if (!on) return;
    h->h_cls.swap(caller);
    h->cand_cls.swap(dev);
    h->cls_off = 0;
    cand_invalidate(h);  // (the pending outcomes are a window's)
  }
};

// One batch: the handle with its node ids local (node_offset 0 until the batch ends), the
// session, and the one push -- the nodes the session changed since the last push, or
// (original) every node it touched as the snapshot had it, to the device.
struct GreedyBatch {
  yoda_t* h;
  const uint32_t node_offset;
  yoda_gs_t* g = nullptr;
  GreedyClasses cls;
  std::vector<uint32_t> ids;
  std::vector<uint64_t> al, cn;
  static constexpr bool kMapped = true;  // (push_node_state)
  explicit GreedyBatch(yoda_t* x) : h(x), node_offset(x->node_offset), cls(x) {
    h->node_offset = 0;
  }
  ~GreedyBatch() {
    h->node_offset = node_offset;
    if (g) yoda_gs_destroy(g);
  }
  int push(bool original = false) {
    const uint32_t cap = (uint32_t)(original ? g->ever_list.size() : g->dirty_list.size());
    if (cap == 0) return YODA_OK;
    ids.resize(cap), al.resize(cap), cn.resize(cap);
    uint32_t got = 0;
    const int r = original
                      ? yoda_gs_touched_original(g, cap, ids.data(), al.data(), cn.data(), &got)
                      : yoda_gs_take_dirty(g, cap, ids.data(), al.data(), cn.data(), &got);
    if (r) return fail(h, r, "greedy: node state");
    for (uint32_t t = 0; t < got; ++t) {  // Allocate -> the static score
      bool z;
      al[t] = static_score(h->h_free_sum[ids[t]], h->h_total_sum[ids[t]], al[t], &z);
    }
    return push_node_state(h, got, ids.data(), al.data(), cn.data(), kMapped);
  }
};

FILE* greedy_trace_file() {
  static FILE* f = [] {
    const char* p = std::getenv("YODA_GREEDY_TRACE");
    return p && *p ? std::fopen(p, "w") : nullptr;
  }();
  return f;
}

// The windowed resolve of the fast record paths.  Each window is evaluated on the device against
// the state at its start and resolved by the session in queue order; what happens to a pod the
// session cannot certify is the mode's policy:
//   flags 0   it is evaluated exactly against the current state, reusing the window's
//             feasibility bits and maxima (greedy_eval_fast: only static scores change inside a
//             window) -- after a mid-window list refresh when the window's lists went stale
//             (greedy_refresh()); once Allocate has wrapped past 2^64 in a window no list
//             certifies any more and the rest of the window is evaluated that way;
//   capacity  it is scheduled exactly (k_one_*) while such pods stay rare in the window, else it
//             opens the next window, so it is evaluated against the current state there; the
//             window size adapts to how far the last window got.
int greedy_windows(GreedyBatch& b, const yoda_pod_soa* pods, bool capacity) {
  using Clock = std::chrono::steady_clock;
  auto ms_since = [](Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
  };
  yoda_t* h = b.h;
  yoda_gs_t* g = b.g;
  const uint32_t P = pods->n_pods, N = h->n_nodes;
  // the chunks' list depth.  Capacity: 8 where the lists are merged deeper (k_topk_merge_deep:
  // the same 64-deep lists as from 16, and a cheaper K2 -- 1.00-1.02 vs 1.07-1.09 s,
  // profiles/r05/pqr/tk_ab.txt), else 16.  Flags 0: 8 (YODA_GREEDY_TOPK=16, A/B knob: 16)
  static const uint32_t kt_env = YODA_KNOB("YODA_GREEDY_TOPK", 0);
  const bool kt_cap = capacity ? !topk_block_ok(h) : kt_env == (uint32_t)topk_k_capacity();
  const uint32_t KT = (uint32_t)(kt_cap ? topk_k_capacity() : topk_k());
  // the capacity lists' depth: KT from the chunks, merged deeper where the block kernels run
  // (k_topk_merge_deep: exact as far as they reach; YODA_GREEDY_CAP_DEPTH, A/B knob: 32 /
  // 64 / 128, 0 = KT).  128 with the exact-fallback scan below (windows 1558 -> 822,
  // capacity 0.97 -> 0.89-0.90 s; 128 alone 0.98 s, the scan alone 0.92-0.93 s;
  // profiles/r06/greedy_scan/)
  static const uint32_t cap_depth = YODA_KNOB("YODA_GREEDY_CAP_DEPTH", 128);
  const uint32_t deep = capacity ? cap_depth : 0u;
  const GreedyRefresh& rf = greedy_refresh();
  // Small windows: the GPU work is the same P x N in total, while fewer nodes are touched per
  // window, so fewer candidate lists lose certification.
  const uint32_t Wmax = greedy_window();
  uint32_t W = Wmax, ws = 0;
  PodGather win;
  std::vector<uint32_t> pos, cnt_w, ti_w, wc_w, ti_s, ti_r;
  std::vector<uint64_t> mx_w;
  std::vector<double> ts_w, ts_s, ts_r;
  int rc;
  while (ws < P) {
    const auto tw = Clock::now();
    if ((rc = b.push())) return rc;
    const uint32_t wn = std::min(W, P - ws);
    win.build(pods, g->order.data() + ws, wn);
    b.cls.window(ws, wn);
    if ((rc = yoda_upload_pods(h, &win.soa))) return rc;
    const double t_up = ms_since(tw);
    if ((rc = prepare_run(h, YODA_MODE_SCV))) return rc;
    // sort the window like any batch (whole waves skip nodes); k_window_out brings the outputs
    // back to window order
    if ((rc = order_pods(h, YODA_MODE_SCV))) return rc;
    h->greedy_prep_ms += ms_since(tw);
    HIP_TRY(h, h->wit.ensure(12 * (size_t)wn * 4));  // (flags 0: staged with the rest, unread)
    if (capacity)
      rc = phase1_witness(h, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(),
                          h->wit.as<uint32_t>(), 0);
    else if (N > 0)
      rc = phase1(h, YODA_MODE_SCV, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(),
                  Maxima::Own);
    if (rc) return rc;
    uint32_t KD = KT;
    // pinned staging of the window's outputs, in window order (k_window_out writes them there
    // from the sorted order in one launch): counts | maxima | wit | top scores | top nodes
    size_t o_cnt = 0, o_mx = 0, o_wit = 0, o_ts = 0, o_ti = 0, total = 0;
    auto layout = [&](uint32_t kd) {
      o_cnt = 0, o_mx = o_cnt + 8 * (size_t)wn, o_wit = o_mx + 48 * (size_t)wn,
      o_ts = o_wit + 48 * (size_t)wn, o_ti = o_ts + 8 * (size_t)kd * wn,
      total = o_ti + 4 * (size_t)kd * wn;
    };
    layout(std::max(KT, deep));
    HIP_TRY(h, h->win_stage.ensure(total));
    unsigned char* st = static_cast<unsigned char*>(h->win_stage.p);
    const uint32_t *cnt_p, *wc_p, *ti_p;
    const uint64_t* mx_p;
    const double* ts_p;
    double t_issued, t_sync;
    if (N > 0) {
      HIP_TRY(h, launch_prep2(h->maxima.as<uint64_t>(), wn, h->rcp.as<double>(),
                               h->stream));
      if ((rc = topk_lists(h, wn, KT, h->counts.as<uint32_t>(), deep, &KD))) return rc;
      layout(KD);
      // (YODA_WIN_DMA=0, A/B knob: k_window_out writes the pinned pages directly)
      static const bool win_dma = YODA_KNOB("YODA_WIN_DMA", 1) != 0;
      if (win_dma) HIP_TRY(h, h->win_dev.ensure(total));
      HIP_TRY(h, h->win_inv.ensure((size_t)wn * 4));
      HIP_TRY(h, launch_window_out(h->counts.as<uint32_t>(), h->maxima.as<uint64_t>(),
                                   h->wit.as<uint32_t>(), h->tk_s.as<double>(),
                                   h->tk_i.as<uint32_t>(),
                                   h->ordered ? h->perm.as<uint32_t>() : nullptr, wn, KD, true,
                                   win_dma ? h->win_dev.as<unsigned char>()
                                           : static_cast<unsigned char*>(h->win_stage.dp),
                                   h->win_inv.as<uint32_t>(), h->stream));
      if (win_dma)
        HIP_TRY(h, hipMemcpyAsync(h->win_stage.p, h->win_dev.p, total, hipMemcpyDeviceToHost,
                                  h->stream));
      if (!capacity) {  // pos[i] = sorted position of window pod i: k_greedy_one's address
        pos.resize(wn);
        HIP_TRY(h, hipMemcpyAsync(pos.data(), h->win_inv.p, (size_t)wn * 4,
                                  hipMemcpyDeviceToHost, h->stream));
      }
      t_issued = ms_since(tw);
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      t_sync = ms_since(tw);
      cnt_p = reinterpret_cast<const uint32_t*>(st + o_cnt);
      mx_p = reinterpret_cast<const uint64_t*>(st + o_mx);
      wc_p = reinterpret_cast<const uint32_t*>(st + o_wit);
      ts_p = reinterpret_cast<const double*>(st + o_ts);
      ti_p = reinterpret_cast<const uint32_t*>(st + o_ti);
    } else {  // no nodes: every pod infeasible
      t_issued = ms_since(tw);
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      t_sync = ms_since(tw);
      cnt_w.assign(2 * (size_t)wn, 0u);
      mx_w.assign(6 * (size_t)wn, 1ull);
      wc_w.assign(12 * (size_t)wn, 0u);
      for (size_t t = 6 * (size_t)wn; t < 12 * (size_t)wn; ++t) wc_w[t] = 0xffffffffu;
      ts_w.assign((size_t)KD * wn, -1.0);
      ti_w.assign((size_t)KD * wn, 0xffffffffu);
      cnt_p = cnt_w.data(), mx_p = mx_w.data(), wc_p = wc_w.data();
      ts_p = ts_w.data(), ti_p = ti_w.data();
    }
    ++h->greedy_windows;
    const double t_win = ms_since(tw);
    h->greedy_window_ms += t_win;
    const auto tr = Clock::now();
    if ((rc = gs_begin_window_at(g, ws, wn, KD, cnt_p, const_cast<double*>(ts_p),
                                 const_cast<uint32_t*>(ti_p), true, N > 0)) ||
        (capacity && (rc = yoda_gs_set_witness(g, mx_p, wc_p, wc_p + 6 * (size_t)wn))))
      return fail(h, rc, "greedy: session window");
    uint32_t next = 0, fails = 0, fb_since = 0;
    double fb_ms = 0;
    uint64_t why0[6];
    std::copy(std::begin(g->why), std::end(g->why), why0);
    for (;;) {
      if ((rc = yoda_gs_resolve(g, &next))) return fail(h, rc, "greedy: resolve");
      if (next >= wn) break;
      const auto tf = Clock::now();
      int32_t pk = YODA_PICK_NONE;
      if (capacity) {
        // YODA_GREEDY_FAIL_DIV (A/B knob): one exact evaluation allowed per that many resolved pods
        static const uint32_t rate = YODA_KNOB("YODA_GREEDY_FAIL_DIV", 0);
        // fall back exactly (instead of restarting the window) when at most
        // YODA_GREEDY_CAP_SCAN_MAX of the next YODA_GREEDY_CAP_SCAN window pods are uncertified
        // already (A/B knobs; 64 / 1: a restart re-runs the window's kernels for one pod whose
        // witness was lost while its successors still hold theirs; 32 / 128 / 256: 0.97 / 0.92 /
        // 0.91 s, 0: 0.97 s)
        static const uint32_t scan_n = YODA_KNOB("YODA_GREEDY_CAP_SCAN", 64);
        static const uint32_t scan_max = YODA_KNOB("YODA_GREEDY_CAP_SCAN_MAX", 1);
        bool fallback = false;
        if (rate) {
          fallback = ++fails <= next / rate;
        } else if (scan_n && wn - next > scan_n) {
          uint64_t saved[6];
          std::copy(std::begin(g->why), std::end(g->why), saved);
          uint32_t unc = 0;
          int32_t dummy;
          for (uint32_t j = next + 1; j <= next + scan_n && unc <= scan_max; ++j)
            unc += g->resolve_capacity(j, g->order[ws + j], &dummy) ? 0u : 1u;
          std::copy(std::begin(saved), std::end(saved), std::begin(g->why));
          fallback = unc <= scan_max;
        }
        if (!fallback) break;
        if ((rc = b.push()) ||
            (rc = greedy_eval_exact(h, pods, g->order[ws + next], b.cls.at(ws + next), &pk)))
          return rc;
      } else {
        if (!g->wrapped && ++fb_since >= rf.every && wn - next >= 2 * rf.scan) {
          fb_since = 0;
          uint32_t unc = 0;
          if ((rc = yoda_gs_uncertified(g, next + 1, rf.scan, &unc)))
            return fail(h, rc, "greedy: scan");
          if (unc >= rf.min) {
            // the window's top-k K2 again, against the current state (its K1 masks and maxima
            // stay valid: only static scores change in this mode); the lists come back in
            // sorted order and go to the session in window order
            if ((rc = b.push()) || (rc = topk_lists(h, wn, KT, h->counts.as<uint32_t>())))
              return rc;
            const size_t ln = (size_t)KT * wn;
            ts_s.resize(ln), ti_s.resize(ln), ts_r.resize(ln), ti_r.resize(ln);
            HIP_TRY(h, hipMemcpyAsync(ts_s.data(), h->tk_s.p, ln * 8, hipMemcpyDeviceToHost,
                                      h->stream));
            HIP_TRY(h, hipMemcpyAsync(ti_s.data(), h->tk_i.p, ln * 4, hipMemcpyDeviceToHost,
                                      h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            for (uint32_t kk = 0; kk < KT; ++kk)
              for (uint32_t j = next; j < wn; ++j) {
                ts_r[(size_t)kk * wn + j] = ts_s[(size_t)kk * wn + pos[j]];
                ti_r[(size_t)kk * wn + j] = ti_s[(size_t)kk * wn + pos[j]];
              }
            if ((rc = yoda_gs_refresh(g, next, ts_r.data(), ti_r.data())))
              return fail(h, rc, "greedy: refresh");
            ++h->greedy_refreshes;
            const uint32_t stuck = next;
            if ((rc = yoda_gs_resolve(g, &next))) return fail(h, rc, "greedy: resolve");
            if (next != stuck) {  // certified now: the resolve went on to a later pod
              fb_ms += ms_since(tf);
              continue;
            }
          }
        }
        if ((rc = b.push()) || (rc = greedy_eval_fast(h, pos[next], &pk))) return rc;
      }
      if ((rc = yoda_gs_assign(g, ws + next, pk))) return fail(h, rc, "greedy: assign");
      ++h->greedy_fallbacks;
      fb_ms += ms_since(tf);
    }
    h->greedy_fallback_ms += fb_ms;
    h->greedy_resolve_ms += ms_since(tr) - fb_ms;
    // YODA_GREEDY_TRACE=<file> (diagnostic, capacity): one line per window -- start, size, pods
    // resolved, the failed certificate (index into why[], -1 = none), pods assigned so far
    FILE* tf = capacity ? greedy_trace_file() : nullptr;
    if (tf) {
      int reason = -1;
      for (int r = 0; r < 6; ++r)
        if (g->why[r] != why0[r]) reason = r;
      uint32_t placed = 0;
      for (uint32_t t = 0; t < next; ++t) placed += g->pick[g->order[ws + t]] >= 0 ? 1u : 0u;
      uint64_t q = 0, nf0 = 0, lq = 0;
      if (next < wn) {
        q = g->need_cards(g->order[ws + next]);
        nf0 = g->counts[next];
        lq = g->lost(q);
      }
      std::fprintf(tf, "%u %u %u %d %u %llu %llu %llu %.1f %.1f %.1f %.1f %.1f\n", ws, wn, next,
                   reason, placed, (unsigned long long)q, (unsigned long long)nf0,
                   (unsigned long long)lq, 1e3 * ms_since(tw), 1e3 * t_up, 1e3 * t_issued,
                   1e3 * t_sync, 1e3 * t_win);
      std::fflush(tf);
    }
    if (next < wn) {
      // pod ws + next could not be certified: it opens the next window (evaluated against the
      // current state, so it is always resolved there), sized after this one's progress
      ++h->greedy_restarts;
      W = yoda_greedy_next_window(next, Wmax);
      ws += next;
    } else {
      ws += wn;
      W = std::min(2 * W, Wmax);
    }
  }
  if (capacity && std::getenv("YODA_GREEDY_DEBUG"))
    std::fprintf(stderr,
                 "greedy capacity: windows %u restarts %u; failed certificates: wrap %llu, "
                 "few-left %llu, zero-total %llu, maxima %llu, list-lost %llu, threshold %llu; "
                 "resolves %llu, lost-node scans %llu visiting %llu nodes\n",
                 h->greedy_windows, h->greedy_restarts, (unsigned long long)g->why[0],
                 (unsigned long long)g->why[1], (unsigned long long)g->why[2],
                 (unsigned long long)g->why[3], (unsigned long long)g->why[4],
                 (unsigned long long)g->why[5], (unsigned long long)g->n_resolve,
                 (unsigned long long)g->n_scan, (unsigned long long)g->n_scan_nodes);
  return YODA_OK;
}

}  // namespace

static int greedy_batch(yoda_t* h, const yoda_pod_soa* pods, int mode, uint32_t flags,
                        int32_t* pick) {
  const bool capacity = (flags & YODA_GREEDY_CARD_CAPACITY) != 0;
  const uint32_t P = pods->n_pods;
  int rc;
  GreedyBatch b(h);
  {
    const HostNodes hn(h, capacity && !h->generic);
    // (the pods' arrays outlive the batch: the session reads them in place)
    if ((rc = gs_create(&hn.nv, pods, capacity ? YODA_GREEDY_CARD_CAPACITY : 0u, true, &b.g)))
      return fail(h, rc, "greedy: session setup failed");
  }
  yoda_gs_t* g = b.g;
  // candidates on (yoda_greedy_candidates): the capacity certificate tells F' from F by the
  // words and classes (host mirrors: local ids, input order); then the classes go to queue order
  if (capacity && h->cand_classes &&
      (rc = yoda_gs_set_candidates(g, h->cand_classes, h->h_cand.data(),
                                   h->h_cls.empty() ? nullptr : h->h_cls.data())))
    return fail(h, rc, "greedy: session candidates");
  if ((rc = b.cls.begin(g->order.data(), P))) return rc;
  if (h->generic) {
    // The U64 normalize check can change after every pick: every pod is evaluated exactly
    // against the current state, in queue order.
    for (uint32_t i = 0; i < P; ++i) {
      int32_t pk = YODA_PICK_NONE;
      b.cls.window(i, 1);  // (the one-pod batch's class)
      if ((rc = b.push()) || (rc = greedy_eval_one(h, pods, g->order[i], mode, &pk))) return rc;
      if ((rc = yoda_gs_assign(g, i, pk))) return fail(h, rc, "greedy: assign");
      ++h->greedy_fallbacks;
    }
  } else if ((rc = greedy_windows(b, pods, capacity))) {
    return rc;
  }
  if ((rc = yoda_gs_picks(g, pick, nullptr, nullptr))) return fail(h, rc, "greedy: picks");
  for (uint32_t p = 0; p < P; ++p)  // the one place the local ids become the caller's
    if (pick[p] >= 0) pick[p] += (int32_t)b.node_offset;
  if (std::getenv("YODA_GREEDY_DEBUG"))
    std::fprintf(stderr, "greedy: windows %u (%.1f ms, of which host prep %.1f ms), fallbacks %u "
                 "(%.1f ms), resolve %.1f ms; mid-window list refreshes %u\n", h->greedy_windows,
                 h->greedy_window_ms, h->greedy_prep_ms, h->greedy_fallbacks,
                 h->greedy_fallback_ms, h->greedy_resolve_ms, h->greedy_refreshes);
  // leave the uploaded snapshot as it was
  if ((rc = b.push(true))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->ran = false;
  return YODA_OK;
}

// Mode B reads no assumed-pod state: independent cycles, in queue order (sort.Less,
// sort.go:8-10 -- scv/priority descending, then input index).  With candidates on (both
// yoda_mode_b_follow and yoda_greedy_candidates) the class array goes to queue order for the run.
static int greedy_mode_b(yoda_t* h, const yoda_pod_soa* pods, int32_t* pick) {
  const uint32_t P = pods->n_pods;
  int rc;
  std::vector<uint32_t> order;
  queue_order(pods->priority, P, order);
  GreedyClasses cls(h);
  if ((rc = cls.begin(order.data(), P))) return rc;
  PodGather all;
  all.build(pods, order.data(), P);
  if ((rc = yoda_upload_pods(h, &all.soa)) || (rc = run_private(h, YODA_MODE_DISKIO, 0, false)))
    return rc;
  std::vector<int32_t> pk(P);
  // the handle's stream may be non-blocking: copy and wait on it, not on the null stream
  HIP_TRY(h, hipMemcpyAsync(pk.data(), h->pick.p, P * 4ull, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (uint32_t i = 0; i < P; ++i) pick[order[i]] = pk[i];
  return YODA_OK;
}

// ---- multi-GPU step inside libyoda (RCCL, no torch) ---------------------------------------
// One node shard per handle; a step is the sharded evaluation of yoda_shard_* with the
// exchanges done here:
//   1. one group of two all-reduces: MAX (u64) over [maxima 6P | score bits, node-id bits]
//      -- CollectMaxValues is a reduction over all nodes; the two trailing words make every
//      shard take the same phase-2 form -- and SUM (u32) over the feasible / zero-total
//      counts [2P];
//   2. fast record paths (and Mode B): the packed-key merge -- each shard's (best score,
//      lowest node reaching it) as one u64 key, all-reduce(MAX) [P], then the winners' tie
//      counts all-reduce(SUM) [P] (k_pack_key / k_unpack_key); the U64 path in Mode A, whose
//      normalize check needs the lowest score too, all-gathers each shard's ShardRec [P]
//      (best, lowest index reaching it, ties, lowest) and folds them (k_merge_rec);
//   3. (rare) the U64 path's exact-normalize records, all-gathered and merged;
//   4. only when the shards draw (yoda_shard_tie_draw beside yoda_set_tie_draw, yoda_comm_run*
//      only): each shard's MIN draw key per tied pod, all-reduce(MIN) [P] u64, then the apply.
// `hs` are the shards this process drives: one handle with an RCCL communicator
// (yoda_comm_run), or every shard of the batch on one device with device copies as the
// transport (yoda_comm_run_local, for tests and single-process use).
static uint32_t bit_length(uint64_t v) {
  uint32_t b = 0;
  while (b < 64 && (v >> b)) ++b;
  return b;
}

// The words every shard contributes to exchange 1 (MAX-reduced with the maxima):
//   [0] score bits and [1] node-id bits this shard needs (the phase-2 form: packed key or
//       records);
//   [2] the shard's largest small card field (bandwidth / clock / core / power) and [3] 1 when
//       the shard's block K2 computes its small-field quotients in f32 (N32 path, every small
//       field <= kF32SmallMax).  The exchanged maxima are the GLOBAL ones, so an
//       f32 shard is exact only while the global small-field max is <= kF32SmallMax too;
//       otherwise the shards must re-upload with YODA_UPLOAD_F64_QUOTIENTS (dist.agree_on_path
//       does) -- quotient_disagreement names that instead of returning inexact scores.
//   [4] a digest of the shard's draw settings (enable, seed, pod_base; 0: no draw in this step)
//       and [5] its bitwise complement: after the MAX the two are complements of each other iff
//       every shard sent the same digest (max d == min d), so every rank sees a disagreement.
//   [6] a digest of the shard's candidate state (yoda_shard_candidates, n_classes, the class
//       array's length and a hash of its bytes; 0: candidates off) and [7] its complement, the same
//       scheme: the counts are SUMMED over the shards, so a shard that narrows by other classes
//       would give wrong picks silently.  The words differ per shard by design and are not in it.
constexpr int kAgreeWords = 8;
constexpr size_t kAgreeBytes = 8 * kAgreeWords;

static uint64_t draw_digest(const yoda_t* h) {
  if (!h->shard_draws()) return 0;
  return tie_mix64(tie_mix64(h->tie_seed) ^ (h->tie_pod_base + 0x9E3779B97F4A7C15ull)) | 1ull;
}

static uint64_t cand_digest(const yoda_t* h) {
  if (!h->cand_classes) return 0;
  uint64_t d = tie_mix64(((uint64_t)h->cand_classes << 1) | (h->shard_cand ? 1u : 0u));
  d = tie_mix64(d ^ ((uint64_t)h->h_cls.size() + 0x9E3779B97F4A7C15ull));
  return tie_mix64(d ^ h->cls_hash) | 1ull;
}

// draw: an evaluation step (yoda_comm_run*): it may end in the draw and may run with candidate
// classes on; the greedy's steps never do either
static void agreement_words(const yoda_t* h, int mode, uint64_t* w, bool draw = false) {
  w[4] = draw ? draw_digest(h) : 0;
  w[5] = ~w[4];
  w[6] = draw ? cand_digest(h) : 0;
  w[7] = ~w[6];
  w[0] = h->generic && mode == YODA_MODE_SCV ? 64u : bit_length(h->score_bound);
  w[1] = bit_length((uint64_t)h->node_offset + h->n_nodes + 1);
  const bool f32q = mode == YODA_MODE_SCV && h->path == Path::N32 && h->q32;
  w[2] = mode == YODA_MODE_SCV ? h->small_max : 0;
  w[3] = f32q ? 1 : 0;
}

static const char* quotient_disagreement(uint64_t global_small_max, uint64_t any_f32) {
  if (any_f32 && global_small_max > kF32SmallMax)
    return "shards disagree on the quotient type: a shard computes f32 small-field quotients "
           "but another shard holds a small card field beyond 55738, so the reduced maxima "
           "break the f32 lemma; upload every shard with YODA_UPLOAD_F64_QUOTIENTS (see "
           "yoda_small_field_max)";
  return nullptr;
}

static int comm_step(yoda_t* const* hs, int n, int world, int mode, bool local, bool draw) {
  yoda_t* h0 = hs[0];
  const uint32_t P = h0->n_pods;
  const size_t n1 = 6 * (size_t)P + kAgreeWords;  // maxima | agreement words
  for (int i = 0; i < n; ++i) {  // (before any shard's run is prepared)
    // candidates on: only the evaluation step, with yoda_shard_candidates on, in Mode A and with
    // a class array that fits the batch; checked on every shard before any of them launches
    if (hs[i]->samp_m)
      return fail(h0, samp_refuse(hs[i], "yoda_comm_run"), hs[i]->last_error);
    if (hs[i]->cand_classes) {
      int rc = cand_refuse(hs[i], "yoda_comm_run", draw);
      if (!rc && mode == YODA_MODE_DISKIO) rc = mode_b_absent(hs[i], mode);
      if (!rc && hs[i]->has_pods) rc = cand_ready(hs[i]);
      if (rc) return fail(h0, rc, hs[i]->last_error);
    }
    if (hs[i]->n_absent && mode == YODA_MODE_DISKIO)
      return fail(h0, mode_b_absent(hs[i], mode), hs[i]->last_error);
  }
  for (int i = 0; i < n; ++i) {
    yoda_t* h = hs[i];
    if (h->n_pods != P) return fail(h0, YODA_ERR_INVALID_ARG, "shards hold different batches");
    // the fast record paths exchange in the caller's pod order, so each shard runs its private
    // order (padded counting sort, block-grouped nodes: xfer); the U64 path, whose exact-
    // normalize records go per sorted position, keeps the radix order all shards share
    h->xo = !h->generic;
    int rc = prepare_run(h, mode, h->xo);
    if (rc) return rc;
    if ((rc = order_pods(h, mode))) return rc;
    HIP_TRY(h, h->ex1.ensure(n1 * 8));
    HIP_TRY(h, h->rec.ensure((size_t)std::max<uint32_t>(P, 1) * sizeof(ShardRec)));
    HIP_TRY(h, h->rec_all.ensure((size_t)world * std::max<uint32_t>(P, 1) * sizeof(ShardRec)));
    if ((rc = xo_ensure(h))) return rc;
    if (P == 0) continue;
    uint64_t* ex = h->ex1.as<uint64_t>();
    if (h->xo) {
      if ((rc = phase1(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>()))) return rc;
      if ((rc = xfer(h, true, {{h->maxima.p, ex, 6, 8}, {h->counts.p, h->xcnt.p, 2, 4}})))
        return rc;
    } else if ((rc = phase1(h, mode, ex, h->counts.as<uint32_t>()))) {
      return rc;
    }
    // agreement words (pinned staging, one slot per shard; the previous step's copies
    // finished before its read-back below)
    uint64_t agree[kAgreeWords];
    agreement_words(h, mode, agree, draw);
    HIP_TRY(h0, h0->win_stage.ensure(kAgreeBytes * ((size_t)n + 1)));
    unsigned char* slot =
        static_cast<unsigned char*>(h0->win_stage.p) + kAgreeBytes * ((size_t)i + 1);
    std::memcpy(slot, agree, kAgreeBytes);
    HIP_TRY(h, hipMemcpyAsync(ex + 6 * (size_t)P, slot, kAgreeBytes, hipMemcpyHostToDevice,
                              h->stream));
  }
  if (P == 0) {
    for (int i = 0; i < n; ++i) hs[i]->ran = true, hs[i]->diag_done = false;
    return YODA_OK;
  }
  // the caller-order views of the exchanged buffers (the handle's own ones on the U64 path)
  auto cnt_x = [](yoda_t* h) { return h->xo ? h->xcnt.as<uint32_t>() : h->counts.as<uint32_t>(); };
  auto best_x = [](yoda_t* h) { return h->xo ? h->xbest.as<int64_t>() : h->best.as<int64_t>(); };
  auto idx_x = [](yoda_t* h) { return h->xo ? h->xidx.as<uint32_t>() : h->idx.as<uint32_t>(); };
  auto ties_x = [](yoda_t* h) { return h->xo ? h->xties.as<uint32_t>() : h->ties.as<uint32_t>(); };
  auto low_x = [](yoda_t* h) { return h->xo ? h->xlow.as<int64_t>() : h->lowest.as<int64_t>(); };
  if (local) {  // exchange 1: elementwise MAX / SUM over the shards, back to each
    PtrList l{}, c{};
    for (int i = 0; i < n; ++i) {
      l.p[i] = hs[i]->ex1.p;
      c.p[i] = cnt_x(hs[i]);
    }
    HIP_TRY(h0, h0->rec.ensure(std::max<size_t>(2 * (size_t)P * 4, (size_t)P * sizeof(ShardRec))));
    HIP_TRY(h0, launch_max_multi(l, (uint32_t)n, n1, h0->ex1.as<uint64_t>(), h0->stream));
    HIP_TRY(h0, launch_sum_multi_u32(c, (uint32_t)n, 2 * (uint64_t)P, h0->rec.as<uint32_t>(),
                                     h0->stream));
    for (int i = 0; i < n; ++i) {
      if (i > 0)
        HIP_TRY(h0, hipMemcpyAsync(hs[i]->ex1.p, h0->ex1.p, n1 * 8, hipMemcpyDeviceToDevice,
                                   h0->stream));
      HIP_TRY(h0, hipMemcpyAsync(cnt_x(hs[i]), h0->rec.p, 2 * (size_t)P * 4,
                                 hipMemcpyDeviceToDevice, h0->stream));
    }
  } else {
    rccl().group_start();
    ncclResult_t r = rccl().all_reduce(h0->ex1.p, h0->ex1.p, n1, ncclUint64, ncclMax, h0->comm,
                                       h0->stream);
    const ncclResult_t r2 = rccl().all_reduce(cnt_x(h0), cnt_x(h0), 2 * (size_t)P,
                                              ncclUint32, ncclSum, h0->comm, h0->stream);
    const ncclResult_t r3 = rccl().group_end();
    if (r == ncclSuccess) r = r2;
    if (r == ncclSuccess) r = r3;
    if (r != ncclSuccess)
      return fail(h0, YODA_ERR_HIP, std::string("ncclAllReduce: ") + rccl().error_string(r));
  }
  // the agreed phase-2 form (every shard reads the same reduced words; one host wait per step)
  uint64_t agreed[kAgreeWords] = {64, 64, 0, 0, 0, ~0ull};
  HIP_TRY(h0, hipMemcpyAsync(h0->win_stage.p, h0->ex1.as<uint64_t>() + 6 * (size_t)P,
                             kAgreeBytes, hipMemcpyDeviceToHost, h0->stream));
  HIP_TRY(h0, hipStreamSynchronize(h0->stream));
  std::memcpy(agreed, h0->win_stage.p, kAgreeBytes);
  // every rank reads the same reduced words, so every rank fails here together
  if (const char* why = quotient_disagreement(agreed[2], agreed[3]))
    return fail(h0, YODA_ERR_STATE, why);
  if (agreed[4] != ~agreed[5]) {
    for (int i = 0; i < n; ++i)
      fail(hs[i], YODA_ERR_STATE,
           "shards disagree on the draw settings: yoda_set_tie_draw (enable, seed, pod_base) and "
           "yoda_shard_tie_draw must be the same on every shard of a batch");
    return YODA_ERR_STATE;
  }
  if (agreed[6] != ~agreed[7]) {
    for (int i = 0; i < n; ++i)
      fail(hs[i], YODA_ERR_STATE,
           "shards disagree on the candidate state: yoda_shard_candidates, n_classes "
           "(yoda_set_candidates) and the class array (yoda_set_pod_classes) must be the same on "
           "every shard of a batch");
    return YODA_ERR_STATE;
  }
  const bool drawing = agreed[4] != 0;  // (so every shard of the batch has it enabled)
  const uint32_t ib = (uint32_t)std::max<uint64_t>(1, agreed[1]);
  const bool packed = agreed[0] + ib <= 63 && ib <= 40;
  for (int i = 0; i < n; ++i) {
    yoda_t* h = hs[i];
    uint64_t* ex = h->ex1.as<uint64_t>();
    int rc;
    if (h->xo) {
      if ((rc = xfer(h, false, {{h->maxima.p, ex, 6, 8}, {h->counts.p, h->xcnt.p, 2, 4}})))
        return rc;
    } else {
      HIP_TRY(h, hipMemcpyAsync(h->maxima.p, ex, 6 * (size_t)P * 8, hipMemcpyDeviceToDevice,
                                h->stream));
    }
    rc = phase2(h, mode, h->maxima.as<uint64_t>(), h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>());
    if (rc) return rc;
    if (h->xo && (rc = xfer(h, true, {{h->best.p, h->xbest.p, 1, 8}, {h->idx.p, h->xidx.p, 1, 4},
                                      {h->ties.p, h->xties.p, 1, 4},
                                      {h->lowest.p, h->xlow.p, 1, 8}})))
      return rc;
    if (packed)
      HIP_TRY(h, launch_pack_key(best_x(h), idx_x(h), P, ib, h->rec.as<uint64_t>(), h->stream));
    else
      HIP_TRY(h, launch_pack_rec(best_x(h), idx_x(h), ties_x(h), low_x(h), P,
                                 h->rec.as<ShardRec>(), h->stream));
  }
  if (packed) {  // exchange 2: MAX of the keys, then SUM of the winners' ties
    if (local) {
      PtrList l{};
      for (int i = 0; i < n; ++i) l.p[i] = hs[i]->rec.p;
      HIP_TRY(h0, launch_max_multi(l, (uint32_t)n, P, h0->rec_all.as<uint64_t>(), h0->stream));
      for (int i = 0; i < n; ++i)
        HIP_TRY(h0, hipMemcpyAsync(hs[i]->rec.p, h0->rec_all.p, (size_t)P * 8,
                                   hipMemcpyDeviceToDevice, h0->stream));
    } else {
      const ncclResult_t r = rccl().all_reduce(h0->rec.p, h0->rec.p, P, ncclUint64, ncclMax,
                                               h0->comm, h0->stream);
      if (r != ncclSuccess)
        return fail(h0, YODA_ERR_HIP, std::string("ncclAllReduce: ") + rccl().error_string(r));
    }
    for (int i = 0; i < n; ++i) {
      yoda_t* h = hs[i];
      HIP_TRY(h, launch_unpack_key(h->rec.as<uint64_t>(), P, ib, best_x(h), idx_x(h), ties_x(h),
                                   low_x(h), h->stream));
    }
    if (local) {
      PtrList t{};
      for (int i = 0; i < n; ++i) t.p[i] = ties_x(hs[i]);
      HIP_TRY(h0, launch_sum_multi_u32(t, (uint32_t)n, P, h0->rec_all.as<uint32_t>(), h0->stream));
      for (int i = 0; i < n; ++i)
        HIP_TRY(h0, hipMemcpyAsync(ties_x(hs[i]), h0->rec_all.p, (size_t)P * 4,
                                   hipMemcpyDeviceToDevice, h0->stream));
    } else {
      const ncclResult_t r = rccl().all_reduce(ties_x(h0), ties_x(h0), P, ncclUint32, ncclSum,
                                               h0->comm, h0->stream);
      if (r != ncclSuccess)
        return fail(h0, YODA_ERR_HIP, std::string("ncclAllReduce: ") + rccl().error_string(r));
    }
  } else {
    const size_t rb = (size_t)P * sizeof(ShardRec);
    if (local) {  // exchange 2: every shard's records to every shard
      for (int r = 0; r < n; ++r)
        for (int i = 0; i < n; ++i)
          HIP_TRY(h0, hipMemcpyAsync(hs[i]->rec_all.as<unsigned char>() + r * rb, hs[r]->rec.p,
                                     rb, hipMemcpyDeviceToDevice, h0->stream));
    } else {
      const ncclResult_t r = rccl().all_gather(h0->rec.p, h0->rec_all.p, rb / 8, ncclUint64,
                                               h0->comm, h0->stream);
      if (r != ncclSuccess)
        return fail(h0, YODA_ERR_HIP, std::string("ncclAllGather: ") + rccl().error_string(r));
    }
    for (int i = 0; i < n; ++i) {
      yoda_t* h = hs[i];
      HIP_TRY(h, launch_merge_rec(h->rec_all.as<ShardRec>(), P, (uint32_t)world, best_x(h),
                                  idx_x(h), ties_x(h), low_x(h), h->stream));
    }
  }
  for (int i = 0; i < n; ++i) {
    yoda_t* h = hs[i];
    int rc;
    if (h->xo && (rc = xfer(h, false, {{h->best.p, h->xbest.p, 1, 8}, {h->idx.p, h->xidx.p, 1, 4},
                                       {h->ties.p, h->xties.p, 1, 4},
                                       {h->lowest.p, h->xlow.p, 1, 8}})))
      return rc;
    rc = finalize(h, mode, h->counts.as<uint32_t>(), h->best.as<int64_t>(),
                  h->idx.as<uint32_t>(), h->ties.as<uint32_t>(), h->lowest.as<int64_t>(), true);
    if (rc) return rc;
    h->ran = true;
    h->diag_done = false;
    h->ran_bitmask = false;
    h->last_mode = mode;
    h->draw_stage = 1;
  }
  // exchange 3 (rare: U64 pods whose NormalizeScore can overflow int64, scheduler.go:176-179):
  // every shard's exact-normalize records to every shard, then the merge (all shards flag the
  // same pods, so all of them take this branch)
  if (h0->k3_pending) {
    const size_t rb = (size_t)h0->n_work * sizeof(ShardRec);
    for (int i = 0; i < n; ++i) HIP_TRY(hs[i], hs[i]->k3all.ensure(rb * (size_t)world));
    if (local) {
      for (int r = 0; r < n; ++r)
        for (int i = 0; i < n; ++i)
          HIP_TRY(h0, hipMemcpyAsync(hs[i]->k3all.as<unsigned char>() + r * rb, hs[r]->k3rec.p,
                                     rb, hipMemcpyDeviceToDevice, h0->stream));
    } else {
      const ncclResult_t r = rccl().all_gather(h0->k3rec.p, h0->k3all.p, rb / 8, ncclUint64,
                                               h0->comm, h0->stream);
      if (r != ncclSuccess)
        return fail(h0, YODA_ERR_HIP, std::string("ncclAllGather: ") + rccl().error_string(r));
    }
    for (int i = 0; i < n; ++i) {
      int rc = yoda_shard_exact_merge(hs[i], hs[i]->k3all.p, world);
      if (rc) return rc;
    }
  }
  // exchange 4 (only with the shard draw on): every shard's MIN draw key per tied pod over its
  // own top-scored nodes, all-reduce(MIN) [P] u64, then every shard takes the winner's node
  if (drawing) {
    for (int i = 0; i < n; ++i) {
      yoda_t* h = hs[i];
      HIP_TRY(h, h->xkeys.ensure((size_t)P * 8));
      int rc = yoda_shard_draw_keys(h, mode, h->xkeys.as<uint64_t>());
      if (rc) return rc;
    }
    if (local) {
      PtrList l{};
      for (int i = 0; i < n; ++i) l.p[i] = hs[i]->xkeys.p;
      HIP_TRY(h0, launch_min_multi(l, (uint32_t)n, P, h0->rec_all.as<uint64_t>(), h0->stream));
      for (int i = 0; i < n; ++i)
        HIP_TRY(h0, hipMemcpyAsync(hs[i]->xkeys.p, h0->rec_all.p, (size_t)P * 8,
                                   hipMemcpyDeviceToDevice, h0->stream));
    } else {
      const ncclResult_t r = rccl().all_reduce(h0->xkeys.p, h0->xkeys.p, P, ncclUint64, ncclMin,
                                               h0->comm, h0->stream);
      if (r != ncclSuccess)
        return fail(h0, YODA_ERR_HIP, std::string("ncclAllReduce: ") + rccl().error_string(r));
    }
    for (int i = 0; i < n; ++i) {
      int rc = yoda_shard_draw_apply(hs[i], hs[i]->xkeys.as<uint64_t>());
      if (rc) return rc;
    }
  }
  return YODA_OK;
}

// Collectives of the libyoda-driven multi-GPU paths: over RCCL (one handle per process, the
// handle's communicator) or, for tests on one device, over the `n` handles of this process
// (host-staged: every handle's buffer read back, reduced or concatenated, written back).
struct Coll {
  yoda_t* const* hs;
  int n, world;
  bool local;
  uint32_t* calls = nullptr;  // collective launches made (yoda_comm_greedy_stats): a group of
                              // collectives (begin() .. end()) counts once
  bool in_group = false;
  int nccl(ncclResult_t r, const char* what) const {
    if (r == ncclSuccess) return YODA_OK;
    return fail(hs[0], YODA_ERR_HIP, std::string(what) + ": " + rccl().error_string(r));
  }
  void count() const {
    if (calls && !in_group) ++*calls;
  }
  // ncclGroupStart / End: the collectives issued in between run as ONE launch (RCCL fuses
  // them); the local transport runs each at once
  void begin() {
    if (!local) rccl().group_start();
    in_group = true;
  }
  int end() {
    in_group = false;
    count();
    return local ? YODA_OK : nccl(rccl().group_end(), "ncclGroupEnd");
  }
  // in-place elementwise all-reduce of `count` u64 or u32 device words (MAX / SUM / MIN)
  int allreduce(const std::vector<void*>& bufs, size_t count, bool u64, ncclRedOp_t op) const {
    if (count == 0) return YODA_OK;
    this->count();
    if (!local)
      return nccl(rccl().all_reduce(bufs[0], bufs[0], count, u64 ? ncclUint64 : ncclUint32, op,
                                    hs[0]->comm, hs[0]->stream),
                  "ncclAllReduce");
    const size_t w = u64 ? 8 : 4;
    std::vector<unsigned char> acc(count * w), one(count * w);
    for (int i = 0; i < n; ++i) {
      HIP_TRY(hs[i], hipMemcpyAsync(i ? one.data() : acc.data(), bufs[i], count * w,
                                    hipMemcpyDeviceToHost, hs[i]->stream));
      HIP_TRY(hs[i], hipStreamSynchronize(hs[i]->stream));
      if (i == 0) continue;
      for (size_t e = 0; e < count; ++e) {
        if (u64) {
          uint64_t& a = reinterpret_cast<uint64_t*>(acc.data())[e];
          const uint64_t b = reinterpret_cast<const uint64_t*>(one.data())[e];
          a = op == ncclMax ? std::max(a, b) : op == ncclMin ? std::min(a, b) : a + b;
        } else {
          uint32_t& a = reinterpret_cast<uint32_t*>(acc.data())[e];
          const uint32_t b = reinterpret_cast<const uint32_t*>(one.data())[e];
          a = op == ncclMax ? std::max(a, b) : op == ncclMin ? std::min(a, b) : a + b;
        }
      }
    }
    for (int i = 0; i < n; ++i) {
      HIP_TRY(hs[i], hipMemcpyAsync(bufs[i], acc.data(), count * w, hipMemcpyHostToDevice,
                                    hs[i]->stream));
      HIP_TRY(hs[i], hipStreamSynchronize(hs[i]->stream));
    }
    return YODA_OK;
  }
  // all-gather of host blocks: out = the world's `bytes`-byte blocks in rank order (RCCL:
  // staged through the first handle's device scratch).  In a group: allgather_issue before
  // end(), allgather_finish after it (the copies back must follow the collective's launch).
  int allgather(const std::vector<const void*>& in, size_t bytes,
                std::vector<unsigned char>& out) const {
    int rc = allgather_issue(in, bytes, out);
    return rc ? rc : allgather_finish(bytes, out);
  }
  int allgather_issue(const std::vector<const void*>& in, size_t bytes,
                      std::vector<unsigned char>& out) const {
    out.resize((size_t)world * bytes);
    count();
    if (local) {
      for (int i = 0; i < n; ++i) std::memcpy(out.data() + (size_t)i * bytes, in[i], bytes);
      return YODA_OK;
    }
    yoda_t* h = hs[0];
    const size_t b8 = (bytes + 7) / 8 * 8;
    HIP_TRY(h, h->cg_gather.ensure(b8 * ((size_t)world + 1)));
    unsigned char* d = h->cg_gather.as<unsigned char>();
    HIP_TRY(h, hipMemcpyAsync(d, in[0], bytes, hipMemcpyHostToDevice, h->stream));
    return nccl(rccl().all_gather(d, d + b8, b8 / 8, ncclUint64, h->comm, h->stream),
                "ncclAllGather");
  }
  int allgather_finish(size_t bytes, std::vector<unsigned char>& out) const {
    if (local) return YODA_OK;
    yoda_t* h = hs[0];
    const size_t b8 = (bytes + 7) / 8 * 8;
    unsigned char* d = h->cg_gather.as<unsigned char>();
    for (int r = 0; r < world; ++r)
      HIP_TRY(h, hipMemcpyAsync(out.data() + (size_t)r * bytes, d + b8 * ((size_t)r + 1), bytes,
                                hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return YODA_OK;
  }
};

static int comm_step(yoda_t* const* hs, int n, int world, int mode, bool local,
                     bool draw = false);

// the capacity windows' list depth across shards (YODA_GREEDY_CAP_DEPTH, as yoda_greedy's)
static uint32_t greedy_cap_depth() {
  static const uint32_t d = YODA_KNOB("YODA_GREEDY_CAP_DEPTH", 64);
  return std::max<uint32_t>(d, (uint32_t)topk_k_capacity());
}

// Greedy batch over node shards, inside libyoda ("Across GPUs"): the protocol of
// dist.sharded_greedy with RCCL (or the in-process transport): per window, K1 on every shard,
// maxima MAX / counts SUM (capacity mode: + the witnesses), the shards' candidate lists
// all-gathered and merged, the host session (identical on every rank, over `all`, the FULL
// snapshot) resolves the window; an uncertified pod is scored exactly on every shard and the
// (score, node) candidates all-gathered (capacity mode: it opens the next window).  The U64
// record path has no candidate lists: every pod is a sharded exact step (comm_step) against
// the current state.  The shards' node state is restored at the end.
static int comm_greedy(yoda_t* const* hs, int n, int world, bool local, const yoda_node_soa* all,
                       const yoda_pod_soa* pods, int mode, uint32_t flags, int32_t* pick) {
  yoda_t* h0 = hs[0];
  Coll co{hs, n, world, local};
  uint32_t* st = h0->comm_greedy_stats;  // windows, exact pods, restarts, refreshes, collectives
  std::fill(st, st + 5, 0u);
  co.calls = st + 4;
  const uint32_t P = pods->n_pods;
  for (int i = 0; i < n; ++i)
    if (!hs[i]->has_nodes) return fail(h0, YODA_ERR_NO_NODES, "no node snapshot uploaded");
  for (int i = 0; i < n; ++i) {
    if (hs[i]->cand_classes || hs[i]->samp_m)
      return fail(h0, cand_refuse(hs[i], "yoda_comm_greedy"), hs[i]->last_error);
    if (hs[i]->n_absent && mode == YODA_MODE_DISKIO)
      return fail(h0, mode_b_absent(hs[i], mode), hs[i]->last_error);
  }
  if (P == 0) return YODA_OK;
  int rc;
  PodGather win;
  if (mode == YODA_MODE_DISKIO) {  // Mode B reads no assumed-pod state: independent cycles
    std::vector<uint32_t> idx(P);
    for (uint32_t i = 0; i < P; ++i) idx[i] = i;
    win.build(pods, idx.data(), P);
    for (int i = 0; i < n; ++i)
      if ((rc = yoda_upload_pods(hs[i], &win.soa))) return rc;
    if ((rc = comm_step(hs, n, world, mode, local))) return rc;
    HIP_TRY(h0, hipMemcpyAsync(pick, h0->pick.p, (size_t)P * 4, hipMemcpyDeviceToHost,
                               h0->stream));
    HIP_TRY(h0, hipStreamSynchronize(h0->stream));
    return YODA_OK;
  }
  yoda_gs_t* g = nullptr;
  if ((rc = yoda_gs_create(all, pods, flags, &g))) return fail(h0, rc, "greedy: session setup");
  struct Guard {
    yoda_gs_t* g;
    ~Guard() { yoda_gs_destroy(g); }
  } guard{g};
  const bool capacity = (flags & YODA_GREEDY_CARD_CAPACITY) != 0;
  const bool generic = h0->generic;
  for (int i = 0; i < n; ++i)
    if (hs[i]->generic != generic)
      return fail(h0, YODA_ERR_STATE, "shards on different record paths");
  if (!generic) {  // the quotient type too (comm_step's agreement words [2], [3]), once per batch
    std::vector<void*> bq;
    std::vector<uint64_t> w((size_t)kAgreeWords * n);  // alive until the stream syncs below
    for (int i = 0; i < n; ++i) {
      uint64_t* wi = w.data() + (size_t)kAgreeWords * i;
      agreement_words(hs[i], YODA_MODE_SCV, wi);
      HIP_TRY(hs[i], hs[i]->cg_max.ensure(2 * 8));
      HIP_TRY(hs[i], hipMemcpyAsync(hs[i]->cg_max.p, wi + 2, 16, hipMemcpyHostToDevice,
                                    hs[i]->stream));
      bq.push_back(hs[i]->cg_max.p);
    }
    if ((rc = co.allreduce(bq, 2, true, ncclMax))) return rc;
    uint64_t q[2] = {0, 0};
    HIP_TRY(h0, hipMemcpyAsync(q, h0->cg_max.p, 16, hipMemcpyDeviceToHost, h0->stream));
    HIP_TRY(h0, hipStreamSynchronize(h0->stream));
    if (const char* why = quotient_disagreement(q[0], q[1])) return fail(h0, YODA_ERR_STATE, why);
  }
  std::vector<uint32_t> ids;
  std::vector<uint64_t> al, cn;
  auto push = [&](bool original) -> int {  // the session's node changes -> every shard
    const uint32_t cap = std::max<uint32_t>(g->N, 1);
    ids.resize(cap), al.resize(cap), cn.resize(cap);
    uint32_t got = 0;
    int r = original ? yoda_gs_touched_original(g, cap, ids.data(), al.data(), cn.data(), &got)
                     : yoda_gs_take_dirty(g, cap, ids.data(), al.data(), cn.data(), &got);
    if (r) return fail(h0, r, "greedy: node state");
    if (got == 0) return YODA_OK;
    for (int i = 0; i < n; ++i)
      if ((r = yoda_set_node_state(hs[i], got, ids.data(), al.data(), cn.data()))) return r;
    return YODA_OK;
  };
  auto run = [&]() -> int {
    if (generic) {  // every pod exactly, in queue order, against the current state
      for (uint32_t q = 0; q < P; ++q) {
        if ((rc = push(false))) return rc;
        win.build(pods, g->order.data() + q, 1);
        for (int i = 0; i < n; ++i)
          if ((rc = yoda_upload_pods(hs[i], &win.soa))) return rc;
        if ((rc = comm_step(hs, n, world, YODA_MODE_SCV, local))) return rc;
        int32_t pk = 0;
        HIP_TRY(h0, hipMemcpyAsync(&pk, h0->pick.p, 4, hipMemcpyDeviceToHost, h0->stream));
        HIP_TRY(h0, hipStreamSynchronize(h0->stream));
        if ((rc = yoda_gs_assign(g, q, pk))) return fail(h0, rc, "greedy: assign");
        ++h0->greedy_fallbacks;
        ++st[1];
      }
      return push(false);
    }
    const uint32_t K = (uint32_t)(capacity ? topk_k_capacity() : topk_k()),
                   W0 = std::min<uint32_t>(P, greedy_window());
    // capacity windows: each shard's lists merged deeper (shard_topk_impl, exact down to their
    // last entry), the union cut where a shard's unlisted nodes could enter (merge_shard_lists);
    // the same depth on every rank
    const uint32_t KL = capacity ? greedy_cap_depth() : K;
    std::vector<uint32_t> counts, ti, wit_h;
    std::vector<double> ts;
    std::vector<uint64_t> mx_h;
    std::vector<unsigned char> gathered, mine, one;
    uint32_t ws = 0, W = W0;
    while (ws < P) {
      const uint32_t wn = std::min(W, P - ws);
      if ((rc = push(false))) return rc;
      win.build(pods, g->order.data() + ws, wn);
      std::vector<void*> bmax, bcnt, bwc, bwn;
      for (int i = 0; i < n; ++i) {
        yoda_t* h = hs[i];
        if ((rc = yoda_upload_pods(h, &win.soa))) return rc;
        HIP_TRY(h, h->cg_max.ensure(12ull * wn * 8));  // the maxima, and a local copy
        HIP_TRY(h, h->cg_cnt.ensure(2ull * wn * 4));
        HIP_TRY(h, h->cg_wit.ensure(12ull * wn * 4));
        uint64_t* dmax = h->cg_max.as<uint64_t>();
        if (capacity) {
          if ((rc = yoda_shard_phase1_witness(h, dmax, h->cg_cnt.as<uint32_t>(),
                                              h->cg_wit.as<uint32_t>())))
            return rc;
          HIP_TRY(h, hipMemcpyAsync(dmax + 6ull * wn, dmax, 6ull * wn * 8,
                                    hipMemcpyDeviceToDevice, h->stream));
        } else if ((rc = yoda_shard_phase1(h, YODA_MODE_SCV, dmax, h->cg_cnt.as<uint32_t>()))) {
          return rc;
        }
        bmax.push_back(dmax);
        bcnt.push_back(h->cg_cnt.p);
        bwc.push_back(h->cg_wit.p);
        bwn.push_back(h->cg_wit.as<uint32_t>() + 6ull * wn);
      }
      // window exchange 1 (one group): maxima MAX, counts SUM
      co.begin();
      rc = co.allreduce(bmax, 6ull * wn, true, ncclMax);
      const int rc2 = co.allreduce(bcnt, 2ull * wn, false, ncclSum);
      const int rc3 = co.end();
      if (rc || (rc = rc2) || (rc = rc3)) return rc;
      if (capacity) {
        for (int i = 0; i < n; ++i) {
          uint64_t* dmax = hs[i]->cg_max.as<uint64_t>();
          if ((rc = yoda_shard_witness_prepare(hs[i], dmax, dmax + 6ull * wn,
                                               hs[i]->cg_wit.as<uint32_t>())))
            return rc;
        }
      }
      // the shards' candidate lists, all-gathered and merged: the first K of the union in
      // (score desc, node asc) order contain the global top K (window pods [from, wn) only).
      // Window exchange 2 (one group): the lists' all-gather and, in capacity mode, the
      // witness counts SUM and lowest witnesses MIN (they need only exchange 1's maxima)
      counts.resize(2ull * wn);
      auto merged_lists = [&](uint32_t from, bool with_witness) -> int {
        const size_t lb = (size_t)KL * wn * 12;  // per shard: KL x wn scores (f64) + nodes (u32)
        mine.resize((size_t)n * lb);
        for (int i = 0; i < n; ++i) {
          unsigned char* m = mine.data() + (size_t)i * lb;
          int r = shard_topk_impl(hs[i], hs[i]->cg_max.as<uint64_t>(),
                                  hs[i]->cg_cnt.as<uint32_t>(), K, KL > K ? KL : 0u,
                                  counts.data(), reinterpret_cast<double*>(m),
                                  reinterpret_cast<uint32_t*>(m + (size_t)KL * wn * 8));
          if (r) return r;
        }
        std::vector<const void*> ins;
        for (int i = 0; i < n; ++i) ins.push_back(mine.data() + (size_t)i * lb);
        co.begin();
        int r = with_witness ? co.allreduce(bwc, 6ull * wn, false, ncclSum) : YODA_OK;
        if (!r && with_witness) r = co.allreduce(bwn, 6ull * wn, false, ncclMin);
        if (!r) r = co.allgather_issue(ins, lb, gathered);
        const int re = co.end();
        if (r || (r = re) || (r = co.allgather_finish(lb, gathered))) return r;
        ts.assign((size_t)KL * wn, -1.0);
        ti.assign((size_t)KL * wn, 0xffffffffu);
        std::vector<const double*> sc(world);
        std::vector<const uint32_t*> nd(world);
        for (int rk = 0; rk < world; ++rk) {
          const unsigned char* b = gathered.data() + (size_t)rk * lb;
          sc[rk] = reinterpret_cast<const double*>(b);
          nd[rk] = reinterpret_cast<const uint32_t*>(b + (size_t)KL * wn * 8);
        }
        merge_shard_lists(world, wn, KL, KL > K, from, sc.data(), nd.data(), ts.data(),
                          ti.data());
        return YODA_OK;
      };
      if ((rc = merged_lists(0, capacity))) return rc;
      if ((rc = yoda_gs_begin_window(g, ws, wn, KL, counts.data(), ts.data(), ti.data())))
        return fail(h0, rc, "greedy: begin window");
      ++h0->greedy_windows;
      ++st[0];
      if (capacity) {
        mx_h.resize(6ull * wn);
        wit_h.resize(12ull * wn);
        if ((rc = yoda_shard_witness_download(h0, h0->cg_max.as<uint64_t>(),
                                              h0->cg_wit.as<uint32_t>(), mx_h.data(),
                                              wit_h.data())))
          return rc;
        if ((rc = yoda_gs_set_witness(g, mx_h.data(), wit_h.data(), wit_h.data() + 6ull * wn)))
          return fail(h0, rc, "greedy: witnesses");
        uint32_t nxt = 0;
        if ((rc = yoda_gs_resolve(g, &nxt))) return fail(h0, rc, "greedy: resolve");
        if (nxt < wn) {  // the uncertified pod opens the next window (yoda_greedy's rule)
          ++h0->greedy_restarts;
          ++st[2];
          ws += nxt;
          W = yoda_greedy_next_window(nxt, W0);
        } else {
          ws += wn;
          W = std::min<uint32_t>(W0, 2 * W);
        }
        continue;
      }
      // mid-window list refresh (yoda_greedy's, greedy_refresh()): every shard's top-k runs
      // again against the current state and the merged lists replace the old ones
      const uint32_t kFbCheck = greedy_refresh().every, kScan = greedy_refresh().scan,
                     kScanMin = greedy_refresh().min;
      uint32_t fb_since = 0;
      for (;;) {
        uint32_t nxt = 0;
        if ((rc = yoda_gs_resolve(g, &nxt))) return fail(h0, rc, "greedy: resolve");
        if (nxt >= wn) break;
        if (++fb_since >= kFbCheck && wn - nxt >= 2 * kScan && !g->wrapped) {
          fb_since = 0;
          uint32_t unc = 0;
          if ((rc = yoda_gs_uncertified(g, nxt + 1, kScan, &unc))) return fail(h0, rc, "greedy");
          if (unc >= kScanMin) {
            if ((rc = push(false))) return rc;
            if ((rc = merged_lists(nxt, false))) return rc;
            if ((rc = yoda_gs_refresh(g, nxt, ts.data(), ti.data())))
              return fail(h0, rc, "greedy: refresh");
            ++h0->greedy_refreshes;
            ++st[3];
            uint32_t again = 0;
            if ((rc = yoda_gs_resolve(g, &again))) return fail(h0, rc, "greedy: resolve");
            if (again >= wn) break;
            nxt = again;
          }
        }
        if ((rc = push(false))) return rc;
        one.resize((size_t)n * 16);
        for (int i = 0; i < n; ++i) {
          double sc = -1.0;
          int32_t nd = -1;
          if ((rc = yoda_shard_best_one(hs[i], nxt, &sc, &nd))) return rc;
          const int64_t nd64 = nd;
          std::memcpy(one.data() + 16 * (size_t)i, &sc, 8);
          std::memcpy(one.data() + 16 * (size_t)i + 8, &nd64, 8);
        }
        std::vector<const void*> in1;
        for (int i = 0; i < n; ++i) in1.push_back(one.data() + 16 * (size_t)i);
        if ((rc = co.allgather(in1, 16, gathered))) return rc;
        double bs = -1.0;
        int64_t bn = -1;
        for (int r = 0; r < world; ++r) {
          double sc;
          int64_t nd;
          std::memcpy(&sc, gathered.data() + 16 * (size_t)r, 8);
          std::memcpy(&nd, gathered.data() + 16 * (size_t)r + 8, 8);
          if (nd >= 0 && (sc > bs || (sc == bs && nd < bn))) {
            bs = sc;
            bn = nd;
          }
        }
        if (bn < 0) return fail(h0, YODA_ERR_STATE, "greedy: no feasible node for a window pod");
        if ((rc = yoda_gs_assign(g, ws + nxt, (int32_t)bn))) return fail(h0, rc, "greedy: assign");
        ++h0->greedy_fallbacks;
        ++st[1];
      }
      ws += wn;
    }
    return push(false);
  };
  h0->greedy_windows = h0->greedy_fallbacks = h0->greedy_restarts = h0->greedy_refreshes = 0;
  {  // a greedy batch on every shard: its pushes keep the block bounds valid (no rebuilds)
    std::vector<std::unique_ptr<GreedyScope>> scopes;
    for (int i = 0; i < n; ++i) scopes.emplace_back(new GreedyScope(hs[i]));
    rc = run();
  }
  const int rr = push(true);  // restore the shards' original node state
  if (rc) return rc;
  if (rr) return rr;
  uint32_t resolved = 0, assigned = 0;
  return yoda_gs_picks(g, pick, &resolved, &assigned);
}

extern "C" {
int yoda_greedy_cap_depth(void) { return (int)greedy_cap_depth(); }

int yoda_shard_topk_deep(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_counts,
                         uint32_t k, uint32_t deep, uint32_t* counts, double* top_score,
                         uint32_t* top_node) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (deep > 1024) return fail(h, YODA_ERR_INVALID_ARG, "yoda_shard_topk_deep: deep > 1024");
  return shard_topk_impl(h, d_maxima, d_counts, k, deep, counts, top_score, top_node);
}

int yoda_comm_greedy_stats(const yoda_t* h, uint32_t* out) {
  if (!h || !out) return YODA_ERR_INVALID_ARG;
  std::copy(h->comm_greedy_stats, h->comm_greedy_stats + 5, out);
  return YODA_OK;
}

int yoda_comm_unique_id(uint8_t* id) {
  if (!id) return YODA_ERR_INVALID_ARG;
  if (!rccl().load()) return YODA_ERR_HIP;
  ncclUniqueId u;
  if (rccl().get_unique_id(&u) != ncclSuccess) return YODA_ERR_HIP;
  std::memcpy(id, &u, sizeof(u));
  return YODA_OK;
}

int yoda_device_bus_id(const yoda_t* h, char* out, int len) {
  if (!h || !out || len < 2) return YODA_ERR_INVALID_ARG;
  std::memset(out, 0, (size_t)len);
  if (hipDeviceGetPCIBusId(out, len - 1, h->device) != hipSuccess) return YODA_ERR_HIP;
  return YODA_OK;
}

// The host's identity for the device check: FNV-1a 64 of the hostname and the kernel's boot id
// (what NCCL's hostHash takes), so identical servers -- equal PCI bus ids -- still differ.
static uint64_t host_hash() {
  uint64_t x = 1469598103934665603ull;
  const auto mix = [&](const char* s, size_t n) {
    for (size_t i = 0; i < n; ++i) x = (x ^ (unsigned char)s[i]) * 1099511628211ull;
  };
  char name[256] = {0};
  gethostname(name, sizeof(name) - 1);
  mix(name, strnlen(name, sizeof(name)));
  if (FILE* f = std::fopen("/proc/sys/kernel/random/boot_id", "r")) {
    char b[64] = {0};
    const size_t n = std::fread(b, 1, sizeof(b) - 1, f);
    std::fclose(f);
    mix(b, n);
  }
  return x;
}

int yoda_device_key(const yoda_t* h, char* out, int len) {
  if (!h || !out || len < 32) return YODA_ERR_INVALID_ARG;
  char bus[YODA_BUS_ID_BYTES];
  int rc = yoda_device_bus_id(h, bus, sizeof(bus));
  if (rc) return rc;
  const int n = std::snprintf(out, (size_t)len, "%016llx/%s", (unsigned long long)host_hash(), bus);
  return n > 0 && n < len ? YODA_OK : YODA_ERR_INVALID_ARG;
}

int yoda_comm_check_devices(const char* bus_ids, int world, int stride, int* rank_a,
                            int* rank_b) {
  if (!bus_ids || world < 1 || stride < 1) return YODA_ERR_INVALID_ARG;
  const auto id = [&](int r) {
    const char* p = bus_ids + (size_t)r * stride;
    return std::string(p, strnlen(p, (size_t)stride));
  };
  for (int a = 0; a < world; ++a) {
    const std::string ia = id(a);
    if (ia.empty()) return YODA_ERR_INVALID_ARG;
    for (int b = a + 1; b < world; ++b)
      if (ia == id(b)) {
        if (rank_a) *rank_a = a;
        if (rank_b) *rank_b = b;
        return YODA_ERR_SAME_DEVICE;
      }
  }
  return YODA_OK;
}

int yoda_comm_init(yoda_t* h, const uint8_t* id, int rank, int world) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!id || world < 1 || rank < 0 || rank >= world)
    return fail(h, YODA_ERR_INVALID_ARG, "bad communicator id / rank / world");
  if (!rccl().load()) return fail(h, YODA_ERR_HIP, rccl().err);
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->comm) {
    (void)rccl().comm_destroy(h->comm);
    h->comm = nullptr;
  }
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t r = rccl().comm_init_rank(&h->comm, world, u, rank);
  if (r != ncclSuccess) {
    h->comm = nullptr;
    std::string msg = std::string("ncclCommInitRank: ") + rccl().error_string(r);
    if (r == ncclInvalidUsage)  // the usual cause: two ranks on one GPU
      msg += " (RCCL refuses two ranks of one communicator on the same GPU: check the "
             "ranks' devices with yoda_device_bus_id / yoda_comm_check_devices)";
    return fail(h, YODA_ERR_HIP, msg);
  }
  h->comm_rank = rank;
  h->comm_world = world;
  return YODA_OK;
}

int yoda_comm_run(yoda_t* h, int mode) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!h->comm) return fail(h, YODA_ERR_STATE, "yoda_comm_run before yoda_comm_init");
  try {
    yoda_t* hs[1] = {h};
    return comm_step(hs, 1, h->comm_world, mode, false, true);
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_comm_greedy(yoda_t* h, const yoda_node_soa* all_nodes, const yoda_pod_soa* pods,
                     int mode, uint32_t flags, int32_t* pick) {
  if (!h) return YODA_ERR_INVALID_ARG;
  if (!all_nodes || !pods || !pick) return fail(h, YODA_ERR_INVALID_ARG, "NULL argument");
  if (!h->comm) return fail(h, YODA_ERR_STATE, "yoda_comm_greedy before yoda_comm_init");
  try {
    HIP_TRY(h, hipSetDevice(h->device));
    yoda_t* hs[1] = {h};
    return comm_greedy(hs, 1, h->comm_world, false, all_nodes, pods, mode, flags, pick);
  } catch (const std::bad_alloc&) {
    return fail(h, YODA_ERR_INVALID_ARG, "host allocation failed");
  } catch (...) {
    return fail(h, YODA_ERR_INVALID_ARG, "unexpected exception");
  }
}

int yoda_comm_greedy_local(yoda_t* const* hs, int world, const yoda_node_soa* all_nodes,
                           const yoda_pod_soa* pods, int mode, uint32_t flags, int32_t* pick) {
  if (!hs || world < 1 || world > kMaxLocalShards || !all_nodes || !pods || !pick)
    return YODA_ERR_INVALID_ARG;
  for (int i = 0; i < world; ++i)
    if (!hs[i]) return YODA_ERR_INVALID_ARG;
  for (int i = 1; i < world; ++i)
    if (hs[i]->device != hs[0]->device)
      return fail(hs[0], YODA_ERR_INVALID_ARG, "local exchange: shards on different devices");
  // one stream for every shard (the device copies order after the kernels); a shard's own
  // queued work is ordered before it (switch_stream), and the shared stream's after it on exit
  std::vector<hipStream_t> saved(world);
  for (int i = 0; i < world; ++i) {
    saved[i] = hs[i]->stream;
    if (switch_stream(hs[i], hs[0]->stream) != YODA_OK) {
      for (int j = 0; j < i; ++j) (void)switch_stream(hs[j], saved[j]);
      return YODA_ERR_HIP;
    }
  }
  int rc;
  try {
    rc = hipSetDevice(hs[0]->device) == hipSuccess
             ? comm_greedy(hs, world, world, true, all_nodes, pods, mode, flags, pick)
             : YODA_ERR_HIP;
  } catch (...) {
    rc = fail(hs[0], YODA_ERR_INVALID_ARG, "unexpected exception");
  }
  for (int i = 0; i < world; ++i)
    if (switch_stream(hs[i], saved[i]) != YODA_OK && rc == YODA_OK) rc = YODA_ERR_HIP;
  return rc;
}

int yoda_comm_run_local(yoda_t* const* hs, int world, int mode) {
  if (!hs || world < 1 || world > kMaxLocalShards) return YODA_ERR_INVALID_ARG;
  for (int i = 0; i < world; ++i)
    if (!hs[i]) return YODA_ERR_INVALID_ARG;
  for (int i = 1; i < world; ++i)
    if (hs[i]->device != hs[0]->device)
      return fail(hs[0], YODA_ERR_INVALID_ARG, "local exchange: shards on different devices");
  // one stream for every shard (the device copies order after the kernels); a shard's own
  // queued work is ordered before it (switch_stream), and the shared stream's after it on exit
  std::vector<hipStream_t> saved(world);
  for (int i = 0; i < world; ++i) {
    saved[i] = hs[i]->stream;
    if (switch_stream(hs[i], hs[0]->stream) != YODA_OK) {
      for (int j = 0; j < i; ++j) (void)switch_stream(hs[j], saved[j]);
      return YODA_ERR_HIP;
    }
  }
  int rc;
  try {
    rc = comm_step(hs, world, world, mode, true, true);
  } catch (...) {
    rc = fail(hs[0], YODA_ERR_INVALID_ARG, "unexpected exception");
  }
  if (rc == YODA_OK && hipStreamSynchronize(hs[0]->stream) != hipSuccess) rc = YODA_ERR_HIP;
  for (int i = 0; i < world; ++i)
    if (switch_stream(hs[i], saved[i]) != YODA_OK && rc == YODA_OK) rc = YODA_ERR_HIP;
  return rc;
}

}  // extern "C"
