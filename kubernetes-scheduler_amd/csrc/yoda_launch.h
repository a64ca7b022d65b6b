// yoda_launch.h — the host-callable interface of the .hip translation units: every launch_*
// function and the few plain queries beside them, declared once.  yoda_kernels.hip and
// yoda_order.hip define them and yoda_capi.cpp calls them; all three include this header, so a
// definition that drifts from its declaration does not compile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "yoda_layout.h"

namespace yoda {
// ---- yoda_kernels.hip ----
hipError_t launch_k1(int K, Path path, const unsigned char* nodes, const unsigned char* sum,
                     const unsigned char* sum2, const unsigned char* mix,
                     uint32_t n_nodes, uint32_t chunk_nodes, uint32_t C, const PodParams& pp,
                     uint32_t n_pods, const Partials& part, uint64_t* bm, uint32_t bm_stride,
                     BlockMask* bs, uint32_t bs_stride, uint64_t* blk, uint32_t blk_stride,
                     unsigned long long* stats, hipStream_t s);
// rcp non-null: also the reciprocals (k_prep2 fused; the wave variant runs it after)
// nw: the block K1's partial words (kNarrowWords / kWideWords), 0: u64 partials [6][C][P]
// lpt_w / lpt_order non-null: also the block K2's heaviest-first pod-block order (k_lpt_order;
// in k_reduce1's grid as one extra workgroup where that kernel runs)
hipError_t launch_reduce1(const Partials& part, uint32_t C, uint32_t n_pods, uint32_t nw,
                          uint64_t* maxima, uint32_t* counts, double* rcp,
                          const MemTab& mt, hipStream_t s,
                          uint32_t* lpt_w = nullptr, uint32_t* lpt_order = nullptr,
                          const uint64_t* cmask = nullptr);
hipError_t launch_lpt_order(uint32_t* wts, uint32_t n_pods, uint32_t* order, hipStream_t s);
// The block K1's heaviest-first pod-block order: k1_probe's per-wave weights into wts, ranked by
// k_lpt_order into order (n_pb entries); rec (optional): the waves' K1WaveRec records.
hipError_t launch_k1_order(int K, const PodParams& pp, uint32_t n_pods, uint32_t n_nodes,
                           uint32_t* wts, uint32_t* order, K1WaveRec* rec, hipStream_t s);
hipError_t launch_mem_rank(const uint64_t* m_u, uint32_t n_pods, const MemTab& mt, uint32_t* m32,
                           hipStream_t s);
hipError_t launch_prep2(const uint64_t* maxima, uint32_t n_pods, double* rcp,
                        hipStream_t s);
hipError_t launch_window_out(const uint32_t* counts, const uint64_t* maxima, const uint32_t* wit,
                             const double* tk_s, const uint32_t* tk_i, const uint32_t* perm,
                             uint32_t wn, uint32_t kt, bool lists_row_major, unsigned char* out,
                             uint32_t* inv_scratch, hipStream_t s);
hipError_t launch_k2(int K, Path path, const unsigned char* nodes, const unsigned char* sum2,
                     const uint64_t* blk, uint32_t blk_stride, uint32_t n_nodes,
                     uint32_t chunk_nodes, uint32_t C, const PodParams& pp, const uint64_t* maxima,
                     const double* rcp, uint32_t n_pods,
                     const uint64_t* bm, uint32_t bm_stride, const BlockMask* bs,
                     uint32_t bs_stride, const Partials& part, int64_t* rows,
                     unsigned long long* stats, const uint32_t* counts, hipStream_t s);
// Mode B (yoda_modeb.h).  ea: the run's eligibility (yoda_mode_b_follow) -- the table, the pod
// classes' selectors, the pods' class bytes and the counts; an empty one (elig == nullptr) is an
// unrestricted run and takes the kernels' ELIG = false instances.  launch_draw takes it too.
struct DiskElig;
struct DiskEligArgs;
struct DiskWalk;
struct DiskSampArgs;
struct DiskDrawArgs;
// The table build: elig [n_nodes], cnt [kDiskSelCount], from the candidate words (nullptr: off)
// and the presence bitmap.
hipError_t launch_modeb_elig_build(const uint64_t* words, const uint64_t* pres, uint32_t n_nodes,
                                   DiskElig* elig, uint32_t* cnt, hipStream_t s);
hipError_t launch_k2b_rows(const NodeRecB* nodes, uint32_t n_nodes, const PodParams& pp,
                           uint32_t n_pods, const Partials& part, int64_t* rows,
                           const DiskEligArgs& ea, hipStream_t s, const DiskWalk* walk = nullptr);
// Mode B under node sampling (yoda_mode_b_sampling): the rank tables bits / pfx
// [kDiskSelCount][ceil(n_nodes / 64)] from the eligibility table; the plan (counts [2][P], the
// maxima, a's n_found / next_start / walk); the score over each pod's walk, with the selectHost
// draw inside it when draw != nullptr.  walk (the rows launch above): the plan's records.
hipError_t launch_modeb_rank_build(const DiskElig* elig, uint32_t n_nodes, uint64_t* bits,
                                   uint32_t* pfx, hipStream_t s);
hipError_t launch_k2b_samp_plan(const DiskSampArgs& a, uint64_t* maxima, uint32_t* counts,
                                hipStream_t s);
hipError_t launch_k2b_sampled(const NodeRecB* nodes, const PodParams& pp, const DiskLevels& lv,
                              const DiskSampArgs& a, const DiskDrawArgs* draw, int64_t* best,
                              uint32_t* idx, uint32_t* ties, int64_t* low, hipStream_t s);
DiskPlan diskio_plan(uint32_t n_nodes, uint32_t n_cls);
hipError_t launch_k2b(const NodeRecB* nodes, uint32_t n_nodes, const double* cab,
                      uint32_t n_cls, const DiskLevels& lv, const DiskPlan& pl, uint32_t* plc,
                      uint32_t* pidx, const DiskEligArgs& ea, hipStream_t s);
// (one kernel for both: it skips the empty partials that only a run with eligibility writes)
hipError_t launch_reduce2b(const uint32_t* plc, const uint32_t* pidx, uint32_t C, uint32_t n_cls,
                           const uint32_t* cls, uint32_t n_pods, uint32_t node_offset,
                           int64_t* best, uint32_t* idx, uint32_t* ties, int64_t* low,
                           hipStream_t s);
hipError_t launch_rows_transpose(const int64_t* in, uint32_t n_nodes, uint32_t n_pods,
                                 const uint32_t* perm,
                                 int64_t* out, hipStream_t s);
hipError_t launch_reduce2(const Partials& part, uint32_t C, uint32_t n_pods, bool is_f64,
                          uint32_t node_offset, int64_t* best, uint32_t* idx, uint32_t* ties,
                          int64_t* low, hipStream_t s, const uint64_t* cmask = nullptr);
hipError_t launch_merge_prepare(const int64_t* best_global, const int64_t* best_local,
                                uint32_t n_pods, uint32_t* idx, uint32_t* ties, hipStream_t s);
hipError_t launch_fill_diskio_state(uint32_t n_pods, uint32_t n_nodes, uint64_t* maxima,
                                    uint32_t* counts, const DiskEligArgs& ea, hipStream_t s);
hipError_t launch_finalize(const uint32_t* counts, const int64_t* best, const uint32_t* idx,
                           const uint32_t* ties_in, const int64_t* lowest, uint32_t n_pods,
                           bool generic, int32_t* pick, int32_t* status, uint32_t* ties_out,
                           uint32_t* flagged, uint32_t* n_flagged, const FinalScatter& sc,
                           hipStream_t s);
// launch_reduce2 and launch_finalize of an ordered run off the generic path in one kernel
// (C <= 48 chunks; beyond, the two launches): best / idx / ties / low in sorted order as
// launch_reduce2 leaves them, pick / status / ties_out and sc's arrays in the caller's order.
hipError_t launch_reduce2_finalize(const Partials& part, uint32_t C, uint32_t n_pods,
                                   bool is_f64, uint32_t node_offset, const uint64_t* cmask,
                                   const uint32_t* counts, int64_t* best, uint32_t* idx,
                                   uint32_t* ties, int64_t* low, int32_t* pick, int32_t* status,
                                   uint32_t* ties_out, const FinalScatter& sc, hipStream_t s);
hipError_t launch_k3(int K, const unsigned char* nodes, uint32_t n_nodes, uint32_t chunk_nodes,
                     uint32_t C, const PodParams& pp, const uint64_t* maxima, uint32_t n_pods,
                     const uint64_t* bm, uint32_t bm_stride, const uint32_t* flagged,
                     const uint32_t* n_flagged,
                     const int64_t* best, const int64_t* low, const Partials& part,
                     uint32_t max_flagged, hipStream_t s);
hipError_t launch_reduce3_rec(const Partials& part, uint32_t C, const uint32_t* flagged,
                              const uint32_t* n_flagged, uint32_t max_flagged,
                              uint32_t node_offset, ShardRec* rec, hipStream_t s);
hipError_t launch_merge3(const ShardRec* all, uint32_t n_pods, uint32_t world,
                         const uint32_t* flagged, const uint32_t* n_flagged, uint32_t max_flagged,
                         int32_t* pick, int32_t* status, uint32_t* ties, hipStream_t s);
hipError_t launch_reduce3(const Partials& part, uint32_t C, const uint32_t* flagged,
                          const uint32_t* n_flagged, uint32_t max_flagged, uint32_t node_offset,
                          int32_t* pick, int32_t* status, uint32_t* ties, hipStream_t s);
hipError_t launch_bitmask_transpose(const uint64_t* bm, uint32_t bm_stride, const BlockMask* bs,
                                    uint32_t bs_stride, const uint64_t* blk, uint32_t blk_stride,
                                    uint32_t n_nodes,
                                    uint32_t W, uint32_t n_pods, const uint32_t* perm,
                                    uint32_t* out, hipStream_t s);
// Resident 256-thread workgroups of one K1 / K2 instantiation on the whole device (occupancy
// API x CUs), for grid sizing.  which: 1 = K1, 2 = K2.
int kernel_capacity(int K, Path path, int which, int mode_diskio);
hipError_t launch_k2_topk(int K, Path path, const unsigned char* nodes, uint32_t n_nodes,
                          uint32_t chunk_nodes, uint32_t C, const PodParams& pp,
                          const double* rcp, uint32_t n_pods,
                          const uint64_t* bm, uint32_t bm_stride, const BlockMask* bs,
                          uint32_t bs_stride, const uint64_t* blk, uint32_t blk_stride,
                          const Partials& part, double* tk_s, uint32_t* tk_i, int tk,
                          hipStream_t s);
hipError_t launch_topk_merge(const double* tk_s, const uint32_t* tk_i, uint32_t C,
                             uint32_t n_pods, uint32_t node_offset, double* out_s,
                             uint32_t* out_i, int tk, hipStream_t s);
// The block K2's packed-key top-k (N32 path with node summaries; DESIGN.md §5 greedy):
// keys [C][P][tk], merged by launch_topk_merge_keys.  counts: the pods' feasible-node counts
// (a pod with none takes no part in the wave's bounds).
hipError_t launch_k2_topk_block(int K, const unsigned char* nodes, const unsigned char* sum2,
                                const uint64_t* blk, uint32_t blk_stride, uint32_t n_nodes,
                                uint32_t chunk_nodes, uint32_t C, const PodParams& pp,
                                const double* rcp, uint32_t n_pods,
                                const uint64_t* bm, uint32_t bm_stride, const BlockMask* bs,
                                uint32_t bs_stride, const uint32_t* counts, uint64_t* keys,
                                uint32_t ib, int tk, hipStream_t s);
// The 16-deep chunk lists merged into ko-deep exact-prefix lists (k_topk_merge_deep).
hipError_t launch_topk_merge_deep(const uint64_t* keys, uint32_t C, uint32_t n_pods, uint32_t ib,
                                  uint32_t node_offset, double* out_s, uint32_t* out_i, int tk,
                                  int ko, hipStream_t s);
hipError_t launch_topk_merge_keys(const uint64_t* keys, uint32_t C, uint32_t n_pods, uint32_t ib,
                                  uint32_t node_offset, double* out_s, uint32_t* out_i, int tk,
                                  hipStream_t s);
hipError_t launch_set_static(unsigned char* nodes, uint32_t stride, const uint32_t* node,
                             const uint64_t* value, const uint64_t* card_number, uint32_t count,
                             unsigned char* sum, uint32_t sum_stride, unsigned char* sum2,
                             uint32_t sum2_stride, const PermCopy& pc, hipStream_t s);
hipError_t launch_bsum_cn(const unsigned char* sum, uint32_t sum_stride, uint32_t n_nodes,
                          uint32_t* bsum, uint32_t bsw, hipStream_t s);
hipError_t launch_set_cards(unsigned char* nodes, uint32_t stride, const uint32_t* node,
                            const uint32_t* rows, uint32_t row_words, uint32_t count, int K,
                            uint32_t* sum, uint32_t* sum2, uint32_t* mix, uint32_t* x1,
                            const PermCopy& pc, hipStream_t s);
// Mode B's node records of the listed nodes (node == nullptr: of nodes 0 .. count - 1).
hipError_t launch_set_node_metrics(NodeRecB* nodes_b, const uint32_t* node, const NodeRecB* recs,
                                   uint32_t count, uint32_t n_nodes, hipStream_t s);
hipError_t launch_bsum_build(int K, const uint32_t* sum, const uint32_t* sum2, const uint32_t* x1,
                             const uint32_t* mix, uint32_t n_nodes, uint32_t* bsum,
                             hipStream_t s);
hipError_t launch_block_ub(int K, const uint32_t* sum2, const uint32_t* tab, uint32_t n_nodes,
                           uint32_t* out, const uint32_t* levels, hipStream_t s);
hipError_t launch_block_dec(int K, const uint32_t* sum2, const uint32_t* mix, uint32_t n_nodes,
                            uint32_t* out, const uint32_t* levels, MemTab mt, hipStream_t s);
hipError_t launch_gtable(int K, const uint32_t* sum2, const uint32_t* mix, uint32_t n_nodes,
                         const uint64_t* g_max,
                         uint32_t* tab, uint32_t* rcp_out, MemTab mt, hipStream_t s);
int topk_k();
int topk_k_capacity();
uint32_t greedy_one_blocks();
hipError_t launch_greedy_one(int K, Path path, const unsigned char* nodes,
                             const unsigned char* sum2, uint32_t n_nodes,
                             const PodParams& pp, const double* rcp,
                             uint32_t n_pods, uint32_t s, const uint64_t* bm, uint32_t bm_stride,
                             const BlockMask* bs, uint32_t bs_stride, const uint64_t* blk,
                             uint32_t blk_stride, double* part_s, uint32_t* part_i, uint32_t* done, uint32_t* out,
                             hipStream_t st);
hipError_t launch_k1_witness(int K, Path path, const unsigned char* nodes, uint32_t n_nodes,
                             uint32_t chunk_nodes, uint32_t C, const PodParams& pp,
                             uint32_t n_pods, uint64_t* pmax, uint32_t* pwit, uint32_t* pcnt,
                             uint64_t* bm, uint32_t bm_stride, hipStream_t s);
// The block K1 with witnesses (one-model N32 snapshots with summaries): sparse masks, blk.
hipError_t launch_k1_block_witness(int K, const unsigned char* nodes, const unsigned char* sum,
                                   const unsigned char* sum2, const unsigned char* mix,
                                   uint32_t n_nodes, uint32_t chunk_nodes, uint32_t C,
                                   const PodParams& pp, uint32_t n_pods, uint64_t* pmax,
                                   uint32_t* pwit, uint32_t* pcnt, uint64_t* bm,
                                   uint32_t bm_stride, BlockMask* bs, uint32_t bs_stride,
                                   uint64_t* blk, uint32_t blk_stride, hipStream_t s);
hipError_t launch_reduce_wit(const uint64_t* pmax, const uint32_t* pwit, const uint32_t* pcnt,
                             uint32_t C, uint32_t n_pods, uint32_t node_offset, uint64_t* maxima,
                             uint32_t* counts, uint32_t* wcount, uint32_t* wnode, const MemTab& mt, hipStream_t s);
hipError_t launch_wit_prepare(const uint64_t* gmax, const uint64_t* lmax, uint32_t n_pods,
                              uint32_t* wit, hipStream_t s);
uint32_t one_blocks();
// cand_w != nullptr: the pod names candidate class cls_bit (< 64) -- k_one_filter_cand, whose
// feasible set is F' = F and bit cls_bit of cand_w[n] (upload order) while its maxima stay over F
hipError_t launch_one(int K, Path path, const unsigned char* nodes, uint32_t n_nodes,
                      const OnePod& pod, uint64_t* feas, void* part, uint32_t* done,
                      OneOut* out, const MemTab& mt, hipStream_t s,
                      const uint64_t* cand_w = nullptr, uint32_t cls_bit = 0);
hipError_t launch_norm_rows(const int64_t* rows, uint32_t n_nodes, uint32_t n_pods,
                            const int64_t* best, const int64_t* lowest, int64_t* norm,
                            hipStream_t s);
hipError_t launch_pack_rec(const int64_t* best, const uint32_t* idx, const uint32_t* ties,
                           const int64_t* low, uint32_t n_pods, ShardRec* rec, hipStream_t s);
hipError_t launch_merge_rec(const ShardRec* all, uint32_t n_pods, uint32_t world, int64_t* best,
                            uint32_t* idx, uint32_t* ties, int64_t* low, hipStream_t s);
hipError_t launch_sum_multi_u32(const PtrList& src, uint32_t k, uint64_t n, uint32_t* dst,
                                hipStream_t s);
hipError_t launch_pack_key(const int64_t* best, const uint32_t* idx, uint32_t n_pods, uint32_t ib,
                           uint64_t* key, hipStream_t s);
hipError_t launch_unpack_key(const uint64_t* key, uint32_t n_pods, uint32_t ib, int64_t* best,
                             uint32_t* idx, uint32_t* ties, int64_t* low, hipStream_t s);
hipError_t launch_max_multi(const PtrList& src, uint32_t k, uint64_t n, uint64_t* dst,
                            hipStream_t s);
hipError_t launch_draw(int K, Path path, int mode_diskio, const unsigned char* nodes,
                       const NodeRecB* nodes_b, uint32_t n_nodes, const PodParams& pp,
                       const double* rcp, const uint64_t* maxima, const int64_t* low,
                       const uint64_t* bm, uint32_t bm_stride, const BlockMask* bs,
                       uint32_t bs_stride, const uint64_t* blk, uint32_t blk_stride,
                       const DrawArgs& a, const DiskEligArgs& ea, hipStream_t s);
// The sharded draw (yoda_shard_draw_keys / _apply): a.keys is the dense caller-order [n_pods]
// key buffer; a.best / a.status / a.ties the GLOBAL outcome; a.norm_top the exact merge's.
hipError_t launch_shard_draw_keys(int K, Path path, int mode_diskio, const unsigned char* nodes,
                                  const NodeRecB* nodes_b, uint32_t n_nodes, const PodParams& pp,
                                  const double* rcp, const uint64_t* maxima, const int64_t* low,
                                  const uint64_t* bm, uint32_t bm_stride, const BlockMask* bs,
                                  uint32_t bs_stride, const uint64_t* blk, uint32_t blk_stride,
                                  const DrawArgs& a, hipStream_t s);
hipError_t launch_shard_draw_apply(const DrawArgs& a, const uint64_t* keys, hipStream_t s);
hipError_t launch_merge3_top(const ShardRec* all, uint32_t n_pods, uint32_t world,
                             const uint32_t* flagged, const uint32_t* n_flagged,
                             uint32_t max_flagged, int64_t* norm_top, hipStream_t s);
hipError_t launch_min_multi(const PtrList& src, uint32_t k, uint64_t n, uint64_t* dst,
                            hipStream_t s);
// Candidate classes (yoda_set_candidates).  launch_cand_build: the table of one node order
// (out, or nullptr for the table's own order), its per-block AND and the blocks' zero_total
// bits; launch_cand_update: a sparse list of words into the table and its block-grouped copy;
// launch_cand_narrow: K1's masks and counts from F to F' in place, after launch_reduce1.
hipError_t launch_cand_build(const uint64_t* words, const uint32_t* ids,
                             const unsigned char* nodes, uint32_t stride, uint32_t n_nodes,
                             uint64_t* out, uint64_t* band, uint64_t* zt, hipStream_t s);
hipError_t launch_cand_update(const uint32_t* node, const uint64_t* value, uint32_t count,
                              uint64_t* words, const uint32_t* inv, uint64_t* words_p,
                              hipStream_t s);
hipError_t launch_cand_narrow(const CandArgs& a, hipStream_t s);
// Node sampling (yoda_set_node_sampling).  launch_samp_zt: the blocks' zero_total bits of the
// upload order.  launch_samp_pass: K1's masks and counts from F' to the sample S in place, after
// launch_reduce1 and launch_cand_narrow (count, scan, cut); n_found / next_start in the caller's
// pod order.  samp_scratch_words: the u32 words of SampArgs' scratch, carved by samp_scratch.
hipError_t launch_samp_zt(const unsigned char* nodes, uint32_t stride, uint32_t n_nodes,
                          uint64_t* zt, hipStream_t s);
size_t samp_scratch_words(uint32_t n_work, uint32_t n_nodes);
void samp_scratch(SampArgs& a, uint32_t* scratch);
hipError_t launch_samp_pass(const SampArgs& a, hipStream_t s);
// Filter diagnosis (yoda_diagnose / yoda_reason_rows).  launch_diag_select: the pods of a
// completed run whose n_feasible is 0 (all: every pod) into list / *n_list (zero on entry), and
// counts [n_pods][4] zeroed for them, all ones for the others.  launch_diagnose: the sweep
// (k1_diagnose; rows: the per-node codes instead of the counts); it chooses target_tasks.
hipError_t launch_diag_select(const uint32_t* n_feasible, uint32_t n_pods, bool all,
                              uint32_t* list, uint32_t* n_list, uint32_t* counts, hipStream_t s);
hipError_t launch_diagnose(int K, Path path, bool rows, DiagArgs a, hipStream_t s);

// ---- yoda_order.hip ----
// Scratch for the sort: keys[2][P] u64, idx[2][P] u32, then hipcub's temp storage.
size_t order_scratch_bytes(uint32_t n_pods);
// perm[i] = the original index of the i-th pod in sorted order.
hipError_t launch_order_pods(const uint64_t* number, const uint64_t* m_u, const uint64_t* c_u,
                             const uint32_t* need_mem, uint32_t n_pods, const uint32_t key_bits[3],
                             const uint64_t* groups, uint32_t n_groups, void* scratch,
                             size_t scratch_bytes, uint32_t* perm, const uint32_t* m32, hipStream_t s);
// t: the pod arrays (src = caller order, dst = sorted order); scratch: slot, bkt [P] u32.
hipError_t launch_order_count(const OrderMeta& o, const uint64_t* number, const uint32_t* m32,
                              const uint32_t* c32, const uint32_t* need_mem, uint32_t n_pods,
                              uint32_t* hist, uint32_t* bstart, uint32_t* slot, uint32_t* bkt,
                              const PermTable& t, const uint32_t* pad, uint32_t n_pad,
                              uint64_t* zero, uint32_t n_zero, uint32_t* perm, hipStream_t s);
hipError_t launch_permute(const PermTable& t, const uint32_t* perm, uint32_t n_pods, bool scatter,
                          hipStream_t s);
}  // namespace yoda
