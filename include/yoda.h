/*
 * yoda.h — C-ABI of libyoda, the MI355X-native Yoda Filter/Score hot path.
 *
 * This is the drop-in boundary a Go kube-scheduler plugin binds through cgo (see
 * INTEGRATION.md).  It replaces the per-pair Go calls the scheduler framework makes into
 * the reference plugin with one call per pod batch:
 *
 *   reference (Mr-LvGJ/kubernetes-scheduler)            replaced by
 *   ---------------------------------------------       -----------------------------------
 *   filter.PodFitsNumber/Memory/Clock                   yoda_run  (K1: feasibility sweep)
 *     pkg/yoda/filter/filter.go:11-58
 *   collection.CollectMaxValues (PreScore)              yoda_run  (K1: per-pod maxima)
 *     pkg/yoda/collection/collection.go:30-76
 *   score.CalculateBasicScore/Card/Allocate/Actual      yoda_run  (K2: integer card score)
 *     pkg/yoda/score/algorithm.go:96,264-310
 *   score.BalancedCpuDiskIOPriority (live Mode B)       yoda_run  (mode YODA_MODE_DISKIO)
 *     pkg/yoda/score/algorithm.go:99-119
 *   Yoda.Score + filter.Uint64ToInt64                   yoda_run  (K2)
 *     pkg/yoda/scheduler.go:116-156, filter.go:84-86
 *   Yoda.NormalizeScore + k8s v1.22.3 selectHost        yoda_run  (K2 argmax + finalize)
 *     pkg/yoda/scheduler.go:158-183
 *   sort.Less / GetPodPriority (greedy batch order)     yoda_greedy
 *     pkg/yoda/sort/sort.go:8-18
 *
 * Conventions:
 *   - every entry point returns int: YODA_OK (0) or a negative YODA_ERR_* code; the
 *     message of the last failure is in yoda_last_error();
 *   - no C++ exception crosses the boundary; all buffers are caller-owned;
 *   - a handle is NOT thread-safe: one handle per goroutine, or guard it;
 *   - "d_" pointer arguments are device pointers (HIP global memory on the handle's
 *     device); everything else is host memory.
 *
 * Integer widths follow the reference on GOARCH=amd64 (Makefile:4): Go `uint` is 64-bit.
 */
#ifndef YODA_H_
#define YODA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YODA_ABI_VERSION 1

/* Maximum card slots per node (SCV Status.CardList length). */
#define YODA_MAX_CARDS 16

/* ---- status codes ------------------------------------------------------------------ */
#define YODA_OK 0
#define YODA_ERR_INVALID_ARG -1   /* NULL handle/pointer, bad size, bad mode            */
#define YODA_ERR_HIP -2           /* a HIP runtime call failed                          */
#define YODA_ERR_NO_NODES -3      /* yoda_run/yoda_eval before yoda_upload_nodes        */
#define YODA_ERR_NO_PODS -4       /* yoda_run before yoda_upload_pods                   */
#define YODA_ERR_RANGE -5         /* input outside what the library can represent       */
#define YODA_ERR_NO_DEVICE -6     /* no HIP device / bad device ordinal                 */
#define YODA_ERR_STATE -7         /* call out of sequence (e.g. phase2 before phase1)   */
#define YODA_ERR_SAME_DEVICE -8   /* two ranks of one communicator on the same GPU      */

/* ---- scoring modes ----------------------------------------------------------------- */
/* Mode A: the SCV GPU path (filter.go + collection.go + algorithm.go:264-310 composed as
 * algorithm.go:96).  Mode B: the score the shipped binary computes
 * (BalancedCpuDiskIOPriority, algorithm.go:99-119; Filter is a pass-through). */
#define YODA_MODE_SCV 0
#define YODA_MODE_DISKIO 1

/* ---- per-pod outcome (the framework Status the reference would produce) ------------ */
#define YODA_PICK_NONE (-1)  /* no feasible node: Unschedulable                          */
#define YODA_PICK_ERROR (-2) /* framework Error (see status)                             */

#define YODA_STATUS_OK 0             /* pick is a node index                              */
#define YODA_STATUS_UNSCHEDULABLE 1  /* no node passed Filter                              */
#define YODA_STATUS_DIV_ZERO 2       /* a scored node has TotalMemorySum == 0: the
                                        reference panics (algorithm.go:294 / :309)        */
#define YODA_STATUS_SCORE_RANGE 3    /* NormalizeScore produced a score outside [0,100]
                                        (int64 overflow at scheduler.go:178); k8s rejects */

/* Node snapshot, struct-of-arrays.  Node i's card slot j lives at [i * max_cards + j];
 * slots j >= card_count[i] are ignored.  Mirrors the SCV CRD Status
 * (github.com/NJUPT-ISL/SCV api/v1 @46b36eeed646, types pinned by use: filter.go:13,22,53,57,
 * collection.go:14-20, algorithm.go:294,305-309). */
typedef struct yoda_node_soa {
  uint32_t n_nodes;
  uint32_t max_cards;                /* stride of the card arrays, 1..YODA_MAX_CARDS        */
  const uint64_t* card_number;       /* [N] Status.CardNumber                              */
  const uint32_t* card_count;        /* [N] len(Status.CardList), <= max_cards             */
  const uint64_t* free_memory_sum;   /* [N] Status.FreeMemorySum                           */
  const uint64_t* total_memory_sum;  /* [N] Status.TotalMemorySum                          */
  const uint64_t* alloc_memory;      /* [N] sum of scv/memory labels of pods already bound
                                        to the node (algorithm.go:299-303); may be NULL=0   */
  const uint64_t* card_free_memory;  /* [N*K] Card.FreeMemory                              */
  const uint64_t* card_total_memory; /* [N*K] Card.TotalMemory                             */
  const uint64_t* card_clock;        /* [N*K] Card.Clock                                   */
  const uint64_t* card_bandwidth;    /* [N*K] Card.Bandwidth                               */
  const uint64_t* card_core;         /* [N*K] Card.Core                                    */
  const uint64_t* card_power;        /* [N*K] Card.Power                                   */
  const uint8_t* card_healthy;       /* [N*K] Card.Health == "Healthy"                     */
  /* Mode B inputs: advisor.NodeInfo (advisor.go:26-32).  May be NULL for Mode A. */
  const double* cpu;                 /* [N] NodeInfo.Cpu   (percent)                       */
  const double* disk_io;             /* [N] NodeInfo.DiskIO (MB/s)                         */
} yoda_node_soa;

/* Pod requests, struct-of-arrays, already parsed from labels with the reference's Go
 * semantics (strconv.Atoi; negative values wrap to uint64 — filter.go:60-74). */
typedef struct yoda_pod_soa {
  uint32_t n_pods;
  const uint8_t* has_number;   /* [P] label scv/number present (filter.go:12)               */
  const uint64_t* number;      /* [P] strToUint(scv/number)                                */
  const uint8_t* has_memory;   /* [P] label scv/memory present (filter.go:19)               */
  const uint64_t* memory;      /* [P] StrToUint64(scv/memory)                              */
  const uint8_t* has_clock;    /* [P] label scv/clock present (filter.go:36)                */
  const uint64_t* clock;       /* [P] strToUint(scv/clock)                                 */
  const int64_t* priority;     /* [P] Atoi(scv/priority) (sort.go:12-18); may be NULL = 0   */
  /* Mode B: may be NULL for Mode A. */
  const double* rio;           /* [P] ParseFloat(annotations["diskIO"], 32) (algorithm.go:103) */
  const int64_t* rcpu;         /* [P] CalculatePodResourceRequest(cpu) millicores (:104,238) */
} yoda_pod_soa;

/* Per-pod outputs of yoda_eval / yoda_download.  Any pointer may be NULL. */
typedef struct yoda_eval_out {
  int32_t* pick;         /* [P] node index (global), YODA_PICK_NONE or YODA_PICK_ERROR     */
  int32_t* status;       /* [P] YODA_STATUS_*                                              */
  uint32_t* n_feasible;  /* [P] nodes that passed Filter                                   */
  uint32_t* n_ties;      /* [P] nodes sharing the top normalized score (the set k8s
                            selectHost draws from at random)                              */
  int64_t* top_score;    /* [P] raw Score (after Uint64ToInt64) of the picked node         */
  uint64_t* maxima;      /* [P*6] Mode A PreScore maxima in MaxValue order (collection.go:
                            14-21): Bandwidth, Clock, Core, FreeMemory, Power, TotalMemory */
} yoda_eval_out;

typedef struct yoda_handle yoda_t;

/* ---- lifecycle ---------------------------------------------------------------------- */
int yoda_abi_version(void);
/* One handle drives one GPU (device ordinal).  Multi-GPU: one handle per GPU, each holding
 * a node shard, merged by the caller's collectives through the yoda_shard_* entry points. */
int yoda_create(int device, yoda_t** out);
int yoda_destroy(yoda_t* h);
const char* yoda_last_error(const yoda_t* h);
/* Launch all work on this HIP stream (hipStream_t passed as void*; NULL = the HIP null
 * stream, e.g. PyTorch's default stream).  Until called, the handle uses a non-blocking
 * stream of its own; yoda_use_own_stream switches back to it.  Work the handle already
 * queued on its previous stream (e.g. an upload's copies) is ordered before the new
 * stream's next work (an event wait on the device, no host synchronization). */
int yoda_set_stream(yoda_t* h, void* hip_stream);
int yoda_use_own_stream(yoda_t* h);
int yoda_synchronize(yoda_t* h);

/* ---- node snapshot ------------------------------------------------------------------ */
/* Upload a node snapshot (or a shard of one).  node_offset is the global index of this
 * shard's first node: picks are reported as node_offset + local index.  Replaces the
 * previous snapshot.  Chooses the narrowest exact record format the value ranges allow
 * (DESIGN.md §Exactness).  Every copy of the upload is ordered on the handle's stream: a step
 * already queued there (e.g. a yoda_shard_phase1 behind the caller's own work) still reads the
 * previous snapshot.  The call returns after a synchronisation of that stream. */
#define YODA_UPLOAD_FORCE_GENERIC 1u /* always the exact-u64 path                     */
#define YODA_UPLOAD_FORCE_F64 2u     /* never the narrow path (tests)                 */
#define YODA_UPLOAD_NO_UNIFORM 4u    /* disable the per-node GPU-model factoring (tests) */
#define YODA_UPLOAD_PER_NODE_K1 8u   /* N32: per-node K1 sweep instead of the block-
                                        classified one (tests, A/B measurements)      */
#define YODA_UPLOAD_PER_NODE_K2 16u  /* N32: per-pod K2 scoring instead of the block-
                                        classified one (tests, A/B measurements)      */
#define YODA_UPLOAD_NO_GTAB 32u      /* N32: no G table (the block K2 computes every
                                        node's card terms itself; tests, A/B)         */
#define YODA_UPLOAD_MEM_RANKS 64u    /* N32: memory ranks even when every memory field
                                        fits 32 bits (tests, A/B)                     */
#define YODA_UPLOAD_F64_QUOTIENTS 128u /* N32: small-field quotients in f64 even when
                                        every bandwidth/clock/core/power <= 55738 --
                                        for a node shard whose peers hold wider
                                        fields (yoda_small_field_max); a shard with
                                        mixed-model nodes then takes YODA_PATH_F64    */
int yoda_upload_nodes(yoda_t* h, const yoda_node_soa* nodes, uint32_t node_offset,
                      uint32_t flags);
/* 1 if the uploaded snapshot runs on the generic (u64) path, 0 on a fast path. */
int yoda_uses_generic_path(const yoda_t* h);
/* Record format of the uploaded snapshot: YODA_PATH_N32 (u32 fields; f32 or f64 quotients,
 * DESIGN.md §5), YODA_PATH_F64 (exact f64) or YODA_PATH_U64 (exact uint64 wrap-around). */
#define YODA_PATH_N32 0
#define YODA_PATH_F64 1
#define YODA_PATH_U64 2
int yoda_record_path(const yoda_t* h);
/* 1 if the N32 snapshot holds its FreeMemory / TotalMemory as ranks (fields beyond 32 bits,
 * e.g. bytes: the u32 fields keep every comparison and maximum, value tables give the
 * quotients and the maxima -- DESIGN.md §3), 0 if as values; -1 for a NULL handle.  The
 * PreScore maxima returned and exchanged are values either way. */
int yoda_memory_ranks(const yoda_t* h);
/* The largest bandwidth, clock, core or power of any card of the uploaded snapshot.  N32
 * computes their quotients in f32 while every maximum it divides by is <= 55738 and in f64
 * beyond (every bandwidth/clock/core/power up to 2^32 - 2 stays on N32 when every node holds
 * one GPU model with one TotalMemory).  Node shards exchange maxima, so all shards must agree:
 * when the MAX of this over the shards exceeds 55738, re-upload the others with
 * YODA_UPLOAD_F64_QUOTIENTS (yoda_amd/dist.py agree_on_path) before agreeing on the record
 * path.  0 for a NULL handle. */
uint64_t yoda_small_field_max(const yoda_t* h);
/* An upper bound on every raw Score of the uploaded snapshot whatever its allocated memory
 * (Basic at the largest clock + the largest Allocate 300 + Actual); ~0 when unbounded.  The
 * sharded merge packs (score, node) into one 64-bit key when it fits (yoda_amd/dist.py). */
uint64_t yoda_score_bound(const yoda_t* h);
/* Replace alloc_memory (the Allocate-score input) without re-uploading the cards. */
int yoda_update_alloc(yoda_t* h, const uint64_t* alloc_memory);

/* ---- one-shot evaluation ------------------------------------------------------------ */
/* Schedule every pod independently against the uploaded snapshot (each pod sees the same
 * snapshot: a batch of independent scheduling cycles).  Equivalent to
 * yoda_upload_pods + yoda_run + yoda_download. */
int yoda_eval(yoda_t* h, const yoda_pod_soa* pods, int mode, yoda_eval_out* out);

/* selectHost: when enabled, a pod whose cycle ends YODA_STATUS_OK with n_ties >= 2 gets as its
 * pick the node of its tie set (the set n_ties counts) with the smallest draw word
 * yoda_tie_hash(seed, pod_base + p, node), p = the pod's index in the uploaded batch (the
 * CALLER's order), node = its GLOBAL id (node_offset + upload-order index).  Every other output
 * (status, n_feasible, n_ties, top_score, maxima) and every other pod's pick are unchanged.
 * Default: disabled (the lowest node of the set).  Takes effect from the next yoda_run/yoda_eval.
 *
 * The draw word, with mix64 the splitmix64 finalizer (x ^= x>>30; x *= 0xBF58476D1CE4E5B9;
 * x ^= x>>27; x *= 0x94D049BB133111EB; x ^= x>>31) and fmix32 the murmur3 32-bit finalizer
 * (h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16):
 *   s = mix64(seed + 0x9E3779B97F4A7C15 * (pod + 1))              (mod 2^64, once per pod)
 *   yoda_tie_hash = fmix32(fmix32(node ^ lo32(s)) + hi32(s))      (mod 2^32)
 * and the pick is the argmin of (hash << 32) | node over the tie set: a plain 64-bit MIN.  The
 * word depends on (seed, pod, node) alone -- not on the chunking, the pod order, the
 * block-grouped node order or the record path.  A caller that slices a batch across processes
 * passes its slice's first index as pod_base (the slices' picks are then the unsliced batch's);
 * one that wants fresh draws per batch changes the seed.  On the U64 record path the pods that
 * go through the exact normalize draw over the nodes of the top NORMALIZED score.
 * yoda_run / yoda_eval draw; the node-sharded evaluation step (yoda_comm_run*, yoda_shard_*)
 * draws once yoda_shard_tie_draw turns it on as well (below), with picks bit-identical to one
 * handle holding the whole snapshot.  yoda_greedy*, yoda_comm_greedy*, the greedy-window entry
 * points and yoda_score_rows* keep the lowest-node rule whether or not a draw is enabled.
 * YODA_ERR_INVALID_ARG on a NULL handle. */
int yoda_set_tie_draw(yoda_t* h, int enable, uint64_t seed, uint64_t pod_base);
/* Host only.  For fixed (seed, pod) a bijection of the 32-bit node ids: no two nodes share a word. */
uint32_t yoda_tie_hash(uint64_t seed, uint64_t pod, uint32_t node);

/* ---- split evaluation (device-resident timing, multi-GPU) --------------------------- */
int yoda_upload_pods(yoda_t* h, const yoda_pod_soa* pods);
/* Run filter+prescore+score+normalize+select for the uploaded pods; results stay on the
 * device until yoda_download.  Asynchronous on the handle's stream. */
#define YODA_RUN_BITMASK 1u /* also materialise the feasibility bitmask for download      */
int yoda_run(yoda_t* h, int mode, uint32_t flags);
int yoda_download(yoda_t* h, yoda_eval_out* out);
/* Feasibility bitmask of the last yoda_run with YODA_RUN_BITMASK: bit (n & 31) of
 * words[p * ((N + 31) / 32) + n / 32] is set iff node n (local) passed Filter for pod p. */
int yoda_download_bitmask(yoda_t* h, uint32_t* words, uint64_t n_words);

/* Framework-plugin row mode: for the uploaded pods (a handful — one per
 * scheduling cycle), return the Filter result and the raw Score of EVERY node, so the
 * plugin's Filter and Score become lookups and NormalizeScore/selectHost stay the
 * reference's code.  bitmask: [P][ceil(N/32)] as yoda_download_bitmask; scores: [P][N]
 * int64, the value Yoda.Score returns (after Uint64ToInt64), -1 where Filter fails.
 * Also leaves the picks for yoda_download.  Either output may be NULL. */
int yoda_score_rows(yoda_t* h, int mode, uint32_t* bitmask, uint64_t n_bitmask_words,
                    int64_t* scores, uint64_t n_scores);
/* yoda_score_rows plus the normalized scores, computed on the device: norm [P][N] int64 =
 * Yoda.NormalizeScore (scheduler.go:158-183) over each pod's feasible nodes -- highest =
 * max(0, max raw), lowest = min raw, lowest-- when equal, (raw - lowest) * 100 /
 * (highest - lowest) in Go's int64 arithmetic -- and -1 where Filter fails.  k8s then adds
 * the plugin weight and validates [0, 100] (RunScorePlugins). */
int yoda_score_rows_norm(yoda_t* h, int mode, uint32_t* bitmask, uint64_t n_bitmask_words,
                         int64_t* scores, uint64_t n_scores, int64_t* norm, uint64_t n_norm);

/* Sharded evaluation.  Each rank holds a node shard; between phases the caller reduces
 * the exchange buffers across ranks (RCCL all-reduce) with the op named per buffer.
 *   phase1 -> d_maxima [6*P] u64 (MAX), d_counts [2*P] u32 (SUM: n_feasible, n_zero_total)
 *   phase2 (reads reduced maxima/counts) -> d_best [P] i64 (MAX), d_idx [P] u32, d_ties [P]
 *            u32, d_lowest [P] i64 (MIN)
 *   prepare_merge (reads reduced d_best) -> masks d_idx (MIN) and d_ties (SUM) in place
 *   finalize (reads reduced buffers) -> picks into the handle, then yoda_download. */
/* yoda_shard_exchange_order(h, 1): the exchange buffers above are in the CALLER's pod order
 * (the order of yoda_upload_pods), so each shard sorts its pods and nodes privately -- the
 * padded counting order and block-grouped node order of yoda_run -- instead of the
 * reproducible radix order all shards must otherwise share (one shard of config 3: 5.7x
 * faster).  Every shard of a batch must use the same setting.  Evaluation batches only (the
 * greedy-window entry points below refuse it); the U64 record path ignores it.  Default 0. */
int yoda_shard_exchange_order(yoda_t* h, int caller_order);
int yoda_shard_phase1(yoda_t* h, int mode, uint64_t* d_maxima, uint32_t* d_counts);
int yoda_shard_phase2(yoda_t* h, int mode, const uint64_t* d_maxima, const uint32_t* d_counts,
                      int64_t* d_best, uint32_t* d_idx, uint32_t* d_ties, int64_t* d_lowest);
int yoda_shard_prepare_merge(yoda_t* h, const int64_t* d_best_global, const int64_t* d_best_local,
                             uint32_t* d_idx, uint32_t* d_ties);
int yoda_shard_finalize(yoda_t* h, int mode, const uint32_t* d_counts, const int64_t* d_best,
                        const uint32_t* d_idx, const uint32_t* d_ties, const int64_t* d_lowest);
/* Generic path only: pods whose NormalizeScore can overflow int64 are re-evaluated with
 * the exact normalize (scheduler.go:176-179).  Returns the number of such pods in *n_pods
 * (after yoda_shard_finalize: nonzero means the exchange below is needed). */
int yoda_shard_overflow_count(yoda_t* h, uint32_t* n_pods);
/* When yoda_shard_overflow_count reports pods after yoda_shard_finalize, their exact normalize
 * is split across the shards: yoda_shard_exact_records writes this shard's per-pod records
 * (d_rec: [P] x 24 bytes, device), the caller ALL-GATHERS them over the ranks in rank order
 * (d_all: [world][P] x 24 bytes) and yoda_shard_exact_merge folds them into the picks (best
 * normalized score, lowest node, ties summed, a score outside [0, 100] -> STATUS_SCORE_RANGE),
 * completing the step.  yoda_comm_run does this itself. */
int yoda_shard_exact_records(yoda_t* h, void* d_rec);
int yoda_shard_exact_merge(yoda_t* h, const void* d_all, int world);

/* Node shards draw too.  Default 0.  With it on AND yoda_set_tie_draw enabled on the handle,
 * the sharded evaluation step ends in the draw: yoda_comm_run / yoda_comm_run_local do it
 * themselves; a caller driving yoda_shard_* adds the exchange below.  Every shard of a batch
 * must use the same (enable, seed, pod_base).  The greedy-window entry points, yoda_comm_greedy*
 * and yoda_score_rows* keep the lowest node regardless.  With it off (or yoda_set_tie_draw
 * off) the sharded step launches what it always did. */
int yoda_shard_tie_draw(yoda_t* h, int enable);
/* After yoda_shard_finalize.  When yoda_shard_overflow_count reports pods, after
 * yoda_shard_exact_merge instead.  Writes d_keys [P] u64 (device), ALWAYS in the caller's pod
 * order whatever yoda_shard_exchange_order says.  A pod that ended YODA_STATUS_OK with GLOBAL
 * n_ties >= 2 gets the MIN of (yoda_tie_hash << 32 | global node) over THIS shard's nodes
 * that are feasible and score the pod's GLOBAL best.  On the U64 path a pod sent through the
 * exact normalize uses the global top NORMALIZED score instead.  ~0 when this shard holds no
 * such node or the pod does not draw. */
int yoda_shard_draw_keys(yoda_t* h, int mode, uint64_t* d_keys);
/* The caller all-reduces d_keys with an unsigned 64-bit MIN over the ranks (8 P bytes per
 * rank), then: pick <- the key's low 32 bits where key != ~0.  Only pick changes: status,
 * n_feasible, n_ties, top_score and maxima stay what the step gave.
 * Both calls: YODA_ERR_INVALID_ARG for a NULL handle or buffer; YODA_ERR_STATE, the picks left
 * as they were, before a sharded finalize, while exact-normalize pods are pending, after a
 * private yoda_run, with the shard draw or the handle's draw disabled, and for
 * yoda_shard_draw_apply without this step's yoda_shard_draw_keys before it. */
int yoda_shard_draw_apply(yoda_t* h, const uint64_t* d_keys);

/* ---- multi-GPU without a host framework: RCCL inside libyoda ------------------------
 * For callers that have no torch.distributed (the Go plugin through cgo, C).  One handle per
 * GPU holds a node shard (yoda_upload_nodes with its node_offset) and the same pod batch.
 * Rank 0 calls yoda_comm_unique_id and hands the id to the other ranks out of band (a file,
 * the k8s API, MPI ...); every rank then calls yoda_comm_init (collective).  yoda_comm_run is
 * one whole sharded step on the handle's stream -- phase 1; ONE group of all-reduces: MAX of
 * the maxima (+ two agreement words: score bits, node-id bits) and SUM of the counts; phase 2;
 * on the fast record paths the packed-key merge: all-reduce(MAX) of each shard's
 * (best << ib | 2^ib - 1 - node) key, then all-reduce(SUM) of the winners' tie counts (the
 * U64 path in Mode A all-gathers (best, index, ties, lowest) records instead); finalize --
 * then, only with yoda_shard_tie_draw on, the draw: all-reduce(MIN) of the shards' draw keys
 * [P] u64 -- and leaves the picks for yoda_download, like yoda_run.  The first all-reduce also
 * carries a digest of the draw settings and its complement: shards that disagree on them all
 * fail with YODA_ERR_STATE (the handles stay usable).  All shards must run the same
 * record path.  librccl.so.1 is opened at the first call (not a link dependency).
 * yoda_comm_run_local runs the same step for `world` shard handles of ONE process on one
 * device, with device copies as the transport (tests, single-process use). */
#define YODA_COMM_ID_BYTES 128
int yoda_comm_unique_id(uint8_t* id);
int yoda_comm_init(yoda_t* h, const uint8_t* id, int rank, int world);
/* RCCL refuses two ranks on one GPU ("invalid usage").  Before yoda_comm_init every rank
 * exchanges its device key (yoda_device_key, YODA_DEVICE_KEY_BYTES, NUL-terminated: a 16-hex
 * hash of the hostname and boot id, '/', the PCI bus id of yoda_device_bus_id -- bus ids alone
 * repeat across identical servers) along with the communicator id, and checks the gathered keys
 * (rank-major, `stride` bytes apart): YODA_ERR_SAME_DEVICE when two ranks share one, with
 * *rank_a < *rank_b the first such pair (either pointer may be NULL).  Host only: no HIP call. */
#define YODA_BUS_ID_BYTES 32
#define YODA_DEVICE_KEY_BYTES 64
int yoda_device_bus_id(const yoda_t* h, char* out, int len);
int yoda_device_key(const yoda_t* h, char* out, int len);
int yoda_comm_check_devices(const char* bus_ids, int world, int stride, int* rank_a,
                            int* rank_b);
int yoda_comm_run(yoda_t* h, int mode);
int yoda_comm_run_local(yoda_t* const* handles, int world, int mode);
/* The greedy batch (yoda_greedy's semantics) over the ranks' node shards, driven inside libyoda
 * (collective: every rank passes the same pods and the SAME full snapshot `all_nodes`, which the
 * host-side resolve reads; its handle holds this rank's shard).  Per window the maxima / counts
 * (capacity mode: and the maxima witnesses) are all-reduced and the shards' top-k candidate
 * lists all-gathered; an uncertified pod is scored on every shard and the (score, node)
 * candidates all-gathered.  U64 snapshots: every pod one sharded exact step.  pick [P]: global
 * node ids in input order.  The shards' node state is restored at the end.  The C/cgo twin of
 * the Python driver dist.sharded_greedy (the Go plugin's ShardedGreedy calls it); the same
 * picks, but its capacity windows take yoda_greedy's deeper lists (each shard's merged to 64,
 * the union cut where it stops being certain), so it runs fewer windows than the Python driver.
 * _local: the same over `world` handles of this process on one device (tests). */
int yoda_comm_greedy(yoda_t* h, const yoda_node_soa* all_nodes, const yoda_pod_soa* pods,
                     int mode, uint32_t flags, int32_t* pick);
/* Work counters of the last yoda_comm_greedy[_local] on this handle (the first handle for
 * _local): out[5] = {windows, pods evaluated one by one (exchanges), capacity restarts,
 * mid-window list refreshes, collective calls}. */
int yoda_comm_greedy_stats(const yoda_t* h, uint32_t* out);
int yoda_comm_greedy_local(yoda_t* const* handles, int world, const yoda_node_soa* all_nodes,
                           const yoda_pod_soa* pods, int mode, uint32_t flags, int32_t* pick);

/* ---- batch ordering ---------------------------------------------------------------- */
/* Mode A runs of more than 128 pods (yoda_run, yoda_score_rows, yoda_shard_phase1) sort the
 * batch on the device by the Filter's inputs so that whole wavefronts skip infeasible nodes;
 * every output is returned in the caller's pod order, so results never depend on it.
 * enable = 0 turns the ordering off; 1 (default) orders, a private run (yoda_run) padding each
 * (clock, number, has-memory) group to a wave boundary when that adds at most 1/8 of the
 * batch; 2 orders without the padding.  Takes effect from the next run. */
int yoda_set_pod_order(yoda_t* h, int enable);
/* The batch order (diagnostic): out[4] = {(clock, number, has-memory) groups of the uploaded
 * batch (0: too many for the counting sort), its sorted positions with every group padded to
 * a wave, the sorted positions of the last run, how that run was ordered (0 not, 1 radix sort,
 * 2 counting sort)}. */
int yoda_order_info(const yoda_t* h, uint32_t* out);
/* The node snapshot's order in private runs (diagnostic): *grouped = 1 when its one-model nodes
 * are dealt into 64-node blocks of one clock for yoda_run (copies of the summaries in that
 * order), 0 when the upload order is used. */
int yoda_node_order(const yoda_t* h, uint32_t* grouped);

/* ---- kernel timing ----------------------------------------------------------------- */
/* enable != 0: every subsequent K1 / K2 launch is bracketed by HIP events recorded on the
 * launch stream.  yoda_profile_read synchronizes, returns the summed K1 and K2 durations
 * (ms) and launch count since the last read, and clears them. */
int yoda_profile(yoda_t* h, int enable);
int yoda_profile_read(yoda_t* h, double* k1_ms, double* k2_ms, uint32_t* n_launches);

/* ---- work classes ------------------------------------------------------------------ */
/* Device counters of how the block-classified kernels (N32 path) split the
 * (pod wave, node) pairs of the runs made while enabled (one atomic per wave and chunk).
 * read: {K1 ALL, K1 NONE, K1 PART, K2 U, K2 FAST, K2 EXACT, K2 skipped,
 * K2 (wave, chunk)s with uniform maxima, K2 (wave, chunk)s, (wave, node) pairs,
 * K2 FAST pairs served by node records, K2 per-pod pairs of non-uniform waves,
 * the most per-pod nodes of one (wave, chunk), K1 (wave, 64-node block)s the block summaries
 * decide NONE, ... decide ALL, K1 (wave, block)s classified node by node, K2 (wave, block)s
 * pruned by their bound,
 * K2 (wave, block)s worked on}: out[18]; resets them. */
int yoda_class_stats_enable(yoda_t* h, int enable);
int yoda_class_stats_read(yoda_t* h, uint64_t* out);
/* Diagnostic: with YODA_K2_TRACE=<slots> set when the counters are enabled, the block K2
 * records per (pod wave, chunk) {start, end (100 MHz clock), per-pod nodes, uniform maxima}
 * at slot wave * chunks + chunk; out[4 * n_slots]. */
int yoda_k2_trace_read(yoda_t* h, uint64_t* out, uint64_t n_slots);

/* ---- greedy batch ------------------------------------------------------------------- */
/* Schedule the pods one after another in queue order (sort.go:8-10: scv/priority
 * descending, then input index), each pick feeding the next cycle through the node's
 * Allocate score (alloc_memory += scv/memory, algorithm.go:299-303; the scheduler-cache
 * "assume" of SURVEY §3.4).  YODA_GREEDY_CARD_CAPACITY additionally decrements the picked
 * node's CardNumber by the pod's number (saturating at 0): a build-defined extension,
 * batched as well (a window restarts at the first pod the capacity certificate cannot
 * clear).  The uploaded snapshot is left unchanged.
 *   While candidate classes are on (yoda_set_candidates) it returns YODA_ERR_STATE unless
 * yoda_greedy_candidates is on: each pod's cycle is then the candidate-class cycle against the
 * current state, the pod's class taken from the yoda_set_pod_classes array at its input index. */
#define YODA_GREEDY_CARD_CAPACITY 1u
int yoda_greedy(yoda_t* h, const yoda_pod_soa* pods, int mode, uint32_t flags, int32_t* pick);
/* Work counters of the last yoda_greedy: GPU top-k windows, pods evaluated one by one
 * (uncertified candidates, or every pod on the exact sequential path), and host wall time
 * (ms) in times_ms[0..2] = {window candidate passes, sequential resolve, exact fallbacks}
 * (times_ms may be NULL). */
int yoda_greedy_stats(const yoda_t* h, uint32_t* windows, uint32_t* fallbacks,
                      double* times_ms);
/* YODA_GREEDY_CARD_CAPACITY: windows of the last yoda_greedy that ended early at a pod the
 * capacity certificate could not clear (that pod then opens the next window).  The capacity
 * mode restarts on every uncertified pod by default (no exact fallbacks: the fallback count
 * stays 0); the YODA_GREEDY_FAIL_DIV environment knob re-enables one-by-one fallbacks for
 * A/B runs. */
int yoda_greedy_restarts(const yoda_t* h, uint32_t* restarts);
/* flags == 0: mid-window list refreshes of the last yoda_greedy (the window's top-k lists
 * recomputed against the current state once many of its remaining pods had gone uncertified;
 * DESIGN.md §5). */
int yoda_greedy_refreshes(const yoda_t* h, uint32_t* refreshes);

/* ---- sharded greedy batch (node shards on several GPUs) ------------------------------
 * yoda_greedy's windowed algorithm split at its exchange points, so each rank's handle holds
 * a node shard (reference semantics as yoda_greedy: sort.go:8-10 order, the scheduler-cache
 * assume of algorithm.go:299-303).  Per window of W pods, on every rank:
 *   yoda_upload_pods(window) ; yoda_shard_phase1 ; all-reduce maxima MAX, counts SUM ;
 *   yoda_shard_topk -> the shard's best yoda_topk_k() (score, global node) per pod, sorted by
 *     score desc / node asc, -1.0 / 0xFFFFFFFF padding, plus the reduced counts, all in the
 *     window's pod order ;
 *   merge the shards' lists (keep the first yoda_topk_k() of their union in that order) ;
 *   yoda_gs_begin_window ; loop { yoda_gs_resolve -> next ; if next == W break ;
 *     [mid-window refresh, every 8th such pod: when yoda_gs_uncertified(next + 1, 256) >= 16,
 *      push yoda_gs_take_dirty, yoda_shard_topk again on every shard (the window's phase-1
 *      masks and maxima stay valid: only static scores change), merge as above and
 *      yoda_gs_refresh(next, merged) -- then resolve again] ;
 *     push yoda_gs_take_dirty to every shard (yoda_set_node_state) ;
 *     yoda_shard_best_one(next) on every shard ; pick = max score, lowest node ;
 *     yoda_gs_assign(ws + next, pick) } ; push yoda_gs_take_dirty.
 * That is the flags == 0 protocol on the fast record paths (N32 / F64).  With
 * YODA_GREEDY_CARD_CAPACITY each window runs the witness phase 1 below instead, and the first
 * pod the session cannot certify opens the next window (sized by yoda_greedy_next_window);
 * no pod is evaluated one by one.  On the U64 path every pod is one exact sharded step
 * (yoda_shard_phase1 / phase2 / finalize over a one-pod batch) fed to yoda_gs_assign. */
int yoda_topk_k(void);
/* The capacity windows' list depth: yoda_shard_topk returns this many candidates per pod after
 * yoda_shard_phase1_witness (yoda_topk_k() after yoda_shard_phase1). */
int yoda_topk_k_capacity(void);
/* Set the allocated memory (and CardNumber) of the listed nodes (GLOBAL ids; ids outside
 * this handle's shard are ignored) and refresh their static score on the device.  An id may
 * appear more than once in the list: its LAST entry wins, on the device and in the host copies
 * alike (the earlier ones are dropped before anything is written).  count == 0 is a no-op.  An
 * allocation above the node's total memory is accepted: its Allocate score is 0, as in the
 * reference (algorithm.go:305-307).  YODA_ERR_RANGE (a static score beyond the fast paths'
 * range) leaves the handle as it was before the call. */
int yoda_set_node_state(yoda_t* h, uint32_t count, const uint32_t* nodes, const uint64_t* alloc,
                        const uint64_t* card_number);
/* Replace the dynamic SCV metrics of the listed nodes -- every card's FreeMemory and Health,
 * and FreeMemorySum -- without re-uploading the snapshot.  nodes: GLOBAL ids (ids outside this
 * handle's shard are ignored); card arrays [count * max_cards], slot j of entry t at
 * [t * max_cards + j], slots >= the node's uploaded card_count ignored; an id listed more than
 * once keeps its LAST entry; count == 0 is a no-op.  Card count, CardNumber, TotalMemory[Sum],
 * clock, bandwidth, core, power are NOT changed by this call (CardNumber: yoda_set_node_state;
 * the rest: yoda_replace_nodes).  max_cards: 1..16 and at least the uploaded card count of every
 * listed node.  After it the handle answers every entry point as a handle freshly uploaded with
 * the modified snapshot would.  YODA_ERR_RANGE: a value the uploaded snapshot's format cannot
 * hold -- on the 32-bit record path a FreeMemory above 0xFFFFFFFE or, with memory ranks
 * (yoda_memory_ranks), one that is not a card FreeMemory value of the uploaded snapshot; on the
 * f64 path a FreeMemory above 2^44; on either a static score (new FreeMemorySum, current
 * allocation) of 2^51 or more.  Everything is validated before anything is written: a failed
 * call leaves the handle exactly as it was; re-upload. */
int yoda_update_node_cards(yoda_t* h, uint32_t count, const uint32_t* nodes, uint32_t max_cards,
                           const uint64_t* card_free_memory, const uint8_t* card_healthy,
                           const uint64_t* free_memory_sum);
/* Take the listed nodes out of the uploaded snapshot (present[t] == 0) or back in (!= 0) without
 * a re-upload: a node that left the cluster's node set (drain, NotReady, a deleted SCV) or came
 * back.  nodes: GLOBAL ids (ids outside this handle's shard are ignored); an id listed more than
 * once keeps its LAST entry; count == 0 is a no-op; YODA_ERR_NO_NODES before an upload,
 * YODA_ERR_INVALID_ARG for a NULL array.  The work is ordered on the handle's stream as the card
 * updates are, and pending run, phase-1 and top-k state is invalidated.  yoda_upload_nodes makes
 * every node present again.
 *   While a node is absent every Mode A entry point answers exactly as a handle freshly uploaded
 * with the snapshot WITHOUT that node would, the surviving nodes keeping their ids -- in the
 * reference a removed SCV, which CollectMaxValues (collection.go:39-52), Filter and Score never
 * see: the node is in no pick, in no n_feasible or n_ties, contributes to no PreScore maximum and
 * to no witness, its feasibility bit is 0 and its raw and normalized row scores are -1; the
 * single-feasible-node rule and YODA_STATUS_DIV_ZERO follow from the reduced counts; n_nodes,
 * the node ids and node_offset do not change.  yoda_set_node_state, yoda_update_alloc and
 * yoda_update_node_cards on an absent node apply their values and leave it absent: it shows them
 * when it returns.  yoda_greedy* leaves the presence as it found it.
 *   Mode B (YODA_MODE_DISKIO) has no Filter and does not read the bit: while any node is absent
 * its entry points return YODA_ERR_STATE and do nothing else; with every node present it is
 * untouched.  yoda_mode_b_follow (below) makes its single-handle batch path follow the node set.
 *   This is NOT a per-cycle candidate mask for other plugins' Filter results (cordon, taints,
 * nodeSelector): in the reference such a node's SCV still feeds CollectMaxValues, an absent
 * node's does not.  That mask is yoda_set_candidates (below).
 *   Cost: the listed nodes' rows and every table derived from them, as yoda_update_node_cards; a
 * 64-node block with an absent node is classified node by node instead of as a whole.  Measured
 * at 100k pods x 100k nodes (profiles/nodepresent/timing.txt): the call plus the first run after
 * it 0.9-1.5 ms up to 1,024 nodes and 6-9 ms at 16,384, against 110-150 ms for a re-upload of the
 * compacted snapshot; the step with up to 1,024 absent nodes is the compacted snapshot's, with
 * 16,384 (a sixth of the fleet) 0.10 ms (10-27 %) above it.  Re-upload the compacted snapshot
 * instead only when about that many nodes stay absent for more than a thousand steps. */
int yoda_set_node_present(yoda_t* h, uint32_t count, const uint32_t* nodes,
                          const uint8_t* present);
/* Diagnostic (host only): how many nodes of this handle's snapshot are absent. */
int yoda_nodes_absent(const yoda_t* h, uint32_t* n_absent);
/* Replace the WHOLE record of the listed nodes -- card count, CardNumber, every card field, the
 * memory sums, the allocation, and Mode B's cpu / disk_io -- without re-uploading the snapshot: a
 * machine whose GPUs were swapped, a changed card count, TotalMemory[Sum], clock, bandwidth, core
 * or power.  recs: a yoda_node_soa with n_nodes == count whose entry t is the complete new record
 * of node nodes[t] (GLOBAL id); recs->max_cards (1..16) is its own stride; every array means what
 * it means for yoda_upload_nodes (alloc_memory == NULL: 0; cpu / disk_io: required when the
 * snapshot was uploaded with them, ignored when it was not).  Ids outside this handle's shard are
 * ignored, so one list serves every shard; an id listed more than once keeps its LAST entry (the
 * earlier ones are neither checked nor written); count == 0 is a no-op.  YODA_ERR_NO_NODES before
 * an upload; YODA_ERR_INVALID_ARG for a NULL array, recs->n_nodes != count, a card_count above
 * recs->max_cards or missing cpu / disk_io.  The work is ordered on the handle's stream; pending
 * run, phase-1, top-k, draw and diagnosis state is invalidated.
 *   After the call the handle answers every entry point -- both modes, all three record paths,
 * yoda_greedy*, the yoda_shard_* and yoda_comm_* calls, yoda_snapshot_check with every mismatch
 * word 0 -- as a handle freshly uploaded with the modified snapshot and the same upload flags
 * would once it is brought to the same presence bits, candidate words, pod classes and settings.
 * The node keeps its presence bit: an absent node takes the record and stays absent, and the
 * record counts for the PreScore maxima when it returns.  The node keeps its candidate word
 * (yoda_update_candidates changes it).  One documented exception: yoda_score_bound and
 * yoda_small_field_max only grow -- they stay valid upper bounds, not the fresh upload's tight
 * ones.  The block grouping, the K2 bound levels and the hot-block hint stay as uploaded (speed
 * only, no result depends on them).
 *   New nodes (scale-up) are served by spare slots: upload placeholder nodes (card_count 0), take
 * them out with yoda_set_node_present, and when a node joins replace one placeholder with its
 * record and put it back.  n_nodes itself never changes.
 *   YODA_ERR_RANGE: the record does not fit the format the upload chose (NOT the one a fresh
 * upload of the new snapshot would choose, which may be narrower: the handle keeps the wider one).
 * A card count above the snapshot's card stride (the uploaded largest count rounded up to 1, 2,
 * 4, 8 or 16).  On the 32-bit record path: a clock, bandwidth, core or power above 0xFFFFFFFE, or
 * above 65535 / 55738 when the upload packed them in 16 bits / took f32 quotients (every uploaded
 * value was that small); a node with several GPU models or TotalMemory values when it did not take
 * f32 quotients; 800 + 100 * clock / max(bandwidth, 1), times the card stride, of 2^32 or more; a
 * FreeMemory or TotalMemory above 0xFFFFFFFE or, with memory ranks (yoda_memory_ranks), one that
 * is no card FreeMemory resp. TotalMemory value of the uploaded snapshot.  On the f64 path a card
 * field above 2^44.  On both a static score of 2^51 or more, or card stride * (800 + 100 * clock)
 * + static score of 2^52 or more.  The exact-u64 path takes everything.  Everything is validated
 * before anything is written: a failed call leaves the handle exactly as it was; re-upload.
 *   Cost: that of yoda_update_node_cards for the same list (the same writer and rebuilds). */
int yoda_replace_nodes(yoda_t* h, uint32_t count, const uint32_t* nodes,
                       const yoda_node_soa* recs);
/* Mode B's node inputs, NodeInfo.Cpu and NodeInfo.DiskIO (live metrics, re-read in every PreScore:
 * scheduler.go:101-114), without a re-upload.  Sparse form: nodes holds GLOBAL ids, entry t the
 * new cpu[t] / disk_io[t] of node nodes[t]; ids outside this handle's shard are ignored, the LAST
 * entry of a repeated id wins, count == 0 is a no-op.  Dense form: nodes == NULL and
 * count == n_nodes, entry i is local node i (the whole fleet after a scrape).  YODA_ERR_NO_NODES
 * before an upload; YODA_ERR_STATE when the snapshot was uploaded without cpu / disk_io;
 * YODA_ERR_INVALID_ARG for a NULL cpu / disk_io or a dense count other than n_nodes.  The stored
 * records are bit-identical to a fresh upload's (the same host division).  Ordered on the handle's
 * stream; pending run state is invalidated.  Presence bits, candidate words, pod classes and
 * settings stay, and the eligibility table of yoda_mode_b_follow, which does not read the metrics,
 * is NOT rebuilt (yoda_mode_b_info's build counter).  Mode A never reads these records. */
int yoda_update_node_metrics(yoda_t* h, uint32_t count, const uint32_t* nodes, const double* cpu,
                             const double* disk_io);
/* ---- Candidate classes: other plugins' Filter results in the batch path ----
 * In kube-scheduler a node is scored for a pod only if EVERY Filter plugin passed it (cordon,
 * taints, nodeSelector / affinity, resource fit), while CollectMaxValues
 * (pkg/yoda/collection/collection.go:39-52) walks every SCV under Yoda's own predicates alone.
 * With cand(p, n) the other plugins' verdict: the PreScore maxima are unchanged (over every
 * present node that passes Yoda's Filter, candidate or not); the feasible set is
 * F'(p) = {n : Yoda's Filter passes and cand(p, n)}; a node outside F' has feasibility bit 0 and
 * raw and normalized row scores of -1 and is in no tie set and no draw; a node of F' scores what
 * it scores without candidates; n_feasible, the single-feasible-node rule, UNSCHEDULABLE,
 * DIV_ZERO (a node of F' with TotalMemorySum == 0 and |F'| >= 2), NormalizeScore's highest and
 * lowest, n_ties, top_score, the lowest-node pick and the draw of yoda_set_tie_draw all follow F'.
 * An absent node (yoda_set_node_present) stays out of everything whatever its word says.
 *   Pods with the same scheduling constraints share one node set: each node carries a 64-bit
 * word, bit c set when it is a candidate for class c; each pod carries a class byte.  Cordoning
 * a node is one yoda_update_candidates entry with word 0.
 *   Honoured by yoda_eval, yoda_run (with and without YODA_RUN_BITMASK), yoda_download,
 * yoda_download_bitmask, yoda_score_rows and yoda_score_rows_norm in Mode A.  While candidates
 * are on (and until the opt-in settings below say otherwise), Mode B, yoda_greedy*, yoda_shard_*
 * and yoda_comm_* return YODA_ERR_STATE and do nothing else -- every shard call that starts,
 * advances or reads a step, the exact-normalize, merge, witness and draw calls included; only
 * the settings (yoda_shard_tie_draw, yoda_shard_exchange_order, yoda_shard_candidates) and the
 * host queries (yoda_shard_topk_depth, yoda_shard_overflow_count) answer.  A change of the
 * candidate state also drops a sharded step's pending exact merge.  With candidates off they
 * run as they always did.  Mode B's
 * single-handle batch path honours the classes once yoda_mode_b_follow (below) is on, and
 * yoda_greedy on one handle once yoda_greedy_candidates (below) is on; the sharded Mode A
 * evaluation step (yoda_shard_phase1 .. yoda_shard_draw_apply, yoda_comm_run[_local]) once
 * yoda_shard_candidates (below) is on; the sharded and communicator greedy calls and Mode B on
 * shards keep refusing.
 *   The calls are ordered on the handle's stream and invalidate pending run, phase-1 and top-k
 * state, as yoda_set_node_present does; each validates its arguments before it writes anything.
 *   Cost: one pass over K1's masks after the Filter kernel (k_cand_narrow); the K2 pruning seeds
 * are off while candidates are on.  Measured at 100k pods x 100k nodes, config 3
 * (profiles/candidates/timing.txt): the step 0.38 ms with candidates never set (the parent's),
 * 0.42 ms with all-ones words and one class (0.025 ms of lost seeds, 0.016 ms of a pass that
 * visits nothing), 0.82 / 0.96 ms with 8 classes that each lack 1 % / 30 % of the nodes, of which
 * the pass is 0.39 / 0.43 ms -- 2.6 times K1, because with 8 classes in every pod wave no block is
 * skipped; yoda_set_candidates 0.1 ms, yoda_update_candidates of up to 1,024 nodes under 0.07 ms. */
#define YODA_MAX_CAND_CLASSES 64
#define YODA_CAND_ANY 0xFFu /* the pod is unrestricted: every node is a candidate */
/* words[n_nodes of this handle's shard], upload order.  n_classes 1..64; bits >= n_classes are
 * ignored.  n_classes == 0 (words may be NULL) turns candidates off; so does yoda_upload_nodes.
 * YODA_ERR_NO_NODES before an upload. */
int yoda_set_candidates(yoda_t* h, uint32_t n_classes, const uint64_t* words);
/* Sparse: replace the words of the listed nodes.  GLOBAL ids; ids outside the shard are ignored;
 * the LAST entry of a repeated id wins; count == 0 is a no-op.  YODA_ERR_STATE while candidates
 * are off. */
int yoda_update_candidates(yoda_t* h, uint32_t count, const uint32_t* nodes,
                           const uint64_t* words);
/* The class of every pod of the batches run from now on: cls[n_pods], each < n_classes or
 * YODA_CAND_ANY.  NULL or n_pods == 0 makes every pod YODA_CAND_ANY again.  Stays on the handle
 * across uploads of pods; a run with candidates on whose class array is not as long as the
 * uploaded batch returns YODA_ERR_STATE and launches nothing. */
int yoda_set_pod_classes(yoda_t* h, uint32_t n_pods, const uint8_t* cls);
/* Diagnostic, host only: out[3] = {n_classes (0 = off), the length of the class array, nodes
 * whose word lacks at least one of the n_classes bits}. */
int yoda_candidates_info(const yoda_t* h, uint32_t* out);
/* Diagnostic: the narrowing pass's time (HIP events, ms) summed over the runs that the
 * yoda_profile_read calls since the last call of this one have read (yoda_profile on). */
int yoda_candidates_profile(yoda_t* h, double* narrow_ms);
/* ---- Node sampling: score only the first numFeasibleNodesToFind nodes ----
 * kube-scheduler v1.22.3 does not hand Score every feasible node (findNodesThatPassFilters /
 * numFeasibleNodesToFind, generic_scheduler.go): it walks the node list from a rotating start
 * index, stops Filter once num_to_find nodes have passed, and scores those.  Read at parallelism
 * 1 (the deterministic stand-in, in the spirit of the lowest-node rule), for a pod p with
 * F'(p) today's feasible set (present, Yoda's Filter, a candidate of the pod's class) and the
 * rotated order the GLOBAL ids start[p], start[p] + 1, ..., node_offset + N - 1, node_offset,
 * ..., start[p] - 1 (absent nodes skipped: they are not in the scheduler's list; start[p] may
 * itself be absent):
 *   S(p) = the first min(M, |F'|) nodes of F' in rotated order, M = num_to_find.
 * The PreScore maxima do not move (CollectMaxValues walks every SCV).  Everything downstream of
 * Filter follows S exactly as it follows F' without sampling: n_feasible = |S|, the
 * single-feasible-node rule, UNSCHEDULABLE, DIV_ZERO (a zero-total node of S with |S| >= 2),
 * NormalizeScore's highest and lowest, n_ties, top_score, the lowest-node pick, the draw of
 * yoda_set_tie_draw, the feasibility bitmask, the raw and normalized rows (-1 outside S) and the
 * U64 path's exact normalize.  n_found[p] = |F'(p)|, the count before the cut.  next_start[p]: if
 * |F'| > M the GLOBAL id of the (M+1)-th node of F' in rotated order (the walk stops at it and
 * does not count it, so the next cycle begins there), else start[p] as given (the walk went full
 * circle).  A pod with M >= |F'| has the outputs it has without sampling.
 *   Honoured by yoda_eval, yoda_run (with and without YODA_RUN_BITMASK), yoda_download,
 * yoda_download_bitmask, yoda_score_rows and yoda_score_rows_norm in Mode A, with or without
 * candidate classes, absent nodes and the draw, and by the same calls in Mode B once
 * yoda_mode_b_sampling (below) is on.  While sampling is on, Mode B without that setting,
 * yoda_greedy*, every yoda_shard_* and yoda_comm_* call that starts, advances or reads a step, yoda_reason_rows and
 * yoda_diagnose with YODA_DIAG_ALL return YODA_ERR_STATE and do nothing else; the default
 * yoda_diagnose works unchanged (a pod with |S| = 0 has |F'| = 0: every node was visited).  With
 * sampling off nothing launches differently.
 *   Out of scope, refused as above: sampling in yoda_greedy (either mode) and on node shards and
 * communicators; chaining next_start from pod to pod inside one batch (a sequential dependency: the
 * caller feeds next_start into the NEXT batch's start); K1 stopping early once a pod's sample is
 * full (the maxima need the whole sweep).
 *   Cost: three launches after the Filter kernel and the narrowing pass (k_samp_count,
 * k_samp_scan, k_samp_cut), no host round trip.  A sampled run reads the upload-order node tables
 * (a mask position is then a node id), which costs the block-grouped order's speed and nothing
 * else, and the K2 pruning seeds are off, as under candidates and for the same reason.  Measured
 * at 100k pods x 100k nodes, config 3, M = 5000 and a uniform random start per pod
 * (profiles/sampling/timing.txt): the step 0.38 ms with sampling never set (inside the parent's
 * process-to-process spread), 0.91 ms with sampling on and nothing cut (M = N: the upload-order
 * tables and the lost seeds), 2.72 ms sampled -- K1 0.37, the pass 1.27, K2 1.00 ms: a wave's 64
 * pods keep 64 different stretches of the node list, so K2 finds almost no node whole -- and
 * 3.73 ms with 8 candidate classes as well; yoda_set_node_sampling of 100,000 starts 0.06-0.10
 * ms.  Sampling is for the deployed scheduler's picks, not a saving.  Unmeasured: starts shared
 * inside a wave, the F64 / U64 paths, K other than 8. */
/* Host only, 64-bit arithmetic: n_nodes when n_nodes < 100 or percentage >= 100; else with
 * a = percentage, or max(5, 50 - n_nodes / 125) for percentage <= 0, max(n_nodes * a / 100, 100).
 * (100000, 0) -> 5000; (5000, 0) -> 500; (4608, 0) -> 645. */
uint32_t yoda_num_feasible_to_find(uint32_t n_nodes, int32_t percentage);
/* num_to_find == 0 turns sampling off; so does yoda_upload_nodes.  start[n_pods]: GLOBAL ids in
 * the caller's pod order; NULL: every pod starts at node_offset.  The array stays on the handle
 * across uploads of pods, as the class array does; a run whose start array is neither empty nor
 * as long as the uploaded batch returns YODA_ERR_STATE and launches nothing.  YODA_ERR_NO_NODES
 * before an upload; YODA_ERR_RANGE for an id outside [node_offset, node_offset + n_nodes) -- the
 * call validates before it writes.  Ordered on the handle's stream; invalidates pending run,
 * phase-1, top-k, draw and diagnosis state. */
int yoda_set_node_sampling(yoda_t* h, uint32_t num_to_find, uint32_t n_pods, const uint32_t* start);
/* n_found[n_pods], next_start[n_pods] of the last run, caller order; either may be NULL.  Answers
 * when yoda_download would, after a sampled run; otherwise YODA_ERR_STATE. */
int yoda_download_sampling(yoda_t* h, uint32_t* n_found, uint32_t* next_start);
/* Diagnostic, host only: out[3] = {num_to_find (0 = off), the length of the start array, 1 when
 * the last run ran the sampling pass}. */
int yoda_sampling_info(const yoda_t* h, uint32_t* out);
/* Diagnostic: the sampling pass's time (HIP events, ms), as yoda_candidates_profile. */
int yoda_sampling_profile(yoda_t* h, double* pass_ms);
/* ---- yoda_greedy honours the candidate classes (opt-in) ----
 * enable != 0: yoda_greedy on this handle runs while candidates are on, each pod's cycle being
 * the candidate-class cycle above against the CURRENT node state of the batch (the assumes of
 * the pods before it in queue order; with YODA_GREEDY_CARD_CAPACITY at the current CardNumber):
 * the PreScore maxima over every present node that passes Yoda's Filter now, a candidate or not;
 * F'(p) = the nodes of that set with cand(p, n); |F'| = 0 YODA_PICK_NONE, |F'| = 1 that node
 * without scoring, |F'| >= 2 with a zero-total node of F' YODA_PICK_ERROR, otherwise the lowest
 * node among the top-scored of F' (U64 path: the exact normalize over F', SCORE_RANGE ->
 * YODA_PICK_ERROR).  The assume is unchanged, and a pod without a pick assumes nothing.  The
 * candidate words do not change inside a batch.
 *   The pods' classes are the yoda_set_pod_classes array indexed by the pod's position in `pods`
 * (input order, not queue order): as long as pods->n_pods, or empty (every pod YODA_CAND_ANY);
 * otherwise YODA_ERR_STATE and nothing is launched.  After the call, success or failure, the
 * handle holds the node state, presence, candidate words and class array (host and device) it
 * held before.
 *   Mode B (YODA_MODE_DISKIO) honours the classes only when yoda_mode_b_follow is on too: the
 * independent cycles of yoda_run in queue order, each pod with its own class; with it off the
 * Mode B refusal stands.
 *   Off (the default): yoda_greedy returns YODA_ERR_STATE while candidates are on, exactly as
 * before.  A setting: it stays across uploads until changed.  YODA_ERR_INVALID_ARG on a NULL
 * handle.  Unchanged with the setting on: yoda_shard_*, yoda_comm_* and yoda_comm_greedy* (and
 * the Python driver dist.sharded_greedy on top of the shard calls) keep returning YODA_ERR_STATE
 * while candidates are on (the sharded evaluation step: until yoda_shard_candidates is on).
 *   Cost: with candidates never set nothing on yoda_greedy's path changes.  With them on, every
 * window runs the narrowing pass after its Filter kernel, and a capacity window's exact fallback
 * reads one 8-byte word per node more (profiles/greedycand/timing.txt). */
int yoda_greedy_candidates(yoda_t* h, int enable);
/* ---- Node shards honour the candidate classes in the evaluation step (opt-in) ----
 * enable != 0: while candidates are on, the sharded Mode A evaluation step runs on this handle --
 * yoda_shard_phase1, _phase2, _prepare_merge, _finalize, _exact_records, _exact_merge, _draw_keys,
 * _draw_apply, yoda_comm_run and yoda_comm_run_local.  Each shard holds the words of ITS nodes
 * (yoda_set_candidates: upload order of the shard; yoda_update_candidates takes GLOBAL ids and
 * ignores those of other shards, so one list serves every shard) and the WHOLE batch's class
 * array.  After the step yoda_download gives, on every shard, exactly what one handle holding
 * the whole snapshot gives from yoda_run under the same words (each node's at its global id) and
 * classes, by the contract above: the maxima over F (the exchanged MAX, unchanged); n_feasible,
 * the single-feasible-node rule, UNSCHEDULABLE and DIV_ZERO (a zero-total node of F' with
 * |F'| >= 2, both counted over all shards) follow the global F'; so do NormalizeScore's bounds,
 * n_ties, top_score and the lowest-node pick, and with yoda_shard_tie_draw the seeded draw -- on
 * the three record paths (the U64 path's exact-normalize exchange included), in both exchange
 * orders, through the packed-key merge and the record merge.  Phase 1 narrows the shard's masks
 * and counts before they are exchanged; every later kernel of the step reads Filter state
 * through those masks alone.  The K2 pruning seeds are off, as in yoda_run.
 *   A step with candidates on whose class array is not as long as the batch returns
 * YODA_ERR_STATE and launches nothing, as yoda_run.
 *   Agreement.  The counts are summed over the shards, so shards that disagree on the candidate
 * state give wrong picks silently.  yoda_comm_run[_local] check it: the first all-reduce carries
 * a digest of (this setting, n_classes, the class array's length, a 64-bit hash of its bytes) and
 * its complement, as for the draw settings; on disagreement every shard fails with
 * YODA_ERR_STATE and the handles stay usable.  Two states are refused on the shard itself, BEFORE
 * it launches or exchanges anything, because that is their contract (the old refusal, and
 * "launches nothing"): candidates on with this setting off, and a class array whose length is
 * not the batch's.  In one process (yoda_comm_run_local) every shard is checked before any of
 * them runs, so all fail together.  Over RCCL (yoda_comm_run) the refusing rank returns while
 * the others enter the all-reduce and wait for it: give every rank the same setting, as for
 * yoda_shard_exchange_order, and check the class array's length against the batch on every rank
 * (yoda_candidates_info out[1]) before a collective step.  The digest then catches what a rank
 * cannot see alone: another n_classes, other class bytes, candidates off on one rank.  The
 * words differ per shard by design and are in no digest.  A caller that drives yoda_shard_*
 * itself OWNS the agreement: dist.ShardExchange checks the same digest, in the MAX reduce that
 * checks the draw settings.
 *   Off (the default): every yoda_shard_* and yoda_comm_* call returns YODA_ERR_STATE while
 * candidates are on, with the same messages and launches as before.  A setting: it stays across
 * uploads until changed.  YODA_ERR_INVALID_ARG on a NULL handle.
 *   Refused whatever the setting, while candidates are on: Mode B on shards, the greedy-window
 * shard calls (yoda_shard_topk[_deep], _best_one, _phase1_witness, _witness_prepare,
 * _witness_download), yoda_comm_greedy[_local] and dist.sharded_greedy.  They are the next step.
 *   Cost: with candidates never set, the first exchange is 16 bytes longer and nothing else
 * changes.  With them on, each shard runs the narrowing pass over its own nodes after its K1
 * (the single handle's figures above: 0.82 / 0.96 ms a step, 0.39 / 0.43 ms of it the pass).
 * Measured at 100k pods x 100k nodes, config 3, every shard in ONE process on one MI355X through
 * yoda_comm_run_local (profiles/shardcand/timing.txt), 8 classes that each lack 1 % / 30 % of
 * the nodes: the sharded step 1.31 / 1.63 ms at world 2 and 3.08 / 3.69 ms at world 8 (0.82 and
 * 2.21 ms with candidates never set), the pass 0.42 / 0.46 ms and 0.83 / 0.88 ms of it (24-32 %).
 * Candidates never set, against the parent commit in interleaved fresh processes: inside the
 * parent's process-to-process spread at world 8 (2.213 against 2.208 ms), 0.002 ms above its
 * slowest process at world 2 (0.822 against 0.811 ms).  World sizes above 1 on separate GPUs are
 * not measured. */
int yoda_shard_candidates(yoda_t* h, int enable);
/* ---- Mode B follows the absent nodes and the candidate classes (opt-in) ----
 * Mode B's Filter is a pass-through (scheduler.go:96-99), so the nodes a Mode B pod may land on
 * are decided by the node set and the other plugins' Filter alone.  With the setting on,
 * E(p) = {n : n present and cand(p, n)} -- cand always true while candidates are off or for a
 * YODA_CAND_ANY pod; an absent node is in no E whatever its word says -- and pod p's cycle is
 * exactly the reference's Mode B cycle on the sub-snapshot holding only the nodes of E(p), picks
 * reported as ids of the uploaded snapshot (n_nodes, the ids and node_offset do not change):
 * n_feasible = |E|; |E| = 0 is YODA_STATUS_UNSCHEDULABLE with no pick, n_ties 0 and top_score 0;
 * |E| = 1 is that node with n_ties 1 and its raw score; otherwise top_score is the best level
 * over E, n_ties the nodes of E at it, the pick the lowest of them, or with yoda_set_tie_draw the
 * one with the smallest yoda_tie_hash.  There is no DIV_ZERO in Mode B.  In the score rows a node
 * outside E has feasibility bit 0 and raw and normalized scores of -1, a node of E scores what it
 * scores without the setting, and NormalizeScore takes highest and lowest over E.
 *   Followed by yoda_eval, yoda_run, yoda_download, yoda_score_rows and yoda_score_rows_norm
 * (their bitmask_out included), the single-handle draw, and yoda_greedy in Mode B: while nodes
 * are absent, and with candidate classes once yoda_greedy_candidates is on as well (without it
 * yoda_greedy refuses candidate classes in either mode).  Unchanged with the
 * setting on: yoda_shard_* and yoda_comm_* in Mode B, the shard draw calls included, keep
 * returning YODA_ERR_STATE while a node is absent or candidates are on, and
 * yoda_run(YODA_MODE_DISKIO, YODA_RUN_BITMASK) + yoda_download_bitmask keeps its "run Mode A"
 * refusal.  A run with candidates on needs a class array as long as the batch, as in Mode A.
 *   Off (the default): Mode B refuses with YODA_ERR_STATE while a node is absent or candidates
 * are on, exactly as before.  A setting: it stays across uploads until changed.
 *   Cost: nothing while every E is the whole snapshot (no node absent, and candidates off or
 * every pod YODA_CAND_ANY): the unrestricted kernels run.  Otherwise sibling kernels read one
 * 16-byte eligibility record per node beside its 16-byte Mode B record, rebuilt (one small
 * kernel, with the 65 class counts) on the first Mode B run after yoda_upload_nodes,
 * yoda_set_node_present, yoda_set_candidates or yoda_update_candidates; the batch's pod classes
 * are then the distinct (alpha, beta, candidate class) triples.  Measured at 100k pods x 100k
 * nodes (profiles/modebfollow/timing.txt) against the unrestricted step for the same pods: one
 * pod spec 0.018 ms -> 0.021 ms with 1,024 absent nodes (x1.2) and 0.029 ms with 8 classes lacking
 * 1 % or 30 % of the nodes (x1.65: 9 effective classes instead of 1); a distinct request per pod
 * 2.29 ms -> 4.85 ms (x2.1) in each of those states -- the test and the masked step roughly double
 * the per-pair instructions of an FP64-issue-bound kernel.  Never enabled, or enabled with every
 * E whole, the step is inside the parent's run-to-run spread (profiles/modebfollow/ab.txt). */
int yoda_mode_b_follow(yoda_t* h, int enable);
/* Diagnostic, host only: out[4] = {enabled, effective classes D' of the last Mode B batch run,
 * 1 if that run took the eligibility kernels (0: the unchanged ones), eligibility-table builds
 * since the upload}.  out[1] and out[2] describe the last UNSAMPLED Mode B batch run: a run under
 * yoda_mode_b_sampling builds no pod classes and leaves them as they were
 * (yoda_mode_b_sampling_info reports that run). */
int yoda_mode_b_info(const yoda_t* h, uint32_t* out);
/* ---- Mode B honours node sampling (opt-in): the deployed scheduler's own cycle ----
 * The reference ships Mode B scoring together with percentageOfNodesToScore: 0
 * (deploy/yoda-scheduler.yaml:18), so the cycle the deployed binary runs is a Mode B score over
 * the first numFeasibleNodesToFind nodes of a rotating walk.  enable != 0: with sampling on
 * (yoda_set_node_sampling: M = num_to_find, start[p]) Mode B's single-handle batch path scores,
 * for pod p, S(p) = the first min(M, |E(p)|) nodes of E(p) in the rotated order of Mode A's
 * sampling (GLOBAL ids, wrap-around, absent nodes skipped, start[p] may be outside E).  E(p) is
 * yoda_mode_b_follow's set: the whole snapshot while no node is absent and candidates are off or
 * every pod is YODA_CAND_ANY; an absent node or candidate classes still need yoda_mode_b_follow,
 * and without it the refusals above stay as they are.
 *   The cycle is the reference's Mode B cycle on the sub-snapshot of S(p); picks are ids of the
 * uploaded snapshot.  n_feasible = |S|; |S| = 0 is YODA_STATUS_UNSCHEDULABLE; |S| = 1 is that node
 * with its raw score and n_ties 1; otherwise top_score is the best level over S, n_ties the nodes
 * of S at it, and the pick the LOWEST id among them (not the first in walk order: after a wrap it
 * lies in [node_offset, next_start)), or with yoda_set_tie_draw the tie-set member with the
 * smallest yoda_tie_hash.  There is no DIV_ZERO.  yoda_download_sampling answers after such a
 * run: n_found[p] = |E(p)|, next_start[p] the (M+1)-th node of E in rotated order when |E| > M,
 * else start[p].  In the score rows a node outside S has feasibility bit 0 and raw and normalized
 * scores of -1, a node of S scores what it scores unsampled, and NormalizeScore's highest and
 * lowest are taken over S.  A pod with M >= |E| has exactly the outputs it has without sampling.
 *   Honoured by yoda_run, yoda_eval, yoda_download, yoda_download_sampling, the single-handle
 * draw, yoda_score_rows and yoda_score_rows_norm (their bitmask_out included).  With sampling on
 * these keep refusing, setting or not: yoda_greedy in Mode B, every yoda_shard_* and yoda_comm_*
 * call, and yoda_run(YODA_MODE_DISKIO, YODA_RUN_BITMASK) + yoda_download_bitmask keeps its "run
 * Mode A" refusal.
 *   Off (the default): Mode B refuses with YODA_ERR_STATE while sampling is on, exactly as
 * before.  A setting: it stays across uploads until changed (sampling itself is turned off by
 * yoda_upload_nodes).  With the setting off or sampling off nothing launches differently.
 *   Cost: a plan kernel (one thread per pod) and one scoring kernel (one wave per pod over its
 * walk, the draw inside it), no chunk partials and no reduce.  With eligibility the plan reads
 * rank tables (65 selectors x ceil(N / 64) blocks: a bit word and a prefix count each, about 1.2
 * MB at 100k nodes), rebuilt with the eligibility table of yoda_mode_b_follow.  Measured at 100k
 * pods x 100k nodes, M = 5000, a random start per pod (profiles/modebsampling/timing.txt): with a
 * distinct request per pod 0.31 ms against 2.31 ms unsampled with every E whole, 0.35 ms against
 * 4.82 ms with 1,024 absent nodes or 8 classes, and with the draw 0.64-0.75 ms against 13.4-20.4
 * ms; with one pod spec 0.30-0.44 ms against 0.018-0.025 ms (unsampled that batch is one pod
 * class; sampled, every pod scores its own walk).  The plan is 0.007-0.010 ms of it. */
int yoda_mode_b_sampling(yoda_t* h, int enable);
/* Diagnostic, host only: out[4] = {enabled, 1 if the last Mode B run took the sampled kernels,
 * rank-table builds since the upload, 1 if that run used the eligibility instances}. */
int yoda_mode_b_sampling_info(const yoda_t* h, uint32_t* out);
/* ---- Filter diagnosis: why a node was rejected ----
 * kube-scheduler builds a Pending pod's FitError event ("0/N nodes are available: a ..., b ...")
 * and its PostFilter walk from the per-node Filter statuses.  The reference's Filter is three
 * predicates with three meanings (pkg/yoda/filter/filter.go:11-58), called in the order of
 * pkg/yoda/collection/collection.go:41-44; the batch path evaluates all three and, without
 * these calls, hands back n_feasible alone.  One reason per (pod, node):
 *   YODA_REASON_NONE           the node is in F'(p) (the candidate-class block above): it passes
 *   YODA_REASON_NUMBER         PodFitsNumber fails (filter.go:11-16): not enough cards
 *   YODA_REASON_MEMORY         number passes, PodFitsMemory fails (filter.go:18-33): too few
 *                              healthy cards with that much free memory
 *   YODA_REASON_CLOCK          number and memory pass, PodFitsClock fails (filter.go:35-50): too
 *                              few healthy cards at that clock
 *   YODA_REASON_NOT_CANDIDATE  another plugin's Filter rejected it: the pod's class bit is clear
 *                              in the node's word (yoda_set_candidates)
 *   YODA_REASON_ABSENT         the node is not in the node set (yoda_set_node_present)
 * Precedence: absent > not a candidate > number > memory > clock.  Not-a-candidate goes before
 * Yoda's own reasons because the in-tree Filter plugins run before an out-of-tree one in a
 * profile: such a node never reaches Yoda's Filter, and the caller gets Yoda's reasons over
 * exactly the candidate nodes (it knows its own per-class rejection counts).  A YODA_CAND_ANY
 * pod, or candidates off, never gives YODA_REASON_NOT_CANDIDATE.  YODA_REASON_NONE holds exactly
 * where the feasibility bit of yoda_download_bitmask / yoda_score_rows is set.
 *   Mode A only.  Mode B has no Filter of its own (scheduler.go:96-99): its rejected nodes are
 * n_nodes - absent - n_feasible, and the calls below refuse it.
 *
 * The batch path: counts per pod.  yoda_diagnose runs after a completed Mode A run whose results
 * are still pending -- exactly when yoda_download would answer: after yoda_run, yoda_eval,
 * yoda_score_rows[_norm], and on a shard handle after a step through yoda_shard_finalize or
 * yoda_comm_run[_local] with no exact-normalize pods pending.  Asynchronous on the handle's
 * stream; it does not disturb the run (yoda_download before and after it gives the same bytes),
 * and calling it twice gives the same counts.  It evaluates the state the run evaluated: the live
 * records (yoda_set_node_state, yoda_update_node_cards), the presence bits, the candidate words
 * and the class array.  yoda_set_node_state and yoda_update_alloc never invalidated a pending
 * run: a diagnosis after them reads the pushed CardNumber, while the selection and n_feasible
 * stay the run's.  It selects the pods whose final n_feasible is 0 -- on a shard the global
 * count after the exchange -- or with YODA_DIAG_ALL every pod; the selection is made on the
 * device, with no host round trip between run and diagnosis.
 *   yoda_download_diagnosis: counts[4 * p ..] = {not a candidate, number, memory, clock} nodes of
 * pod p, in the caller's pod order whatever yoda_set_pod_order says; a pod that was not selected
 * has all four words 0xFFFFFFFF.  Absent nodes are counted nowhere, so for a selected pod the
 * four counts + n_feasible = n_nodes - absent -- unless yoda_set_node_state or yoda_update_alloc
 * came between the run and the diagnosis (above): the counts then follow the pushed CardNumber
 * and n_feasible does not.  The counts are over the handle's own nodes: on a shard handle this
 * shard's, and the caller sums the shards' downloads.
 *   YODA_ERR_INVALID_ARG: a NULL handle or buffer, unknown flag bits, n_counts != 4 * n_pods.
 * YODA_ERR_STATE, with nothing launched: no pending run; the last run was Mode B or yoda_greedy*;
 * any call since the run that invalidates pending run state (whatever invalidates yoda_download:
 * an upload of nodes or pods, yoda_update_node_cards, yoda_set_node_present, the candidate calls,
 * yoda_reason_rows, the start of a sharded step); yoda_download_diagnosis without this run's
 * yoda_diagnose before it.
 *
 * The row path: a reason per node.  yoda_reason_rows serves the uploaded pods (a handful, as
 * yoda_score_rows: P * N <= 2^31), synchronously, into host memory: reasons[p * N + n] is the
 * code of (pod p, local node n), 0 exactly where bit (p, n) of yoda_score_rows' bitmask is set.
 * Mode A semantics; it honours the candidates, the class array (the length rule and
 * YODA_ERR_STATE of yoda_run) and the absent nodes, needs no previous run, and invalidates what
 * yoda_score_rows invalidates (a pending run, phase-1, top-k and draw state): call it before
 * yoda_score_rows when the picks of the latter are wanted.  YODA_ERR_NO_NODES / YODA_ERR_NO_PODS
 * before the uploads, YODA_ERR_INVALID_ARG for a NULL buffer or n_reasons != P * N.
 *
 * Cost: nothing on any other entry point (one sibling kernel family, k1_diagnose; the K1 / K2
 * kernels are unchanged).  The sweep reads every node record once per selected pod wave through
 * the scalar path, as the per-node K1 sweep does, without the maxima fold; its (pod wave, node
 * chunk) tasks are sized on the device from the selection, so a few unschedulable pods still
 * fill the GPU.  Measured at 100k pods x 100k nodes, config 3 (profiles/diagnosis/timing.txt,
 * medians over fresh processes, HIP events): yoda_diagnose 0.048 ms with one unschedulable pod,
 * 3.63 ms with the workload's own 21,440 (the step: 0.385 ms), 16.34 ms with YODA_DIAG_ALL --
 * against 19.44 ms for the per-node K1 sweep (YODA_UPLOAD_PER_NODE_K1) over the same 10^10 pairs,
 * which folds the maxima
 * as well; yoda_reason_rows 0.060 ms for 1 pod and 0.228 ms for 24 (host wall clock) beside 0.244
 * and 1.063 ms for yoda_score_rows.  Never called: the step 0.3903 against the parent's 0.3896 ms
 * in interleaved fresh processes, inside the parent's spread (0.3876-0.3912 ms).  Not measured:
 * shard handles, the F64 / U64 record paths, K other than 8. */
#define YODA_REASON_NONE 0
#define YODA_REASON_NUMBER 1
#define YODA_REASON_MEMORY 2
#define YODA_REASON_CLOCK 3
#define YODA_REASON_NOT_CANDIDATE 4
#define YODA_REASON_ABSENT 5
#define YODA_DIAG_ALL 1u /* every pod, not only those with n_feasible == 0 */
int yoda_diagnose(yoda_t* h, uint32_t flags);
int yoda_download_diagnosis(yoda_t* h, uint32_t* counts /* [P][4] */, uint64_t n_counts);
int yoda_reason_rows(yoda_t* h, uint8_t* reasons /* [P][N] */, uint64_t n_reasons);
/* Diagnostic (synchronizes).  digest[8]: a 64-bit hash per table over its words as the device
 * holds them -- records, K1 summaries, K2 summaries, per-card model rows, K1 mixed tiles, block
 * summaries, G table, G maxima + reciprocals (0 where the record path has none).  mismatch[4]:
 * words of the block-grouped copies that differ from the base rows permuted by the node order;
 * words of the stored upload-order block summaries that differ from a fresh build (k_bsum_build,
 * the builder of the upload and of the card updates, run now into a zeroed scratch buffer): a
 * stale or loose row after yoda_set_node_state or a card update, or a padding word an older
 * snapshot left; the same for the block-grouped order; words of the host mirrors that differ
 * from the device.  CardNumber bounds are tightened first if node-state pushes left them
 * loose. */
int yoda_snapshot_check(yoda_t* h, uint64_t* digest, uint32_t* mismatch);
/* After yoda_shard_phase1 (or _phase1_witness) and the caller's reduction of its buffers
 * (d_maxima, d_counts as there).  k = the list depth of that phase 1, yoda_shard_topk_depth(h)
 * (yoda_topk_k() after yoda_shard_phase1, yoda_topk_k_capacity() after the witness phase 1);
 * any other k is rejected with YODA_ERR_INVALID_ARG, so the caller's buffers always match.
 * Host outputs: counts [2][P] (n_feasible, n_zero_total), top_score [k][P] (f64, exact
 * integers), top_node [k][P]. */
int yoda_shard_topk_depth(const yoda_t* h);
int yoda_shard_topk(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_counts, uint32_t k,
                    uint32_t* counts, double* top_score, uint32_t* top_node);
/* Capacity windows across shards (the window sequence of yoda_comm_greedy and yoda_greedy):
 * yoda_shard_topk after yoda_shard_phase1_witness, but the lists are `deep` long
 * (yoda_greedy_cap_depth()) -- the chunks' k-deep lists merged deeper, exact down to their last
 * entry (at least the first min(k, n_feasible), as yoda_shard_topk lists them) and
 * 0xFFFFFFFF-ended past it; top_score / top_node are [deep][P]. */
int yoda_greedy_cap_depth(void);
int yoda_shard_topk_deep(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_counts,
                         uint32_t k, uint32_t deep, uint32_t* counts, double* top_score,
                         uint32_t* top_node);
/* The shards' list merge of the sharded greedy (host only, no handle): scores / nodes are the
 * world's gathered lists, [world][kl][wn] in shard order (yoda_shard_topk[_deep]'s layout);
 * out_score / out_node [kl][wn] get, for window pods [from, wn), the first kl of the union in
 * (score desc, node asc) order, -1.0 / 0xFFFFFFFF past its end.  Deep lists (kl >
 * yoda_topk_k_capacity()) are cut where a node some shard left unlisted could enter (after the
 * first yoda_topk_k(), at the latest of the shards' last entries).  yoda_comm_greedy merges
 * with this same function. */
int yoda_merge_shard_lists(uint32_t world, uint32_t wn, uint32_t kl, uint32_t from,
                           const double* scores, const uint32_t* nodes, double* out_score,
                           uint32_t* out_node);
/* Exact best node of pod `pod` (index in the batch of the last yoda_shard_topk) over this
 * shard against the CURRENT node state: *node = global id or -1 (no feasible node here),
 * *score = its raw score (lowest node among equal scores). */
int yoda_shard_best_one(yoda_t* h, uint32_t pod, double* score, int32_t* node);

/* YODA_GREEDY_CARD_CAPACITY across shards (fast record paths).  Per window, instead of
 * yoda_shard_phase1: yoda_shard_phase1_witness also writes d_wit [2][6][P] u32 -- per PreScore
 * maxima field the shard's witness count (nodes whose qualifying cards reach the shard's
 * maximum) and its lowest witness (GLOBAL id).  Exchange: keep a copy of the local d_maxima,
 * all-reduce d_maxima MAX and d_counts SUM, yoda_shard_witness_prepare(global, local, d_wit)
 * (clears the fields where this shard does not reach the global maximum), then SUM-reduce
 * d_wit[0, 6P) and MIN-reduce (unsigned) d_wit[6P, 12P).  yoda_shard_topk with
 * k = yoda_topk_k_capacity() (the deeper lists of the capacity windows); then
 * yoda_shard_witness_download gives maxima [6][P] and wit [12][P] in the caller's pod order
 * for yoda_gs_set_witness.  A pod the session cannot certify starts the next window.
 * For a field whose maximum is the floor 1 the witness words are unspecified (the session
 * never reads them: no node's value decides such a maximum). */
int yoda_shard_phase1_witness(yoda_t* h, uint64_t* d_maxima, uint32_t* d_counts,
                              uint32_t* d_wit);
int yoda_shard_witness_prepare(yoda_t* h, const uint64_t* d_maxima_global,
                               const uint64_t* d_maxima_local, uint32_t* d_wit);
int yoda_shard_witness_download(yoda_t* h, const uint64_t* d_maxima, const uint32_t* d_wit,
                                uint64_t* maxima, uint32_t* wit);

/* Host-side sequential resolve over the GLOBAL node set (no GPU); identical on every rank. */
typedef struct yoda_greedy_session yoda_gs_t;
/* nodes: the full snapshot (card_number, free/total memory sums, alloc_memory (may be NULL)
 * are read); pods: the whole batch (number/memory/priority are read). */
int yoda_gs_create(const yoda_node_soa* nodes, const yoda_pod_soa* pods, uint32_t flags,
                   yoda_gs_t** out);
int yoda_gs_destroy(yoda_gs_t* g);
/* order[q] = input index of the pod at queue position q (sort.go:8-10). */
int yoda_gs_queue_order(const yoda_gs_t* g, uint32_t* order);
/* Window = queue positions [ws, ws + wn); arrays in window order as yoda_shard_topk's.  A
 * pod's list may end (0xFFFFFFFF entries) before min(counts[i], k) entries: it then holds its
 * best nodes only down to its last entry (every unlisted node scored at most that, in score
 * desc / node asc order), which becomes the pod's threshold, and is never taken for the whole
 * feasible set (libyoda's own capacity windows pass such lists, merged deeper than exact). */
int yoda_gs_begin_window(yoda_gs_t* g, uint32_t ws, uint32_t wn, uint32_t k,
                         const uint32_t* counts, const double* top_score,
                         const uint32_t* top_node);
/* YODA_GREEDY_CARD_CAPACITY sessions: the window's PreScore maxima [6][wn] with their
 * witnesses -- per field the number of window-start feasible nodes whose qualifying cards
 * reach the maximum, and the lowest such node (GLOBAL id, 0xFFFFFFFF if none) -- window
 * order as yoda_gs_begin_window's arrays; call after it.  Without them a capacity session
 * certifies a pod only while no node it could use has lost cards in the window. */
int yoda_gs_set_witness(yoda_gs_t* g, const uint64_t* maxima, const uint32_t* wit_count,
                        const uint32_t* wit_node);
/* Capacity sessions: the candidate words [N] (index = GLOBAL node id, as yoda_set_candidates) and
 * the pods' classes [P] in input order (NULL: every pod YODA_CAND_ANY).  Copied.  Before the first
 * window; YODA_ERR_STATE after one began; YODA_ERR_RANGE for a class >= n_classes that is not
 * YODA_CAND_ANY; n_classes 0 clears them.  flags == 0 sessions accept and ignore them.
 *   The windows of such a session carry counts and lists over F' = F and cand (what the narrowed
 * masks give) and maxima with witnesses over F (Yoda's Filter alone); the certificate counts a
 * lost node against the feasible set only if it is the pod's candidate, and against the
 * witnesses either way. */
int yoda_gs_set_candidates(yoda_gs_t* g, uint32_t n_classes, const uint64_t* words,
                           const uint8_t* cls);
/* Resolve the window in queue order; *next = the first window pod it cannot certify (wn when
 * the window is done).  flags == 0: the caller scores that pod exactly against the current
 * state (yoda_shard_best_one) and feeds it to yoda_gs_assign.  YODA_GREEDY_CARD_CAPACITY:
 * the caller starts the next window at that pod instead (the certificate of DESIGN.md §5
 * also tracks CardNumber decrements: feasibility and, through the witnesses, the maxima). */
int yoda_gs_resolve(yoda_gs_t* g, uint32_t* next);
int yoda_gs_assign(yoda_gs_t* g, uint32_t queue_pos, int32_t pick);
/* flags == 0: *count = window pods [from, from + scan) with >= 2 feasible nodes whose lists no
 * longer certify them (they stay so: scores only drop) -- the refresh trigger; 0 once some
 * node's Allocate has wrapped (no list certifies then, so a refresh cannot help).
 * YODA_ERR_STATE for capacity sessions. */
int yoda_gs_uncertified(const yoda_gs_t* g, uint32_t from, uint32_t scan, uint32_t* count);
/* New candidate lists for window pods [from, wn) ([k][wn] in window order, as
 * yoda_gs_begin_window's, scored against the CURRENT node state with the window's phase-1
 * masks and maxima): each list's threshold becomes its refresh-time k-th score.  Every listed
 * node is validated first (YODA_ERR_RANGE leaves the session unchanged); capacity sessions
 * restart windows instead and get YODA_ERR_STATE. */
int yoda_gs_refresh(yoda_gs_t* g, uint32_t from, const double* top_score,
                    const uint32_t* top_node);
/* YODA_GREEDY_CARD_CAPACITY: the size of the window that a restart at window index `progress`
 * opens (130 % of the progress in whole waves, at least 64, at most wmax) -- the one rule of
 * yoda_greedy, yoda_comm_greedy and the Python driver. */
uint32_t yoda_greedy_next_window(uint32_t progress, uint32_t wmax);
/* Nodes whose state changed since the last call (at most cap), with their current state. */
int yoda_gs_take_dirty(yoda_gs_t* g, uint32_t cap, uint32_t* nodes, uint64_t* alloc,
                       uint64_t* card_number, uint32_t* count);
/* Every node the session ever changed, with its ORIGINAL state (to restore the shards). */
int yoda_gs_touched_original(const yoda_gs_t* g, uint32_t cap, uint32_t* nodes, uint64_t* alloc,
                             uint64_t* card_number, uint32_t* count);
/* pick [P] in input order; pods certified from candidate lists; pods assigned by the caller. */
int yoda_gs_picks(const yoda_gs_t* g, int32_t* pick, uint32_t* resolved, uint32_t* assigned);

#ifdef __cplusplus
}
#endif

#endif /* YODA_H_ */
