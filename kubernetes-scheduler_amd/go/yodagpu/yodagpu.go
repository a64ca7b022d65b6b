// Package yodagpu binds libyoda (include/yoda.h) through cgo for the Yoda kube-scheduler
// plugin (github.com/Mr-LvGJ/Yoda-Scheduler/pkg/yoda).  It is the Go half of the drop-in
// boundary documented in INTEGRATION.md.
//
// cgo pointer rules: libyoda's SoA structs (yoda_node_soa, yoda_pod_soa, yoda_eval_out) hold
// pointers, so every array they point at lives in C memory (cArrays below), never in the Go
// heap; a Go pointer is passed to C only directly as an argument, to memory that holds no
// pointers (output slices of plain numbers).  Runs clean under GODEBUG=cgocheck=1
// (yodagpu_test.go).
//
// NOT COMPILED IN THIS REPOSITORY'S CI: the build image has no Go toolchain.  The C-ABI it
// calls is exercised from C (tools/capi_example.c) and Python ctypes (yoda_amd/capi.py).
package yodagpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../yoda_amd -lyoda -Wl,-rpath,${SRCDIR}/../../yoda_amd
#include <stdlib.h>
#include "yoda.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"strconv"
	"unsafe"

	scv "github.com/NJUPT-ISL/SCV/api/v1"
	v1 "k8s.io/api/core/v1"

	"github.com/Mr-LvGJ/Yoda-Scheduler/pkg/yoda/filter"
	"github.com/Mr-LvGJ/Yoda-Scheduler/pkg/yoda/score"
)

// Mode selects the score: the SCV GPU path (Mode A) or the shipped diskIO balance (Mode B).
type Mode int

const (
	ModeSCV    Mode = C.YODA_MODE_SCV
	ModeDiskIO Mode = C.YODA_MODE_DISKIO
)

// Status codes of a pod's outcome (include/yoda.h YODA_STATUS_*).
const (
	StatusOK            = C.YODA_STATUS_OK
	StatusUnschedulable = C.YODA_STATUS_UNSCHEDULABLE
	StatusDivZero       = C.YODA_STATUS_DIV_ZERO
	StatusScoreRange    = C.YODA_STATUS_SCORE_RANGE
)

// cArray is a grow-only block of C memory.
type cArray struct {
	p unsafe.Pointer
	n uintptr
}

func (a *cArray) ensure(bytes uintptr) unsafe.Pointer {
	if bytes == 0 {
		bytes = 8
	}
	if bytes > a.n {
		C.free(a.p)
		a.p = C.calloc(1, C.size_t(bytes))
		if a.p == nil {
			panic("yodagpu: out of C memory")
		}
		a.n = bytes
	}
	return a.p
}

func (a *cArray) free() {
	C.free(a.p)
	a.p, a.n = nil, 0
}

// Go views of C memory (Go 1.15-compatible: no unsafe.Slice).
func u64s(a *cArray, n int) []uint64 {
	return (*[1 << 30]uint64)(a.ensure(uintptr(n) * 8))[:n:n]
}
func u32s(a *cArray, n int) []uint32 {
	return (*[1 << 30]uint32)(a.ensure(uintptr(n) * 4))[:n:n]
}
func i64s(a *cArray, n int) []int64 {
	return (*[1 << 30]int64)(a.ensure(uintptr(n) * 8))[:n:n]
}
func i32s(a *cArray, n int) []int32 {
	return (*[1 << 30]int32)(a.ensure(uintptr(n) * 4))[:n:n]
}
func u8s(a *cArray, n int) []uint8 {
	return (*[1 << 31]uint8)(a.ensure(uintptr(n)))[:n:n]
}
func f64s(a *cArray, n int) []float64 {
	return (*[1 << 30]float64)(a.ensure(uintptr(n) * 8))[:n:n]
}

// nodeArrays / podArrays: the SoA inputs, in C memory, reused across calls.
type nodeArrays struct {
	cardNumber, freeSum, totalSum, alloc, free, total, clock, bw, core, power cArray
	cardCount, healthy, cpu, disk                                            cArray
}

type podArrays struct {
	hasNumber, hasMemory, hasClock, number, memory, clock, priority, rio, rcpu cArray
	pick, status                                                               cArray
}

// Handle owns one libyoda handle (one GPU, one node snapshot).  Not safe for concurrent
// use: the framework calls PreFilter once per pod cycle, cycles are serial.
type Handle struct {
	h         *C.yoda_t
	nodes     []string
	index     map[string]int
	zeroTotal []bool // Status.TotalMemorySum == 0 (the reference divides by it when scoring)
	na        nodeArrays
	pa        podArrays
}

// Error is a libyoda error code (include/yoda.h YODA_ERR_*) with the call that returned it.
type Error struct {
	Code int
	msg  string
}

func (e *Error) Error() string { return e.msg }

// IsRange reports whether err is YODA_ERR_RANGE: the uploaded snapshot's record format cannot
// hold a new value, the handle is unchanged, and the caller uploads the snapshot again.
func IsRange(err error) bool {
	var e *Error
	return errors.As(err, &e) && e.Code == int(C.YODA_ERR_RANGE)
}

func check(h *C.yoda_t, rc C.int, what string) error {
	if rc == C.YODA_OK {
		return nil
	}
	msg := ""
	if h != nil {
		msg = C.GoString(C.yoda_last_error(h))
	}
	return &Error{Code: int(rc), msg: fmt.Sprintf("%s: libyoda error %d: %s", what, int(rc), msg)}
}

// New opens a handle on GPU `device`.
func New(device int) (*Handle, error) {
	var h *C.yoda_t
	if err := check(nil, C.yoda_create(C.int(device), &h), "yoda_create"); err != nil {
		return nil, err
	}
	g := &Handle{h: h}
	runtime.SetFinalizer(g, (*Handle).Close)
	return g, nil
}

// Close releases the device memory and the C-side arrays.
func (g *Handle) Close() {
	if g.h != nil {
		C.yoda_destroy(g.h)
		g.h = nil
	}
	g.na.release()
	for _, a := range []*cArray{&g.pa.hasNumber, &g.pa.hasMemory, &g.pa.hasClock, &g.pa.number,
		&g.pa.memory, &g.pa.clock, &g.pa.priority, &g.pa.rio, &g.pa.rcpu, &g.pa.pick,
		&g.pa.status} {
		a.free()
	}
}

// UploadNodes packs the SCV records (one per node, in the order of `names`) into the
// struct-of-arrays of yoda_node_soa and uploads them.  allocMemory[i] is the sum of the
// scv/memory labels of pods already on node i (score.CalculateAllocateScore's loop,
// algorithm.go:299-303); cpu/diskIO are advisor.NodeInfo values (Mode B, may be nil).
// scvs == nil: nodes without SCV records (Mode B, which reads none of them).
func (g *Handle) UploadNodes(names []string, scvs []*scv.Scv, allocMemory []uint64,
	cpu, diskIO []float64) error {
	return g.UploadShard(names, scvs, allocMemory, cpu, diskIO, 0)
}

// UploadShard is UploadNodes for one node shard of a multi-GPU snapshot: offset is the global
// index of names[0] (picks and node ids are global; see CommInit).  Shards exchange maxima, so
// they must agree on the record path and the N32 quotient type: exchange SmallFieldMax and
// RecordPath out of band and, when another shard's SmallFieldMax exceeds 55738, upload again
// with UploadShardFlags(..., UploadF64Quotients), then with UploadForceF64 where any shard
// reports PathF64 (include/yoda.h yoda_small_field_max; yoda_amd/dist.py agree_on_path).
func (g *Handle) UploadShard(names []string, scvs []*scv.Scv, allocMemory []uint64,
	cpu, diskIO []float64, offset uint32) error {
	return g.UploadShardFlags(names, scvs, allocMemory, cpu, diskIO, offset, 0)
}

// Upload flags (include/yoda.h YODA_UPLOAD_*) and record paths (YODA_PATH_*).
const (
	UploadForceF64     = uint32(C.YODA_UPLOAD_FORCE_F64)
	UploadF64Quotients = uint32(C.YODA_UPLOAD_F64_QUOTIENTS)
	PathN32            = int(C.YODA_PATH_N32)
	PathF64            = int(C.YODA_PATH_F64)
	PathU64            = int(C.YODA_PATH_U64)
)

// SmallFieldMax is the largest card bandwidth / clock / core / power of the uploaded snapshot.
func (g *Handle) SmallFieldMax() uint64 { return uint64(C.yoda_small_field_max(g.h)) }

// RecordPath is the uploaded snapshot's record format (PathN32, PathF64 or PathU64).
func (g *Handle) RecordPath() int { return int(C.yoda_record_path(g.h)) }

// UploadShardFlags is UploadShard with YODA_UPLOAD_* flags.
func (g *Handle) UploadShardFlags(names []string, scvs []*scv.Scv, allocMemory []uint64,
	cpu, diskIO []float64, offset uint32, flags uint32) error {
	n := len(names)
	if (scvs != nil && len(scvs) != n) || (allocMemory != nil && len(allocMemory) != n) {
		return errors.New("yodagpu: names/allocMemory do not match the SCV list")
	}
	if scvs == nil {
		scvs = make([]*scv.Scv, n)
		for i := range scvs {
			scvs[i] = &scv.Scv{}
		}
	}
	soa, zero, err := g.na.pack(scvs, allocMemory, cpu, diskIO)
	if err != nil {
		return err
	}
	// &soa is a Go pointer to memory holding only C pointers: allowed
	if err := check(g.h, C.yoda_upload_nodes(g.h, &soa, C.uint32_t(offset), C.uint32_t(flags)),
		"yoda_upload_nodes"); err != nil {
		return err
	}
	g.nodes = names
	g.zeroTotal = zero
	g.index = make(map[string]int, len(names))
	for i, name := range names {
		g.index[name] = i
	}
	return nil
}

// pack fills the C-side arrays of yoda_node_soa from the SCV records; zero[i]: node i has
// TotalMemorySum == 0.
func (a *nodeArrays) pack(scvs []*scv.Scv, allocMemory []uint64, cpu, diskIO []float64) (
	C.yoda_node_soa, []bool, error) {
	n := len(scvs)
	if (cpu == nil) != (diskIO == nil) || (cpu != nil && (len(cpu) != n || len(diskIO) != n)) {
		return C.yoda_node_soa{}, nil,
			errors.New("yodagpu: cpu/diskIO must both be nil or both have one value per node")
	}
	k := 1
	for _, s := range scvs {
		if len(s.Status.CardList) > k {
			k = len(s.Status.CardList)
		}
	}
	if k > C.YODA_MAX_CARDS {
		return C.yoda_node_soa{}, nil, errors.New("yodagpu: more than YODA_MAX_CARDS cards on a node")
	}
	cardNumber, cardCount := u64s(&a.cardNumber, n), u32s(&a.cardCount, n)
	freeSum, totalSum, alloc := u64s(&a.freeSum, n), u64s(&a.totalSum, n), u64s(&a.alloc, n)
	free, total, clock := u64s(&a.free, n*k), u64s(&a.total, n*k), u64s(&a.clock, n*k)
	bw, core, power := u64s(&a.bw, n*k), u64s(&a.core, n*k), u64s(&a.power, n*k)
	healthy := u8s(&a.healthy, n*k)
	zero := make([]bool, n)
	for i, s := range scvs {
		cardNumber[i] = uint64(s.Status.CardNumber)
		cardCount[i] = uint32(len(s.Status.CardList))
		freeSum[i] = s.Status.FreeMemorySum
		totalSum[i] = s.Status.TotalMemorySum
		zero[i] = s.Status.TotalMemorySum == 0
		alloc[i] = 0
		if allocMemory != nil {
			alloc[i] = allocMemory[i]
		}
		for j := 0; j < k; j++ {
			o := i*k + j
			free[o], total[o], clock[o], bw[o], core[o], power[o], healthy[o] = 0, 0, 0, 0, 0, 0, 0
		}
		for j, c := range s.Status.CardList {
			o := i*k + j
			free[o], total[o] = c.FreeMemory, c.TotalMemory
			clock[o], bw[o] = uint64(c.Clock), uint64(c.Bandwidth)
			core[o], power[o] = uint64(c.Core), uint64(c.Power)
			if c.Health == "Healthy" { // filter.go:53,57
				healthy[o] = 1
			}
		}
	}
	soa := C.yoda_node_soa{
		n_nodes: C.uint32_t(n), max_cards: C.uint32_t(k),
		card_number:      (*C.uint64_t)(a.cardNumber.p),
		card_count:       (*C.uint32_t)(a.cardCount.p),
		free_memory_sum:  (*C.uint64_t)(a.freeSum.p),
		total_memory_sum: (*C.uint64_t)(a.totalSum.p),
		alloc_memory:     (*C.uint64_t)(a.alloc.p),
		card_free_memory: (*C.uint64_t)(a.free.p), card_total_memory: (*C.uint64_t)(a.total.p),
		card_clock: (*C.uint64_t)(a.clock.p), card_bandwidth: (*C.uint64_t)(a.bw.p),
		card_core: (*C.uint64_t)(a.core.p), card_power: (*C.uint64_t)(a.power.p),
		card_healthy: (*C.uint8_t)(a.healthy.p),
	}
	if cpu != nil {
		copy(f64s(&a.cpu, n), cpu)
		copy(f64s(&a.disk, n), diskIO)
		soa.cpu = (*C.double)(a.cpu.p)
		soa.disk_io = (*C.double)(a.disk.p)
	}
	return soa, zero, nil
}

func (a *nodeArrays) release() {
	for _, x := range []*cArray{&a.cardNumber, &a.freeSum, &a.totalSum, &a.alloc, &a.free,
		&a.total, &a.clock, &a.bw, &a.core, &a.power, &a.cardCount, &a.healthy, &a.cpu, &a.disk} {
		x.free()
	}
}

// SetNodeState updates the allocated scv/memory (and CardNumber) of a few nodes on the
// device without re-uploading the snapshot (yoda_set_node_state): the scheduler's assumes
// and binds between two cycles.  idx are snapshot positions.
func (g *Handle) SetNodeState(idx []uint32, alloc, cardNumber []uint64) error {
	if len(idx) != len(alloc) || len(idx) != len(cardNumber) {
		return errors.New("yodagpu: SetNodeState arrays differ in length")
	}
	if len(idx) == 0 {
		return nil
	}
	// plain-number Go slices passed directly as arguments: allowed by the cgo rules
	rc := C.yoda_set_node_state(g.h, C.uint32_t(len(idx)), (*C.uint32_t)(unsafe.Pointer(&idx[0])),
		(*C.uint64_t)(unsafe.Pointer(&alloc[0])), (*C.uint64_t)(unsafe.Pointer(&cardNumber[0])))
	return check(g.h, rc, "yoda_set_node_state")
}

// UpdateCards replaces the dynamic SCV metrics of a few nodes on the device -- every card's
// FreeMemory and Health, and FreeMemorySum -- without re-uploading the snapshot
// (yoda_update_node_cards).  idx are snapshot positions; free and healthy hold maxCards slots
// per listed node.  An error that wraps YODA_ERR_RANGE leaves the handle as it was: upload the
// snapshot again.
func (g *Handle) UpdateCards(idx []uint32, maxCards int, free []uint64, healthy []uint8, freeSum []uint64) error {
	if len(idx) != len(freeSum) || len(free) != len(idx)*maxCards || len(healthy) != len(free) {
		return errors.New("yodagpu: UpdateCards arrays differ in length")
	}
	if len(idx) == 0 {
		return nil
	}
	// plain-number Go slices passed directly as arguments: allowed by the cgo rules
	rc := C.yoda_update_node_cards(g.h, C.uint32_t(len(idx)), (*C.uint32_t)(unsafe.Pointer(&idx[0])),
		C.uint32_t(maxCards), (*C.uint64_t)(unsafe.Pointer(&free[0])),
		(*C.uint8_t)(unsafe.Pointer(&healthy[0])), (*C.uint64_t)(unsafe.Pointer(&freeSum[0])))
	return check(g.h, rc, "yoda_update_node_cards")
}

// ReplaceNodes replaces the WHOLE record of a few nodes on the device -- card count, CardNumber,
// every card field, the memory sums, the allocation and, when the snapshot holds them, Mode B's
// cpu / diskIO -- without re-uploading the snapshot (yoda_replace_nodes): a machine whose GPUs
// were swapped, a changed card count or TotalMemory.  idx are snapshot positions; scvs[t] is the
// new record of node idx[t]; allocMemory may be nil (0); cpu / diskIO as for UploadNodes.  A node
// keeps its presence (SetNodePresent) and its candidate word.  New nodes take spare slots:
// upload placeholder records with an empty CardList, take them out with SetNodePresent, and when
// a node joins replace one and put it back (the node count itself never changes).  IsRange(err):
// the record does not fit the format the upload chose; the handle is unchanged -- upload the
// snapshot again.
func (g *Handle) ReplaceNodes(idx []uint32, scvs []*scv.Scv, allocMemory []uint64,
	cpu, diskIO []float64) error {
	if len(idx) != len(scvs) || (allocMemory != nil && len(allocMemory) != len(idx)) {
		return errors.New("yodagpu: ReplaceNodes arrays differ in length")
	}
	if len(idx) == 0 {
		return nil
	}
	for _, i := range idx {
		if int(i) >= len(g.nodes) {
			return errors.New("yodagpu: ReplaceNodes position outside the snapshot")
		}
	}
	soa, zero, err := g.na.pack(scvs, allocMemory, cpu, diskIO)
	if err != nil {
		return err
	}
	rc := C.yoda_replace_nodes(g.h, C.uint32_t(len(idx)), (*C.uint32_t)(unsafe.Pointer(&idx[0])),
		&soa)
	if err := check(g.h, rc, "yoda_replace_nodes"); err != nil {
		return err
	}
	for t, i := range idx { // (a repeated position keeps its last entry, as on the device)
		g.zeroTotal[i] = zero[t]
	}
	return nil
}

// UpdateNodeMetrics replaces Mode B's node inputs, NodeInfo.Cpu and NodeInfo.DiskIO (live
// metrics the reference re-reads in every PreScore, scheduler.go:101-114), without re-uploading
// the snapshot (yoda_update_node_metrics).  idx are snapshot positions with one cpu / diskIO
// value each; idx == nil is the dense form: one value per node of the snapshot, in its order.
// Absent nodes, candidate words and pod classes stay, and ModeBFollow's eligibility table is not
// rebuilt.
func (g *Handle) UpdateNodeMetrics(idx []uint32, cpu, diskIO []float64) error {
	if len(cpu) != len(diskIO) || (idx != nil && len(idx) != len(cpu)) ||
		(idx == nil && len(cpu) != len(g.nodes)) {
		return errors.New("yodagpu: UpdateNodeMetrics arrays differ in length")
	}
	if len(cpu) == 0 {
		return nil
	}
	var ip *C.uint32_t
	if idx != nil {
		ip = (*C.uint32_t)(unsafe.Pointer(&idx[0]))
	}
	// plain-number Go slices passed directly as arguments: allowed by the cgo rules
	rc := C.yoda_update_node_metrics(g.h, C.uint32_t(len(cpu)), ip,
		(*C.double)(unsafe.Pointer(&cpu[0])), (*C.double)(unsafe.Pointer(&diskIO[0])))
	return check(g.h, rc, "yoda_update_node_metrics")
}

// SetNodePresent takes a few nodes out of the uploaded snapshot (present[i] == 0) or back in
// without re-uploading it (yoda_set_node_present): a node that left the node set -- drained,
// NotReady, its SCV deleted -- or returned.  idx are snapshot positions; the other nodes keep
// theirs.  While a node is absent Mode A answers as a snapshot without it would; Mode B returns
// an error that wraps YODA_ERR_STATE until every node is back.  Not a per-cycle mask for other
// plugins' Filter results: a cordoned node's SCV still feeds CollectMaxValues, an absent one's
// does not.
func (g *Handle) SetNodePresent(idx []uint32, present []uint8) error {
	if len(idx) != len(present) {
		return errors.New("yodagpu: SetNodePresent arrays differ in length")
	}
	if len(idx) == 0 {
		return nil
	}
	// plain-number Go slices passed directly as arguments: allowed by the cgo rules
	rc := C.yoda_set_node_present(g.h, C.uint32_t(len(idx)), (*C.uint32_t)(unsafe.Pointer(&idx[0])),
		(*C.uint8_t)(unsafe.Pointer(&present[0])))
	return check(g.h, rc, "yoda_set_node_present")
}

// CandAny is the class byte of an unrestricted pod (YODA_CAND_ANY): every node is a candidate.
const CandAny uint8 = 0xFF

// SetCandidates hands the batch path the other plugins' Filter results as candidate classes
// (yoda_set_candidates): words[i] is node i's 64-bit word, bit c set when the node is a
// candidate for class c; nClasses 1..64.  nClasses 0 turns candidates off (words may be nil), as
// UploadNodes does.  The PreScore maxima do not move -- CollectMaxValues never sees another
// plugin's Filter -- while Filter, the counts, NormalizeScore and the picks follow the
// candidates.  While on, Mode B, greedy, shard and communicator calls return an error that
// wraps YODA_ERR_STATE.
func (g *Handle) SetCandidates(nClasses uint32, words []uint64) error {
	var p *C.uint64_t
	if len(words) > 0 {
		p = (*C.uint64_t)(unsafe.Pointer(&words[0]))
	}
	return check(g.h, C.yoda_set_candidates(g.h, C.uint32_t(nClasses), p), "yoda_set_candidates")
}

// UpdateCandidates replaces the candidate words of a few nodes (yoda_update_candidates); idx
// are GLOBAL node ids (the snapshot position plus the handle's node offset; ids outside the
// handle's shard are ignored), a repeated one keeps its last word.  Cordoning a node is word 0.
func (g *Handle) UpdateCandidates(idx []uint32, words []uint64) error {
	if len(idx) != len(words) {
		return errors.New("yodagpu: UpdateCandidates arrays differ in length")
	}
	if len(idx) == 0 {
		return nil
	}
	rc := C.yoda_update_candidates(g.h, C.uint32_t(len(idx)), (*C.uint32_t)(unsafe.Pointer(&idx[0])),
		(*C.uint64_t)(unsafe.Pointer(&words[0])))
	return check(g.h, rc, "yoda_update_candidates")
}

// SetPodClasses sets the class byte of every pod of the batches run from now on
// (yoda_set_pod_classes): below nClasses, or CandAny.  nil makes every pod CandAny again.
func (g *Handle) SetPodClasses(cls []uint8) error {
	var p *C.uint8_t
	if len(cls) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&cls[0]))
	}
	return check(g.h, C.yoda_set_pod_classes(g.h, C.uint32_t(len(cls)), p), "yoda_set_pod_classes")
}

// CandidatesInfo reports {nClasses (0: off), length of the class array, nodes that are not a
// candidate of every class} (yoda_candidates_info; host only).
func (g *Handle) CandidatesInfo() ([3]uint32, error) {
	var out [3]uint32
	rc := C.yoda_candidates_info(g.h, (*C.uint32_t)(unsafe.Pointer(&out[0])))
	return out, check(g.h, rc, "yoda_candidates_info")
}

// NumFeasibleToFind is numFeasibleNodesToFind of k8s v1.22.3 for percentageOfNodesToScore pct
// (yoda_num_feasible_to_find; host only): 5,000 of 100,000 nodes at pct 0.
func NumFeasibleToFind(nNodes uint32, pct int32) uint32 {
	return uint32(C.yoda_num_feasible_to_find(C.uint32_t(nNodes), C.int32_t(pct)))
}

// SetNodeSampling makes the Mode A batch path score only the first numToFind feasible nodes of
// each pod's walk (yoda_set_node_sampling): pod p's walk begins at the GLOBAL node id start[p]
// (nil: at the handle's node offset), wraps past the last node and skips absent nodes.  The
// PreScore maxima do not move; everything downstream of Filter follows the sample.  numToFind 0
// turns sampling off, as UploadNodes does.  While on, Mode B, greedy, shard and communicator
// calls, the reason rows and the all-pods diagnosis return an error that wraps YODA_ERR_STATE.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) SetNodeSampling(numToFind uint32, start []uint32) error {
	var p *C.uint32_t
	if len(start) > 0 {
		p = (*C.uint32_t)(unsafe.Pointer(&start[0]))
	}
	rc := C.yoda_set_node_sampling(g.h, C.uint32_t(numToFind), C.uint32_t(len(start)), p)
	return check(g.h, rc, "yoda_set_node_sampling")
}

// DownloadSampling fills nFound (|F'| before the cut) and nextStart (the GLOBAL id the pod's next
// walk begins at) of the last sampled run, one entry per pod of the batch
// (yoda_download_sampling); either may be nil.
func (g *Handle) DownloadSampling(nFound, nextStart []uint32) error {
	var f, x *C.uint32_t
	if len(nFound) > 0 {
		f = (*C.uint32_t)(unsafe.Pointer(&nFound[0]))
	}
	if len(nextStart) > 0 {
		x = (*C.uint32_t)(unsafe.Pointer(&nextStart[0]))
	}
	return check(g.h, C.yoda_download_sampling(g.h, f, x), "yoda_download_sampling")
}

// SamplingInfo reports {numToFind (0: off), length of the start array, 1 if the last run ran the
// sampling pass} (yoda_sampling_info; host only).
func (g *Handle) SamplingInfo() ([3]uint32, error) {
	var out [3]uint32
	rc := C.yoda_sampling_info(g.h, (*C.uint32_t)(unsafe.Pointer(&out[0])))
	return out, check(g.h, rc, "yoda_sampling_info")
}

// ModeBFollow makes Mode B's batch path (ScoreRow, Batch, Greedy with absent nodes) follow
// SetNodePresent and the candidate classes (yoda_mode_b_follow): a pod's cycle runs over the
// present nodes that are candidates of its class.  Off, the default, Mode B refuses while a node
// is absent or candidates are on.  A setting: it stays across uploads.  ShardedBatch and
// ShardedGreedy keep refusing either way.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) ModeBFollow(enable bool) error {
	on := C.int(0)
	if enable {
		on = 1
	}
	return check(g.h, C.yoda_mode_b_follow(g.h, on), "yoda_mode_b_follow")
}

// ModeBSampling makes Mode B's batch path (ScoreRow, Batch, the draw) honour SetNodeSampling
// (yoda_mode_b_sampling): a pod's cycle runs over the first numToFind nodes of its eligible set
// (ModeBFollow's: the whole snapshot while nothing is absent and candidates are off) in the walk
// that begins at its start id -- the cycle the deployed scheduler runs with
// percentageOfNodesToScore: 0.  DownloadSampling answers after such a run.  Off, the default,
// Mode B refuses while sampling is on.  A setting: it stays across uploads.  Greedy, ShardedBatch
// and ShardedGreedy keep refusing sampling either way.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) ModeBSampling(enable bool) error {
	on := C.int(0)
	if enable {
		on = 1
	}
	return check(g.h, C.yoda_mode_b_sampling(g.h, on), "yoda_mode_b_sampling")
}

// ModeBSamplingInfo reports {enabled, 1 if the last Mode B run took the sampled kernels,
// rank-table builds since the upload, 1 if that run used the eligibility instances}
// (yoda_mode_b_sampling_info; host only).
func (g *Handle) ModeBSamplingInfo() ([4]uint32, error) {
	var out [4]uint32
	rc := C.yoda_mode_b_sampling_info(g.h, (*C.uint32_t)(unsafe.Pointer(&out[0])))
	return out, check(g.h, rc, "yoda_mode_b_sampling_info")
}

// GreedyCandidates makes Greedy on this handle honour the candidate classes
// (yoda_greedy_candidates): each pod's cycle is the candidate-class cycle against the batch's
// current node state, its class the SetPodClasses entry at the pod's input index (an array as
// long as the batch, or none).  Mode B needs ModeBFollow as well.  Off, the default, Greedy
// refuses while candidates are on.  A setting: it stays across uploads.  ShardedGreedy keeps
// refusing either way.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) GreedyCandidates(enable bool) error {
	on := C.int(0)
	if enable {
		on = 1
	}
	return check(g.h, C.yoda_greedy_candidates(g.h, on), "yoda_greedy_candidates")
}

// ShardCandidates makes the sharded Mode A evaluation step on this handle (ShardedBatch:
// yoda_comm_run) honour the candidate classes (yoda_shard_candidates): the handle holds the
// candidate words of ITS shard's nodes and the whole batch's class array, and every shard's
// outcome equals one handle's Batch on the whole snapshot.  Every rank needs the same setting,
// class count and class array: yoda_comm_run checks them in its first all-reduce and fails on
// every rank when they differ.  Off, the default, ShardedBatch refuses while candidates are on.
// A setting: it stays across uploads.  ShardedGreedy and Mode B on shards keep refusing either
// way.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) ShardCandidates(enable bool) error {
	on := C.int(0)
	if enable {
		on = 1
	}
	return check(g.h, C.yoda_shard_candidates(g.h, on), "yoda_shard_candidates")
}

// packPods parses the scv/* labels and the diskIO annotation with the reference's own
// helpers (filter.go:60-74, sort.go:12-18, algorithm.go:103-104) into the C-side
// yoda_pod_soa arrays.
func (g *Handle) packPods(pods []*v1.Pod) C.yoda_pod_soa {
	n := len(pods)
	a := &g.pa
	hasNumber, hasMemory, hasClock := u8s(&a.hasNumber, n), u8s(&a.hasMemory, n), u8s(&a.hasClock, n)
	number, memory, clock := u64s(&a.number, n), u64s(&a.memory, n), u64s(&a.clock, n)
	priority, rcpu, rio := i64s(&a.priority, n), i64s(&a.rcpu, n), f64s(&a.rio, n)
	for i, p := range pods {
		l := p.GetLabels()
		has := func(key string) (uint8, uint64) {
			if v, ok := l[key]; ok {
				return 1, filter.StrToUint64(v)
			}
			return 0, 0
		}
		hasNumber[i], number[i] = has("scv/number")
		hasMemory[i], memory[i] = has("scv/memory")
		hasClock[i], clock[i] = has("scv/clock")
		priority[i] = 0
		if v, ok := l["scv/priority"]; ok {
			pr, _ := strconv.Atoi(v) // sort.go:14-15 keeps Atoi's value on error
			priority[i] = int64(pr)
		}
		rio[i], _ = strconv.ParseFloat(p.Annotations["diskIO"], 32) // algorithm.go:103
		rcpu[i] = score.CalculatePodResourceRequest(p, v1.ResourceCPU, true)
	}
	return C.yoda_pod_soa{
		n_pods:     C.uint32_t(n),
		has_number: (*C.uint8_t)(a.hasNumber.p), number: (*C.uint64_t)(a.number.p),
		has_memory: (*C.uint8_t)(a.hasMemory.p), memory: (*C.uint64_t)(a.memory.p),
		has_clock: (*C.uint8_t)(a.hasClock.p), clock: (*C.uint64_t)(a.clock.p),
		priority: (*C.int64_t)(a.priority.p), rio: (*C.double)(a.rio.p),
		rcpu: (*C.int64_t)(a.rcpu.p),
	}
}

// Row is one pod's Filter result and raw Score for every node of the snapshot.
type Row struct {
	Feasible []uint32 // bitmask, bit (n & 31) of word n/32
	Score    []int64  // Yoda.Score's value (after Uint64ToInt64); -1 where Filter fails
}

// ScoreRow evaluates ONE pod against every node: the plugin's PreFilter calls it once per
// scheduling cycle, so Filter and Score become lookups.
func (g *Handle) ScoreRow(pod *v1.Pod, mode Mode) (*Row, error) {
	s := g.packPods([]*v1.Pod{pod})
	if err := check(g.h, C.yoda_upload_pods(g.h, &s), "yoda_upload_pods"); err != nil {
		return nil, err
	}
	n := len(g.nodes)
	row := &Row{Feasible: make([]uint32, (n+31)/32+1), Score: make([]int64, n+1)}
	rc := C.yoda_score_rows(g.h, C.int(mode), (*C.uint32_t)(unsafe.Pointer(&row.Feasible[0])),
		C.uint64_t((n+31)/32), (*C.int64_t)(unsafe.Pointer(&row.Score[0])), C.uint64_t(n))
	if err := check(g.h, rc, "yoda_score_rows"); err != nil {
		return nil, err
	}
	row.Feasible, row.Score = row.Feasible[:(n+31)/32], row.Score[:n]
	return row, nil
}

// Reason is why Filter rejected a (pod, node) pair (YODA_REASON_*): the first that applies in the
// precedence absent > not a candidate > number > memory > clock.
type Reason uint8

const (
	ReasonNone         Reason = C.YODA_REASON_NONE          // the node passes
	ReasonNumber       Reason = C.YODA_REASON_NUMBER        // PodFitsNumber fails (filter.go:11-16)
	ReasonMemory       Reason = C.YODA_REASON_MEMORY        // PodFitsMemory fails (filter.go:18-33)
	ReasonClock        Reason = C.YODA_REASON_CLOCK         // PodFitsClock fails (filter.go:35-50)
	ReasonNotCandidate Reason = C.YODA_REASON_NOT_CANDIDATE // another plugin's Filter (SetCandidates)
	ReasonAbsent       Reason = C.YODA_REASON_ABSENT        // not in the node set (SetNodePresent)
)

// ReasonRow gives the reason code of every node for the pods uploaded last (ScoreRow's pod):
// reasons[n] == ReasonNone exactly where the row's feasibility bit is set (yoda_reason_rows;
// Mode A).  It invalidates a pending run, as ScoreRow does.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) ReasonRow() ([]Reason, error) {
	n := len(g.nodes)
	out := make([]Reason, n+1)
	rc := C.yoda_reason_rows(g.h, (*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(n))
	if err := check(g.h, rc, "yoda_reason_rows"); err != nil {
		return nil, err
	}
	return out[:n], nil
}

// Diagnose counts, after Batch (or ShardedBatch: over this shard's nodes, the caller sums the
// ranks), the nodes each pod lost to each reason: counts[p] = {not a candidate, number, memory,
// clock}, for the pods without a feasible node -- all: for every pod; a pod that was not selected
// has 0xFFFFFFFF in all four.  Absent nodes are counted nowhere (yoda_diagnose +
// yoda_download_diagnosis; Mode A).  nPods: the size of that batch.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) Diagnose(nPods int, all bool) ([][4]uint32, error) {
	flags := C.uint32_t(0)
	if all {
		flags = C.YODA_DIAG_ALL
	}
	if err := check(g.h, C.yoda_diagnose(g.h, flags), "yoda_diagnose"); err != nil {
		return nil, err
	}
	out := make([][4]uint32, nPods+1)
	rc := C.yoda_download_diagnosis(g.h, (*C.uint32_t)(unsafe.Pointer(&out[0])), C.uint64_t(4*nPods))
	if err := check(g.h, rc, "yoda_download_diagnosis"); err != nil {
		return nil, err
	}
	return out[:nPods], nil
}

// Batch schedules many pods independently against the snapshot (configs 2-4).  Picks are
// node indices, -1 unschedulable, -2 error (see statuses).
func (g *Handle) Batch(pods []*v1.Pod, mode Mode) (picks []int32, statuses []int32, err error) {
	if len(pods) == 0 {
		return nil, nil, nil
	}
	s := g.packPods(pods)
	n := len(pods)
	pk, st := i32s(&g.pa.pick, n), i32s(&g.pa.status, n)
	out := C.yoda_eval_out{pick: (*C.int32_t)(g.pa.pick.p), status: (*C.int32_t)(g.pa.status.p)}
	if err = check(g.h, C.yoda_eval(g.h, &s, C.int(mode), &out), "yoda_eval"); err != nil {
		return nil, nil, err
	}
	return append([]int32(nil), pk...), append([]int32(nil), st...), nil
}

// SetTieDraw turns the seeded selectHost draw of Batch on or off (yoda_set_tie_draw): when
// enabled, a pod that ends StatusOK with two or more top-scored nodes is placed on the one with
// the smallest TieHash(seed, podBase+p, node) -- p its index in the batch, node the global node
// id -- instead of the lowest.  podBase: the global index of the batch's first pod when the
// caller slices a larger batch.  ScoreRow and Greedy keep the lowest node either way; the
// node-sharded step (CommRun) draws only once ShardTieDraw is on as well.  Takes effect from
// the next Batch.
func (g *Handle) SetTieDraw(enable bool, seed, podBase uint64) error {
	on := C.int(0)
	if enable {
		on = 1
	}
	return check(g.h, C.yoda_set_tie_draw(g.h, on, C.uint64_t(seed), C.uint64_t(podBase)),
		"yoda_set_tie_draw")
}

// ShardTieDraw lets the node-sharded evaluation step draw too (yoda_shard_tie_draw): with it
// on AND SetTieDraw enabled, CommRun ends in the draw -- one more all-reduce (MIN, 8 bytes a
// pod) -- and the picks are those of one handle holding the whole snapshot.  Every shard of a
// batch must use the same (enable, seed, podBase); CommRun fails on every rank otherwise.
// Like the rest of this file, not compiled in this repository (no Go toolchain in the image).
func (g *Handle) ShardTieDraw(enable bool) error {
	on := C.int(0)
	if enable {
		on = 1
	}
	return check(g.h, C.yoda_shard_tie_draw(g.h, on), "yoda_shard_tie_draw")
}

// ShardDrawKeys and ShardDrawApply are the draw's two passes for a caller that drives the
// yoda_shard_* calls with its own collectives: after the sharded finalize (and the exact
// merge), ShardDrawKeys writes this shard's MIN draw key of every tied pod into dKeys -- DEVICE
// memory, [P] uint64 in the caller's pod order, ^0 where it has none; the caller all-reduces
// the keys over the ranks with an unsigned 64-bit MIN; ShardDrawApply then takes each key's
// low 32 bits as the pod's pick.
func (g *Handle) ShardDrawKeys(mode Mode, dKeys unsafe.Pointer) error {
	return check(g.h, C.yoda_shard_draw_keys(g.h, C.int(mode), (*C.uint64_t)(dKeys)),
		"yoda_shard_draw_keys")
}

func (g *Handle) ShardDrawApply(dKeys unsafe.Pointer) error {
	return check(g.h, C.yoda_shard_draw_apply(g.h, (*C.uint64_t)(dKeys)), "yoda_shard_draw_apply")
}

// TieHash is the draw word of (seed, pod, node) (yoda_tie_hash; host only): for one pod a
// bijection of the 32-bit node ids.
func TieHash(seed, pod uint64, node uint32) uint32 {
	return uint32(C.yoda_tie_hash(C.uint64_t(seed), C.uint64_t(pod), C.uint32_t(node)))
}

// Greedy schedules the pods one after another in sort.Less order, each pick updating the
// node's Allocate score (config 5); cardCapacity also decrements CardNumber.
func (g *Handle) Greedy(pods []*v1.Pod, mode Mode, cardCapacity bool) ([]int32, error) {
	if len(pods) == 0 {
		return nil, nil
	}
	s := g.packPods(pods)
	picks := make([]int32, len(pods))
	flags := C.uint32_t(0)
	if cardCapacity {
		flags = C.YODA_GREEDY_CARD_CAPACITY
	}
	rc := C.yoda_greedy(g.h, &s, C.int(mode), flags, (*C.int32_t)(unsafe.Pointer(&picks[0])))
	return picks, check(g.h, rc, "yoda_greedy")
}

// ---- several GPUs: libyoda's own RCCL exchange (include/yoda.h yoda_comm_*) --------------

// CommUniqueID makes the communicator id on rank 0; hand it to the other ranks out of band
// (a file, a ConfigMap, the k8s API ...).
func CommUniqueID() ([]byte, error) {
	id := make([]byte, C.YODA_COMM_ID_BYTES)
	if err := check(nil, C.yoda_comm_unique_id((*C.uint8_t)(unsafe.Pointer(&id[0]))),
		"yoda_comm_unique_id"); err != nil {
		return nil, err
	}
	return id, nil
}

// DeviceKey identifies this handle's GPU across hosts (yoda_device_key: a hash of the hostname
// and boot id, '/', the PCI bus id -- bus ids alone repeat on identical servers).  Ranks
// exchange it with the communicator id, out of band, and call CheckDevices before CommInit.
func (g *Handle) DeviceKey() (string, error) {
	buf := make([]byte, C.YODA_DEVICE_KEY_BYTES)
	if err := check(g.h, C.yoda_device_key(g.h, (*C.char)(unsafe.Pointer(&buf[0])),
		C.int(len(buf))), "yoda_device_key"); err != nil {
		return "", err
	}
	return C.GoString((*C.char)(unsafe.Pointer(&buf[0]))), nil
}

// DeviceBusID is the PCI bus id of this handle's GPU (yoda_device_bus_id).
func (g *Handle) DeviceBusID() (string, error) {
	buf := make([]byte, C.YODA_BUS_ID_BYTES)
	if err := check(g.h, C.yoda_device_bus_id(g.h, (*C.char)(unsafe.Pointer(&buf[0])),
		C.int(len(buf))), "yoda_device_bus_id"); err != nil {
		return "", err
	}
	return C.GoString((*C.char)(unsafe.Pointer(&buf[0]))), nil
}

// CheckDevices takes every rank's DeviceKey (rank order) and fails, naming the first pair,
// when two ranks would share one GPU (YODA_ERR_SAME_DEVICE: RCCL itself only reports an
// "invalid usage").  Host only.
func CheckDevices(busIDs []string) error {
	if len(busIDs) == 0 {
		return nil
	}
	stride := int(C.YODA_DEVICE_KEY_BYTES)
	flat := make([]byte, stride*len(busIDs))
	for r, id := range busIDs {
		if len(id) >= stride {
			return fmt.Errorf("yodagpu: device key of rank %d too long", r)
		}
		copy(flat[r*stride:], id)
	}
	var a, b C.int
	rc := C.yoda_comm_check_devices((*C.char)(unsafe.Pointer(&flat[0])), C.int(len(busIDs)),
		C.int(stride), &a, &b)
	if rc == C.YODA_ERR_SAME_DEVICE {
		return fmt.Errorf("yodagpu: ranks %d and %d are on the same GPU (%s)", int(a), int(b),
			busIDs[a])
	}
	return check(nil, rc, "yoda_comm_check_devices")
}

// CommInit joins this handle (one GPU holding the node shard uploaded with UploadShard) to the
// communicator of `world` ranks; collective: every rank calls it.
func (g *Handle) CommInit(id []byte, rank, world int) error {
	if len(id) != C.YODA_COMM_ID_BYTES {
		return errors.New("yodagpu: communicator id of the wrong size")
	}
	return check(g.h, C.yoda_comm_init(g.h, (*C.uint8_t)(unsafe.Pointer(&id[0])), C.int(rank),
		C.int(world)), "yoda_comm_init")
}

// ShardedBatch schedules the pods against the node shards of every rank (collective: every
// rank passes the same pods): yoda_comm_run's maxima / packed-key all-reduces.  Picks are
// global node indices.
func (g *Handle) ShardedBatch(pods []*v1.Pod, mode Mode) (picks []int32, statuses []int32, err error) {
	if len(pods) == 0 {
		return nil, nil, nil
	}
	s := g.packPods(pods)
	n := len(pods)
	if err = check(g.h, C.yoda_upload_pods(g.h, &s), "yoda_upload_pods"); err != nil {
		return nil, nil, err
	}
	if err = check(g.h, C.yoda_comm_run(g.h, C.int(mode)), "yoda_comm_run"); err != nil {
		return nil, nil, err
	}
	pk, st := i32s(&g.pa.pick, n), i32s(&g.pa.status, n)
	out := C.yoda_eval_out{pick: (*C.int32_t)(g.pa.pick.p), status: (*C.int32_t)(g.pa.status.p)}
	if err = check(g.h, C.yoda_download(g.h, &out), "yoda_download"); err != nil {
		return nil, nil, err
	}
	return append([]int32(nil), pk...), append([]int32(nil), st...), nil
}

// ShardedGreedy is Greedy across the ranks' node shards (collective; every rank passes the
// same pods and the same full snapshot `all`, which the host-side resolve reads): the windows'
// maxima and candidate lists merged over RCCL inside libyoda (yoda_comm_greedy).
func (g *Handle) ShardedGreedy(all []*scv.Scv, allAlloc []uint64, pods []*v1.Pod, mode Mode,
	cardCapacity bool) ([]int32, error) {
	if len(pods) == 0 {
		return nil, nil
	}
	var full nodeArrays // the full snapshot's C arrays (host only)
	defer full.release()
	soa, _, err := full.pack(all, allAlloc, nil, nil)
	if err != nil {
		return nil, err
	}
	s := g.packPods(pods)
	picks := make([]int32, len(pods))
	flags := C.uint32_t(0)
	if cardCapacity {
		flags = C.YODA_GREEDY_CARD_CAPACITY
	}
	rc := C.yoda_comm_greedy(g.h, &soa, &s, C.int(mode), flags,
		(*C.int32_t)(unsafe.Pointer(&picks[0])))
	return picks, check(g.h, rc, "yoda_comm_greedy")
}

// NodeIndex maps a node name to its row position.
func (g *Handle) NodeIndex(name string) (int, bool) {
	i, ok := g.index[name]
	return i, ok
}

// ZeroTotal reports whether node i has TotalMemorySum == 0: scoring it divides by zero in
// the reference (algorithm.go:294,309), a framework Error here.
func (g *Handle) ZeroTotal(i int) bool { return i >= 0 && i < len(g.zeroTotal) && g.zeroTotal[i] }

// Nodes is the snapshot's node order.
func (g *Handle) Nodes() []string { return g.nodes }
