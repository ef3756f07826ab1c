// Package groothip binds libgroot_hip.so / libgroot_host.so (include/groot_hip.h, include/groot_host.h): the MI355X
// device path of `groot align` behind a Go API shaped for theBoss.mapReads (src/pipeline/boss.go:108-242).
//
// Source only in this repository: the image it was written in has no Go toolchain, so this package has never been
// compiled.  It uses nothing but the C ABI and the standard library; cgo/patch/boss_hip.go is the file that goes into
// the reference's src/pipeline package and uses it.
//
// cgo pointer rules: every groot_hip_submit* call copies the caller's buffers into the ctx's pinned staging BEFORE it
// returns and keeps no caller pointer afterwards, so Go slices are passed directly (&s[0]); results come back as
// pointers into C-owned pinned memory that stay valid until Release.
//
// Build (on a machine with Go, ROCm and this repository's build/ directory):
//
//	CGO_CFLAGS="-I<repo>/include" CGO_LDFLAGS="-L<repo>/build -lgroot_hip -lgroot_host -Wl,-rpath,<repo>/build" go build -tags hip ./...
package groothip

/*
#include <stdlib.h>
#include "groot_hip.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// Trav mirrors groot_trav: one successful traversal of performAlignment with the path ids processTraversal assigned
type Trav struct {
	ReadID, GraphID, Node, Offset uint32
	Ord                           uint16
	Flags, Reserved               uint8
}

// flag bits of Trav.Flags
const (
	TravRC        = 1 // read.RC: the reverse complement aligned (sam.Reverse)
	TravStartClip = 2 // 1H before the M op (alignment.go:72-85)
	TravEndClip   = 4 // 1H after the M op (alignment.go:87-103)
	TravFirst     = 8 // first traversal of its AlignRead call
	TravMapq      = 16 // assignment: Reserved holds the MAPQ of the traversal's records
)

// Counts mirrors groot_counts (the boss counters, boss.go:24-27)
type Counts struct {
	Received, Mapped, Multimapped, Alignments, Seeds, Travs, RevcompPanics, ShortReads, FullSketchReads, WalkedReads, LeanReads uint64
}

// Index owns a flat index (groot_index) loaded from the files `groot index` wrote
type Index struct {
	h    *C.groot_index
	view C.groot_index_view
}

// LoadGob reads <dir>/groot.gg + <dir>/groot.lshe (cmd/align.go:93-107) through the C++ gob reader: the Go process
// never has to flatten its own graph.Store -- both sides read the same two files
func LoadGob(dir string) (*Index, error) {
	gg, lshe := C.CString(dir+"/groot.gg"), C.CString(dir+"/groot.lshe")
	defer C.free(unsafe.Pointer(gg))
	defer C.free(unsafe.Pointer(lshe))
	idx := &Index{}
	if rc := C.groot_index_load_gob(gg, lshe, &idx.h); rc != 0 {
		return nil, fmt.Errorf("groot_index_load_gob: %s", C.GoString(C.groot_host_last_error()))
	}
	C.groot_index_get_view(idx.h, &idx.view)
	return idx, nil
}

// Close frees the index
func (idx *Index) Close() {
	if idx.h != nil {
		C.groot_index_free(idx.h)
		idx.h = nil
	}
}

// NumGraphs, NumNodes, NumWindows of the flat index
func (idx *Index) NumGraphs() int  { return int(idx.view.n_graphs) }
func (idx *Index) NumNodes() int   { return int(idx.view.n_nodes) }
func (idx *Index) NumWindows() int { return int(idx.view.n_windows) }
func (idx *Index) PathWords() int  { return int(idx.view.path_words) }

func u32s(p *C.uint32_t, n int) []uint32 {
	if n == 0 {
		return nil
	}
	return (*[1 << 30]uint32)(unsafe.Pointer(p))[:n:n]
}

// GraphNodeOff[g] .. GraphNodeOff[g+1] = global node indices of graph g, in SortedNodes order
func (idx *Index) GraphNodeOff() []uint32 { return u32s(idx.view.graph_node_off, idx.NumGraphs()+1) }

// GraphPathOff[g] = global path index of local path id 0 of graph g
func (idx *Index) GraphPathOff() []uint32 { return u32s(idx.view.graph_path_off, idx.NumGraphs()+1) }

// NodeSegID[n] = GrootGraphNode.SegmentID of global node n
func (idx *Index) NodeSegID() []uint32 { return u32s(idx.view.node_seg_id, idx.NumNodes()) }

// Ctx is one GPU context (groot_ctx): the replicated index in HBM plus a ring of batches in flight
type Ctx struct {
	h      *C.groot_ctx
	idx    *Index
	device int
	params Params
	// assignment (AssignEnable): kept so that Reopen can hand it to the new ctx
	assignAlpha   []float64
	assignMinPost float64
}

// Params mirrors the fields of groot_params a host sets
type Params struct {
	ContainmentThreshold float64
	NoExactAlign         bool
	MaxReadLen           uint32
	MaxBatchReads        uint32
	PipelineDepth        uint32
	// MemoBudgetMB: 0 = the library's default budget for the memo of groot_hip_open, MemoOff = no memo (a run over a few
	// million reads: the memo costs more at open than it saves), else MiB
	MemoBudgetMB uint32
	// Background: GROOT_OPEN_BACKGROUND -- Open returns once the ctx can take batches and builds the prefix tables and the signature
	// index on a thread of its own (the Index must stay alive, which the Ctx sees to)
	Background bool
}

// MemoOff is GROOT_MEMO_OFF
const MemoOff = uint32(C.GROOT_MEMO_OFF)

// DeviceCount returns the number of visible GPUs
func DeviceCount() int {
	var n C.int
	if C.groot_hip_device_count(&n) != 0 {
		return 0
	}
	return int(n)
}

// Open uploads the index to GPU `device`
func Open(device int, idx *Index, p Params) (*Ctx, error) {
	var prm C.groot_params
	C.groot_params_default(&prm)
	prm.containment_threshold = C.double(p.ContainmentThreshold)
	if p.NoExactAlign {
		prm.no_exact_align = 1
	}
	if p.MaxReadLen != 0 {
		prm.max_read_len = C.uint32_t(p.MaxReadLen)
	}
	if p.MaxBatchReads != 0 {
		prm.max_batch_reads = C.uint32_t(p.MaxBatchReads)
	}
	if p.PipelineDepth != 0 {
		prm.pipeline_depth = C.uint32_t(p.PipelineDepth)
	}
	prm.memo_budget_mb = C.uint32_t(p.MemoBudgetMB)
	c := &Ctx{idx: idx, device: device, params: p}
	if c.params.MaxReadLen == 0 {
		c.params.MaxReadLen = uint32(prm.max_read_len)
	}
	var flags C.uint32_t
	if p.Background {
		flags = C.GROOT_OPEN_BACKGROUND
	}
	if rc := C.groot_hip_open_flags(&c.h, C.int(device), &idx.view, &prm, flags); rc != 0 {
		return nil, fmt.Errorf("groot_hip_open: %s", C.GoString(C.groot_hip_last_error(nil)))
	}
	return c, nil
}

// OpenAbandon tells a background open (Params.Background) to stop at its next checkpoint: for an input that has ended before the
// tables were there.  The ctx keeps working, through the full-width kernels.
func (c *Ctx) OpenAbandon() { C.groot_hip_open_abandon(c.h) }

// MaxReadLen is the longest read the ctx accepts (a longer one fails its batch with GROOT_E_NOSPACE)
func (c *Ctx) MaxReadLen() int { return int(c.params.MaxReadLen) }

// Reopen replaces the ctx by one that accepts reads of up to maxReadLen bases and carries the IncrementSubPath call counts
// over (groot_hip_attempts_export -> close -> open -> groot_hip_attempts_import, in that order): the reference has no read length limit
// (boss.go:145-203), the device sizes its LDS staging and DFS stacks for one.  Nothing may be in flight.
func (c *Ctx) Reopen(maxReadLen int) error {
	var nRows, nWin C.uint32_t
	if rc := C.groot_hip_attempts_export(c.h, nil, nil, 0, &nRows, &nWin); rc != 0 {
		return c.err("groot_hip_attempts_export")
	}
	q := make([]uint32, int(nRows)+1)
	counts := make([]uint32, int(nRows)*int(nWin)+1)
	if rc := C.groot_hip_attempts_export(c.h, (*C.uint32_t)(unsafe.Pointer(&q[0])), (*C.uint32_t)(unsafe.Pointer(&counts[0])), nRows, &nRows, &nWin); rc != 0 {
		return c.err("groot_hip_attempts_export")
	}
	// close first, then open: the index and the tables of groot_hip_open would otherwise sit in HBM twice
	old := c.params
	p := c.params
	p.MaxReadLen = uint32(maxReadLen)
	C.groot_hip_close(c.h)
	c.h = nil
	reopen := func(p Params) (*Ctx, error) {
		n, err := Open(c.device, c.idx, p)
		if err != nil {
			return nil, err
		}
		if rc := C.groot_hip_attempts_import(n.h, (*C.uint32_t)(unsafe.Pointer(&q[0])), (*C.uint32_t)(unsafe.Pointer(&counts[0])), nRows); rc != 0 {
			err := n.err("groot_hip_attempts_import")
			n.Close()
			return nil, err
		}
		if c.assignAlpha != nil {
			if err := n.AssignEnable(c.assignAlpha, c.assignMinPost); err != nil {
				n.Close()
				return nil, err
			}
		}
		return n, nil
	}
	bigger, err := reopen(p)
	if err != nil {
		// the larger ctx could not be had (HBM, a kmerCount outside its range): back to a ctx with the old limit and the counts exported
		// above, so that the caller still holds a working Ctx and loses nothing; only if that fails too is the Ctx dead (c.h == nil)
		if back, err2 := reopen(old); err2 == nil {
			c.h, c.params = back.h, back.params
			return fmt.Errorf("reopen for reads of %d bases: %v (the ctx keeps its limit of %d)", maxReadLen, err, old.MaxReadLen)
		}
		return fmt.Errorf("reopen for reads of %d bases: %v; the ctx could not be restored either and is closed", maxReadLen, err)
	}
	c.h, c.params = bigger.h, bigger.params
	return nil
}

// AssignStats mirrors groot_assign_stats: the reads with records, how they were classed, the records before and after, the traversals
// emptied, and (device only) the kernels launched for assignment since the ctx was opened
type AssignStats struct {
	Reads, Assigned, Unassigned, Below, Ties, RecordsIn, RecordsKept, TravsEmptied, Launches uint64
}

// AssignEnable switches assignment on with a copy of alpha (one value per path of the index, em_reads of an abundance file:
// AbundanceRead) or, with alpha == nil, off (include/groot_hip.h, "assignment"): every batch then keeps, per read, only the records on
// the path of S(r) with the largest alpha, with a MAPQ from its posterior.  Nothing may be in flight.  Not with AcovEnable or PairsEnable.
func (c *Ctx) AssignEnable(alpha []float64, minPosterior float64) error {
	var p *C.double
	if alpha != nil {
		if len(alpha) == 0 {
			return fmt.Errorf("groot_hip_assign_enable: alpha is empty")
		}
		p = (*C.double)(unsafe.Pointer(&alpha[0]))
	}
	if rc := C.groot_hip_assign_enable(c.h, p, C.uint32_t(len(alpha)), C.double(minPosterior)); rc != 0 {
		return c.err("groot_hip_assign_enable")
	}
	c.assignAlpha, c.assignMinPost = nil, 0
	if alpha != nil {
		c.assignAlpha, c.assignMinPost = append([]float64(nil), alpha...), minPosterior
	}
	return nil
}

// AssignBatch returns best (the global path, 0xFFFFFFFF for a read that keeps no record) and mapq of every read of a collected batch;
// the slices are the ctx's and die with Release
func (c *Ctx) AssignBatch(r *Result) (best []uint32, mapq []uint8, err error) {
	var b *C.uint32_t
	var q *C.uint8_t
	if rc := C.groot_hip_assign_batch(c.h, C.uint64_t(r.Ticket), &b, &q); rc != 0 {
		return nil, nil, c.err("groot_hip_assign_batch")
	}
	if r.NumReads == 0 {
		return nil, nil, nil
	}
	return (*[1 << 28]uint32)(unsafe.Pointer(b))[:r.NumReads:r.NumReads], (*[1 << 30]uint8)(unsafe.Pointer(q))[:r.NumReads:r.NumReads], nil
}

// AssignStatsGet returns the counters since AssignEnable or AssignReset (waits for everything in flight)
func (c *Ctx) AssignStatsGet() (AssignStats, error) {
	var st C.groot_assign_stats
	if rc := C.groot_hip_assign_stats(c.h, &st); rc != 0 {
		return AssignStats{}, c.err("groot_hip_assign_stats")
	}
	return AssignStats{uint64(st.reads), uint64(st.assigned), uint64(st.unassigned), uint64(st.below), uint64(st.ties), uint64(st.records_in),
		uint64(st.records_kept), uint64(st.travs_emptied), uint64(st.launches)}, nil
}

// AssignReset zeroes the counters (after waiting for everything in flight)
func (c *Ctx) AssignReset() error {
	if rc := C.groot_hip_assign_reset(c.h); rc != 0 {
		return c.err("groot_hip_assign_reset")
	}
	return nil
}

// AbundanceRead reads an abundance file (`align --abundance`, 4 or 8 columns) into alpha: em_reads per path of the index, 0 for the
// paths the file does not name
func (idx *Index) AbundanceRead(path string) ([]float64, error) {
	cp := C.CString(path)
	defer C.free(unsafe.Pointer(cp))
	alpha := make([]float64, int(idx.view.n_paths)+1)
	var named C.uint64_t
	if rc := C.groot_host_abundance_read(&idx.view, cp, (*C.double)(unsafe.Pointer(&alpha[0])), &named); rc != 0 {
		return nil, fmt.Errorf("groot_host_abundance_read: %s", C.GoString(C.groot_host_last_error()))
	}
	return alpha[:int(idx.view.n_paths)], nil
}

// AssignTravs is the definition of assignment on the CPU (groot_host_assign_travs): travs (in (read, ord) order) and masks (PathWords
// words per traversal) are rewritten in place; best and mapq have one entry per read of the batch
func (idx *Index) AssignTravs(alpha []float64, minPosterior float64, travs []Trav, masks []uint64, firstReadID uint32, numReads int) (best []uint32, mapq []uint8, st AssignStats, err error) {
	best, mapq = make([]uint32, numReads+1), make([]uint8, numReads+1)
	var cs C.groot_assign_stats
	var tp *C.groot_trav
	var mp *C.uint64_t
	var ap *C.double
	if len(travs) > 0 {
		tp, mp = (*C.groot_trav)(unsafe.Pointer(&travs[0])), (*C.uint64_t)(unsafe.Pointer(&masks[0]))
	}
	if len(alpha) > 0 {
		ap = (*C.double)(unsafe.Pointer(&alpha[0]))
	}
	if rc := C.groot_host_assign_travs(&idx.view, ap, C.double(minPosterior), tp, mp, C.uint64_t(len(travs)), C.uint32_t(firstReadID), C.uint32_t(numReads),
		(*C.uint32_t)(unsafe.Pointer(&best[0])), (*C.uint8_t)(unsafe.Pointer(&mapq[0])), &cs); rc != 0 {
		return nil, nil, st, fmt.Errorf("groot_host_assign_travs: %s", C.GoString(C.groot_host_last_error()))
	}
	st = AssignStats{uint64(cs.reads), uint64(cs.assigned), uint64(cs.unassigned), uint64(cs.below), uint64(cs.ties), uint64(cs.records_in),
		uint64(cs.records_kept), uint64(cs.travs_emptied), 0}
	return best[:numReads], mapq[:numReads], st, nil
}

// Close releases the GPU context
func (c *Ctx) Close() {
	if c.h != nil {
		C.groot_hip_close(c.h)
		c.h = nil
	}
}

// AcovEnable switches the assigned-coverage table on or off (include/groot_hip.h, "assigned coverage"): every record grouped by
// (EC of its read, path, Pos, last).  Switching it on switches equivalence classes on.  Nothing may be in flight.
func (c *Ctx) AcovEnable(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_acov_enable(c.h, v); rc != 0 {
		return c.err("groot_hip_acov_enable")
	}
	return nil
}

// AcovExport returns the ctx's ECs (CSR, canonical order) and its table: tuples[4i..4i+4) = (EC index, path, Pos, last), n[i] records
func (c *Ctx) AcovExport() (off []uint64, ids []uint32, count []uint64, tuples []uint32, n []uint64, err error) {
	var ne, ni, nt C.uint64_t
	if rc := C.groot_hip_acov_export(c.h, nil, nil, nil, nil, nil, 0, 0, 0, &ne, &ni, &nt); rc != 0 {
		return nil, nil, nil, nil, nil, c.err("groot_hip_acov_export")
	}
	off = make([]uint64, uint64(ne)+1)
	ids = make([]uint32, uint64(ni)+1)
	count = make([]uint64, uint64(ne)+1)
	tuples = make([]uint32, 4*uint64(nt)+4)
	n = make([]uint64, uint64(nt)+1)
	if rc := C.groot_hip_acov_export(c.h, (*C.uint64_t)(unsafe.Pointer(&off[0])), (*C.uint32_t)(unsafe.Pointer(&ids[0])), (*C.uint64_t)(unsafe.Pointer(&count[0])), (*C.uint32_t)(unsafe.Pointer(&tuples[0])), (*C.uint64_t)(unsafe.Pointer(&n[0])), ne, ni, nt, &ne, &ni, &nt); rc != 0 {
		return nil, nil, nil, nil, nil, c.err("groot_hip_acov_export")
	}
	return off, ids[:ni], count[:ne], tuples[:4*uint64(nt)], n[:nt], nil
}

// AcovStats returns the records and distinct tuples in the table, its slots, the times it grew, the records grouped on the host
// and the kernels launched for it since the ctx was opened
func (c *Ctx) AcovStats() (records, tuples, slots, grows, slowRecords, launches uint64, err error) {
	var r, t, s, g, sr, l C.uint64_t
	if rc := C.groot_hip_acov_stats(c.h, &r, &t, &s, &g, &sr, &l); rc != 0 {
		return 0, 0, 0, 0, 0, 0, c.err("groot_hip_acov_stats")
	}
	return uint64(r), uint64(t), uint64(s), uint64(g), uint64(sr), uint64(l), nil
}

// AcovReset empties the table (after waiting for everything in flight)
func (c *Ctx) AcovReset() error {
	if rc := C.groot_hip_acov_reset(c.h); rc != 0 {
		return c.err("groot_hip_acov_reset")
	}
	return nil
}

// PairsEnable switches paired-end counting on or off: reads 2i and 2i+1 of every batch are then the mates of one fragment, and
// shared reads and equivalence classes count units (include/groot_hip.h, "paired-end reads").  Nothing may be in flight.
func (c *Ctx) PairsEnable(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_pairs_enable(c.h, v); rc != 0 {
		return c.err("groot_hip_pairs_enable")
	}
	return nil
}

// PairsStats returns the fragments counted as joined, split and single since PairsEnable or the last reset of a counter
func (c *Ctx) PairsStats() (joined, split, single uint64, err error) {
	var j, s, o C.uint64_t
	if rc := C.groot_hip_pairs_stats(c.h, &j, &s, &o); rc != 0 {
		return 0, 0, 0, c.err("groot_hip_pairs_stats")
	}
	return uint64(j), uint64(s), uint64(o), nil
}

// GapEcStats mirrors groot_gap_ec_stats
type GapEcStats struct {
	Reads, SlowReads, Launches uint64
}

// GapEcEnable switches the gap-placed reads in the equivalence classes on or off (include/groot_hip.h, "gap-placed reads in the
// equivalence classes"): a read gapped rescue places is then a unit of the classes with the set of paths it was gap-placed on.  Needs
// gapped rescue and the rescued reads in the classes on.  Nothing may be in flight.
func (c *Ctx) GapEcEnable(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_gap_ec_enable(c.h, v); rc != 0 {
		return c.err("groot_hip_gap_ec_enable")
	}
	return nil
}

// GapEcStatsGet returns the gap-rescued reads added to the classes since GapEcEnable or a reset of the classes (waits for everything in flight)
func (c *Ctx) GapEcStatsGet() (GapEcStats, error) {
	var st C.groot_gap_ec_stats
	if rc := C.groot_hip_gap_ec_stats(c.h, &st); rc != 0 {
		return GapEcStats{}, c.err("groot_hip_gap_ec_stats")
	}
	return GapEcStats{uint64(st.reads), uint64(st.slow_reads), uint64(st.launches)}, nil
}

// GapAcovStats mirrors groot_gap_acov_stats
type GapAcovStats struct {
	Placements, Records, HostRecords, Dropped, Launches uint64
}

// GapAcovEnable piles every kept gapped placement of a gap-rescued read up in assigned coverage, two records for a DEL and one for an
// INS (include/groot_hip.h, "gap-placed reads in assigned coverage").  Needs GapEnable and RescueAcovEnable first; it switches the
// gap-placed reads in the classes on itself, and off switches both off.  Only while nothing is in flight.
func (c *Ctx) GapAcovEnable(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_gap_acov_enable(c.h, v); rc != 0 {
		return c.err("groot_hip_gap_acov_enable")
	}
	return nil
}

// GapAcovStatsGet returns the gapped placements and records piled up since GapAcovEnable or a reset of the table (waits for everything in flight)
func (c *Ctx) GapAcovStatsGet() (GapAcovStats, error) {
	var st C.groot_gap_acov_stats
	if rc := C.groot_hip_gap_acov_stats(c.h, &st); rc != 0 {
		return GapAcovStats{}, c.err("groot_hip_gap_acov_stats")
	}
	return GapAcovStats{uint64(st.placements), uint64(st.records), uint64(st.host_records), uint64(st.dropped), uint64(st.launches)}, nil
}

// AcovPairsStats mirrors groot_acov_pairs_stats
type AcovPairsStats struct {
	Records, LeftOut, JoinedReads, SlowFragments uint64
}

// AcovPairsEnable puts the ctx into assigned coverage over fragments (include/groot_hip.h, "assigned coverage over fragments"): it
// switches on whichever of equivalence classes, assigned coverage and pairing is off, and a record of a joined fragment then counts on
// the paths of the fragment's set only.  Off: the rule and assigned coverage go, the classes and pairing stay.  Only while nothing is in flight.
func (c *Ctx) AcovPairsEnable(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_acov_pairs_enable(c.h, v); rc != 0 {
		return c.err("groot_hip_acov_pairs_enable")
	}
	return nil
}

// AcovPairsStatsGet returns the records piled up and left out under the rule since AcovPairsEnable or a reset of the table (waits for everything in flight)
func (c *Ctx) AcovPairsStatsGet() (AcovPairsStats, error) {
	var st C.groot_acov_pairs_stats
	if rc := C.groot_hip_acov_pairs_stats(c.h, &st); rc != 0 {
		return AcovPairsStats{}, c.err("groot_hip_acov_pairs_stats")
	}
	return AcovPairsStats{uint64(st.records), uint64(st.left_out), uint64(st.joined_reads), uint64(st.slow_fragments)}, nil
}

// RescuePairsStats mirrors groot_rescue_pairs_stats
type RescuePairsStats struct {
	ExactRescuedJoined, ExactRescuedSplit, RescuedRescuedJoined, RescuedRescuedSplit uint64
	SingleExact, SingleRescued, RescuedMates, BitmapUnits, Launches                 uint64
}

// RescuePairsEnable puts the ctx into rescued mates in paired-end units (include/groot_hip.h, "rescued mates in paired-end units"): it
// switches on whichever of equivalence classes, pairing and the rescued reads in the classes is off, and a fragment's unit is then made of
// each mate's records or, for a mate mismatch rescue places, of its rescued set.  Needs RescueEnable first.  Off: the rule and the rescued
// classes go, the classes and pairing stay.  Only while nothing is in flight.
func (c *Ctx) RescuePairsEnable(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_rescue_pairs_enable(c.h, v); rc != 0 {
		return c.err("groot_hip_rescue_pairs_enable")
	}
	return nil
}

// RescuePairsStatsGet returns the fragments with a rescued or a lone mate by kind since RescuePairsEnable or EcReset (waits for everything in flight)
func (c *Ctx) RescuePairsStatsGet() (RescuePairsStats, error) {
	var st C.groot_rescue_pairs_stats
	if rc := C.groot_hip_rescue_pairs_stats(c.h, &st); rc != 0 {
		return RescuePairsStats{}, c.err("groot_hip_rescue_pairs_stats")
	}
	return RescuePairsStats{uint64(st.exact_rescued_joined), uint64(st.exact_rescued_split), uint64(st.rescued_rescued_joined), uint64(st.rescued_rescued_split),
		uint64(st.single_exact), uint64(st.single_rescued), uint64(st.rescued_mates), uint64(st.bitmap_units), uint64(st.launches)}, nil
}

// RescueAcovPairsStats mirrors groot_rescue_acov_pairs_stats
type RescueAcovPairsStats struct {
	ExactRecords, ExactLeftOut, RescuedRecords, RescuedLeftOut uint64
	HostRecords, Dropped, LogRows, Launches                    uint64
}

// RescueAcovPairsEnable puts the ctx into rescued mates in assigned coverage over fragments (include/groot_hip.h, "rescued mates in
// assigned coverage over fragments"): it switches on whichever of the classes, pairing, the rescued classes, the rescued mates' rule,
// assigned coverage and its rule over fragments is off, and a record or a kept placement of a mate then counts on the paths of the mate's
// unit.  Needs RescueEnable first.  minSlots: 0 or a power of two, the table's slots at least.  Off: the rule and assigned coverage go, the
// classes, pairing and the rescued mates' rule stay.  Only while nothing is in flight.
func (c *Ctx) RescueAcovPairsEnable(on bool, minSlots uint64) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.groot_hip_rescue_acov_pairs_enable(c.h, v, C.uint64_t(minSlots)); rc != 0 {
		return c.err("groot_hip_rescue_acov_pairs_enable")
	}
	return nil
}

// RescueAcovPairsStatsGet returns the records of fragments with a rescued mate in the pileup since RescueAcovPairsEnable or AcovReset (waits for everything in flight)
func (c *Ctx) RescueAcovPairsStatsGet() (RescueAcovPairsStats, error) {
	var st C.groot_rescue_acov_pairs_stats
	if rc := C.groot_hip_rescue_acov_pairs_stats(c.h, &st); rc != 0 {
		return RescueAcovPairsStats{}, c.err("groot_hip_rescue_acov_pairs_stats")
	}
	return RescueAcovPairsStats{uint64(st.exact_records), uint64(st.exact_left_out), uint64(st.rescued_records), uint64(st.rescued_left_out),
		uint64(st.host_records), uint64(st.dropped), uint64(st.log_rows), uint64(st.launches)}, nil
}

func (c *Ctx) err(what string) error {
	return fmt.Errorf("%s: %s", what, C.GoString(C.groot_hip_last_error(c.h)))
}

// Batch is the wire format of one batch of reads: 2 bits per base, one uint16 length per read, and the list of bytes
// that are not A, C, G or T (their position in the concatenation of all reads of the batch)
type Batch struct {
	Packed  []byte
	Lens    []uint16
	ExcPos  []uint64
	ExcByte []byte
	nBases  uint64
	maxLen  int
}

// Add appends read.Seq to the batch (FASTQread.Seq as it came: no upper-casing, sketch.go:258-282 removed the QC)
func (b *Batch) Add(seq []byte) error {
	if len(seq) > 65535 {
		return fmt.Errorf("read longer than 65535 bases")
	}
	for _, ch := range seq {
		if b.nBases&3 == 0 {
			b.Packed = append(b.Packed, 0)
		}
		b.Packed[len(b.Packed)-1] |= ((ch >> 1) & 3) << (2 * (b.nBases & 3))
		if ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' {
			b.ExcPos = append(b.ExcPos, b.nBases)
			b.ExcByte = append(b.ExcByte, ch)
		}
		b.nBases++
	}
	b.Lens = append(b.Lens, uint16(len(seq)))
	if len(seq) > b.maxLen {
		b.maxLen = len(seq)
	}
	return nil
}

// MaxLen is the length of the longest read in the batch
func (b *Batch) MaxLen() int { return b.maxLen }

// Len is the number of reads in the batch
func (b *Batch) Len() int { return len(b.Lens) }

// Reset empties the batch, keeping its capacity
func (b *Batch) Reset() {
	b.Packed, b.Lens, b.ExcPos, b.ExcByte, b.nBases, b.maxLen = b.Packed[:0], b.Lens[:0], b.ExcPos[:0], b.ExcByte[:0], 0, 0
}

// Submit enqueues the batch (copy to pinned staging -> H2D -> kernels -> D2H, asynchronous).  ErrFull means
// PipelineDepth batches are submitted and not released: Collect + Release first.
func (c *Ctx) Submit(b *Batch) error {
	if b.Len() == 0 {
		return nil
	}
	var packed *C.uint8_t
	if len(b.Packed) > 0 {
		packed = (*C.uint8_t)(unsafe.Pointer(&b.Packed[0]))
	}
	var excPos *C.uint64_t
	var excByte *C.uint8_t
	if len(b.ExcPos) > 0 {
		excPos = (*C.uint64_t)(unsafe.Pointer(&b.ExcPos[0]))
		excByte = (*C.uint8_t)(unsafe.Pointer(&b.ExcByte[0]))
	}
	rc := C.groot_hip_submit_packed16(c.h, packed, (*C.uint16_t)(unsafe.Pointer(&b.Lens[0])), C.uint32_t(len(b.Lens)), 0,
		excPos, excByte, C.uint64_t(len(b.ExcPos)))
	if rc == C.GROOT_E_STATE {
		return ErrFull
	}
	if rc != 0 {
		return c.err("groot_hip_submit_packed16")
	}
	return nil
}

// ErrFull is returned by Submit when every pipeline slot is taken
var ErrFull = fmt.Errorf("groot-hip: pipeline full")

// Result describes one finished batch; Travs / Masks point into pinned memory owned by the ctx and stay valid until Release
type Result struct {
	Ticket    uint64
	NumReads  int
	Counts    Counts
	Travs     []Trav
	Masks     []uint64 // PathWords words per traversal: bit p = local path id p (widened from the compact wire form)
	PathWords int
}

// InFlight is the number of batches submitted and not yet collected
func (c *Ctx) InFlight() int {
	var n, free C.uint32_t
	C.groot_hip_in_flight(c.h, &n, &free)
	return int(n)
}

// Collect blocks until the oldest submitted batch is finished.  The reference's panics come back as errors: a read
// shorter than k (boss.go:164-166), a byte > 'T' reaching RevComplement (seqio.go:126).
func (c *Ctx) Collect() (*Result, error) {
	var r C.groot_batch_result
	rc := C.groot_hip_collect(c.h, &r)
	if rc != 0 {
		return nil, c.err("groot_hip_collect")
	}
	n := int(r.n_travs)
	res := &Result{Ticket: uint64(r.ticket), NumReads: int(r.n_reads), PathWords: int(r.path_words)}
	res.Counts = Counts{uint64(r.counts.received), uint64(r.counts.mapped), uint64(r.counts.multimapped), uint64(r.counts.alignments),
		uint64(r.counts.seeds), uint64(r.counts.travs), uint64(r.counts.revcomp_panics), uint64(r.counts.short_reads), uint64(r.counts.full_sketch_reads), uint64(r.counts.walked_reads), uint64(r.counts.lean_reads)}
	if n > 0 {
		res.Travs = (*[1 << 28]Trav)(unsafe.Pointer(r.travs))[:n:n]
		// the path sets travel compact (as many bytes as the traversal's graph has paths / 8); widen them once per batch
		res.Masks = make([]uint64, n*res.PathWords)
		if rc := C.groot_host_unpack_masks(&c.idx.view, r.travs, C.uint64_t(n), r.masks, (*C.uint64_t)(unsafe.Pointer(&res.Masks[0]))); rc != 0 {
			return nil, fmt.Errorf("groot_host_unpack_masks: %s", C.GoString(C.groot_host_last_error()))
		}
	}
	return res, nil
}

// Release hands the batch's slot back to the ctx; the slices of the Result must not be used afterwards
func (c *Ctx) Release(r *Result) {
	C.groot_hip_release(c.h, C.uint64_t(r.Ticket))
	r.Travs, r.Masks = nil, nil
}

// Weights sums the IncrementSubPath call counts over the ctxs (RCCL all-reduce across GPUs) and replays
// GrootGraph.IncrementSubPath (graph.go:401-451) in the canonical order: KmerFreq per global node, KmerTotal per graph
func Weights(ctxs []*Ctx) (kmerFreq []float64, kmerTotal []uint64, err error) {
	if len(ctxs) == 0 {
		return nil, nil, fmt.Errorf("no ctx")
	}
	hs := make([]*C.groot_ctx, len(ctxs))
	for i, c := range ctxs {
		hs[i] = c.h
	}
	// the array of ctx handles lives in C memory for the call (a Go slice of C pointers is fine too; this keeps vet quiet)
	arr := (**C.groot_ctx)(C.malloc(C.size_t(len(hs)) * C.size_t(unsafe.Sizeof(hs[0]))))
	defer C.free(unsafe.Pointer(arr))
	copy((*[1 << 20]*C.groot_ctx)(unsafe.Pointer(arr))[:len(hs):len(hs)], hs)
	if rc := C.groot_hip_attempts_allreduce(arr, C.int(len(hs))); rc != 0 {
		return nil, nil, ctxs[0].err("groot_hip_attempts_allreduce")
	}
	c := ctxs[0]
	var nRows, nWin C.uint32_t
	if rc := C.groot_hip_attempts_export(c.h, nil, nil, 0, &nRows, &nWin); rc != 0 {
		return nil, nil, c.err("groot_hip_attempts_export")
	}
	q := make([]uint32, int(nRows)+1)
	counts := make([]uint32, int(nRows)*int(nWin)+1)
	if rc := C.groot_hip_attempts_export(c.h, (*C.uint32_t)(unsafe.Pointer(&q[0])), (*C.uint32_t)(unsafe.Pointer(&counts[0])), nRows, &nRows, &nWin); rc != 0 {
		return nil, nil, c.err("groot_hip_attempts_export")
	}
	kmerFreq = make([]float64, c.idx.NumNodes()+1)
	kmerTotal = make([]uint64, c.idx.NumGraphs()+1)
	if rc := C.groot_host_weights_rows(&c.idx.view, (*C.uint32_t)(unsafe.Pointer(&q[0])), nRows, (*C.uint32_t)(unsafe.Pointer(&counts[0])),
		(*C.double)(unsafe.Pointer(&kmerFreq[0])), (*C.uint64_t)(unsafe.Pointer(&kmerTotal[0]))); rc != 0 {
		return nil, nil, fmt.Errorf("groot_host_weights_rows: %s", C.GoString(C.groot_host_last_error()))
	}
	return kmerFreq[:c.idx.NumNodes()], kmerTotal[:c.idx.NumGraphs()], nil
}
