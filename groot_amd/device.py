"""Python mirror of libgroot_hip.so (include/groot_hip.h): the MI355X device path of `groot align`.

Fails loudly when the HIP library or a GPU is missing -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _ffi, host
from ._ffi import IndexView
from .host import GrootError

TRAV_DTYPE = np.dtype([("read_id", "<u4"), ("graph_id", "<u4"), ("node", "<u4"), ("offset", "<u4"), ("ord", "<u2"),
                       ("flags", "u1"), ("reserved", "u1")])
ALN_DTYPE = np.dtype([("read_id", "<u4"), ("graph_id", "<u4"), ("path_id", "<u4"), ("ref_id", "<u4"), ("pos", "<u4"),
                      ("start_clip", "u1"), ("end_clip", "u1"), ("rc", "u1"), ("secondary", "u1")])
SEED_DTYPE = np.dtype([("read_id", "<u4"), ("window_id", "<u4")])
GAP_EVENT_DTYPE = host.GAP_EVENT_DTYPE                     # groot_gap_event
RESCUE_RECORD_DTYPE = np.dtype([("read", "<u4"), ("path", "<u4"), ("pos", "<u4"), ("mm", "<u2", (3,)), ("strand", "u1"), ("d", "u1")])   # groot_rescue_record
GAP_RECORD_DTYPE = np.dtype([("read", "<u4"), ("path", "<u4"), ("pos", "<u4"), ("k", "<u2"), ("mm", "<u2", (3,)), ("strand", "u1"), ("d", "u1"), ("type", "u1"),
                             ("g", "u1")])   # groot_gap_record
GAP_DEL, GAP_INS = 0, 1
GAP_STATS = ("candidates", "rescued", "placements", "del_placements", "ins_placements", "too_short", "events", "dropped", "event_slots", "launches")
TRAV_RC, TRAV_START_CLIP, TRAV_END_CLIP, TRAV_FIRST, TRAV_MAPQ = 1, 2, 4, 8, 16


class Params(C.Structure):
    _fields_ = [("containment_threshold", C.c_double), ("no_exact_align", C.c_uint32), ("max_read_len", C.c_uint32),
                ("max_batch_reads", C.c_uint32), ("max_seeds_per_read", C.c_uint32), ("max_batch_bases", C.c_uint64),
                ("keep_sketches", C.c_uint32), ("pipeline_depth", C.c_uint32), ("results_on_device", C.c_uint32),
                ("memo_budget_mb", C.c_uint32)]


MEMO_OFF = 0xFFFFFFFF


class Counts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("received", "mapped", "multimapped", "alignments", "seeds", "travs",
                                            "revcomp_panics", "short_reads", "full_sketch_reads", "walked_reads", "lean_reads")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class OpenStats(C.Structure):
    _fields_ = [("open_ms", C.c_double), ("memo_ms", C.c_double)] + [(n, C.c_uint64) for n in ("memo_strings", "memo_tabulated", "memo_entries", "text_entries",
                                                                                               "memo_hbm_bytes")]


class StageMs(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("h2d", "sketch_seed", "align", "sort", "total", "schedule", "d2h", "unpack", "first_seed_kernel", "order_kernel", "list_pass", "wall", "lean_pass")]


class BatchBuffers(C.Structure):
    """groot_batch_buffers: the pinned staging of one pipeline slot (groot_hip_acquire)"""
    _fields_ = [("ticket", C.c_uint64), ("packed", C.POINTER(C.c_uint8)), ("seq_len", C.POINTER(C.c_uint16)),
                ("exc_pos", C.POINTER(C.c_uint64)), ("exc_byte", C.POINTER(C.c_uint8)), ("packed_cap", C.c_uint64),
                ("exc_cap", C.c_uint64), ("reads_cap", C.c_uint32), ("reserved", C.c_uint32)]


class BatchResult(C.Structure):
    """groot_batch_result"""
    _fields_ = [("ticket", C.c_uint64), ("first_read_id", C.c_uint32), ("n_reads", C.c_uint32), ("counts", Counts),
                ("travs", C.c_void_p), ("masks", C.c_void_p), ("mask_ckpt", C.c_void_p), ("n_mask_bytes", C.c_uint64),
                ("n_travs", C.c_uint64), ("d_travs", C.c_void_p),
                ("d_masks", C.c_void_p), ("path_words", C.c_uint32), ("status", C.c_int32), ("ms", StageMs)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("GROOT_HIP_LIB") or _ffi.lib_path("libgroot_hip.so")   # (GROOT_HIP_LIB: instrumented builds, tools/)
        if not os.path.exists(path):
            raise ImportError(f"{path} missing: the HIP extension was not built (python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(path)
        L.groot_hip_last_error.restype = C.c_char_p
        L.groot_hip_last_error.argtypes = [C.c_void_p]
        L.groot_hip_close.argtypes = [C.c_void_p]
        L.groot_hip_close.restype = None
        _ffi.rarefy_hip_prototypes(L)
        _ffi.gap_ec_prototypes(L)
        _ffi.gap_acov_prototypes(L)
        _ffi.acov_pairs_prototypes(L)
        _ffi.rescue_pairs_prototypes(L)
        _ffi.rescue_acov_pairs_prototypes(L)
        _lib = L
    return _lib


def device_count():
    n = C.c_int(0)
    rc = lib().groot_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def unpack_masks(index, travs, compact_masks):
    """groot_host_unpack_masks: the compact path sets of collect(copy=False) -> [n, path_words]"""
    travs = np.ascontiguousarray(travs, dtype=TRAV_DTYPE)
    cm = np.ascontiguousarray(compact_masks, dtype=np.uint8)
    out = np.zeros((len(travs), index.view.path_words), dtype=np.uint64)
    host._check(host.lib().groot_host_unpack_masks(C.byref(index.view), travs.ctypes.data_as(C.c_void_p), C.c_uint64(len(travs)),
                                                   _ffi.as_ptr(cm, C.c_uint8), _ffi.as_ptr(out, C.c_uint64)))
    return out


def expand_alns(index, travs, masks):
    """groot_host_expand_alns: traversal records -> one tuple per sam.Record."""
    travs = np.ascontiguousarray(travs, dtype=TRAV_DTYPE)
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    n = C.c_uint64(0)
    H = host.lib()
    rc = H.groot_host_expand_alns(C.byref(index.view), travs.ctypes.data_as(C.c_void_p), _ffi.as_ptr(masks, C.c_uint64),
                                  C.c_uint64(len(travs)), None, C.c_uint64(0), C.byref(n))
    host._check(rc)
    out = np.zeros(n.value, dtype=ALN_DTYPE)
    rc = H.groot_host_expand_alns(C.byref(index.view), travs.ctypes.data_as(C.c_void_p), _ffi.as_ptr(masks, C.c_uint64),
                                  C.c_uint64(len(travs)), out.ctypes.data_as(C.c_void_p), C.c_uint64(len(out)), C.byref(n))
    host._check(rc)
    return out


def em_bootstrap(n_paths, off, ids, count, n_boot, seed=1, n_draws=0, min_iter=host.EM_MIN_ITER, max_iter=host.EM_MAX_ITER, device=0):
    """groot_hip_em_bootstrap: host.em_bootstrap on the device, bit for bit ->
    (boot_count uint64[n_boot, n_ec], alpha float64[n_boot, n_paths], iterations uint32[n_boot])"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if len(off) != len(count) + 1:
        raise ValueError("off must have one entry more than count")
    bc = np.zeros((n_boot, len(count)), dtype=np.uint64)
    alpha = np.zeros((n_boot, n_paths), dtype=np.float64)
    its = np.zeros(n_boot, dtype=np.uint32)
    rc = lib().groot_hip_em_bootstrap(C.c_int(device), C.c_uint32(n_paths), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                      _ffi.as_ptr(count, C.c_uint64), C.c_uint32(n_boot), C.c_uint64(seed), C.c_uint64(n_draws), C.c_uint32(min_iter),
                                      C.c_uint32(max_iter), _ffi.as_ptr(bc, C.c_uint64), _ffi.as_ptr(alpha, C.c_double), _ffi.as_ptr(its, C.c_uint32))
    if rc < 0:
        raise GrootError(rc, lib().groot_hip_last_error(None).decode(errors="replace"))
    return bc, alpha, its


def em_rarefy(n_paths, off, ids, count, n_rep, depths, seed=1, min_iter=host.EM_MIN_ITER, max_iter=host.EM_MAX_ITER, device=0):
    """groot_hip_em_rarefy: host.em_rarefy on the device, bit for bit ->
    (rare_count uint64[n_rep, n_depths, n_ec], alpha float64[n_rep, n_depths, n_paths], iterations uint32[n_rep, n_depths])"""
    off, ids, count = host._ec_arrays(off, ids, count)
    depths = np.ascontiguousarray(depths, dtype=np.uint64).reshape(-1)
    rc = np.zeros((n_rep, len(depths), len(count)), dtype=np.uint64)
    alpha = np.zeros((n_rep, len(depths), n_paths), dtype=np.float64)
    its = np.zeros((n_rep, len(depths)), dtype=np.uint32)
    err = lib().groot_hip_em_rarefy(device, n_paths, len(count), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32), _ffi.as_ptr(count, C.c_uint64), n_rep,
                                    len(depths), _ffi.as_ptr(depths, C.c_uint64), seed, min_iter, max_iter, _ffi.as_ptr(rc, C.c_uint64),
                                    _ffi.as_ptr(alpha, C.c_double), _ffi.as_ptr(its, C.c_uint32))
    if err < 0:
        raise GrootError(err, lib().groot_hip_last_error(None).decode(errors="replace"))
    return rc, alpha, its


def call_support(n_paths, path_len, off, ids, count, tuples, tn, boot_count, alpha, sel_paths, call_depth=1.0, device=0):
    """groot_hip_call_support: host.call_support on the device, bit for bit -> covered uint32[n_boot, n_sel]"""
    path_len, off, ids, count, tuples, tn, n_boot, boot_count, alpha, sel = host._support_arrays(n_paths, path_len, off, ids, count, tuples, tn, boot_count,
                                                                                                alpha, sel_paths)
    cov = np.zeros((n_boot, len(sel)), dtype=np.uint32)
    rc = lib().groot_hip_call_support(C.c_int(device), C.c_uint32(n_paths), _ffi.as_ptr(path_len, C.c_uint32), C.c_uint64(len(count)),
                                      _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32), _ffi.as_ptr(count, C.c_uint64), C.c_uint64(len(tn)),
                                      _ffi.as_ptr(tuples, C.c_uint32), _ffi.as_ptr(tn, C.c_uint64), C.c_uint32(n_boot), _ffi.as_ptr(boot_count, C.c_uint64),
                                      _ffi.as_ptr(alpha, C.c_double), C.c_double(call_depth), C.c_uint32(len(sel)), _ffi.as_ptr(sel, C.c_uint32),
                                      _ffi.as_ptr(cov, C.c_uint32))
    if rc < 0:
        raise GrootError(rc, lib().groot_hip_last_error(None).decode(errors="replace"))
    return cov


def call_support_info():
    """what this thread's last call_support did: {"rows", "width" (bytes per integer: 4 or 8), "chunks" (of paths)}"""
    r, w, c = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    lib().groot_hip_call_support_info(C.byref(r), C.byref(w), C.byref(c))
    return {"rows": r.value, "width": w.value, "chunks": c.value}


class Aligner:
    """One groot_ctx: the replacement for theBoss.mapReads (src/pipeline/boss.go:108-242) on one GPU."""

    def __init__(self, index, device=0, threshold=0.99, no_align=False, max_read_len=256, max_batch_reads=1 << 20,
                 max_seeds_per_read=8, keep_sketches=False, max_batch_bases=0, pipeline_depth=0, results_on_device=False, memo_budget_mb=0,
                 background=False):
        self.index = index
        self.params = Params(threshold, 1 if no_align else 0, max_read_len, max_batch_reads, max_seeds_per_read,
                             max_batch_bases, 1 if keep_sketches else 0, pipeline_depth, 1 if results_on_device else 0, memo_budget_mb)
        self._h = C.c_void_p()
        # (background: GROOT_OPEN_BACKGROUND -- the index arrays must outlive the build: self.index holds them)
        rc = lib().groot_hip_open_flags(C.byref(self._h), C.c_int(device), C.byref(index.view), C.byref(self.params), C.c_uint32(1 if background else 0))
        if rc:
            raise GrootError(rc, lib().groot_hip_last_error(None).decode(errors="replace"))
        self.s = index.view.sketch_size
        self.path_words = index.view.path_words

    def close(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.groot_hip_close(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _check(self, rc):
        if rc < 0:
            raise GrootError(rc, lib().groot_hip_last_error(self._h).decode(errors="replace"))
        return rc

    # ---- batch API ----------------------------------------------------------------------------
    def open_wait(self):
        """groot_hip_open_wait: the background part of the open (prefix tables, signature index) is in place"""
        self._check(lib().groot_hip_open_wait(self._h))

    def open_abandon(self):
        """groot_hip_open_abandon: a background open stops at its next checkpoint; the ctx keeps working without what it was building"""
        self._check(lib().groot_hip_open_abandon(self._h))

    def open_stats(self):
        """groot_hip_open_stats: what open built besides the uploaded index (the memo) and how long it took"""
        st = OpenStats()
        self._check(lib().groot_hip_open_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in OpenStats._fields_}

    def set_stream(self, hip_stream):
        self._check(lib().groot_hip_set_stream(self._h, C.c_void_p(hip_stream)))

    def stream_join(self, hip_stream=None):
        """device-side: `hip_stream` (None = the stream of set_stream) waits for the results of every batch submitted so far"""
        self._check(lib().groot_hip_stream_join(self._h, C.c_void_p(hip_stream)))

    def redo_status(self):
        """(device address of the newest batch's status word, mask of its bits that mean `collect will redo the batch`)"""
        p, m = C.c_void_p(), C.c_uint32()
        self._check(lib().groot_hip_redo_status(self._h, C.byref(p), C.byref(m)))
        return p.value, m.value

    def set_profiling(self, on=True):
        self._check(lib().groot_hip_set_profiling(self._h, C.c_int(1 if on else 0)))

    def submit(self, seq_concat, seq_off, first_read_id=0):
        seq = np.ascontiguousarray(seq_concat, dtype=np.uint8)
        off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        self._keep = (seq, off)
        self._check(lib().groot_hip_submit(self._h, _ffi.as_ptr(seq, C.c_uint8), _ffi.as_ptr(off, C.c_uint64),
                                           C.c_uint32(len(off) - 1), C.c_uint32(first_read_id)))

    def submit_packed(self, packed, seq_off, exc_pos, exc_byte, first_read_id=0):
        """groot_hip_submit_packed: the arguments host.pack_reads() builds from seq_concat"""
        pk = np.ascontiguousarray(packed, dtype=np.uint8)
        off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        ep = np.ascontiguousarray(exc_pos, dtype=np.uint64)
        eb = np.ascontiguousarray(exc_byte, dtype=np.uint8)
        self._keep = (pk, off, ep, eb)
        self._check(lib().groot_hip_submit_packed(self._h, _ffi.as_ptr(pk, C.c_uint8), _ffi.as_ptr(off, C.c_uint64), C.c_uint32(len(off) - 1),
                                                  C.c_uint32(first_read_id), _ffi.as_ptr(ep, C.c_uint64), _ffi.as_ptr(eb, C.c_uint8),
                                                  C.c_uint64(len(ep))))

    def submit_packed16(self, packed, seq_len, exc_pos, exc_byte, first_read_id=0):
        """groot_hip_submit_packed16: 2-bit bases + one u16 length per read + exception list (the wire format)"""
        pk = np.ascontiguousarray(packed, dtype=np.uint8)
        ln = np.ascontiguousarray(seq_len, dtype=np.uint16)
        ep = np.ascontiguousarray(exc_pos, dtype=np.uint64)
        eb = np.ascontiguousarray(exc_byte, dtype=np.uint8)
        self._check(lib().groot_hip_submit_packed16(self._h, _ffi.as_ptr(pk, C.c_uint8), _ffi.as_ptr(ln, C.c_uint16), C.c_uint32(len(ln)),
                                                    C.c_uint32(first_read_id), _ffi.as_ptr(ep, C.c_uint64), _ffi.as_ptr(eb, C.c_uint8),
                                                    C.c_uint64(len(ep))))

    def acquire(self):
        """groot_hip_acquire: numpy views of a free slot's pinned staging (packed, seq_len, exc_pos, exc_byte) + ticket"""
        b = BatchBuffers()
        self._check(lib().groot_hip_acquire(self._h, C.byref(b)))
        views = {"ticket": int(b.ticket),
                 "packed": _ffi._np_view(b.packed, b.packed_cap, np.uint8), "seq_len": _ffi._np_view(b.seq_len, b.reads_cap, np.uint16),
                 "exc_pos": _ffi._np_view(b.exc_pos, b.exc_cap, np.uint64), "exc_byte": _ffi._np_view(b.exc_byte, b.exc_cap, np.uint8)}
        return views

    def submit_acquired(self, ticket, n_reads, n_exc=0, first_read_id=0):
        self._check(lib().groot_hip_submit_acquired(self._h, C.c_uint64(ticket), C.c_uint32(n_reads), C.c_uint64(n_exc), C.c_uint32(first_read_id)))

    def collect(self, check=True, copy=True):
        """groot_hip_collect: blocks for the oldest batch.  Returns a dict with counts, ticket, status and the traversal
        records (copies by default; copy=False gives views of the ctx's pinned memory, valid until release(ticket))."""
        r = BatchResult()
        rc = lib().groot_hip_collect(self._h, C.byref(r))
        if rc < 0 and (check or not r.ticket):
            self._check(rc)
        n = int(r.n_travs)
        if r.travs and n:
            t = _ffi._np_view(C.cast(r.travs, C.POINTER(C.c_uint8)), n * TRAV_DTYPE.itemsize, np.uint8).view(TRAV_DTYPE)
            if copy:
                # the compact path sets widened to path_words words per traversal (groot_host_unpack_masks)
                m = np.zeros((n, r.path_words), dtype=np.uint64)
                host._check(host.lib().groot_host_unpack_masks(C.byref(self.index.view), C.c_void_p(r.travs), C.c_uint64(n), C.c_void_p(r.masks),
                                                               _ffi.as_ptr(m, C.c_uint64)))
                t = t.copy()
            else:
                m = _ffi._np_view(C.cast(r.masks, C.POINTER(C.c_uint8)), int(r.n_mask_bytes), np.uint8)   # compact (bytes), as handed out
        else:
            t, m = np.zeros(0, dtype=TRAV_DTYPE), np.zeros((0, self.path_words), dtype=np.uint64)
        return {"ticket": int(r.ticket), "first_read_id": int(r.first_read_id), "n_reads": int(r.n_reads), "counts": r.counts.as_dict(),
                "status": int(r.status), "n_travs": n, "travs": t, "masks": m, "n_mask_bytes": int(r.n_mask_bytes), "d_travs": r.d_travs,
                "d_masks": r.d_masks,
                "ms": {k: float(getattr(r.ms, k)) for k, _ in StageMs._fields_}}

    def release(self, ticket):
        self._check(lib().groot_hip_release(self._h, C.c_uint64(ticket)))

    def in_flight(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._check(lib().groot_hip_in_flight(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def submit_device(self, d_seq_ptr, d_off_ptr, n_reads, first_read_id=0, max_len=0, mixed=False):
        if mixed:
            max_len |= 0x80000000      # GROOT_MAXLEN_MIXED
        self._check(lib().groot_hip_submit_device(self._h, C.c_void_p(d_seq_ptr), C.c_void_p(d_off_ptr), C.c_uint32(n_reads),
                                                  C.c_uint32(first_read_id), C.c_uint32(max_len)))

    def wait(self, check=True):
        c = Counts()
        rc = lib().groot_hip_wait(self._h, C.byref(c))
        self.last_rc = rc
        if check:
            self._check(rc)
        return c.as_dict()

    def seeds(self):
        n = C.c_uint64(0)
        self._check(lib().groot_hip_read_seeds(self._h, None, C.c_uint64(0), C.byref(n)))
        out = np.zeros(n.value, dtype=SEED_DTYPE)
        self._check(lib().groot_hip_read_seeds(self._h, out.ctypes.data_as(C.c_void_p), C.c_uint64(len(out)), C.byref(n)))
        return out

    def travs(self):
        n = C.c_uint64(0)
        self._check(lib().groot_hip_read_travs(self._h, None, None, C.c_uint64(0), C.byref(n)))
        t = np.zeros(n.value, dtype=TRAV_DTYPE)
        m = np.zeros((n.value, self.path_words), dtype=np.uint64)
        self._check(lib().groot_hip_read_travs(self._h, t.ctypes.data_as(C.c_void_p), _ffi.as_ptr(m, C.c_uint64),
                                               C.c_uint64(len(t)), C.byref(n)))
        return t, m

    def alns(self):
        t, m = self.travs()
        return expand_alns(self.index, t, m)

    def sketches(self):
        n = C.c_uint64(0)
        self._check(lib().groot_hip_read_sketches(self._h, None, C.c_uint64(0), C.byref(n)))
        out = np.zeros((n.value, self.s), dtype=np.uint64)
        self._check(lib().groot_hip_read_sketches(self._h, _ffi.as_ptr(out, C.c_uint64), C.c_uint64(n.value), C.byref(n)))
        return out

    def stage_ms(self):
        m = StageMs()
        self._check(lib().groot_hip_stage_ms(self._h, C.byref(m)))
        return {n: float(getattr(m, n)) for n, _ in StageMs._fields_}

    def path_pass_stats(self):
        """the waited batch's first pass against path text: {"ran": bool, "reads": reads it finished, "ms": its time (profiling on, else 0)}"""
        ran, reads, ms = C.c_uint32(), C.c_uint64(), C.c_float()
        self._check(lib().groot_hip_path_pass_stats(self._h, C.byref(ran), C.byref(reads), C.byref(ms)))
        return {"ran": bool(ran.value), "reads": int(reads.value), "ms": float(ms.value)}

    # ---- weights ------------------------------------------------------------------------------
    def attempts_shape(self):
        nq, nw = C.c_uint32(), C.c_uint32()
        self._check(lib().groot_hip_attempts_shape(self._h, C.byref(nq), C.byref(nw)))
        return nq.value, nw.value

    def attempts_device(self):
        """(device pointer of the [rows][n_windows] uint32 call-count table, rows, n_windows)"""
        p, nr, nw = C.c_void_p(), C.c_uint32(), C.c_uint32()
        self._check(lib().groot_hip_attempts_device(self._h, C.byref(p), C.byref(nr), C.byref(nw)))
        return p.value, nr.value, nw.value

    def attempts(self):
        """dense compatibility view [max_read_len-k+2][n_windows] (rows of kmerCounts that never occurred are zero)"""
        nq, nw = self.attempts_shape()
        out = np.zeros((nq, nw), dtype=np.uint32)
        self._check(lib().groot_hip_attempts_read(self._h, _ffi.as_ptr(out, C.c_uint32), C.c_uint64(out.size)))
        return out

    def attempts_rows(self):
        """groot_hip_attempts_export: (kmerCounts ascending, counts[rows][n_windows])"""
        nr, nw = C.c_uint32(), C.c_uint32()
        self._check(lib().groot_hip_attempts_export(self._h, None, None, C.c_uint32(0), C.byref(nr), C.byref(nw)))
        q = np.zeros(nr.value, dtype=np.uint32)
        cnt = np.zeros((nr.value, nw.value), dtype=np.uint32)
        self._check(lib().groot_hip_attempts_export(self._h, _ffi.as_ptr(q, C.c_uint32), _ffi.as_ptr(cnt, C.c_uint32), C.c_uint32(nr.value),
                                                    C.byref(nr), C.byref(nw)))
        return q, cnt

    def attempts_import(self, q_values, counts):
        """groot_hip_attempts_import: add exported rows back (a re-opened ctx carries its counts over)"""
        q = np.ascontiguousarray(q_values, dtype=np.uint32)
        cnt = np.ascontiguousarray(counts, dtype=np.uint32)
        self._check(lib().groot_hip_attempts_import(self._h, _ffi.as_ptr(q, C.c_uint32), _ffi.as_ptr(cnt, C.c_uint32), C.c_uint32(len(q))))

    def attempts_layout(self, q_values, d_table=None):
        """groot_hip_attempts_layout: fix the rows (ascending kmerCounts); d_table = caller-owned device buffer or None"""
        q = np.ascontiguousarray(q_values, dtype=np.uint32)
        self._check(lib().groot_hip_attempts_layout(self._h, _ffi.as_ptr(q, C.c_uint32), C.c_uint32(len(q)), C.c_void_p(d_table or 0)))

    def attempts_reset(self):
        self._check(lib().groot_hip_attempts_reset(self._h))

    # ---- report coverage (groot_hip_coverage_*) ------------------------------------------------
    def coverage_enable(self, on=True):
        """count records and pileups of every batch from now on (only while nothing is in flight)"""
        self._check(lib().groot_hip_coverage_enable(self._h, C.c_int(1 if on else 0)))

    def coverage(self):
        """(records[n_paths], depth[sum of path_len]) as uint64 over every batch since enable / reset: the inputs of
        host.report_coverage.  Waits for everything in flight."""
        v = self.index.view
        records = np.zeros(v.n_paths, dtype=np.uint64)
        depth = np.zeros(int(self.index.arrays["path_len"].astype(np.uint64).sum()), dtype=np.uint64)
        self._check(lib().groot_hip_coverage_export(self._h, _ffi.as_ptr(records, C.c_uint64), _ffi.as_ptr(depth, C.c_uint64)))
        return records, depth

    def coverage_reset(self):
        self._check(lib().groot_hip_coverage_reset(self._h))

    # ---- shared reads (groot_hip_shared_*) --------------------------------------------------------
    def shared_enable(self, on=True):
        """count, for every pair of paths a <= b, the reads with records on both, from now on (only while nothing is in flight)"""
        self._check(lib().groot_hip_shared_enable(self._h, C.c_int(1 if on else 0)))

    def shared(self):
        """(a, b, count) of every nonzero pair since enable / reset, ascending by (a, b): uint32, uint32, uint64 arrays; the pair
        input of host.shared_from_counts.  Waits for everything in flight."""
        n = C.c_uint64(0)
        self._check(lib().groot_hip_shared_export(self._h, None, None, None, C.c_uint64(0), C.byref(n)))
        a = np.zeros(n.value, dtype=np.uint32)
        b = np.zeros(n.value, dtype=np.uint32)
        cnt = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            m = C.c_uint64(0)
            self._check(lib().groot_hip_shared_export(self._h, _ffi.as_ptr(a, C.c_uint32), _ffi.as_ptr(b, C.c_uint32), _ffi.as_ptr(cnt, C.c_uint64),
                                                      C.c_uint64(n.value), C.byref(m)))
            assert m.value == n.value
        return a, b, cnt

    def shared_stats(self):
        """{"reads", "distinct_sets", "slow_reads"} since enable / reset (groot_hip_shared_stats)"""
        v = [C.c_uint64(0) for _ in range(3)]
        self._check(lib().groot_hip_shared_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("reads", "distinct_sets", "slow_reads"), (x.value for x in v)))

    def shared_reset(self):
        self._check(lib().groot_hip_shared_reset(self._h))

    # ---- equivalence classes (groot_hip_ec_*) -----------------------------------------------------
    def ec_enable(self, on=True):
        """count the reads of every distinct S(r) (equivalence class) from now on (only while nothing is in flight)"""
        self._check(lib().groot_hip_ec_enable(self._h, C.c_int(1 if on else 0)))

    def ecs(self):
        """(off uint64[n_ec + 1], ids uint32, count uint64[n_ec]) of every EC since enable / reset in canonical order (lexicographic
        on the ascending path-ID lists), EC i = ids[off[i]:off[i + 1]]: the input of host.abundance_from_ecs.  Waits for everything
        in flight."""
        ne, ni = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().groot_hip_ec_export(self._h, None, None, None, C.c_uint64(0), C.c_uint64(0), C.byref(ne), C.byref(ni)))
        off = np.zeros(ne.value + 1, dtype=np.uint64)
        ids = np.zeros(ni.value, dtype=np.uint32)
        cnt = np.zeros(ne.value, dtype=np.uint64)
        if ne.value:
            me, mi = C.c_uint64(0), C.c_uint64(0)
            self._check(lib().groot_hip_ec_export(self._h, _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32), _ffi.as_ptr(cnt, C.c_uint64),
                                                  C.c_uint64(ne.value), C.c_uint64(ni.value), C.byref(me), C.byref(mi)))
            assert (me.value, mi.value) == (ne.value, ni.value)
        return off, ids, cnt

    def ec_stats(self):
        """{"reads", "distinct", "slow_reads", "grows"} since enable / reset (groot_hip_ec_stats)"""
        v = [C.c_uint64(0) for _ in range(4)]
        self._check(lib().groot_hip_ec_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("reads", "distinct", "slow_reads", "grows"), (x.value for x in v)))

    def ec_reset(self):
        self._check(lib().groot_hip_ec_reset(self._h))

    # ---- assigned coverage (groot_hip_acov_*) ------------------------------------------------------
    def acov_enable(self, on=True):
        """group every record by (EC of its read, path, Pos, last) from now on (include/groot_hip.h, "assigned coverage"); switches
        equivalence classes on.  Only while nothing is in flight."""
        self._check(lib().groot_hip_acov_enable(self._h, C.c_int(1 if on else 0)))

    def acov(self):
        """(off, ids, count, tuples uint32[n, 4], n uint64[n]): the ctx's ECs as ecs() gives them and the assigned-coverage table,
        tuple = (EC index, path, Pos, last), ascending: the input of host.acov_merge / host.calls_from_table"""
        ne, ni, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        z = C.c_uint64(0)
        self._check(lib().groot_hip_acov_export(self._h, None, None, None, None, None, z, z, z, C.byref(ne), C.byref(ni), C.byref(nt)))
        off = np.zeros(ne.value + 1, dtype=np.uint64)
        ids = np.zeros(max(ni.value, 1), dtype=np.uint32)
        cnt = np.zeros(max(ne.value, 1), dtype=np.uint64)
        tup = np.zeros((max(nt.value, 1), 4), dtype=np.uint32)
        tn = np.zeros(max(nt.value, 1), dtype=np.uint64)
        if ne.value or nt.value:
            me, mi, mt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            self._check(lib().groot_hip_acov_export(self._h, _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32), _ffi.as_ptr(cnt, C.c_uint64),
                                                    _ffi.as_ptr(tup, C.c_uint32), _ffi.as_ptr(tn, C.c_uint64), C.c_uint64(ne.value), C.c_uint64(ni.value),
                                                    C.c_uint64(nt.value), C.byref(me), C.byref(mi), C.byref(mt)))
            assert (me.value, mi.value, mt.value) == (ne.value, ni.value, nt.value)
        return off, ids[:ni.value], cnt[:ne.value], tup[:nt.value], tn[:nt.value]

    def acov_stats(self):
        """{"records", "tuples", "slots", "grows", "slow_records", "launches"} (groot_hip_acov_stats); zeros while off, but for launches"""
        v = [C.c_uint64(0) for _ in range(6)]
        self._check(lib().groot_hip_acov_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("records", "tuples", "slots", "grows", "slow_records", "launches"), (x.value for x in v)))

    def acov_reset(self):
        self._check(lib().groot_hip_acov_reset(self._h))

    # ---- assignment (groot_hip_assign_*) -------------------------------------------------------------
    def assign_enable(self, alpha, min_posterior=0.0):
        """every batch from now on keeps, per read, only the records on the path of S(r) with the largest alpha (include/groot_hip.h,
        "assignment"); alpha None switches it off.  Only while nothing is in flight."""
        if alpha is None:
            self._check(lib().groot_hip_assign_enable(self._h, None, C.c_uint32(0), C.c_double(0.0)))
            return
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        self._check(lib().groot_hip_assign_enable(self._h, _ffi.as_ptr(a, C.c_double), C.c_uint32(len(a)), C.c_double(min_posterior)))

    def assign_batch(self, n_reads, ticket=0):
        """(best uint32[n_reads], mapq uint8[n_reads]) of a collected, unreleased batch, copied (ticket 0: the batch wait() collected)"""
        b, q = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        self._check(lib().groot_hip_assign_batch(self._h, C.c_uint64(ticket), C.byref(b), C.byref(q)))
        if not n_reads:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
        return _ffi._np_view(b, n_reads, np.uint32).copy(), _ffi._np_view(q, n_reads, np.uint8).copy()

    def assign_stats(self):
        """groot_hip_assign_stats: {"reads", "assigned", "unassigned", "below", "ties", "records_in", "records_kept", "travs_emptied",
        "launches"}; zeros while off, but for launches"""
        st = host.AssignStats()
        self._check(lib().groot_hip_assign_stats(self._h, C.byref(st)))
        return st.as_dict()

    def assign_reset(self):
        self._check(lib().groot_hip_assign_reset(self._h))

    # ---- paired-end reads (groot_hip_pairs_*) ------------------------------------------------------
    def pairs_enable(self, on=True):
        """reads 2i and 2i+1 of every batch are the mates of one fragment: shared reads and equivalence classes count units
        (include/groot_hip.h, "paired-end reads").  Only while nothing is in flight; a batch of an odd number of reads is then refused."""
        self._check(lib().groot_hip_pairs_enable(self._h, C.c_int(1 if on else 0)))

    def pairs_stats(self):
        """{"joined", "split", "single"} fragments since enable / reset (groot_hip_pairs_stats)"""
        v = [C.c_uint64(0) for _ in range(3)]
        self._check(lib().groot_hip_pairs_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("joined", "split", "single"), (x.value for x in v)))

    # ---- mismatch rescue of unaligned reads (groot_hip_rescue_*) ------------------------------------
    def rescue_enable(self, max_mismatch=2):
        """from now on, lay every read without a record on the path texts with up to max_mismatch (1..3) substitutions and pile up
        where it lies and what differs (include/groot_hip.h, "mismatch rescue"); 0 switches it off.  Only while nothing is in flight."""
        self._check(lib().groot_hip_rescue_enable(self._h, C.byref(self.index.view), C.c_uint32(max_mismatch)))

    def rescue(self):
        """(depth[sum of path_len], alt[sum of path_len, 4]) as uint64 over every batch since enable / reset: rescued depth and the
        A, C, G, T counts of the mismatching bases, per path base.  Waits for everything in flight."""
        n = int(self.index.arrays["path_len"].astype(np.uint64).sum())
        depth, alt = np.zeros(n, dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        self._check(lib().groot_hip_rescue_export(self._h, _ffi.as_ptr(depth, C.c_uint64), _ffi.as_ptr(alt, C.c_uint64)))
        return depth, alt

    def rescue_stats(self):
        """groot_hip_rescue_stats: {"candidates", "rescued", "exact", "placements", "too_short", "non_acgt", "text_paths", "launches"};
        zeros while off, but for launches"""
        v = (C.c_uint64 * 8)()
        self._check(lib().groot_hip_rescue_stats(self._h, v))
        return dict(zip(("candidates", "rescued", "exact", "placements", "too_short", "non_acgt", "text_paths", "launches"), (int(x) for x in v)))

    def rescue_reset(self):
        self._check(lib().groot_hip_rescue_reset(self._h))

    # ---- gapped rescue of the reads mismatch rescue leaves (groot_hip_gap_*) --------------------------
    def gap_enable(self, max_gap=3, event_slots=0):
        """reads that mismatch rescue leaves unplaced are laid on the path texts with one gap of up to `max_gap` bases (include/groot_hip.h,
        "gapped rescue"); 0 switches it off.  Needs rescue_enable first.  event_slots: a power of two, 0 for the default of 2^22."""
        self._check(lib().groot_hip_gap_enable(self._h, C.c_uint32(max_gap), C.c_uint64(event_slots)))

    def gap(self):
        """(gdepth[sum of path_len] as uint64, events as GAP_EVENT_DTYPE ascending by (path, pos, type, len, seq)) over every batch
        since enable / reset"""
        gdepth = np.zeros(int(self.index.arrays["path_len"].astype(np.int64).sum()), dtype=np.uint64)
        n = C.c_uint64(0)
        cap = int(self.gap_stats()["events"])
        events = np.zeros(cap, dtype=GAP_EVENT_DTYPE)
        self._check(lib().groot_hip_gap_export(self._h, _ffi.as_ptr(gdepth, C.c_uint64), events.ctypes.data_as(C.c_void_p), C.c_uint64(cap), C.byref(n)))
        return gdepth, events[:n.value]

    def gap_stats(self):
        """groot_hip_gap_stats: {"candidates", "rescued", "placements", "del_placements", "ins_placements", "too_short", "events", "dropped",
        "event_slots", "launches"}"""
        v = (C.c_uint64 * 10)()
        self._check(lib().groot_hip_gap_stats(self._h, v))
        return dict(zip(GAP_STATS, (int(x) for x in v)))

    def gap_reset(self):
        self._check(lib().groot_hip_gap_reset(self._h))

    # ---- rescued reads in the equivalence classes (groot_hip_rescue_ec_*) -----------------------------
    def rescue_ec_enable(self, on=True):
        """from now on a rescued read counts in the equivalence classes with the set of paths it was placed on (include/groot_hip.h,
        "rescued reads in the equivalence classes").  Needs rescue_enable and ec_enable first.  Only while nothing is in flight."""
        self._check(lib().groot_hip_rescue_ec_enable(self._h, C.c_int(1 if on else 0)))

    def rescue_ec_stats(self):
        """groot_hip_rescue_ec_stats: {"reads", "slow_reads", "rows", "launches"}; zeros while off, but for launches"""
        v = (C.c_uint64 * 4)()
        self._check(lib().groot_hip_rescue_ec_stats(self._h, v))
        return dict(zip(("reads", "slow_reads", "rows", "launches"), (int(x) for x in v)))

    # ---- rescued reads in assigned coverage (groot_hip_rescue_acov_*) -----------------------------------
    def rescue_acov_enable(self, on=True, min_slots=0):
        """from now on every kept placement of a rescued read is a record of the assigned-coverage table (include/groot_hip.h, "rescued
        reads in assigned coverage").  Needs rescue_enable, ec_enable and acov_enable first and switches the rescued reads in the classes on
        itself.  min_slots: 0 or a power of two, the table's slots at least.  Only while nothing is in flight."""
        self._check(lib().groot_hip_rescue_acov_enable(self._h, C.c_int(1 if on else 0), C.c_uint64(min_slots)))

    def rescue_acov_stats(self):
        """groot_hip_rescue_acov_stats: {"records", "host_records", "dropped", "log_rows", "launches"}; zeros while off, but for launches"""
        v = (C.c_uint64 * 5)()
        self._check(lib().groot_hip_rescue_acov_stats(self._h, v))
        return dict(zip(("records", "host_records", "dropped", "log_rows", "launches"), (int(x) for x in v)))

    # ---- rescued records (groot_hip_rescue_rec_*) -------------------------------------------------------
    def rescue_rec_enable(self, slots_per_batch):
        """from now on every batch hands out one record per kept placement of its rescued reads (include/groot_hip.h, "rescued records"),
        with room for slots_per_batch of them per batch; 0 switches it off.  Needs rescue_enable first.  Only while nothing is in flight."""
        self._check(lib().groot_hip_rescue_rec_enable(self._h, C.c_uint64(slots_per_batch)))

    def rescue_records(self, ticket=0):
        """the rescued records of a collected, unreleased batch as RESCUE_RECORD_DTYPE, copied, in ascending (read, path, strand, pos)
        order (ticket 0: the batch wait() collected)"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self._check(lib().groot_hip_rescue_rec_batch(self._h, C.c_uint64(ticket), C.byref(p), C.byref(n)))
        if not n.value:
            return np.zeros(0, dtype=RESCUE_RECORD_DTYPE)
        buf = (C.c_uint8 * (n.value * RESCUE_RECORD_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=RESCUE_RECORD_DTYPE).copy()

    def rescue_rec_stats(self):
        """groot_hip_rescue_rec_stats: {"records", "reads", "failed", "slots", "launches"}; zeros while off, but for launches"""
        v = (C.c_uint64 * 5)()
        self._check(lib().groot_hip_rescue_rec_stats(self._h, v))
        return dict(zip(("records", "reads", "failed", "slots", "launches"), (int(x) for x in v)))

    # ---- gapped records (groot_hip_gap_rec_*) --------------------------------------------------------------
    def gap_rec_enable(self, slots_per_batch):
        """from now on every batch hands out one record per kept gapped placement of its gap-rescued reads (include/groot_hip.h, "gapped
        records"), with room for slots_per_batch of them per batch; 0 switches it off.  Needs gap_enable first.  Only while nothing is in flight."""
        self._check(lib().groot_hip_gap_rec_enable(self._h, C.c_uint64(slots_per_batch)))

    def gap_records(self, ticket=0):
        """the gapped records of a collected, unreleased batch as GAP_RECORD_DTYPE, copied, in ascending (read, path, strand, pos, type, g)
        order (ticket 0: the batch wait() collected)"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self._check(lib().groot_hip_gap_rec_batch(self._h, C.c_uint64(ticket), C.byref(p), C.byref(n)))
        if not n.value:
            return np.zeros(0, dtype=GAP_RECORD_DTYPE)
        buf = (C.c_uint8 * (n.value * GAP_RECORD_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=GAP_RECORD_DTYPE).copy()

    def gap_rec_stats(self):
        """groot_hip_gap_rec_stats: {"records", "reads", "failed", "slots", "launches"}; zeros while off, but for launches"""
        v = (C.c_uint64 * 5)()
        self._check(lib().groot_hip_gap_rec_stats(self._h, v))
        return dict(zip(("records", "reads", "failed", "slots", "launches"), (int(x) for x in v)))

    # ---- gap-placed reads in the equivalence classes (groot_hip_gap_ec_*) ---------------------------------
    def gap_ec_enable(self, on=True):
        """from now on a gap-rescued read counts in the equivalence classes with the set of paths it was gap-placed on (include/groot_hip.h,
        "gap-placed reads in the equivalence classes").  Needs gap_enable and rescue_ec_enable first.  Only while nothing is in flight."""
        self._check(lib().groot_hip_gap_ec_enable(self._h, C.c_int(1 if on else 0)))

    def gap_ec_stats(self):
        """groot_hip_gap_ec_stats: {"reads", "slow_reads", "launches"}; zeros while off, but for launches"""
        v = (C.c_uint64 * len(_ffi.GAP_EC_STATS))()
        self._check(lib().groot_hip_gap_ec_stats(self._h, v))
        return dict(zip(_ffi.GAP_EC_STATS, (int(x) for x in v)))

    # ---- gap-placed reads in assigned coverage (groot_hip_gap_acov_*) --------------------------------------
    def gap_acov_enable(self, on=True):
        """from now on every kept gapped placement of a gap-rescued read is piled up in assigned coverage: two records for a DEL, one for
        an INS (include/groot_hip.h, "gap-placed reads in assigned coverage").  Needs gap_enable and rescue_acov_enable first, and switches
        the gap-placed reads in the classes on itself; off switches both off.  Only while nothing is in flight."""
        self._check(lib().groot_hip_gap_acov_enable(self._h, C.c_int(1 if on else 0)))

    def gap_acov_stats(self):
        """groot_hip_gap_acov_stats: {"placements", "records", "host_records", "dropped", "launches"}; zeros while off, but for launches"""
        v = (C.c_uint64 * len(_ffi.GAP_ACOV_STATS))()
        self._check(lib().groot_hip_gap_acov_stats(self._h, v))
        return dict(zip(_ffi.GAP_ACOV_STATS, (int(x) for x in v)))

    # ---- assigned coverage over fragments (groot_hip_acov_pairs_*) ------------------------------------------
    def acov_pairs_enable(self, on=True):
        """assigned coverage with paired-end units: switches on whichever of equivalence classes, assigned coverage and pairing is off,
        and the rule that a record of a joined fragment counts on the paths of the fragment's set only (include/groot_hip.h, "assigned
        coverage over fragments").  Off: the rule and assigned coverage go, equivalence classes and pairing stay.  Only while nothing is
        in flight."""
        self._check(lib().groot_hip_acov_pairs_enable(self._h, C.c_int(1 if on else 0)))

    def acov_pairs_stats(self):
        """groot_hip_acov_pairs_stats: {"records", "left_out", "joined_reads", "slow_fragments"}; zeros while off"""
        v = (C.c_uint64 * len(_ffi.ACOV_PAIRS_STATS))()
        self._check(lib().groot_hip_acov_pairs_stats(self._h, v))
        return dict(zip(_ffi.ACOV_PAIRS_STATS, (int(x) for x in v)))

    # ---- rescued mates in paired-end units (groot_hip_rescue_pairs_*) ----------------------------------------
    def rescue_pairs_enable(self, on=True):
        """pairing with the rescued reads in the classes: switches on whichever of equivalence classes, pairing and the rescued reads in the
        classes is off, and the rule that a fragment's unit is made of each mate's records or, for a mate mismatch rescue places, of its
        rescued set (include/groot_hip.h, "rescued mates in paired-end units").  Needs rescue_enable first.  Off: the rule and the rescued
        classes go, equivalence classes and pairing stay.  Only while nothing is in flight."""
        self._check(lib().groot_hip_rescue_pairs_enable(self._h, C.c_int(1 if on else 0)))

    def rescue_pairs_stats(self):
        """groot_hip_rescue_pairs_stats: _ffi.RESCUE_PAIRS_STATS as a dict; zeros while off, but for launches"""
        v = (C.c_uint64 * len(_ffi.RESCUE_PAIRS_STATS))()
        self._check(lib().groot_hip_rescue_pairs_stats(self._h, v))
        return dict(zip(_ffi.RESCUE_PAIRS_STATS, (int(x) for x in v)))

    # ---- rescued mates in assigned coverage over fragments (groot_hip_rescue_acov_pairs_*) -----------------
    def rescue_acov_pairs_enable(self, on=True, min_slots=0):
        """the pileup of --calls over fragments with rescued mates: switches on whichever of the classes, pairing, the rescued classes, the
        rescued mates' rule, assigned coverage and its rule over fragments is off, and the rule that a record or a kept placement of a mate
        counts on the paths of the mate's unit (include/groot_hip.h, "rescued mates in assigned coverage over fragments").  Needs
        rescue_enable first.  min_slots: 0 or a power of two, the table's slots at least.  Off: the rule and assigned coverage go; the
        classes, pairing and the rescued mates' rule stay.  Only while nothing is in flight."""
        self._check(lib().groot_hip_rescue_acov_pairs_enable(self._h, C.c_int(1 if on else 0), C.c_uint64(min_slots)))

    def rescue_acov_pairs_stats(self):
        """groot_hip_rescue_acov_pairs_stats: _ffi.RESCUE_ACOV_PAIRS_STATS as a dict; zeros while off, but for launches"""
        v = (C.c_uint64 * len(_ffi.RESCUE_ACOV_PAIRS_STATS))()
        self._check(lib().groot_hip_rescue_acov_pairs_stats(self._h, v))
        return dict(zip(_ffi.RESCUE_ACOV_PAIRS_STATS, (int(x) for x in v)))

    # ---- fine-grained mirror of Sequence.RunMinHash ------------------------------------------
    def sketch(self, seq_concat, seq_off):
        seq = np.ascontiguousarray(seq_concat, dtype=np.uint8)
        off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        out = np.zeros((len(off) - 1, self.s), dtype=np.uint64)
        self._check(lib().groot_hip_sketch(self._h, _ffi.as_ptr(seq, C.c_uint8), _ffi.as_ptr(off, C.c_uint64),
                                           C.c_uint32(len(off) - 1), _ffi.as_ptr(out, C.c_uint64)))
        return out


def attempts_allreduce(aligners):
    """groot_hip_attempts_allreduce over the ctxs of one process: RCCL across devices, a kernel within a device"""
    arr = (C.c_void_p * len(aligners))(*[a._h for a in aligners])
    rc = lib().groot_hip_attempts_allreduce(arr, C.c_int(len(aligners)))
    aligners[0]._check(rc)


def weights_rows(index, q_values, counts):
    """groot_host_weights_rows: canonical replay of IncrementSubPath from the per-kmerCount rows of the call-count table"""
    q = np.ascontiguousarray(q_values, dtype=np.uint32)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    v = index.view
    kf = np.zeros(v.n_nodes, dtype=np.float64)
    kt = np.zeros(v.n_graphs, dtype=np.uint64)
    host._check(host.lib().groot_host_weights_rows(C.byref(v), _ffi.as_ptr(q, C.c_uint32), C.c_uint32(len(q)), _ffi.as_ptr(cnt, C.c_uint32),
                                                   _ffi.as_ptr(kf, C.c_double), _ffi.as_ptr(kt, C.c_uint64)))
    return kf, kt


def weights(index, attempts):
    """groot_host_weights: canonical replay of IncrementSubPath from the call counts."""
    att = np.ascontiguousarray(attempts, dtype=np.uint32)
    v = index.view
    kf = np.zeros(v.n_nodes, dtype=np.float64)
    kt = np.zeros(v.n_graphs, dtype=np.uint64)
    host._check(host.lib().groot_host_weights(C.byref(v), _ffi.as_ptr(att, C.c_uint32), C.c_uint32(att.shape[0]),
                                              _ffi.as_ptr(kf, C.c_double), _ffi.as_ptr(kt, C.c_uint64)))
    return kf, kt


def prune(index, kmer_freq, min_cov=1.0):
    v = index.view
    gk = np.zeros(v.n_graphs, dtype=np.uint8)
    pk = np.zeros(v.n_paths, dtype=np.uint8)
    nr = np.zeros(v.n_nodes, dtype=np.uint8)
    kf = np.ascontiguousarray(kmer_freq, dtype=np.float64)
    host._check(host.lib().groot_host_prune(C.byref(v), _ffi.as_ptr(kf, C.c_double), C.c_double(min_cov), _ffi.as_ptr(gk, C.c_uint8),
                                            _ffi.as_ptr(pk, C.c_uint8), _ffi.as_ptr(nr, C.c_uint8)))
    return gk, pk, nr
