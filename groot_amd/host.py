"""Python mirror of libgroot_host.so (include/groot_host.h): index build/load/save and the
host steps either side of the device path.  Names follow the reference's packages
(src/pipeline/index.go, src/graph, src/lshe)."""
import ctypes as C
import glob
import os

import numpy as np

from . import _ffi
from ._ffi import IndexParams, IndexView


class GrootError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = _ffi.lib_path("libgroot_host.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'` first")
        L = C.CDLL(path)
        L.groot_host_last_error.restype = C.c_char_p
        L.groot_host_version.restype = C.c_char_p
        L.groot_index_free.argtypes = [C.c_void_p]
        L.groot_index_free.restype = None
        L.groot_index_get_view.argtypes = [C.c_void_p, C.POINTER(IndexView)]
        L.groot_index_get_view.restype = None
        _ffi.rarefy_host_prototypes(L)
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise GrootError(rc, lib().groot_host_last_error().decode(errors="replace"))
    return rc


def index_cache_path(stem):
    """build/<stem>.<key>.gidx, key = hash of the index-builder sources and the view layout: a cached index never
    outlives the code that built it (windowing / merge quirks / file format)."""
    import hashlib

    h = hashlib.sha1()
    for rel in ("groot_amd/csrc/host/index.cpp", "groot_amd/csrc/host/host_common.hpp", "include/groot_index.h"):
        with open(os.path.join(_ffi.REPO, rel), "rb") as f:
            h.update(f.read())
    return os.path.join(_ffi.BUILD_DIR, f"{stem}.{h.hexdigest()[:12]}.gidx")


def index_params(k=31, s=21, w=100, x=8, y=4, max_sketch_span=30, threads=0):
    """defaults of `groot index` (cmd/index.go:45-50)"""
    return IndexParams(k, s, w, x, y, max_sketch_span, threads, 0)


class Index:
    """Owns a groot_index handle; .view is the groot_index_view, .arrays numpy views of it."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        self.view = IndexView()
        lib().groot_index_get_view(self._h, C.byref(self.view))
        self.arrays = _ffi.view_arrays(self.view)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.groot_index_free(self._h)
            self._h = None

    # ---- constructors -------------------------------------------------------------------
    @staticmethod
    def _build(fn, files, params):
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        out = C.c_void_p()
        _check(fn(arr, C.c_uint32(len(files)), C.byref(params), C.byref(out)))
        return Index(out.value)

    @classmethod
    def from_msa_files(cls, files, params=None):
        return cls._build(lib().groot_index_build_msa_files, list(files), params or index_params())

    @classmethod
    def from_gfa_files(cls, files, params=None):
        return cls._build(lib().groot_index_build_gfa_files, list(files), params or index_params())

    @classmethod
    def from_msa_dir(cls, msa_dir, params=None, sketcher=None):
        """sketcher: optional callable (seq_concat uint8[], seq_off uint64[n+1]) -> uint64[n, s] that computes
        the window sketches (e.g. device.Aligner.sketch): groot_index_build_msa_dir_with"""
        out = C.c_void_p()
        p = params or index_params()
        if sketcher is None:
            _check(lib().groot_index_build_msa_dir(msa_dir.encode(), C.byref(p), C.byref(out)))
            return cls(out.value)
        s = p.sketch_size
        FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64))

        def cb(_user, seq, off, n, dst):
            try:
                o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
                sq = np.ctypeslib.as_array(seq, shape=(int(o[n]),)).copy()
                res = np.ascontiguousarray(sketcher(sq, o), dtype=np.uint64)
                np.ctypeslib.as_array(dst, shape=(n * s,))[:] = res.reshape(-1)
                return 0
            except Exception:
                return -1

        fn = FN(cb)
        _check(lib().groot_index_build_msa_dir_with(msa_dir.encode(), C.byref(p), fn, None, C.byref(out)))
        return cls(out.value)

    @classmethod
    def load(cls, path):
        out = C.c_void_p()
        _check(lib().groot_index_load(path.encode(), C.byref(out)))
        return cls(out.value)

    @classmethod
    def load_gob(cls, index_dir):
        """an index directory written by the reference's `groot index`: groot.gg + groot.lshe (cmd/align.go:93-107)"""
        out = C.c_void_p()
        _check(lib().groot_index_load_gob(os.path.join(index_dir, "groot.gg").encode(), os.path.join(index_dir, "groot.lshe").encode(),
                                          C.byref(out)))
        return cls(out.value)

    def save(self, path):
        _check(lib().groot_index_save(self._h, path.encode()))

    def save_gob(self, index_dir, max_sketch_span=30):
        """groot.gg + groot.lshe as the reference's `groot index` writes them (cmd/index.go:130-131)"""
        os.makedirs(index_dir, exist_ok=True)
        _check(lib().groot_index_save_gob(self._h, index_dir.encode(), C.c_uint32(max_sketch_span)))

    # ---- convenience accessors ------------------------------------------------------------
    def path_name(self, global_path):
        a = self.arrays
        o0, o1 = int(a["path_name_off"][global_path]), int(a["path_name_off"][global_path + 1])
        return bytes(a["path_names"][o0:o1]).decode()

    def node_seq(self, node):
        a = self.arrays
        return bytes(a["bases"][int(a["node_seq_off"][node]):int(a["node_seq_off"][node + 1])])

    def path_sequence(self, graph, local_path):
        """Graph2Seqs (graph.go:625-644) for one path."""
        a = self.arrays
        n0, n1 = int(a["graph_node_off"][graph]), int(a["graph_node_off"][graph + 1])
        out = []
        for n in range(n0, n1):
            ps = a["np_path"][int(a["node_np_off"][n]):int(a["node_np_off"][n + 1])]
            if local_path in ps:
                out.append(self.node_seq(n))
        return b"".join(out)


def gob_to_json(data):
    """every top-level value of a Go encoding/gob stream, decoded by the reader behind Index.load_gob"""
    import json

    b = np.frombuffer(bytes(data), dtype=np.uint8)
    need = C.c_uint64(0)
    _check(lib().groot_gob_to_json(_ffi.as_ptr(b, C.c_uint8), C.c_uint64(len(b)), None, C.c_uint64(0), C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _check(lib().groot_gob_to_json(_ffi.as_ptr(b, C.c_uint8), C.c_uint64(len(b)), buf, C.c_uint64(need.value), C.byref(need)))
    return json.loads(buf.value.decode())


def window_sketch(seq, k, s):
    out = np.empty(s, dtype=np.uint64)
    b = np.frombuffer(seq, dtype=np.uint8)
    _check(lib().groot_host_window_sketch(_ffi.as_ptr(b, C.c_uint8), C.c_uint32(len(b)), C.c_uint32(k), C.c_uint32(s),
                                          _ffi.as_ptr(out, C.c_uint64)))
    return out


def msa_files(msa_dir):
    """cluster*.msa in filepath.Glob (lexical) order: cmd/index.go:143"""
    return sorted(glob.glob(os.path.join(msa_dir, "cluster*.msa")))


# ---- FASTQ in / BAM + GFA out (host side of `groot align`) ------------------------------------------
class AlnRecord(C.Structure):
    """groot_aln_record"""
    _fields_ = [("name", C.c_char_p), ("name_len", C.c_uint32), ("seq", C.POINTER(C.c_uint8)), ("qual", C.POINTER(C.c_uint8)),
                ("seq_len", C.c_uint32), ("ref_id", C.c_uint32), ("pos", C.c_uint32), ("start_clip", C.c_uint8),
                ("end_clip", C.c_uint8), ("reverse", C.c_uint8), ("secondary", C.c_uint8)]


class FastqReader:
    """DataStreamer + FastqHandler (src/pipeline/sketch.go:41-77,175-238): batches of reads from FASTQ files"""

    def __init__(self, files):
        self._h = C.c_void_p()
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        _check(lib().groot_fastq_open(arr, C.c_uint32(len(files)), C.byref(self._h)))

    def batches(self, max_reads=1 << 16, max_bases=1 << 24, max_name_bytes=1 << 23):
        L = lib()
        L.groot_fastq_next_batch.restype = C.c_int64
        seq = np.empty(max_bases, dtype=np.uint8)
        qual = np.empty(max_bases, dtype=np.uint8)
        names = np.empty(max_name_bytes, dtype=np.uint8)
        soff = np.empty(max_reads + 1, dtype=np.uint64)
        noff = np.empty(max_reads + 1, dtype=np.uint64)
        while True:
            n = L.groot_fastq_next_batch(self._h, C.c_uint32(max_reads), _ffi.as_ptr(seq, C.c_uint8), _ffi.as_ptr(qual, C.c_uint8),
                                         _ffi.as_ptr(soff, C.c_uint64), C.c_uint64(max_bases), names.ctypes.data_as(C.c_char_p),
                                         _ffi.as_ptr(noff, C.c_uint64), C.c_uint64(max_name_bytes))
            _check(int(n))
            if n == 0:
                return
            nb, nn = int(soff[n]), int(noff[n])
            yield {"n": int(n), "seq": seq[:nb].copy(), "qual": qual[:nb].copy(), "seq_off": soff[: n + 1].copy(),
                   "names": names[:nn].copy(), "name_off": noff[: n + 1].copy()}

    def close(self):
        if self._h:
            lib().groot_fastq_close(self._h)
            self._h = C.c_void_p()

    __del__ = close


class ReadsView(C.Structure):
    """groot_reads_view"""
    _fields_ = [("n_reads", C.c_uint32), ("max_len", C.c_uint32), ("n_bases", C.c_uint64), ("n_exc", C.c_uint64),
                ("packed", C.POINTER(C.c_uint8)), ("seq_len", C.POINTER(C.c_uint16)), ("exc_pos", C.POINTER(C.c_uint64)),
                ("exc_byte", C.POINTER(C.c_uint8)), ("text", C.POINTER(C.c_uint8)), ("name_pos", C.POINTER(C.c_uint32)),
                ("name_len", C.POINTER(C.c_uint32)), ("seq_pos", C.POINTER(C.c_uint32)), ("qual_pos", C.POINTER(C.c_uint32)),
                ("qual_len", C.POINTER(C.c_uint32))]


class ParallelReads:
    """groot_reads_*: parallel FASTQ ingest (reader thread per file, parse + 2-bit pack over all cores); batches carry the
    wire format of groot_hip_submit_packed16 and positions into the FASTQ text"""

    def __init__(self, files, threads=0, block_bytes=0, max_batch_reads=0, max_batch_bases=0, mates=None, interleaved=False):
        """mates: the files of the second mates, read in lockstep with `files` (groot_reads_open_paired: batches of whole fragments,
        read 2i from files, 2i+1 from mates); interleaved: `files` is one stream that holds the mates alternately"""
        self._h = C.c_void_p()
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        if mates is not None or interleaved:
            m = [] if interleaved else list(mates)
            arr2 = (C.c_char_p * len(m))(*[f.encode() for f in m])
            _check(lib().groot_reads_open_paired(arr, C.c_uint32(len(files)), arr2, C.c_uint32(len(m)), C.c_uint32(threads), C.c_uint64(block_bytes),
                                                 C.c_uint32(max_batch_reads), C.c_uint64(max_batch_bases), C.byref(self._h)))
            return
        _check(lib().groot_reads_open(arr, C.c_uint32(len(files)), C.c_uint32(threads), C.c_uint64(block_bytes), C.c_uint32(max_batch_reads),
                                      C.c_uint64(max_batch_bases), C.byref(self._h)))

    def batches(self):
        L = lib()
        L.groot_reads_batch_free.argtypes = [C.c_void_p]
        L.groot_reads_batch_free.restype = None
        L.groot_reads_batch_view.argtypes = [C.c_void_p, C.POINTER(ReadsView)]
        L.groot_reads_batch_view.restype = None
        while True:
            b = C.c_void_p()
            _check(L.groot_reads_next(self._h, C.byref(b)))
            if not b.value:
                return
            v = ReadsView()
            L.groot_reads_batch_view(b, C.byref(v))
            n = v.n_reads
            out = {"n": n, "max_len": v.max_len, "n_bases": int(v.n_bases),
                   "packed": _ffi._np_view(v.packed, (v.n_bases + 3) // 4, np.uint8).copy(),
                   "seq_len": _ffi._np_view(v.seq_len, n, np.uint16).copy(),
                   "exc_pos": _ffi._np_view(v.exc_pos, v.n_exc, np.uint64).copy(),
                   "exc_byte": _ffi._np_view(v.exc_byte, v.n_exc, np.uint8).copy()}
            pos = {k: _ffi._np_view(getattr(v, k), n, np.uint32) for k in ("name_pos", "name_len", "seq_pos", "qual_pos", "qual_len")}
            text_end = max(int((pos["qual_pos"] + pos["qual_len"]).max()), int((pos["seq_pos"] + out["seq_len"]).max())) if n else 0
            text = _ffi._np_view(v.text, text_end, np.uint8)
            out["names"] = [bytes(text[int(p):int(p) + int(l)]) for p, l in zip(pos["name_pos"], pos["name_len"])]
            out["seqs"] = [bytes(text[int(p):int(p) + int(l)]) for p, l in zip(pos["seq_pos"], out["seq_len"])]
            out["quals"] = [bytes(text[int(p):int(p) + int(l)]) for p, l in zip(pos["qual_pos"], pos["qual_len"])]
            L.groot_reads_batch_free(b)
            yield out

    def close(self):
        if self._h:
            lib().groot_reads_close.argtypes = [C.c_void_p]
            lib().groot_reads_close.restype = None
            lib().groot_reads_close(self._h)
            self._h = C.c_void_p()

    __del__ = close


class ReadBatch(C.Structure):
    """groot_read_batch"""
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("seq_off", C.c_void_p), ("names", C.c_void_p), ("name_off", C.c_void_p),
                ("n_reads", C.c_uint32), ("first_read_id", C.c_uint32)]


class BamWriter:
    """setupBAM + the record collector of theBoss (src/pipeline/boss.go:45-105,225-240)"""

    def __init__(self, path, index, date=None):
        self._h = C.c_void_p()
        self.index = index
        _check(lib().groot_bam_open(path.encode() if path else None, C.byref(index.view), date.encode() if date else None,
                                    C.byref(self._h)))

    def write(self, alns, batch, first_read_id=0):
        """alns: expanded records (ALN_DTYPE) of reads held in `batch` (a FastqReader batch dict).
        Seq/Qual of a reverse-complemented read are the reverse complement / reverse (seqio.go:120-133);
        a start-clipped record still carries read.Seq[0:seqLen] (alignment.go:120)."""
        comp = np.zeros(256, dtype=np.uint8)
        for a, b in zip(b"ACGTN", b"TGCAN"):
            comp[a] = b
        recs = (AlnRecord * len(alns))()
        keep = []
        for i, a in enumerate(alns):
            r = int(a["read_id"]) - first_read_id
            s0, s1 = int(batch["seq_off"][r]), int(batch["seq_off"][r + 1])
            n0, n1 = int(batch["name_off"][r]), int(batch["name_off"][r + 1])
            seq, qual = batch["seq"][s0:s1], batch["qual"][s0:s1]
            if a["rc"]:
                seq, qual = comp[seq][::-1], qual[::-1]
            seq_len = (s1 - s0) - int(a["start_clip"]) - int(a["end_clip"])
            seq = np.ascontiguousarray(seq[:seq_len])
            qual = np.ascontiguousarray(qual[:seq_len])
            name = bytes(batch["names"][n0:n1])
            keep.append((seq, qual, name))
            recs[i] = AlnRecord(name, len(name), _ffi.as_ptr(seq, C.c_uint8), _ffi.as_ptr(qual, C.c_uint8), seq_len, int(a["ref_id"]),
                                int(a["pos"]), int(a["start_clip"]), int(a["end_clip"]), int(a["rc"]), int(a["secondary"]))
        _check(lib().groot_bam_write(self._h, recs, C.c_uint64(len(alns))))

    def set_level(self, level):
        """groot_bam_set_level: -1 = zlib default, 0..9, -2 = structural"""
        _check(lib().groot_bam_set_level(self._h, C.c_int(level)))

    def write_travs(self, travs, masks, batch, first_read_id=0):
        """groot_bam_write_travs: traversal records (device.TRAV_DTYPE) + path sets [n, path_words] of reads held in `batch` (a
        FastqReader batch dict) -> the number of records written.  MAPQ 30, or `reserved` where a traversal carries TRAV_MAPQ."""
        t = np.ascontiguousarray(travs)
        m = np.ascontiguousarray(masks, dtype=np.uint64)
        arrs = [np.ascontiguousarray(batch[k], dtype=d) for k, d in (("seq", np.uint8), ("qual", np.uint8), ("seq_off", np.uint64), ("names", np.uint8),
                                                                      ("name_off", np.uint64))]
        rb = ReadBatch(*[a.ctypes.data for a in arrs], len(arrs[2]) - 1, first_read_id)
        n = C.c_uint64(0)
        _check(lib().groot_bam_write_travs(self._h, C.byref(self.index.view), C.byref(rb), t.ctypes.data_as(C.c_void_p), _ffi.as_ptr(m, C.c_uint64),
                                           C.c_uint64(len(t)), C.byref(n)))
        return n.value

    def write_rescued(self, records, names, seqs, quals, gap_records=None):
        """groot_bam_write_rescued: the rescued records (device.RESCUE_RECORD_DTYPE) of a batch whose reads are given as lists of bytes
        (name, sequence, quality line as it came) -> the number of records written, each with NM and MD.  gap_records
        (device.GAP_RECORD_DTYPE, an empty list included): groot_bam_write_rescued_gapped, the two lists merged by read"""
        n = len(names)
        text = np.frombuffer(b"".join(x for t in zip(names, seqs, quals) for x in t) or b"\0", dtype=np.uint8)
        lens = np.array([[len(a), len(s), len(q)] for a, s, q in zip(names, seqs, quals)], dtype=np.int64).reshape(n, 3)
        at = np.r_[0, np.cumsum(lens.reshape(-1))][:-1].reshape(n, 3)
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        keep = dict(seq_len=np.ascontiguousarray(lens[:, 1], dtype=np.uint16), name_pos=u32(at[:, 0]), name_len=u32(lens[:, 0]), seq_pos=u32(at[:, 1]),
                    qual_pos=u32(at[:, 2]), qual_len=u32(lens[:, 2]))
        v = ReadsView()
        v.n_reads, v.max_len, v.n_bases = n, int(lens[:, 1].max()) if n else 0, int(lens[:, 1].sum())
        v.text = _ffi.as_ptr(text, C.c_uint8)
        v.seq_len = _ffi.as_ptr(keep["seq_len"], C.c_uint16)
        for k in ("name_pos", "name_len", "seq_pos", "qual_pos", "qual_len"):
            setattr(v, k, _ffi.as_ptr(keep[k], C.c_uint32))
        rec = np.ascontiguousarray(records)
        assert rec.dtype.itemsize == 20
        out = C.c_uint64(0)
        if gap_records is not None:
            grec = np.ascontiguousarray(gap_records)
            assert grec.dtype.itemsize == 24
            _check(lib().groot_bam_write_rescued_gapped(self._h, C.byref(self.index.view), C.byref(v), rec.ctypes.data_as(C.c_void_p), C.c_uint64(len(rec)),
                                                        grec.ctypes.data_as(C.c_void_p), C.c_uint64(len(grec)), C.byref(out)))
            return out.value
        _check(lib().groot_bam_write_rescued(self._h, C.byref(self.index.view), C.byref(v), rec.ctypes.data_as(C.c_void_p), C.c_uint64(len(rec)), C.byref(out)))
        return out.value

    def close(self):
        if self._h:
            h, self._h = self._h, C.c_void_p()
            _check(lib().groot_bam_close(h))

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                self.close()
            except Exception:
                pass


def pack_reads(seq_concat, threads=0):
    """2 bits per base + the list of bytes that are not ACGT (groot_host_pack_reads) -> (packed, exc_pos, exc_byte)"""
    seq = np.ascontiguousarray(seq_concat, dtype=np.uint8)
    packed = np.empty((len(seq) + 3) // 4, dtype=np.uint8)
    cap = 1024
    while True:
        pos, byte = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint8)
        n = C.c_uint64(0)
        rc = lib().groot_host_pack_reads(_ffi.as_ptr(seq, C.c_uint8), C.c_uint64(len(seq)), _ffi.as_ptr(packed, C.c_uint8),
                                         _ffi.as_ptr(pos, C.c_uint64), _ffi.as_ptr(byte, C.c_uint8), C.c_uint64(cap), C.byref(n),
                                         C.c_uint32(threads))
        if rc == -6 and n.value > cap:      # GROOT_E_NOSPACE: retry with the size it asked for
            cap = int(n.value)
            continue
        _check(rc)
        return packed, pos[: n.value].copy(), byte[: n.value].copy()


def report(bam_path, cov_cutoff=0.97, low_cov=False, out_path=None):
    """`groot report` (src/reporting/reporting.go): list of (name, read count, length, coverage cigar)"""
    import tempfile

    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".report")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_report(bam_path.encode(), C.c_double(cov_cutoff), C.c_int(1 if low_cov else 0), (out_path or tmp).encode(),
                                       C.byref(n)))
        rows = [ln.rstrip("\n").split("\t") for ln in open(out_path or tmp)]
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return [(r[0], int(r[1]), int(r[2]), r[3]) for r in rows]


def variants_write(index, rescued_depth, alt, exact_depth, out_path, min_reads=2, min_share=0.1):
    """the variants file (groot_host_variants_write) from device.Aligner.rescue() -- summed over the ctxs -- and the depth of
    device.Aligner.coverage(); returns the lines written"""
    n_bases = int(index.arrays["path_len"].astype(np.uint64).sum())
    rd = np.ascontiguousarray(rescued_depth, dtype=np.uint64)
    al = np.ascontiguousarray(alt, dtype=np.uint64)
    ed = np.ascontiguousarray(exact_depth, dtype=np.uint64)
    if rd.shape != (n_bases,) or al.size != 4 * n_bases or ed.shape != (n_bases,):
        raise ValueError("rescued depth / alt / exact depth do not match the index")
    n = C.c_uint64(0)
    _check(lib().groot_host_variants_write(C.byref(index.view), _ffi.as_ptr(rd, C.c_uint64), _ffi.as_ptr(al, C.c_uint64), _ffi.as_ptr(ed, C.c_uint64),
                                           C.c_uint64(min_reads), C.c_double(min_share), os.fsencode(out_path), C.byref(n)))
    return n.value


GAP_EVENT_DTYPE = np.dtype([("path", "<u4"), ("pos", "<u4"), ("type", "u1"), ("len", "u1"), ("seq", "<u2"), ("reserved", "<u4"), ("reads", "<u8")])   # groot_gap_event


def indels_write(index, events, gdepth, rescued_depth, exact_depth, out_path, min_reads=2, min_share=0.1):
    """the indels file (groot_host_indels_write) from device.Aligner.gap() -- merged over the ctxs: gdepth summed, events by key -- the
    depth of device.Aligner.rescue() and the depth of device.Aligner.coverage(); returns the lines written"""
    n_bases = int(index.arrays["path_len"].astype(np.uint64).sum())
    ev = np.ascontiguousarray(events, dtype=GAP_EVENT_DTYPE)
    gd, rd, ed = (np.ascontiguousarray(x, dtype=np.uint64) for x in (gdepth, rescued_depth, exact_depth))
    if gd.shape != (n_bases,) or rd.shape != (n_bases,) or ed.shape != (n_bases,):
        raise ValueError("gap depth / rescued depth / exact depth do not match the index")
    n = C.c_uint64(0)
    _check(lib().groot_host_indels_write(C.byref(index.view), ev.ctypes.data_as(C.c_void_p), C.c_uint64(len(ev)), _ffi.as_ptr(gd, C.c_uint64), _ffi.as_ptr(rd, C.c_uint64),
                                         _ffi.as_ptr(ed, C.c_uint64), C.c_uint64(min_reads), C.c_double(min_share), os.fsencode(out_path), C.byref(n)))
    return n.value


def report_coverage(index, records, depth, cov_cutoff=0.97, low_cov=False, out_path=None):
    """the report of `report` from counts instead of a BAM (groot_host_report_coverage): records[n_paths] and depth[sum of
    path_len] as uint64, e.g. device.Aligner.coverage(); same rows as `report` on the BAM whose records they count"""
    import tempfile

    v = index.view
    records = np.ascontiguousarray(records, dtype=np.uint64)
    depth = np.ascontiguousarray(depth, dtype=np.uint64)
    if records.shape != (v.n_paths,) or depth.shape != (int(index.arrays["path_len"].astype(np.uint64).sum()),):
        raise ValueError("records / depth do not match the index")
    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".report")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_report_coverage(C.byref(v), _ffi.as_ptr(records, C.c_uint64), _ffi.as_ptr(depth, C.c_uint64),
                                                C.c_double(cov_cutoff), C.c_int(1 if low_cov else 0), (out_path or tmp).encode(),
                                                C.byref(n)))
        rows = [ln.rstrip("\n").split("\t") for ln in open(out_path or tmp)]
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return [(r[0], int(r[1]), int(r[2]), r[3]) for r in rows]


def _shared_rows(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return [(r[0], r[1], int(r[2])) for r in rows]


def shared_from_counts(index, records, depth, pa, pb, count, cov_cutoff=0.97, low_cov=False, out_path=None):
    """the shared-reads lines (groot_host_shared_from_counts) for the references report_coverage(index, records, depth, ...) reports:
    [(nameA, nameB, reads)]; pa / pb / count as device.Aligner.shared() gives them (any order, repeated pairs summed)"""
    import tempfile

    v = index.view
    records = np.ascontiguousarray(records, dtype=np.uint64)
    depth = np.ascontiguousarray(depth, dtype=np.uint64)
    pa = np.ascontiguousarray(pa, dtype=np.uint32)
    pb = np.ascontiguousarray(pb, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if records.shape != (v.n_paths,) or depth.shape != (int(index.arrays["path_len"].astype(np.uint64).sum()),):
        raise ValueError("records / depth do not match the index")
    if not (len(pa) == len(pb) == len(count)):
        raise ValueError("pa / pb / count differ in length")
    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".shared")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_shared_from_counts(C.byref(v), _ffi.as_ptr(records, C.c_uint64), _ffi.as_ptr(depth, C.c_uint64), C.c_double(cov_cutoff),
                                                   C.c_int(1 if low_cov else 0), C.c_uint64(len(pa)), _ffi.as_ptr(pa, C.c_uint32),
                                                   _ffi.as_ptr(pb, C.c_uint32), _ffi.as_ptr(count, C.c_uint64), (out_path or tmp).encode(),
                                                   C.byref(n)))
        rows = _shared_rows(out_path or tmp)
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return rows


def report_shared(bam_path, cov_cutoff=0.97, low_cov=False, report_out=None, shared_out=None):
    """one pass over a BAM (groot_host_report_shared): (the rows of report(), the shared-reads rows [(nameA, nameB, reads)]), a read
    being one QNAME"""
    import tempfile

    tmps = []
    paths = []
    for p in (report_out, shared_out):
        if p is None:
            fd, p = tempfile.mkstemp(suffix=".tsv")
            os.close(fd)
            tmps.append(p)
        paths.append(p)
    nr, nl = C.c_uint64(0), C.c_uint64(0)
    try:
        _check(lib().groot_host_report_shared(bam_path.encode(), C.c_double(cov_cutoff), C.c_int(1 if low_cov else 0), paths[0].encode(),
                                              paths[1].encode(), C.byref(nr), C.byref(nl)))
        rep = [ln.rstrip("\n").split("\t") for ln in open(paths[0])]
        sh = _shared_rows(paths[1])
    finally:
        for p in tmps:
            os.unlink(p)
    assert len(rep) == nr.value and len(sh) == nl.value
    return [(r[0], int(r[1]), int(r[2]), r[3]) for r in rep], sh


EM_MIN_ITER, EM_MAX_ITER = 50, 10000        # GROOT_EM_MIN_ITER / GROOT_EM_MAX_ITER


def em(n_paths, off, ids, count, min_iter=EM_MIN_ITER, max_iter=EM_MAX_ITER):
    """groot_host_em: src/em/em.go over the ECs (CSR off / ids / count) in the order given -> (alpha float64[n_paths], iterations)"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if len(off) != len(count) + 1:
        raise ValueError("off must have one entry more than count")
    alpha = np.zeros(n_paths, dtype=np.float64)
    it = C.c_uint32(0)
    _check(lib().groot_host_em(C.c_uint32(n_paths), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                               _ffi.as_ptr(count, C.c_uint64), C.c_uint32(min_iter), C.c_uint32(max_iter), _ffi.as_ptr(alpha, C.c_double),
                               C.byref(it)))
    return alpha, it.value


def _abundance_rows(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return [(r[0], int(r[1]), float(r[2]), float(r[3])) for r in rows]


def abundance_from_ecs(index, off, ids, count, min_reads=1.0, out_path=None):
    """the abundance lines (groot_host_abundance_from_ecs) of ECs as device.Aligner.ecs() gives them (any order, repeats summed):
    [(name, reads, em_reads, fraction)]"""
    import tempfile

    v = index.view
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if len(off) != len(count) + 1:
        raise ValueError("off must have one entry more than count")
    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".abundance")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_abundance_from_ecs(C.byref(v), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                                   _ffi.as_ptr(count, C.c_uint64), C.c_double(min_reads), (out_path or tmp).encode(), C.byref(n), None))
        rows = _abundance_rows(out_path or tmp)
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return rows


def report_abundance(bam_path, min_reads=1.0, out_path=None):
    """the abundance lines from a BAM (groot_host_report_abundance), a read being one QNAME: [(name, reads, em_reads, fraction)]"""
    import tempfile

    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".abundance")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_report_abundance(bam_path.encode(), C.c_double(min_reads), (out_path or tmp).encode(), C.byref(n)))
        rows = _abundance_rows(out_path or tmp)
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return rows


def _tuple_arrays(tuples, tn):
    tuples = np.ascontiguousarray(tuples, dtype=np.uint32).reshape(-1, 4)
    tn = np.ascontiguousarray(tn, dtype=np.uint64)
    if len(tuples) != len(tn):
        raise ValueError("one count per tuple")
    return tuples, tn


def acov_merge(n_paths, exports):
    """groot_host_acov_merge: exports = [(off, ids, count, tuples, tn), ...] as device.Aligner.acov() gives them -> one table
    (off, ids, count, tuples[n, 4], tn) with canonical ECs and ascending tuples"""
    ex = [_ec_arrays(o, i, c) + _tuple_arrays(t, n) for o, i, c, t, n in exports]
    k = len(ex)

    def ptrs(j, ct):
        return (C.c_void_p * max(k, 1))(*[C.cast(_ffi.as_ptr(e[j], ct), C.c_void_p).value or 0 for e in ex])

    n_ec = np.array([len(e[2]) for e in ex], dtype=np.uint64)
    n_tp = np.array([len(e[4]) for e in ex], dtype=np.uint64)
    o = np.zeros(int(n_ec.sum()) + 1, dtype=np.uint64)
    i = np.zeros(max(sum(len(e[1]) for e in ex), 1), dtype=np.uint32)
    c = np.zeros(max(int(n_ec.sum()), 1), dtype=np.uint64)
    t = np.zeros((max(int(n_tp.sum()), 1), 4), dtype=np.uint32)
    tn = np.zeros(max(int(n_tp.sum()), 1), dtype=np.uint64)
    ne, nt = C.c_uint64(0), C.c_uint64(0)
    _check(lib().groot_host_acov_merge(C.c_uint32(n_paths), C.c_uint32(k), ptrs(0, C.c_uint64), ptrs(1, C.c_uint32), ptrs(2, C.c_uint64),
                                       _ffi.as_ptr(n_ec, C.c_uint64), ptrs(3, C.c_uint32), ptrs(4, C.c_uint64), _ffi.as_ptr(n_tp, C.c_uint64),
                                       _ffi.as_ptr(o, C.c_uint64), _ffi.as_ptr(i, C.c_uint32), _ffi.as_ptr(c, C.c_uint64), _ffi.as_ptr(t, C.c_uint32),
                                       _ffi.as_ptr(tn, C.c_uint64), C.byref(ne), C.byref(nt)))
    return o[:ne.value + 1].copy(), i[:int(o[ne.value])].copy(), c[:ne.value].copy(), t[:nt.value].copy(), tn[:nt.value].copy()


def acov_depth(n_paths, off, ids, alpha, tuples, tn, path, path_len):
    """groot_host_acov_depth: D_p[path_len] (float64) of one path from a table with canonical ECs and alpha[n_paths]"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    tuples, tn = _tuple_arrays(tuples, tn)
    d = np.zeros(max(path_len, 1), dtype=np.float64)
    _check(lib().groot_host_acov_depth(C.c_uint32(n_paths), C.c_uint64(len(off) - 1), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                       _ffi.as_ptr(alpha, C.c_double), C.c_uint64(len(tn)), _ffi.as_ptr(tuples, C.c_uint32), _ffi.as_ptr(tn, C.c_uint64),
                                       C.c_uint32(path), C.c_uint32(path_len), _ffi.as_ptr(d, C.c_double)))
    return d[:path_len]


def calls_from_table(index, off, ids, count, tuples, tn, out_path, alpha=None, min_reads=1.0, call_depth=1.0, cov_cutoff=0.97):
    """groot_host_calls_from_table: writes the calls file of a table with canonical ECs (acov_merge); alpha None = the EM over the
    ECs.  Returns (lines, called)."""
    off, ids, count = _ec_arrays(off, ids, count)
    tuples, tn = _tuple_arrays(tuples, tn)
    if alpha is not None:
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    nl, nc = C.c_uint64(0), C.c_uint64(0)
    _check(lib().groot_host_calls_from_table(C.byref(index.view), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                             _ffi.as_ptr(count, C.c_uint64), None if alpha is None else _ffi.as_ptr(alpha, C.c_double),
                                             C.c_uint64(len(tn)), _ffi.as_ptr(tuples, C.c_uint32), _ffi.as_ptr(tn, C.c_uint64), C.c_double(min_reads),
                                             C.c_double(call_depth), C.c_double(cov_cutoff), out_path.encode(), C.byref(nl), C.byref(nc)))
    return nl.value, nc.value


def report_calls(bam_path, out_path, min_reads=1.0, call_depth=1.0, cov_cutoff=0.97):
    """groot_host_report_calls: the calls file from a BAM.  Returns (lines, called, tuples)."""
    nl, nc, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().groot_host_report_calls(bam_path.encode(), C.c_double(min_reads), C.c_double(call_depth), C.c_double(cov_cutoff), out_path.encode(),
                                         C.byref(nl), C.byref(nc), C.byref(nt)))
    return nl.value, nc.value, nt.value


def _support_arrays(n_paths, path_len, off, ids, count, tuples, tn, boot_count, alpha, sel_paths):
    off, ids, count = _ec_arrays(off, ids, count)
    tuples, tn = _tuple_arrays(tuples, tn)
    path_len = np.ascontiguousarray(path_len, dtype=np.uint32)
    if len(path_len) != n_paths:
        raise ValueError("path_len must have n_paths values")
    boot_count = np.ascontiguousarray(boot_count, dtype=np.uint64)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    n_boot = alpha.shape[0] if alpha.ndim == 2 else 0
    if alpha.shape != (n_boot, n_paths) or boot_count.shape != (n_boot, len(count)):
        raise ValueError("boot_count must be [n_boot, n_ec] and alpha [n_boot, n_paths]")
    sel = np.ascontiguousarray(sel_paths, dtype=np.uint32).reshape(-1)
    return path_len, off, ids, count, tuples, tn, n_boot, boot_count, alpha, sel


def call_support(n_paths, path_len, off, ids, count, tuples, tn, boot_count, alpha, sel_paths, call_depth=1.0, threads=1):
    """groot_host_call_support: the covered bases of the paths sel_paths in every bootstrap replicate (boot_count [n_boot, n_ec] and
    alpha [n_boot, n_paths] as em_bootstrap returns them) -> covered uint32[n_boot, n_sel]"""
    path_len, off, ids, count, tuples, tn, n_boot, boot_count, alpha, sel = _support_arrays(n_paths, path_len, off, ids, count, tuples, tn, boot_count, alpha,
                                                                                           sel_paths)
    cov = np.zeros((n_boot, len(sel)), dtype=np.uint32)
    _check(lib().groot_host_call_support(C.c_uint32(n_paths), _ffi.as_ptr(path_len, C.c_uint32), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64),
                                         _ffi.as_ptr(ids, C.c_uint32), _ffi.as_ptr(count, C.c_uint64), C.c_uint64(len(tn)), _ffi.as_ptr(tuples, C.c_uint32),
                                         _ffi.as_ptr(tn, C.c_uint64), C.c_uint32(n_boot), _ffi.as_ptr(boot_count, C.c_uint64), _ffi.as_ptr(alpha, C.c_double),
                                         C.c_double(call_depth), C.c_uint32(len(sel)), _ffi.as_ptr(sel, C.c_uint32), C.c_uint32(threads),
                                         _ffi.as_ptr(cov, C.c_uint32)))
    return cov


def calls_support_from_table(index, off, ids, count, tuples, tn, out_path, n_boot, seed=1, threads=1, alpha=None, boot_count=None, boot_alpha=None,
                             covered=None, min_reads=1.0, call_depth=1.0, cov_cutoff=0.97):
    """groot_host_calls_support_from_table: calls_from_table with the three support columns; boot_count / boot_alpha / covered None =
    computed inside on `threads` host threads.  Returns (lines, called)."""
    off, ids, count = _ec_arrays(off, ids, count)
    tuples, tn = _tuple_arrays(tuples, tn)

    def opt(a, dt, ct):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, _ffi.as_ptr(a, ct)

    alpha, p_alpha = opt(alpha, np.float64, C.c_double)
    boot_count, p_bc = opt(boot_count, np.uint64, C.c_uint64)
    boot_alpha, p_ba = opt(boot_alpha, np.float64, C.c_double)
    covered, p_cov = opt(covered, np.uint32, C.c_uint32)
    if boot_count is not None and boot_count.shape != (n_boot, len(count)):
        raise ValueError("boot_count must be [n_boot, n_ec]")
    if boot_alpha is not None and boot_alpha.shape != (n_boot, index.view.n_paths):
        raise ValueError("boot_alpha must be [n_boot, n_paths]")
    if covered is not None and (covered.ndim != 2 or covered.shape[0] != n_boot):
        raise ValueError("covered must be [n_boot, lines]")
    nl, nc = C.c_uint64(0), C.c_uint64(0)
    _check(lib().groot_host_calls_support_from_table(C.byref(index.view), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                                     _ffi.as_ptr(count, C.c_uint64), p_alpha, C.c_uint64(len(tn)), _ffi.as_ptr(tuples, C.c_uint32),
                                                     _ffi.as_ptr(tn, C.c_uint64), C.c_double(min_reads), C.c_double(call_depth), C.c_double(cov_cutoff),
                                                     C.c_uint32(n_boot), C.c_uint64(seed), C.c_uint32(threads), p_bc, p_ba, p_cov, out_path.encode(),
                                                     C.byref(nl), C.byref(nc)))
    return nl.value, nc.value


def report_calls_support(bam_path, out_path, n_boot, seed=1, threads=1, min_reads=1.0, call_depth=1.0, cov_cutoff=0.97):
    """groot_host_report_calls_support: the calls file of a BAM with the three support columns.  Returns (lines, called, tuples)."""
    nl, nc, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().groot_host_report_calls_support(bam_path.encode(), C.c_double(min_reads), C.c_double(call_depth), C.c_double(cov_cutoff), C.c_uint32(n_boot),
                                                 C.c_uint64(seed), C.c_uint32(threads), out_path.encode(), C.byref(nl), C.byref(nc), C.byref(nt)))
    return nl.value, nc.value, nt.value


def _ec_arrays(off, ids, count):
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint64)
    if len(off) != len(count) + 1:
        raise ValueError("off must have one entry more than count")
    return off, ids, count


def em_bootstrap(n_paths, off, ids, count, n_boot, seed=1, n_draws=0, min_iter=EM_MIN_ITER, max_iter=EM_MAX_ITER, threads=1):
    """groot_host_em_bootstrap: n_boot resampled replicates of the ECs (splitmix64 draws, include/groot_host.h), the EM on each ->
    (boot_count uint64[n_boot, n_ec], alpha float64[n_boot, n_paths], iterations uint32[n_boot])"""
    off, ids, count = _ec_arrays(off, ids, count)
    bc = np.zeros((n_boot, len(count)), dtype=np.uint64)
    alpha = np.zeros((n_boot, n_paths), dtype=np.float64)
    its = np.zeros(n_boot, dtype=np.uint32)
    _check(lib().groot_host_em_bootstrap(C.c_uint32(n_paths), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                         _ffi.as_ptr(count, C.c_uint64), C.c_uint32(n_boot), C.c_uint64(seed), C.c_uint64(n_draws), C.c_uint32(min_iter),
                                         C.c_uint32(max_iter), C.c_uint32(threads), _ffi.as_ptr(bc, C.c_uint64), _ffi.as_ptr(alpha, C.c_double),
                                         _ffi.as_ptr(its, C.c_uint32)))
    return bc, alpha, its


def ecs_canonical(n_paths, off, ids, count):
    """groot_host_ecs_canonical: ECs in any order, repeats summed -> (off, ids, count) in canonical order"""
    off, ids, count = _ec_arrays(off, ids, count)
    o = np.zeros(len(count) + 1, dtype=np.uint64)
    i = np.zeros(max(len(ids), 1), dtype=np.uint32)
    c = np.zeros(max(len(count), 1), dtype=np.uint64)
    n = C.c_uint64(0)
    _check(lib().groot_host_ecs_canonical(C.c_uint32(n_paths), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                          _ffi.as_ptr(count, C.c_uint64), _ffi.as_ptr(o, C.c_uint64), _ffi.as_ptr(i, C.c_uint32), _ffi.as_ptr(c, C.c_uint64),
                                          C.byref(n)))
    return o[:n.value + 1].copy(), i[:int(o[n.value])].copy(), c[:n.value].copy()


def _abundance_boot_rows(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return [(r[0], int(r[1])) + tuple(float(x) for x in r[2:]) for r in rows]


def abundance_boot_from_ecs(index, off, ids, count, n_boot, seed=1, boot_alpha=None, threads=1, min_reads=1.0, out_path=None):
    """groot_host_abundance_boot_from_ecs: the abundance lines with the bootstrap columns, from ready-made boot_alpha[n_boot, n_paths]
    (device.em_bootstrap over ecs_canonical) or computed on `threads` host threads:
    [(name, reads, em_reads, fraction, boot_mean, boot_sd, boot_lo, boot_hi)]"""
    import tempfile

    v = index.view
    off, ids, count = _ec_arrays(off, ids, count)
    if boot_alpha is not None:
        boot_alpha = np.ascontiguousarray(boot_alpha, dtype=np.float64)
        if boot_alpha.shape != (n_boot, v.n_paths):
            raise ValueError("boot_alpha must be [n_boot, n_paths]")
    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".abundance")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_abundance_boot_from_ecs(C.byref(v), C.c_uint64(len(count)), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                                        _ffi.as_ptr(count, C.c_uint64), C.c_double(min_reads), C.c_uint32(n_boot), C.c_uint64(seed),
                                                        _ffi.as_ptr(boot_alpha, C.c_double) if boot_alpha is not None else None, C.c_uint32(threads),
                                                        (out_path or tmp).encode(), C.byref(n), None))
        rows = _abundance_boot_rows(out_path or tmp)
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return rows


def report_abundance_boot(bam_path, n_boot, seed=1, threads=1, min_reads=1.0, out_path=None):
    """groot_host_report_abundance_boot: the abundance lines of a BAM with the bootstrap columns"""
    import tempfile

    tmp = None
    if out_path is None:
        fd, tmp = tempfile.mkstemp(suffix=".abundance")
        os.close(fd)
    n = C.c_uint64(0)
    try:
        _check(lib().groot_host_report_abundance_boot(bam_path.encode(), C.c_double(min_reads), C.c_uint32(n_boot), C.c_uint64(seed), C.c_uint32(threads),
                                                      (out_path or tmp).encode(), C.byref(n)))
        rows = _abundance_boot_rows(out_path or tmp)
    finally:
        if tmp:
            os.unlink(tmp)
    assert len(rows) == n.value
    return rows


# ---- rarefaction curves (groot_host.h "rarefaction curves") ----------------------------------------------------------------
RAREFY_STEPS, RAREFY_REPS = 10, 20


def rarefy_depths(n_units, n_steps=RAREFY_STEPS):
    """groot_host_rarefy_depths: m_s of the steps s = 1 .. n_steps (zeros included) -> uint64[n_steps]"""
    m = np.zeros(max(n_steps, 1), dtype=np.uint64)
    _check(lib().groot_host_rarefy_depths(n_units, n_steps, _ffi.as_ptr(m, C.c_uint64)))
    return m[:n_steps]


def em_rarefy(n_paths, off, ids, count, n_rep, depths, seed=1, min_iter=EM_MIN_ITER, max_iter=EM_MAX_ITER, threads=1):
    """groot_host_em_rarefy: n_rep nested subsamples without replacement of the ECs' units at the given depths, the EM on each ->
    (rare_count uint64[n_rep, n_depths, n_ec], alpha float64[n_rep, n_depths, n_paths], iterations uint32[n_rep, n_depths])"""
    off, ids, count = _ec_arrays(off, ids, count)
    depths = np.ascontiguousarray(depths, dtype=np.uint64).reshape(-1)
    rc = np.zeros((n_rep, len(depths), len(count)), dtype=np.uint64)
    alpha = np.zeros((n_rep, len(depths), n_paths), dtype=np.float64)
    its = np.zeros((n_rep, len(depths)), dtype=np.uint32)
    _check(lib().groot_host_em_rarefy(n_paths, len(count), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32), _ffi.as_ptr(count, C.c_uint64), n_rep,
                                      len(depths), _ffi.as_ptr(depths, C.c_uint64), seed, min_iter, max_iter, threads, _ffi.as_ptr(rc, C.c_uint64),
                                      _ffi.as_ptr(alpha, C.c_double), _ffi.as_ptr(its, C.c_uint32)))
    return rc, alpha, its


def rarefy_from_ecs(index, off, ids, count, out_path, n_rep=RAREFY_REPS, n_steps=RAREFY_STEPS, seed=1, threads=1, min_reads=1.0, rare_count=None, rare_alpha=None,
                    tuples=None, tn=None, call_depth=1.0, cov_cutoff=0.97, covered=None):
    """groot_host_rarefy_from_ecs: writes the rarefaction file of a run's ECs; rare_count / rare_alpha (device.em_rarefy over the canonical
    ECs at the drawn depths) and covered (device.call_support) None = computed inside on `threads` host threads.  tuples / tn (the
    table of acov_merge, ECs canonical) add the three called columns.  Returns the number of lines."""
    off, ids, count = _ec_arrays(off, ids, count)
    with_calls = tuples is not None
    if with_calls:
        tuples, tn = _tuple_arrays(tuples, tn)
    rare_count = None if rare_count is None else np.ascontiguousarray(rare_count, dtype=np.uint64)
    rare_alpha = None if rare_alpha is None else np.ascontiguousarray(rare_alpha, dtype=np.float64)
    covered = None if covered is None else np.ascontiguousarray(covered, dtype=np.uint32)
    n_sel = 0 if covered is None else (covered.shape[-1] if covered.ndim >= 2 else 0)
    nl = C.c_uint64(0)
    _check(lib().groot_host_rarefy_from_ecs(C.byref(index.view), len(count), _ffi.as_ptr(off, C.c_uint64), _ffi.as_ptr(ids, C.c_uint32),
                                            _ffi.as_ptr(count, C.c_uint64), min_reads, n_rep, n_steps, seed, threads, _ffi.opt_ptr(rare_count, C.c_uint64),
                                            _ffi.opt_ptr(rare_alpha, C.c_double), 1 if with_calls else 0, len(tn) if with_calls else 0,
                                            _ffi.opt_ptr(tuples, C.c_uint32), _ffi.opt_ptr(tn, C.c_uint64), call_depth, cov_cutoff, n_sel,
                                            _ffi.opt_ptr(covered, C.c_uint32), out_path.encode(), C.byref(nl)))
    return nl.value


def report_rarefy(bam_path, out_path, n_rep=RAREFY_REPS, n_steps=RAREFY_STEPS, seed=1, threads=1, min_reads=1.0, calls=False, call_depth=1.0, cov_cutoff=0.97):
    """groot_host_report_rarefy: the rarefaction file of a BAM (calls=True: with the three called columns).  Returns the number of lines."""
    nl = C.c_uint64(0)
    _check(lib().groot_host_report_rarefy(bam_path.encode(), min_reads, n_rep, n_steps, seed, threads, 1 if calls else 0, call_depth, cov_cutoff,
                                          out_path.encode(), C.byref(nl), None))
    return nl.value


def save_gfa(index, graph, kmer_freq, path_kept, node_removed, total_kmers, file_name, timestamp=None):
    """GrootGraph.SaveGraphAsGFA (src/graph/graphio.go:19-112); returns True if a file was written"""
    kf = np.ascontiguousarray(kmer_freq, dtype=np.float64)
    pk = np.ascontiguousarray(path_kept, dtype=np.uint8)
    nr = np.ascontiguousarray(node_removed, dtype=np.uint8)
    written = C.c_int(0)
    _check(lib().groot_host_save_gfa(C.byref(index.view), C.c_uint32(graph), _ffi.as_ptr(kf, C.c_double), _ffi.as_ptr(pk, C.c_uint8),
                                     _ffi.as_ptr(nr, C.c_uint8), C.c_uint64(total_kmers), timestamp.encode() if timestamp else None,
                                     file_name.encode(), C.byref(written)))
    return bool(written.value)


# ---- assignment: each read to its best allele by EM posterior (groot_host.h "assignment") ----------------------------------
class AssignStats(C.Structure):
    """groot_assign_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("reads", "assigned", "unassigned", "below", "ties", "records_in", "records_kept", "travs_emptied", "launches")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def assign_travs(index, alpha, min_posterior, travs, masks, first_read_id, n_reads):
    """groot_host_assign_travs: the definition on the CPU.  travs (device.TRAV_DTYPE, (read, ord) order) and masks [n, path_words] are
    copied, not changed -> (travs, masks, best uint32[n_reads], mapq uint8[n_reads], stats dict without "launches")"""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    if len(alpha) != index.view.n_paths:
        raise ValueError("alpha must have n_paths values")
    t = np.array(travs, copy=True, order="C")
    if t.dtype.itemsize != 20:
        raise ValueError("travs must be groot_trav records")
    m = np.array(masks, dtype=np.uint64, copy=True, order="C").reshape(len(t), index.view.path_words)
    best = np.zeros(n_reads, dtype=np.uint32)
    mapq = np.zeros(n_reads, dtype=np.uint8)
    st = AssignStats()
    _check(lib().groot_host_assign_travs(C.byref(index.view), _ffi.as_ptr(alpha, C.c_double), C.c_double(min_posterior), t.ctypes.data_as(C.c_void_p),
                                         _ffi.as_ptr(m, C.c_uint64), C.c_uint64(len(t)), C.c_uint32(first_read_id), C.c_uint32(n_reads),
                                         _ffi.as_ptr(best, C.c_uint32), _ffi.as_ptr(mapq, C.c_uint8), C.byref(st)))
    d = st.as_dict()
    del d["launches"]
    return t, m, best, mapq, d


def abundance_read(index, path):
    """groot_host_abundance_read: an abundance file (4 or 8 columns) -> (alpha float64[n_paths], lines)"""
    alpha = np.zeros(index.view.n_paths, dtype=np.float64)
    n = C.c_uint64(0)
    _check(lib().groot_host_abundance_read(C.byref(index.view), path.encode(), _ffi.as_ptr(alpha, C.c_double), C.byref(n)))
    return alpha, n.value


def bam_write_rescued_gapped(writer, records, gap_records, names, seqs, quals):
    """groot_bam_write_rescued_gapped on an open BamWriter: one BAM record per entry of both lists of a batch (device.RESCUE_RECORD_DTYPE,
    device.GAP_RECORD_DTYPE), merged by read -> the number of records written"""
    return writer.write_rescued(records, names, seqs, quals, gap_records=gap_records)
