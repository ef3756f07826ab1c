"""Batch after batch through ONE groot_ctx: the statistics of the latest finished batch choose how the next one runs (groot_hip.hip,
refreshed at collect l.914-929): the processing order (radix sort or stream compaction, or the list the text lookup appends itself),
whether a first pass runs and how many workgroups it gets, how large align_kernel's persistent grid is, whether the outcome table's
text lookup is tried, how much of the results the copy-out behind the kernels takes.  None of that may change a result: every batch of
these scripted streams equals a fresh oracle run of the same reads -- counters, seeds, every record field, the call-count delta.

Each case first asserts, from the observed counts of the batch before it, the state that puts the batch on its path (HEUR mirrors the
constants), so a retuned heuristic makes the case fail loudly instead of passing beside the path it was written for."""
import numpy as np
import pytest

import oracle_check
from groot_amd import device, synth
from oracle import oracle_py as O
from test_coverage import clipped_reads, expand_coverage
from test_shared_reads import _multi_graph_reads
from test_signature_path import mixed_batch

pytestmark = pytest.mark.gpu

# The launch choices of groot_hip.hip as of this module (line numbers of that file):
HEUR = dict(
    block=256,            # kBlock: lanes per workgroup
    no_first_pass=0.02,   # dfs_frac below which no first pass runs (l.551-552)
    sparse=0.05,          # kSparseBelow: stream compaction instead of the radix sort, list mode of the text lookup (l.127, 238-239, 309-322, 378)
    dense=0.6,            # dfs_frac below which align_kernel's grid is halved and refill is 48 (l.173, 382, 414)
    shrink=0.25,          # lean_left_frac below which align_kernel's grid is cut to max(want, n_cu) workgroups (l.387-390)
    spare_blocks=64,      # the first pass's workgroups beyond dfs_frac * 1.05 * n / 256 (l.445)
    slack=1.05,
    left_slack=1.25,      # want = lean_left_frac * 1.25 * n / 64 / 4 + 1 (l.388)
    max_first_len=256,    # kLeanMaxLen (device_types.hpp): longest read the first pass takes
    text_hit=0.7,         # share of a batch the text lookup answered above which it is used for the next batch (l.240)
    text_gap=8,           # ... else it is tried again after 8, 16, ... 256 batches (ctx.hpp groot_ctx::text_retry_gap, l.932)
    text_gap_max=256,
)
N_CU = 256                # compute units of an MI355X: the floor of the shrunk grid

STAGES = {"path": {}, "lean": {"GROOT_LEAN": "1"}, "no_path": {"GROOT_NO_PATH_PASS": "1"}}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    assert device.device_count() > 0, "no MI355X visible: the HIP path has no CPU fallback"


@pytest.fixture(params=sorted(STAGES))
def stage(request, monkeypatch):
    for v in ("GROOT_NO_PATH_PASS", "GROOT_LEAN", "GROOT_NO_SIG", "GROOT_NO_TEXT_TABLE", "GROOT_NO_OUTCOME_TABLE", "GROOT_TEST_SMALL_BUFFERS",
              "GROOT_TEST_POISON"):
        monkeypatch.delenv(v, raising=False)
    for k, v in STAGES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


# ---- inputs: made once per module, keyed by name --------------------------------------------------------------------------------

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rows(reads):
    return O.pack_reads([bytes(r) for r in reads])


def _perfect(index, n, first, L=100):
    cat, o, lens = synth.reference_sequences(index)
    seq, off, _ = synth.reads_np(cat, o, lens, n, L, first=first)
    return seq, off


def _random(n, L, seed):
    """random ACGT reads: no seed window, never walked"""
    return np.random.default_rng(seed).choice(_ACGT, n * L), np.arange(n + 1, dtype=np.uint64) * L


def _sparse(index, n, walk, first, seed):
    """n 100-mers of which `walk` are error-free (walked with the memo off) and the rest random, shuffled"""
    p, _ = _perfect(index, walk, first)
    r, _ = _random(n - walk, 100, seed)
    rows = np.concatenate([p.reshape(-1, 100), r.reshape(-1, 100)])
    np.random.default_rng(seed).shuffle(rows, axis=0)
    return rows.reshape(-1).copy(), np.arange(n + 1, dtype=np.uint64) * 100


def _substituted(seq, rate, seed):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    hit = rng.random(len(out)) < rate
    code = np.searchsorted(_ACGT, np.where(np.isin(out, _ACGT), out, ord("A")))
    out[hit] = _ACGT[(code[hit] + 1 + rng.integers(0, 3, int(hit.sum()))) % 4]
    return out


def _edge_n(index, n, first, seed):
    """error-free 100-mers with an N on their first or last base: most keep every minimiser and are walked, and every first pass
    leaves them to align_kernel (a byte other than ACGT)"""
    seq, off = _perfect(index, n, first)
    rows = seq.reshape(-1, 100).copy()
    at = np.where(np.random.default_rng(seed).integers(0, 2, n) == 0, 0, 99)
    rows[np.arange(n), at] = ord("N")
    return rows.reshape(-1).copy(), off


def _unanswerable(index, n, first, seed):
    """100-mers the outcome table cannot answer: 95 % random, 5 % with an N on an end (most of those are walked: about 3 % of the batch)"""
    k = n * 5 // 100
    p, _ = _edge_n(index, k, first, seed)
    r, _ = _random(n - k, 100, seed + 1)
    rows = np.concatenate([p.reshape(-1, 100), r.reshape(-1, 100)])
    np.random.default_rng(seed).shuffle(rows, axis=0)
    return rows.reshape(-1).copy(), np.arange(n + 1, dtype=np.uint64) * 100


def _with_long(index, L, first):
    """19 800 error-free 100-mers (walked: the ctx keeps choosing a first pass) and 200 reads of L bases (reads longer than the index's
    windows have no seed): the batch's longest read is L"""
    a, _ = _perfect(index, 19_800, first)
    b, _ = _perfect(index, 200, first + 19_800, L)
    reads = [a[i * 100:(i + 1) * 100].tobytes() for i in range(19_800)] + [b[i * L:(i + 1) * L].tobytes() for i in range(200)]
    np.random.default_rng(L).shuffle(reads)
    return _rows(reads)


def _graph_of_path(index):
    gpo = index.arrays["graph_path_off"].astype(np.int64)
    return np.repeat(np.arange(len(gpo) - 1), np.diff(gpo)), np.diff(gpo)


def _single_path(index, n, seed):
    """100-mers of graphs that hold one path: one byte of path set per record"""
    cat, o, lens = synth.reference_sequences(index)
    gop, npg = _graph_of_path(index)
    ok = np.flatnonzero((npg[gop] == 1) & (lens >= 100))
    rng = np.random.default_rng(seed)
    p = ok[rng.integers(0, len(ok), n)]
    st = (rng.random(n) * (lens[p] - 99)).astype(np.int64)
    return _rows([cat[o[q] + s:o[q] + s + 100].tobytes() for q, s in zip(p, st)])


def _wide_reads(index, step=31):
    """100-mers along every path of the graph with the most paths (sets of more than 64 paths)"""
    cat, o, lens = synth.reference_sequences(index)
    gpo = index.arrays["graph_path_off"].astype(np.int64)
    wide = int(np.argmax(np.diff(gpo)))
    out = []
    for p in range(int(gpo[wide]), int(gpo[wide + 1])):
        s = bytes(cat[int(o[p]):int(o[p]) + int(lens[p])])
        out += [s[i:i + 100] for i in range(0, max(1, len(s) - 100), step)]
    return out


def _make(index, name):
    if name == "sparse3":                       # dfs in [0.02, 0.05): compaction order, the first pass on a narrow grid
        return _sparse(index, 100_000, 3_000, 10_000_000, 1)
    if name == "sparse30":                      # dfs in [0.05, 0.6): radix order, halved grid, refill 48
        return _sparse(index, 100_000, 30_000, 11_000_000, 2)
    if name == "sparse1":                       # dfs < 0.02: no first pass next
        return _sparse(index, 100_000, 1_000, 12_000_000, 3)
    if name == "full200k":
        return _perfect(index, 200_000, 1_000_000)
    if name == "exact_and_sub":
        a, _ = _perfect(index, 60_000, 13_000_000)
        b, _ = _perfect(index, 60_000, 14_000_000)
        rows = np.concatenate([a.reshape(-1, 100), _substituted(b, 0.01, 4).reshape(-1, 100)])
        np.random.default_rng(4).shuffle(rows, axis=0)
        return rows.reshape(-1).copy(), np.arange(120_001, dtype=np.uint64) * 100
    if name == "finish100k":
        return _perfect(index, 100_000, 2_000_000)
    if name == "long300":
        return _with_long(index, 300, 3_000_000)
    if name == "edge_n400k":
        return _edge_n(index, 400_000, 4_000_000, 5)
    if name.startswith("exact20k_"):
        return _perfect(index, 20_000, 5_000_000 + 100_000 * int(name.split("_")[1]))
    if name == "tier100":
        return _perfect(index, 20_000, 6_000_000)
    if name.startswith("tier"):
        return _with_long(index, int(name[4:]), 6_000_000 + 1000 * int(name[4:]))
    if name == "memo_exact":
        return _perfect(index, 6_000, 7_000_000)
    if name == "memo_exact2":
        return _perfect(index, 6_000, 7_100_000)
    if name == "memo_mixed":
        return mixed_batch(index, 6000, seed=17)
    if name.startswith("miss_"):
        return _unanswerable(index, 2_000, 7_200_000 + 2_000 * int(name[5:]), 100 + int(name[5:]))
    if name == "unmapped20k":
        return _random(20_000, 100, 9)
    if name == "wide_multi":
        return _rows(_multi_graph_reads(index, 400, 71) + _wide_reads(index) + clipped_reads(index, 2000, 73, 100, 150))
    if name == "single20k":
        return _single_path(index, 20_000, 10)
    if name == "wide_in_random":
        w = _wide_reads(index)
        r, _ = _random(20_000 - len(w), 100, 11)
        reads = w + [r[i * 100:(i + 1) * 100].tobytes() for i in range(20_000 - len(w))]
        np.random.default_rng(11).shuffle(reads)
        return _rows(reads)
    raise KeyError(name)


_INPUTS, _ORACLE = {}, {}


def _input(index, name):
    if name not in _INPUTS:
        seq, off = _make(index, name)
        _INPUTS[name] = (np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64))
    return _INPUTS[name]


def _oracle(index, name):
    """the oracle's answer for one input as a batch of its own (first read id 0): the same whatever the stage, made once"""
    if name not in _ORACLE:
        run = oracle_check.oracle_run(index, *_input(index, name))
        _ORACLE[name] = {"counts": run.counts(), "seeds": run.seeds().astype(device.SEED_DTYPE), "alns": run.alns().astype(device.ALN_DTYPE),
                         "attempts": run.attempts().copy()}
        del run
    return _ORACLE[name]


# ---- the ctx's statistics, mirrored from the observed counts ----------------------------------------------------------------------

def _mask_bytes(index, travs):
    """compact path-set bytes of these records: max(1, ceil(paths of the graph / 8)) each (groot_hip.hip h_graph_words)"""
    gop, npg = _graph_of_path(index)
    return int(np.maximum(1, (npg[travs["graph_id"].astype(np.int64)] + 7) // 8).sum())


def lean_slots(dfs, n):
    """slots the first pass takes (l.445); the walked reads beyond them go to align_kernel behind the list the pass leaves (l.452-455)"""
    B = HEUR["block"]
    return min((n + B - 1) // B, int(dfs * HEUR["slack"] * n / B) + HEUR["spare_blocks"]) * B


def shrunk_lanes(left, n):
    """lanes of align_kernel's grid when the batch before left less than HEUR["shrink"] to it (l.387-390), at most"""
    want = int(left * HEUR["left_slack"] * n / 64.0 / (HEUR["block"] / 64)) + 1
    return max(want, N_CU) * HEUR["block"]


def copy_out(tpr, bpt, n, pw=3):
    """(records, path-set bytes) the copy-out behind the kernels takes (l.727-731)"""
    margin = 1.0 + max(0.01, 4.0 / np.sqrt(n + 1.0))
    copied = int(n * tpr * margin) + 1024
    return copied, int(copied * (bpt if bpt > 0 else 8.0 * pw) * margin) + 4096


class Mirror:
    """what the ctx remembers of its latest finished batch (l.914-929) and what that selects for the next one (l.173-445)"""

    def __init__(self, stage, memo=False):
        self.stage, self.memo = stage, memo
        self.dfs, self.left, self.tpr, self.bpt = 1.0, 1.0, 1.25, 0.0
        self.text_hit, self.text_gap, self.without = 1.0, HEUR["text_gap"], 0

    # -- what the next batch (n reads, longest max_len) gets --
    def first_pass(self, max_len):
        return self.stage != "no_path" and max_len <= HEUR["max_first_len"] and self.dfs >= HEUR["no_first_pass"]

    def lean_slots(self, n):
        return lean_slots(self.dfs, n)

    def shrunk_lanes(self, n):
        return shrunk_lanes(self.left, n)

    def copy_out(self, n):
        return copy_out(self.tpr, self.bpt, n)

    def text_try(self):
        """(l.240; the counter is advanced only when the first operand is false)"""
        if self.text_hit >= HEUR["text_hit"]:
            return True
        return self.without + 1 >= self.text_gap

    # -- the batch has finished --
    def update(self, b, text_used=None):
        c, n = b["counts"], b["counts"]["received"]
        if not n:
            return
        first = self.first_pass(b["max_len"])
        if self.stage == "path":
            assert b["pp"]["ran"] == first, ("the first pass ran where the mirror says it does not, or the other way round", b["pp"], self.dfs)
        self.tpr = c["travs"] / n
        self.dfs = c["walked_reads"] / n
        if first:
            fin = b["pp"]["reads"] if self.stage == "path" else c["lean_reads"]
            self.left = (c["walked_reads"] - min(c["walked_reads"], fin)) / n
        if self.memo and text_used is not None:
            if not text_used and self.text_hit < HEUR["text_hit"]:
                self.without += 1
            if text_used:
                self.without = 0
                self.text_hit = 1.0 - c["full_sketch_reads"] / n
                self.text_gap = HEUR["text_gap"] if self.text_hit >= HEUR["text_hit"] else min(HEUR["text_gap_max"], 2 * self.text_gap)
            else:
                self.text_hit = 0.0     # (tab_reads / n, not a count the API gives: the unanswerable batches below hold no table string)
        if c["travs"] and "mask_bytes" in b:
            self.bpt = b["mask_bytes"] / c["travs"]


def _finished(stage, b):
    """reads the first pass finished"""
    return b["pp"]["reads"] if stage == "path" else b["counts"]["lean_reads"]


# ---- one batch, compared -------------------------------------------------------------------------------------------------------

def _check(al, index, name, att, where=""):
    """one batch through `al` (wait), compared with the oracle's answer for the same input; returns what the batch's successor is chosen by"""
    seq, off = _input(index, name)
    al.submit(seq, off)
    counts = al.wait()
    o = _oracle(index, name)
    where = (where, name)
    for k in oracle_check.COUNTS:
        assert counts[k] == o["counts"][k], (where, k, counts[k], o["counts"][k])
    assert np.array_equal(al.seeds(), o["seeds"]), (where, "seeds")
    t, m = al.travs()
    got, exp = device.expand_alns(index, t, m), o["alns"]
    assert len(got) == len(exp), (where, "alignments", len(got), len(exp))
    for f in exp.dtype.names:
        assert np.array_equal(got[f], exp[f]), (where, f, np.flatnonzero(got[f] != exp[f])[:8])
    a2 = al.attempts().copy()
    delta = a2.astype(np.int64)
    delta[: att.shape[0]] -= att
    oatt = o["attempts"]
    assert np.array_equal(delta[: oatt.shape[0]], oatt) and not delta[oatt.shape[0]:].any(), (where, "call counts")
    lens = np.diff(off.astype(np.int64))
    return {"name": name, "counts": counts, "pp": al.path_pass_stats(), "max_len": int(lens.max()), "n": len(lens),
            "mask_bytes": _mask_bytes(index, t)}, a2


def _open(index, R, **kw):
    return device.Aligner(index, max_batch_reads=R, max_read_len=kw.pop("max_read_len", 256), memo_budget_mb=kw.pop("memo_budget_mb", device.MEMO_OFF), **kw)


def _sequence(al, index, stage, names, check_each=None, memo=False):
    """the batches in order; check_each(i, mirror before batch i, result of batch i - 1) asserts the preconditions"""
    att = np.zeros((0, index.view.n_windows), dtype=np.uint32)
    mir, prev, out = Mirror(stage, memo), None, []
    for i, name in enumerate(names):
        _input(index, name)
        if check_each:
            check_each(i, mir, prev)
        b, att = _check(al, index, name, att, where=(stage, i))
        mir.update(b)
        out.append(b)
        prev = b
    return out, mir


# ---- 1. the first pass on a grid sized by a sparse batch: slots beyond it go straight to align_kernel -------------------------------

@pytest.mark.parametrize("sparse", ["sparse3", "sparse30"])
def test_first_pass_too_narrow(argannot_index, stage, sparse):
    """a sparse batch (3 % / 30 % walked), then 200 000 error-free reads: the first pass gets dfs * 1.05 * n / 256 + 64 workgroups, the
    walked reads in slots past them reach align_kernel through LeanLeft's `i >= lean_slots` arm (list-mode / radix order respectively)"""
    index = argannot_index
    al = _open(index, 200_000)
    try:
        seen = {}

        def pre(i, mir, prev):
            if i == 1:
                lo, hi = (HEUR["no_first_pass"], HEUR["sparse"]) if sparse == "sparse3" else (HEUR["sparse"], HEUR["dense"])
                assert lo <= mir.dfs < hi, ("the sparse batch's walked share is off the path", mir.dfs)
                seen["slots"] = mir.lean_slots(200_000)

        (_, b), _ = _sequence(al, index, stage, [sparse, "full200k"], pre)
    finally:
        al.close()
    if stage != "no_path":
        slots = seen["slots"]
        assert b["counts"]["walked_reads"] >= slots + 50_000, (b["counts"], slots)
        assert 0 < _finished(stage, b) <= slots, (b["pp"], b["counts"], slots)


# ---- 2. no first pass after a batch with fewer than 2 % walked ----------------------------------------------------------------------

def test_no_first_pass_after_a_sparse_batch(argannot_index, stage):
    index = argannot_index
    al = _open(index, 120_000)
    try:
        def pre(i, mir, prev):
            if i == 1:
                assert mir.dfs < HEUR["no_first_pass"], mir.dfs
                assert not mir.first_pass(100)

        (_, b), _ = _sequence(al, index, stage, ["sparse1", "exact_and_sub"], pre)
    finally:
        al.close()
    assert b["counts"]["walked_reads"] > 50_000, b["counts"]
    assert not b["pp"]["ran"] and b["counts"]["lean_reads"] == 0, (b["pp"], b["counts"])


# ---- 3. align_kernel's grid cut to what the first pass left in the batch before ------------------------------------------------------

@pytest.mark.parametrize("between", ["none", "long"])
def test_second_pass_shrunk(argannot_index, stage, between):
    """a batch the first pass nearly finishes, then 400 000 reads it leaves to align_kernel (an N on their first or last base): the
    persistent grid is max(want, n_cu) workgroups, far fewer lanes than reads; `long`: a batch with 300-base reads in between (no first
    pass: the share it left stays that of the error-free batch).  Then two small error-free batches: the second one reuses the work set of
    the N batch, whose first-pass flags must not leak into it."""
    index = argannot_index
    names = ["finish100k"] + (["long300"] if between == "long" else []) + ["edge_n400k", "exact20k_0", "exact20k_1"]
    ix = names.index("edge_n400k")
    al = _open(index, 400_000, max_read_len=320)
    try:
        seen = {}

        def pre(i, mir, prev):
            if i == ix and stage != "no_path":
                assert mir.first_pass(100) and mir.left < HEUR["shrink"], (mir.left, mir.dfs)
                seen["lanes"] = mir.shrunk_lanes(400_000)
            if names[i] == "edge_n400k" and between == "long":
                assert prev["max_len"] > HEUR["max_first_len"] and not prev["pp"]["ran"] and prev["counts"]["lean_reads"] == 0

        bs, _ = _sequence(al, index, stage, names, pre)
    finally:
        al.close()
    b = bs[ix]
    if stage != "no_path":
        left = b["counts"]["walked_reads"] - _finished(stage, b)
        assert left >= 3 * seen["lanes"], (left, seen["lanes"], b["counts"], b["pp"])
        assert _finished(stage, bs[-1]) > 0.5 * bs[-1]["counts"]["walked_reads"]


# ---- 4. read-length tiers through the same work sets ---------------------------------------------------------------------------------

def test_read_length_tiers(argannot_index, stage):
    """longest read <= 128 bases (2-bit codes in 2 words), 129-256 (4 words), > 256 (no first pass), <= 128 again, on a ctx opened for 320
    (the batches after the first hold 200 reads of the tier's length among 100-mers: longer reads have no seed in windows of 100)"""
    index = argannot_index
    names = ["tier100", "tier200", "tier300", "tier120"]
    al = _open(index, 20_000, max_read_len=320)
    try:
        bs, _ = _sequence(al, index, stage, names)
    finally:
        al.close()
    assert [b["max_len"] for b in bs] == [100, 200, 300, 120]
    for b in bs:
        ran = b["pp"]["ran"] or b["counts"]["lean_reads"] > 0
        assert ran == (stage != "no_path" and b["max_len"] <= HEUR["max_first_len"]), (b["name"], b["pp"], b["counts"])


# ---- 5. memo on: the text lookup, its list mode and its retries ----------------------------------------------------------------------

def test_text_lookup_history(argannot_index, stage):
    """error-free reads (the text lookup answers them), a mixed batch (the lookup, in list mode: it appends the processing order itself),
    22 batches of 2 000 reads the lookup cannot answer (the first tries it and misses: the next try comes 16 batches later), error-free
    reads again.  Which route a batch took is not a count the API gives (full_sketch_reads is the list pass's share on either route):
    the retry batch is derived from the constants, and the walked share before it shows list mode."""
    index = argannot_index
    n_miss = 22
    names = ["memo_exact", "memo_mixed"] + ["miss_%d" % i for i in range(n_miss)] + ["memo_exact2"]
    al = _open(index, 8192, memo_budget_mb=0)
    assert al.open_stats()["text_entries"] > 0
    att = np.zeros((0, index.view.n_windows), dtype=np.uint32)
    mir, tried, bs = Mirror(stage, memo=True), [], []
    try:
        for i, name in enumerate(names):
            use = mir.text_try()
            tried.append(use)
            if name == "memo_mixed":
                assert use and mir.dfs < HEUR["sparse"], (mir.text_hit, mir.dfs)       # the lookup in list mode
            b, att = _check(al, index, name, att, where=(stage, i))
            mir.update(b, text_used=use)
            bs.append(b)
    finally:
        al.close()
    miss = [i for i, n in enumerate(names) if n.startswith("miss_")]
    assert 1 - bs[0]["counts"]["full_sketch_reads"] / bs[0]["n"] >= HEUR["text_hit"], bs[0]["counts"]
    assert 1 - bs[1]["counts"]["full_sketch_reads"] / bs[1]["n"] >= HEUR["text_hit"], bs[1]["counts"]
    retries = [i for i in miss if tried[i]]
    # the first unanswerable batch still tries the lookup (the mixed one was answered), then once more 2 * 8 batches later
    assert retries == [miss[0], miss[0] + 2 * HEUR["text_gap"]], (retries, tried)
    r = retries[1]
    assert bs[r - 1]["counts"]["walked_reads"] / bs[r - 1]["n"] < HEUR["sparse"], bs[r - 1]["counts"]    # the retry is in list mode


# ---- 6. a copy-out sized by a batch with few, narrow records -------------------------------------------------------------------------

@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("kind", ["unmapped", "single_path"])
def test_copy_out_prediction_too_small(argannot_index, stage, kind, rod):
    """`unmapped`: random reads (no record: 0 records per read predicted), then reads in several graphs and on the widest graph's paths
    (records and path-set bytes past the copy-out); `single_path`: reads of one-path graphs (1 byte per record), then the widest graph's
    reads among random ones (fewer records than predicted, path-set bytes past the copy-out).  Collect fetches the rest; with results
    on the device nothing is copied out."""
    index = argannot_index
    names = ["unmapped20k", "wide_multi"] if kind == "unmapped" else ["single20k", "wide_in_random"]
    al = _open(index, 20_000, results_on_device=rod)
    try:
        seen = {}

        def pre(i, mir, prev):
            if i == 1:
                seen["pred"] = mir.copy_out(len(_input(index, names[1])[1]) - 1)

        bs, _ = _sequence(al, index, stage, names, pre)
    finally:
        al.close()
    copied, copied_bytes = seen["pred"]
    b = bs[1]
    if kind == "unmapped":
        assert bs[0]["counts"]["travs"] == 0 and b["counts"]["travs"] > copied, (b["counts"], copied)
    else:
        assert b["counts"]["travs"] <= copied, (b["counts"], copied)
    assert b["mask_bytes"] > copied_bytes, (b["mask_bytes"], copied_bytes)
    oa = _oracle(index, names[1])["alns"]
    assert np.bincount(np.unique(oa["read_id"].astype(np.int64) * 4096 + oa["ref_id"]) >> 12).max() > 64      # sets past one mask word


# ---- 7 / 8. pipelined: three batches in flight, statistics that lag ------------------------------------------------------------------

PIPE = ["sparse3", "finish100k", "unmapped20k", "full200k", "edge_n400k", "wide_multi", "sparse30", "single20k", "exact20k_0", "wide_in_random"]


def _sets(alns):
    """{read: frozenset of refs} -> the pairs and ECs of test_shared_reads / test_abundance, over distinct (read, ref) keys in numpy"""
    key = np.unique(alns["read_id"].astype(np.int64) * 4096 + alns["ref_id"].astype(np.int64))
    rid, ref = key >> 12, key & 4095
    starts = np.flatnonzero(np.r_[True, rid[1:] != rid[:-1]])
    sets = {}
    for s, e in zip(starts, np.r_[starts[1:], len(rid)]):
        t = ref[s:e].tobytes()
        sets[t] = sets.get(t, 0) + 1
    return {tuple(np.frombuffer(t, dtype=np.int64).tolist()): c for t, c in sets.items()}


@pytest.mark.parametrize("accumulate", [False, True])
def test_pipelined(argannot_index, stage, accumulate):
    """cases 1, 3 and 6 interleaved with pipeline_depth=3, collected oldest first: a batch is launched with the statistics of whichever batch
    finished last, up to three behind, so which launch choices it got is timing (the script holds sparse, nearly finished, left-behind,
    unmapped and wide batches next to each other).  Counts and records of every batch equal the oracle's, the call-count table equals the
    oracle's over the stream; `accumulate`: coverage, shared reads and ECs over the stream equal those of the oracle's records."""
    index = argannot_index
    R = max(len(_input(index, n)[1]) - 1 for n in PIPE)
    al = _open(index, R, pipeline_depth=3)
    if accumulate:
        al.coverage_enable()
        al.shared_enable()
        al.ec_enable()
    firsts, first = [], 0
    for n in PIPE:
        firsts.append(first)
        first += len(_input(index, n)[1]) - 1
    got = []
    try:
        def take():
            r = al.collect()
            al.release(r["ticket"])
            got.append(r)

        for i, n in enumerate(PIPE):
            seq, off = _input(index, n)
            al.submit(seq, off, first_read_id=firsts[i])
            if i >= 2:
                take()
        while len(got) < len(PIPE):
            take()
        att = al.attempts().copy()
        if accumulate:
            cov, pairs, ecs = al.coverage(), al.shared(), al.ecs()
    finally:
        al.close()
    dfs = []
    oatt = np.zeros_like(att, dtype=np.int64)
    all_alns = []
    for i, (n, r) in enumerate(zip(PIPE, got)):
        o = _oracle(index, n)
        assert r["first_read_id"] == firsts[i]
        for k in oracle_check.COUNTS:
            assert r["counts"][k] == o["counts"][k], (stage, i, n, k)
        a = device.expand_alns(index, r["travs"], r["masks"])
        a["read_id"] -= firsts[i]
        assert len(a) == len(o["alns"]), (stage, i, n)
        for f in o["alns"].dtype.names:
            assert np.array_equal(a[f], o["alns"][f]), (stage, i, n, f)
        oa = o["attempts"]
        oatt[: oa.shape[0]] += oa
        dfs.append(r["counts"]["walked_reads"] / r["counts"]["received"])
        g = o["alns"].copy()
        g["read_id"] += firsts[i]
        all_alns.append(g)
    assert np.array_equal(att.astype(np.int64), oatt)
    assert min(dfs) < HEUR["sparse"] and max(dfs) > HEUR["dense"], dfs
    if accumulate:
        alns = np.concatenate(all_alns)
        off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(_input(index, n)[1].astype(np.int64)) for n in PIPE]))])
        rec, depth = expand_coverage(index, alns, off)
        assert np.array_equal(cov[0], rec) and np.array_equal(cov[1], depth)
        sets = _sets(alns)
        want_pairs = {}
        for s, c in sets.items():
            for x in range(len(s)):
                for y in range(x, len(s)):
                    want_pairs[(s[x], s[y])] = want_pairs.get((s[x], s[y]), 0) + c
        dev_pairs = {(int(x), int(y)): int(z) for x, y, z in zip(*pairs)}
        assert dev_pairs == want_pairs
        eo, ei, ec = ecs
        dev_ecs = sorted((tuple(ei[eo[i]:eo[i + 1]].tolist()), int(ec[i])) for i in range(len(ec)))
        assert dev_ecs == sorted(sets.items())


# ---- 9. the same with what the seed stage leaves per read wiped first ----------------------------------------------------------------

@pytest.mark.parametrize("case", ["first_pass_too_narrow", "copy_out"])
def test_poisoned_work_sets(argannot_index, stage, monkeypatch, case):
    """GROOT_TEST_POISON=1: a work set's per-read buffers are wiped before the seed stage writes them, so nothing may rely on what the
    set's previous batch left there"""
    monkeypatch.setenv("GROOT_TEST_POISON", "1")
    index = argannot_index
    names = ["sparse3", "full200k"] if case == "first_pass_too_narrow" else ["unmapped20k", "wide_multi"]
    al = _open(index, 200_000 if case == "first_pass_too_narrow" else 20_000)
    try:
        bs, _ = _sequence(al, index, stage, names)
    finally:
        al.close()
    if case == "first_pass_too_narrow":
        assert HEUR["no_first_pass"] <= bs[0]["counts"]["walked_reads"] / bs[0]["n"] < HEUR["sparse"]
    else:
        assert bs[0]["counts"]["travs"] == 0 and bs[1]["counts"]["travs"] > 1024 * 4


# ---- 10. the same at the size bench.py runs ------------------------------------------------------------------------------------------

@pytest.mark.timeout(1800)
def test_after_a_sparse_batch_at_benchmark_size(argannot_index, monkeypatch):
    """10 M reads of which 3 % are walked, then the 10 M error-free reads of configs[2]: the second batch's records and path sets equal
    those of the same batch on a fresh ctx, read by read, and the oracle's on 20 000 of them"""
    import torch

    for v in ("GROOT_NO_PATH_PASS", "GROOT_LEAN", "GROOT_NO_SIG", "GROOT_TEST_POISON"):
        monkeypatch.delenv(v, raising=False)
    index = argannot_index
    dev = torch.device("cuda", 0)
    cat, o, lens = synth.reference_sequences(index)
    cat_t, off_t, lens_t = (torch.from_numpy(x).to(dev) for x in (cat, o, lens))
    R, L = 10_000_000, 100

    def reads(first):
        d = torch.zeros(R * L + 64, dtype=torch.uint8, device=dev)
        for c0 in range(0, R, 1_000_000):
            p, _, _ = synth.reads_torch(cat_t, off_t, lens_t, 1_000_000, L, first=first + c0)
            d[c0 * L:(c0 + 1_000_000) * L] = p[: 1_000_000 * L]
        return d

    d_off = torch.arange(0, R + 1, dtype=torch.int64, device=dev) * L
    sparse = reads(50_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    rows = sparse[: R * L].view(R, L)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    keep = torch.arange(R, device=dev) % 100 < 3
    for c0 in range(0, R, 1_000_000):
        blk = rows[c0:c0 + 1_000_000]
        rnd = acgt[torch.randint(0, 4, blk.shape, generator=g, device=dev)]
        rows[c0:c0 + 1_000_000] = torch.where(keep[c0:c0 + 1_000_000, None], blk, rnd)
    c2 = reads(0)
    torch.cuda.synchronize()

    def run(batches):
        al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, memo_budget_mb=device.MEMO_OFF)
        out = []
        try:
            for d in batches:
                al.submit_device(d.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
                c = al.wait()
                out.append((c, al.path_pass_stats()))
            t, m = al.travs()
            return out, t, m, al.attempts().copy()
        finally:
            al.close()

    hist, t, m, _ = run([sparse, c2])
    (c_sp, _), (c_b, pp_b) = hist
    dfs = c_sp["walked_reads"] / R
    assert HEUR["no_first_pass"] <= dfs < HEUR["sparse"], c_sp
    slots = lean_slots(dfs, R)
    assert pp_b["ran"] and c_b["walked_reads"] > slots + 50_000 and pp_b["reads"] <= slots, (c_b, pp_b, slots)
    fresh, tf, mf, _ = run([c2])
    (c_f, _), = fresh
    assert {k: v for k, v in c_b.items() if k != "lean_reads"} == {k: v for k, v in c_f.items() if k != "lean_reads"}
    assert np.array_equal(t, tf) and np.array_equal(m, mf)
    del tf, mf
    rng = np.random.default_rng(6)
    pick = np.sort(rng.choice(R, 20_000, replace=False))
    host_seq = c2[: R * L].view(R, L)[torch.from_numpy(pick).to(dev)].cpu().numpy().reshape(-1)
    orun = O.Run(index, 0.99)
    orun.batch(host_seq, np.arange(len(pick) + 1, dtype=np.uint64) * L)
    oal = orun.alns()
    sel = np.isin(t["read_id"], pick)
    got = device.expand_alns(index, t[sel], m[sel])
    assert len(got) == len(oal)
    assert np.array_equal(np.searchsorted(pick, got["read_id"]), oal["read_id"])
    for f in ("graph_id", "path_id", "ref_id", "pos", "start_clip", "end_clip", "rc", "secondary"):
        assert np.array_equal(got[f], oal[f]), f
