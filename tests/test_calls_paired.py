"""Assigned coverage over fragments (groot_hip_acov_pairs_enable, `align --calls --callsPaired`; the kPaired kernels of kernels_acov.hpp).

The rule is quoted in acov_pairs_def.py, which restates it over the CPU oracle's records: every expectation below comes from
paired_table_of_alns, never from device output -- tuples as sorted integer arrays, ECs, stats, no tolerance -- and every GPU test first
asserts, from those records, that its input holds the case it was written for.

The inputs are test_paired.py's case (a) (seven graphs sharing segments) and case (b) (the intersection empties the segment of a graph both
mates share), with fragments added to case (a) whose records are clipped or cut at path_len - 1.

One class of the issue cannot be built: "a mate with two records on one path, one per strand".  The aligner settles on one orientation per
(read, graph) -- the first seed that aligns ends the graph's search (oracle/groot_oracle.c, the loop of graphminion.go:57-95) -- and a path
lies in one graph, so no read has records on both strands of one path; test_calls.py found the same (FLOOR["both_strands_read"] = 0).  The
count is asserted to be what it is, 0, and the kernel reads no strand bit: a record is a record."""
import numpy as np
import pytest

import test_paired as tp
from acov_pairs_def import paired_table_of_alns, unit_sets_of_alns
from groot_amd import device, host, synth
from oracle import oracle_py as O
from test_calls import Table, _dev_table, merge_tables, table_of_alns
from test_counter_edges import L, THR, _bad_batch, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_path_pass import _COMP

case_a, case_b = tp.case_a, tp.case_b


# ---- expectations ---------------------------------------------------------------------------------------------------------------

class _Want:
    """what one batch of fragments adds, from the oracle's records of it"""

    def __init__(self, index, b):
        run = O.Run(index, THR)
        run.batch(b.seq, b.off)
        al = self.alns = run.alns().astype(device.ALN_DTYPE)
        self.n = b.n
        self.table, self.left = paired_table_of_alns(index, al, b.off)
        self.unit, self.joined_reads = unit_sets_of_alns(al, b.n)
        self.sets = [set() for _ in range(b.n)]
        for r, p in zip(al["read_id"].tolist(), al["ref_id"].tolist()):
            self.sets[r].add(p)
        gpo = index.arrays["graph_path_off"].astype(np.int64)
        self.graph_of = lambda p: int(np.searchsorted(gpo, p, side="right")) - 1
        self.lens = index.arrays["path_len"].astype(np.int64)
        assert int(self.table.n.sum()) + self.left == len(al)

    def joined(self):
        """the joined fragments"""
        return [i for i in range(self.n // 2) if self.sets[2 * i] & self.sets[2 * i + 1]]

    def unit_graphs(self, i):
        return len({self.graph_of(p) for p in self.sets[2 * i] & self.sets[2 * i + 1]})

    def slow_fragments(self, max_segs=4):
        return sum(1 for i in self.joined() if self.unit_graphs(i) > max_segs)


def _want(index, b):
    if getattr(b, "_cpw", None) is None:
        b._cpw = _Want(index, b)
    return b._cpw


def _classes(w):
    """how often the batch holds each case of the issue, from the oracle's records"""
    n = {k: 0 for k in ("A=B", "strict", "split", "single_even", "single_odd", "none", "clipped", "cut", "both_strands", "left_even", "left_odd")}
    for i in range(w.n // 2):
        a, b = w.sets[2 * i], w.sets[2 * i + 1]
        u = a & b
        n["A=B"] += bool(u) and a == b
        n["strict"] += bool(u) and u < a and u < b
        n["split"] += bool(a) and bool(b) and not u
        n["single_even"] += bool(a) and not b
        n["single_odd"] += bool(b) and not a
        n["none"] += not a and not b
    al = w.alns
    rid, ref, pos = al["read_id"].astype(np.int64), al["ref_id"].astype(np.int64), al["pos"].astype(np.int64)
    counts = np.array([p in w.unit[r] for r, p in zip(rid.tolist(), ref.tolist())], dtype=bool)
    m = L - al["start_clip"].astype(np.int64) - al["end_clip"].astype(np.int64)
    n["clipped"] = int((counts & ((al["start_clip"] > 0) | (al["end_clip"] > 0))).sum())        # counting records with a clip
    n["cut"] = int((counts & (pos + m > w.lens[ref] - 1)).sum())                               # counting records cut at path_len - 1
    n["left_even"], n["left_odd"] = int((~counts & (rid % 2 == 0)).sum()), int((~counts & (rid % 2 == 1)).sum())
    key = rid * 1024 + ref
    n["both_strands"] = len(set(key[al["rc"] == 0].tolist()) & set(key[al["rc"] == 1].tolist()))
    return n


FLOOR_A = {"A=B": 50, "strict": 50, "split": 50, "single_even": 50, "single_odd": 50, "none": 50, "clipped": 20, "cut": 20, "left_even": 50, "left_odd": 50}


def _assert_case_a(w):
    n = _classes(w)
    print(n)
    assert all(n[k] >= v for k, v in FLOOR_A.items()) and n["both_strands"] == 0, n
    assert w.left > 0 and w.slow_fragments() >= 50 and w.joined_reads == 2 * len(w.joined())


def _assert_case_b(w):
    """global paths: 0 = T0:(a,c), 1 = T0:(b,d), 2 = T1:(a,d), 3 = T1:(b,c).  Mates on {0, 2} and {1, 2} share both graphs, and the
    unit {2} leaves T0 without a path: the mates' records on paths 0 and 1 are left out"""
    k = sum(1 for i in range(w.n // 2) if w.sets[2 * i] == {0, 2} and w.sets[2 * i + 1] == {1, 2})
    assert k >= 50 and w.left >= 2 * k and _classes(w)["both_strands"] == 0
    assert all(r[1] == 2 for r in w.table.rows[w.table.rows[:, 0] == [ids for ids, _ in w.table.ecs].index((2,))].tolist())


def _flip(m, at):
    """base `at` replaced by one that matches nowhere (alignment is exact): a 1H clip at an end"""
    return m[:at] + bytes([_COMP[m[at]]]) + m[at + 1:]


def _with_edges(c, b, seed, per=60):
    """batch b of case (a) with fragments behind it whose records are cut at path_len - 1 (a mate on the last L bases of a path, its
    mate in the head of the same graph: A = B = every path of the graph) or clipped (a wrong first or last base)"""
    rng = np.random.default_rng(seed)
    reads = [bytes(b.seq[i * L:(i + 1) * L]) for i in range(b.n)]
    for j in range(per):
        g = int(rng.integers(0, 7))
        fr = [(c.text(g, int(rng.integers(0, tp.NP[g])))[-L:], c.in_head(rng, g)),
              (_flip(c.in_seg(rng, "A"), 0), c.in_seg(rng, "A")),
              (c.in_seg(rng, "B"), _flip(c.in_seg(rng, "B"), L - 1)),
              (_flip(c.in_seg(rng, "F", 4), 0), c.in_spacer(rng, 4, 0))]
        for k, (x, y) in enumerate(fr):
            reads += [x, tp._rc(y) if (j + k) & 1 else y]
    return _of_reads(b.name + " + edges", reads)


@pytest.fixture(scope="module")
def pcase_a(case_a):
    index, batches, c = case_a
    return index, [_with_edges(c, b, 900 + i) for i, b in enumerate(batches)]


# ---- running and checking -------------------------------------------------------------------------------------------------------

def _open(index, batches, rule=True, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(index, threshold=THR, max_batch_reads=max(1024, max(b.n for b in batches)), **kw)
    if rule:
        al.acov_pairs_enable()
    return al


def _same_table(got, want):
    assert got.ecs == want.ecs
    assert got.rows.shape == want.rows.shape and np.array_equal(got.rows, want.rows), (got.rows.shape, want.rows.shape)
    assert np.array_equal(got.n, want.n), np.flatnonzero(got.n != want.n)[:10]


def _check(al, wants, max_segs=4):
    want = merge_tables([w.table for w in wants])
    got = _dev_table(al)
    _same_table(got, want)
    st, ps = al.acov_stats(), al.acov_pairs_stats()
    print("acov", st, "pairs rule", ps)
    assert st["records"] == int(want.n.sum()) and st["tuples"] == len(want.n), st
    assert ps == {"records": int(want.n.sum()), "left_out": sum(w.left for w in wants), "joined_reads": sum(w.joined_reads for w in wants),
                  "slow_fragments": sum(w.slow_fragments(max_segs) for w in wants)}, ps
    assert ps["records"] + ps["left_out"] == sum(len(w.alns) for w in wants)
    return got, st, ps


# ---- CPU: the inputs, and the two consequences of the rule --------------------------------------------------------------------------

def test_inputs_hold_every_case(pcase_a, case_b):
    index, batches = pcase_a
    for b in batches:
        assert b.n % 2 == 0 and b.n <= 7000
        _assert_case_a(_want(index, b))
    index, batches, _ = case_b
    for b in batches:
        _assert_case_b(_want(index, b))


def test_split_and_single_fragments_give_the_unpaired_table(pcase_a):
    """consequence 1 of the rule, on the restatement itself"""
    index, (b0, _) = pcase_a
    w = _want(index, b0)
    keep = [i for i in range(b0.n // 2) if not w.sets[2 * i] & w.sets[2 * i + 1]]
    sub = b0.take([r for i in keep for r in (2 * i, 2 * i + 1)], "no joined fragment")
    ws = _want(index, sub)
    assert ws.left == 0 and ws.joined_reads == 0 and len(ws.alns) > 1000
    _same_table(ws.table, table_of_alns(index, ws.alns, sub.off))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_case_at_once(pcase_a, case_b, hip_lib, monkeypatch, which, stage):
    """two batches of every class through one ctx under each align stage: table, ECs and stats are the restatement's"""
    index, batches = pcase_a if which == "a" else case_b[:2]
    wants = [_want(index, b) for b in batches]
    for w in wants:
        (_assert_case_a if which == "a" else _assert_case_b)(w)
    _stage(monkeypatch, stage)
    al = _open(index, batches)
    try:
        _feed(al, batches)
        _, st, ps = _check(al, wants)
        assert (ps["slow_fragments"] > 0) == (which == "a") and ps["left_out"] > 0
        assert al.pairs_stats()["joined"] * 2 == ps["joined_reads"]
    finally:
        al.close()


@pytest.mark.gpu
def test_odd_first_read_id_and_boundaries(pcase_a, hip_lib, monkeypatch):
    """the fragment index is batch-relative (first_read_id = 7); and joined fragments with records left out lie across the 64-traversal
    edge of a wavefront and the 256-traversal edge of a block (where they lie is read from the batch's own traversal list; what they
    must add is the restatement's)"""
    index, (b0, _) = pcase_a
    w = _want(index, b0)
    _assert_case_a(w)
    _stage(monkeypatch, "path_first")
    al = _open(index, [b0])
    try:
        al.submit(b0.seq, b0.off, first_read_id=7)
        assert al.wait()["received"] == b0.n
        t, _ = al.travs()
        frag = (t["read_id"].astype(np.int64) - 7) >> 1
        assert np.all(np.diff(frag) >= 0)
        idx = np.arange(len(frag))
        lo, hi = {}, {}
        for f, i in zip(frag.tolist(), idx.tolist()):
            lo.setdefault(f, i)
            hi[f] = i
        filtered = [i for i in w.joined() if w.sets[2 * i] != w.sets[2 * i + 1]]
        assert sum(1 for i in filtered if lo[i] // 64 != hi[i] // 64) >= 10 and sum(1 for i in filtered if lo[i] // 256 != hi[i] // 256) >= 2
        _check(al, [w])
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("parts", [1, 2, 5])
def test_same_reads_in_any_batches(pcase_a, hip_lib, monkeypatch, parts, depth):
    """the table depends on the reads and their pairing alone: one batch cut into 1, 2 and 5, one or three batches in flight"""
    index, (b0, _) = pcase_a
    w = _want(index, b0)
    _assert_case_a(w)
    cuts = [2 * round(b0.n // 2 * k / parts) for k in range(parts + 1)]
    seq = [b0.take(np.arange(cuts[k], cuts[k + 1]), "part %d" % k) for k in range(parts)]
    assert sum(b.n for b in seq) == b0.n and all(b.n % 2 == 0 for b in seq)
    _stage(monkeypatch, "path_first")
    al = _open(index, seq, pipeline_depth=depth)
    try:
        assert _feed_pipelined(al, seq, depth=depth) == [0] * parts
        _check(al, [w])
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "b"])
def test_forced_slow_mode(pcase_a, case_b, hip_lib, monkeypatch, which):
    """GROOT_TEST_SHARED_SLOW (max_segs = 1): a joined fragment whose intersection spans two graphs and more is folded on the host, with
    the filter to its set and each mate's own length"""
    index, batches = pcase_a if which == "a" else case_b[:2]
    wants = [_want(index, b) for b in batches]
    multi = sum(w.slow_fragments(1) for w in wants)
    assert multi >= 100 and sum(w.left for w in wants) > 0
    # case (a): among them fragments with records outside their set, which only the host's filter can leave out (case (b)'s fragments
    # in both graphs have A = B, every path; its filtered fragments have a unit in one graph and stay on the device)
    assert which == "b" or sum(1 for w in wants for i in w.joined() if w.unit_graphs(i) > 1 and w.sets[2 * i] != w.sets[2 * i + 1]) >= 50
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    al = _open(index, batches)
    try:
        _feed(al, batches)
        _, st, ps = _check(al, wants, max_segs=1)
        assert ps["slow_fragments"] == multi > 0 and st["slow_records"] > 0
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_table_grows_at_collect_while_a_later_batch_is_in_flight(pcase_a, hip_lib, monkeypatch, depth):
    """GROOT_TEST_ACOV_SLOTS=8: the first batch's claim runs out of room, and by the time collect has grown the table and counts the batch
    again, the next batch -- other fragments -- has overwritten the unit rows and the per-batch table.  The redo reads what the slot owns"""
    index, (b0, b1) = pcase_a
    wants = [_want(index, b0), _want(index, b1)]
    _assert_case_a(wants[0])
    assert wants[0].unit[:2000] != wants[1].unit[:2000] and wants[0].left and wants[1].left
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    al = _open(index, [b0, b1], pipeline_depth=depth)
    try:
        assert _feed_pipelined(al, [b0, b1, b0], depth=depth) == [0, 0, 0]
        _, st, _ = _check(al, wants + [wants[0]])
        # a growth is twofold (a table half full) or fourfold (a claim that ran out of room, counted again behind it): some were fourfold
        assert st["grows"] > 0 and st["slots"] > 8 * 2 ** st["grows"], st
    finally:
        al.close()


@pytest.mark.gpu
def test_failing_and_redone_batches_count_once(pcase_a, hip_lib, monkeypatch):
    """a batch that fails with GROOT_E_NOSPACE adds nothing; under GROOT_TEST_SMALL_BUFFERS every batch's first pass is redone at collect,
    and only the redo counts"""
    index, (b0, b1) = pcase_a
    bad, adds = _bad_batch(index, b1, "long")
    assert adds == []
    _stage(monkeypatch, "path_first")
    al = _open(index, [b0, bad], max_read_len=64)
    try:
        first = _feed(al, [b0])
        al.submit(bad.seq, bad.off, first_read_id=first)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6
        _check(al, [_want(index, b0)])
        _feed(al, [b1], first + bad.n)
        _check(al, [_want(index, b0), _want(index, b1)])
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    al = _open(index, [b0, b1])
    try:
        _feed(al, [b0, b1])
        _check(al, [_want(index, b0), _want(index, b1)])
    finally:
        al.close()


@pytest.mark.gpu
def test_doubled_reads_on_argannot(argannot_index, hip_lib, monkeypatch):
    """consequence 2: fragments (r, r) on the arg-annot index (path sets of three words) have the ECs of the unpaired run of the
    originals, and every n doubled"""
    index = argannot_index
    assert index.view.path_words == 3
    seq, off, _ = synth.reads_np(*synth.reference_sequences(index), 3000, 100)
    reads = [bytes(seq[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    dseq, doff = O.pack_reads([r for r in reads for _ in (0, 1)])
    run = O.Run(index, 0.99)
    run.batch(seq, off)
    single = table_of_alns(index, run.alns().astype(device.ALN_DTYPE), off)
    run = O.Run(index, 0.99)
    run.batch(dseq, doff)
    want, left = paired_table_of_alns(index, run.alns().astype(device.ALN_DTYPE), doff)
    assert left == 0 and len(single.n) > 1000
    _same_table(want, Table(single.ecs, single.rows, 2 * single.n))
    _stage(monkeypatch, "path_first")
    al = device.Aligner(index, max_batch_reads=8192)
    try:
        al.acov_pairs_enable()
        al.submit(dseq, doff)
        al.wait()
        _same_table(_dev_table(al), want)
        ps = al.acov_pairs_stats()
        assert ps["left_out"] == 0 and ps["records"] == 2 * int(single.n.sum()) and ps["joined_reads"] == 2 * sum(c for _, c in single.ecs)
    finally:
        al.close()


@pytest.mark.gpu
def test_two_contexts_merge_to_the_table_of_one(pcase_a, hip_lib, monkeypatch):
    index, (b0, b1) = pcase_a
    half = (b0.n // 2) & ~1
    parts = [b0.take(np.arange(half), "a"), b1, b0.take(np.arange(half, b0.n), "c")]
    wants = [_want(index, b) for b in parts]
    assert all(w.left for w in wants)
    _stage(monkeypatch, "path_first")
    exports = []
    for mine in (parts[0::2], parts[1::2]):
        al = _open(index, parts)
        try:
            _feed(al, mine)
            exports.append(al.acov())
        finally:
            al.close()
    want = merge_tables([w.table for w in wants])
    off, ids, cnt, rows, n = host.acov_merge(index.view.n_paths, exports)
    w_off, w_ids, w_cnt, w_rows, w_n = want.arrays()
    assert np.array_equal(off, w_off) and np.array_equal(ids, w_ids) and np.array_equal(cnt, w_cnt)
    assert np.array_equal(rows, w_rows) and np.array_equal(n, w_n)
    assert len(exports[0][4]) + len(exports[1][4]) > len(w_n)          # tuples both contexts hold


def _refused(call, code=-10):
    with pytest.raises(host.GrootError) as e:
        call()
    assert e.value.code == code, e.value.code


@pytest.mark.gpu
def test_switching(pcase_a, hip_lib, monkeypatch):
    """the enable / disable sequences of include/groot_hip.h, the refusals that stay, acov_reset, and the rule off"""
    index, (b0, b1) = pcase_a
    small = b0.take(np.arange(2000), "2000")
    w, w1 = _want(index, small), _want(index, b1)
    assert w.left > 0 and w.joined_reads > 0
    zero = {"records": 0, "left_out": 0, "joined_reads": 0, "slow_fragments": 0}
    _stage(monkeypatch, "path_first")
    al = _open(index, [b0, b1], rule=False)
    try:
        assert al.acov_pairs_stats() == zero
        # the two refusals that stay: each enable with the other one on
        al.pairs_enable()
        _refused(al.acov_enable)
        al.pairs_enable(False)
        al.acov_enable()
        _refused(al.pairs_enable)
        al.acov_enable(False)
        al.ec_enable(False)
        # on: equivalence classes, assigned coverage and pairing come with it, whichever is off
        al.acov_pairs_enable()
        assert al.ec_stats()["reads"] == 0 and al.acov_stats()["slots"] > 0 and al.pairs_stats() == {"joined": 0, "split": 0, "single": 0}
        al.acov_pairs_enable()                              # (again: nothing changes)
        al.pairs_enable()                                   # (pairing is on already, and the rule allows it beside assigned coverage)
        _feed(al, [small])
        _check(al, [w])
        al.submit(b1.seq, b1.off, first_read_id=small.n)
        _refused(lambda: al.acov_pairs_enable(False), -9)   # something is in flight
        al.wait()
        _check(al, [w, w1])
        # acov_reset: the tuples and the rule's counts go, the ECs stay
        ecs = al.ecs()
        al.acov_reset()
        assert al.acov_pairs_stats() == zero and al.acov_stats()["records"] == 0
        assert all(np.array_equal(x, y) for x, y in zip(ecs, al.ecs())) and al.ec_stats()["reads"] > 0
        # off: the rule and assigned coverage go, ECs and pairing stay; the two refusals are back
        al.acov_pairs_enable(False)
        assert al.acov_pairs_stats() == zero and al.acov_stats()["slots"] == 0 and al.ec_stats()["reads"] > 0
        assert al.pairs_stats()["joined"] > 0
        _refused(al.acov_enable)
        # on with equivalence classes and pairing on already
        al.ec_reset()
        al.acov_pairs_enable()
        _feed(al, [small])
        _check(al, [w])
        # pairs_enable(0) with the rule on takes the rule and assigned coverage with it
        al.pairs_enable(False)
        assert al.acov_pairs_stats() == zero and al.acov_stats()["slots"] == 0
        _refused(al.pairs_stats, -9)
        # acov_enable(0) with the rule on: the rule goes too, pairing stays, and pairs_enable(1) is fine again
        al.acov_pairs_enable()
        al.acov_enable(False)
        assert al.acov_pairs_stats() == zero and al.pairs_stats() == {"joined": 0, "split": 0, "single": 0}
        _refused(al.acov_enable)
        # with the rule off the ctx counts what it counts today: assigned coverage per read
        al.pairs_enable(False)
        al.ec_reset()
        al.acov_enable()
        _feed(al, [small])
        _same_table(_dev_table(al), table_of_alns(index, w.alns, small.off))
        assert al.acov_pairs_stats() == zero
        # not beside assignment
        al.acov_enable(False), al.ec_enable(False)
        al.assign_enable(np.ones(index.view.n_paths))
        _refused(al.acov_pairs_enable)
        al.assign_enable(None)
        al.acov_pairs_enable()
        _refused(lambda: al.assign_enable(np.ones(index.view.n_paths)))
    finally:
        al.close()


@pytest.mark.gpu
def test_not_beside_the_rescued_reads_in_the_classes(pcase_a, hip_lib, monkeypatch):
    index, (b0, _) = pcase_a
    _stage(monkeypatch, "path_first")
    al = _open(index, [b0], rule=False)
    try:
        al.rescue_enable(2)
        al.ec_enable()
        al.rescue_ec_enable()
        _refused(al.acov_pairs_enable)
        al.rescue_ec_enable(False)
        al.acov_pairs_enable()
        _refused(al.rescue_ec_enable)
        _refused(lambda: al.rescue_acov_enable())
    finally:
        al.close()
