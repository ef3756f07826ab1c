"""Rescued reads in the equivalence classes (groot_hip_rescue_ec_*, kernels_rescue_ec.hpp) against a brute force of the definition
(tests/rescue_sets_def.py): the device's ECs == the oracle's records' ECs plus the rescued reads' sets, integers throughout.

The index is the eight graphs of test_rescue.py's `case` plus a ninth with a 64-base stretch twice in its one path (kept placements at two
x of one path).  The batch is test_rescue's batch of every class plus: 40-base stretches of the shared segments of test_counter_edges.SEGS
with one substitution in the middle -- rescued under M = 1 only (M = 2 candidates need 48 bases, the segments have 45) onto every path of
the 4, 4, 5, 7, 2 and 3 graphs that share the segment, so M = 1 is where the sets in more than four graphs (the bitmaps) are met for their
real reason -- and 48-base stretches of the ninth graph's repeat with one substitution."""
import numpy as np
import pytest

from groot_amd import device, host
from rescue_def import Tables, _rc, path_texts
from rescue_sets_def import ecs_plus, rescued_sets
from test_abundance import _dev_ecs, ecs_of_alns
from test_counter_edges import NP, SEGS, THR, _feed, _feed_pipelined, _first_diff, _graph, _of_reads
from test_coverage import STAGES, _stage
from test_path_pass import _gfa, _seq
from test_rescue import _extra_graph, _has_record, _make_reads, _mut, _plain, _reads_of

FLOOR = 20


def _repeat_graph(rng, path):
    """graph 8: U1 . R . U2 . R . U3 with the 64 bases of R twice, one path"""
    rep = _seq(rng, 64)
    nodes = {1: _seq(rng, 60), 2: rep, 3: _seq(rng, 40), 4: rep, 5: _seq(rng, 60)}
    return _gfa(path, nodes, [(1, 2), (2, 3), (3, 4), (4, 5)], [("r0", [1, 2, 3, 4, 5])]), rep.encode()


class _Case:
    """the index, the batch, and per M the definition's S+(r) of every read of the batch"""

    def __init__(self, tmp):
        rng = np.random.default_rng(13)
        self.shared = {name: _seq(rng, 45) for name, _ in SEGS}
        files = [_graph(rng, tmp / ("g%d.gfa" % g), g, self.shared)[0] for g in range(len(NP))] + [_extra_graph(rng, tmp / "g7.gfa")]
        f8, rep = _repeat_graph(rng, tmp / "g8.gfa")
        self.index = host.Index.from_gfa_files(files + [f8], host.index_params(k=7, s=10, w=64))
        texts = path_texts(self.index)
        assert self.index.view.n_paths == sum(NP) + 3 and all(t is not None for t in texts) and self.index.view.path_words == 3
        named = _make_reads(np.random.default_rng(14), texts)
        rng = np.random.default_rng(17)
        for name, _ in SEGS:
            seg = self.shared[name].encode()
            for k in range(30):
                x = int(rng.integers(0, 6))
                r = _mut(rng, seg[x:x + 40], [20]) if k < 26 else seg[x:x + 40]        # (four of them error-free)
                named.append(("seg" + name, _rc(r) if k & 1 else r))
        for k in range(30):
            x = int(rng.integers(0, 17))
            r = _mut(rng, rep[x:x + 48], [int(rng.integers(48))])
            named.append(("repeat", _rc(r) if k & 1 else r))
        order = np.random.default_rng(15).permutation(len(named))
        self.names = [named[i][0] for i in order]
        self.batch = _of_reads("classes", [named[i][1] for i in order])
        self.reads = _reads_of(self.batch)
        self.gpo = self.index.arrays["graph_path_off"].astype(np.int64)
        self._by_m, self._tables = {}, Tables(self.index, 1)          # (the windows of the texts, shared by every M)

    def exact(self, batch=None):
        """{read: S(r)} of the reads with a record, and the number of graphs of each"""
        w = (batch or self.batch).want(self.index)
        r, p = w.read_ref >> 10, w.read_ref & 1023
        starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
        return {int(r[s]): tuple(int(v) for v in p[s:e]) for s, e in zip(starts, np.r_[starts[1:], len(r)])}

    def rescued(self, M):
        if M not in self._by_m:
            self._by_m[M] = rescued_sets(self.index, M, self.reads, _has_record(self.batch, self.index), self._tables)
        return self._by_m[M]

    def graphs_of(self, ids):
        return len(set((np.searchsorted(self.gpo, np.array(ids), side="right") - 1).tolist()))

    def expect(self, M, reads=None, max_segs=4, on=True):
        """-> (ECs, rescued reads added, slow ones among them, reads with a record, slow ones among them) over `reads` of the batch"""
        res = self.rescued(M)[0] if on else {}
        ex = self.exact()
        reads = range(self.batch.n) if reads is None else reads
        added = [i for i in reads if i in res]
        mapped = [i for i in reads if i in ex]
        slow = lambda s: self.graphs_of(s) > max_segs
        return (ecs_plus(ex, res, reads), len(added), sum(slow(res[i].paths) for i in added), len(mapped), sum(slow(ex[i]) for i in mapped))


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return _Case(tmp_path_factory.mktemp("rescue_ec"))


# ---- CPU: the brute force alone puts every class at its floor ---------------------------------------------------------------------------

def test_inputs_hold_every_class(case):
    res, left = case.rescued(1)
    ex = case.exact()
    assert not set(res) & set(ex) and not set(left) & set(ex)                       # a candidate has no record
    # the ECs of the definition over the whole batch == ecs_of_alns over the oracle's records plus the rescued sets
    want = dict(ecs_of_alns(case.batch.want(case.index).alns))
    for r in res.values():
        want[r.paths] = want.get(r.paths, 0) + 1
    assert case.expect(1)[0] == want
    per_graphs = np.bincount([case.graphs_of(r.paths) for r in res.values()], minlength=8)
    print("M = 1: rescued", len(res), "left", len(left), "sets by graphs", per_graphs.tolist())
    for g in (1, 4, 5, 7):
        assert per_graphs[g] >= FLOOR, (g, per_graphs)
    pw = case.index.view.path_words
    first = case.gpo[np.searchsorted(case.gpo, 0, side="right") - 1]

    def every_word(ids):                    # more than 64 paths of one graph, and a bit in every mask word of that graph's segment
        ids = np.array(ids)
        g = np.searchsorted(case.gpo, ids, side="right") - 1
        return any((g == x).sum() > 64 and len(set(((ids[g == x] - case.gpo[x]) >> 6).tolist())) == pw for x in set(g.tolist()))

    exact_sets = set(ex.values())
    count = lambda f: sum(1 for r in res.values() if f(r))
    assert first == 0 and count(lambda r: every_word(r.paths)) >= FLOOR
    assert count(lambda r: len(r.strands) == 2) >= FLOOR
    assert count(lambda r: r.multi_x) >= FLOOR
    assert count(lambda r: r.paths in exact_sets) >= FLOOR
    assert count(lambda r: r.paths not in exact_sets) >= FLOOR
    by_set = {}
    for r in res.values():
        by_set[r.paths] = by_set.get(r.paths, 0) + 1
    assert sum(1 for c in by_set.values() if c >= 2) >= 10, sorted(by_set.values())
    assert count(lambda r: r.d == 0) > 0 and len(left) > 0
    # the other thresholds: sets in one graph, and wide ones, and both fast and no slow sets
    for M in (2, 3):
        resm, leftm = case.rescued(M)
        assert len(resm) >= 10 * FLOOR and len(leftm) > 0 and sum(1 for r in resm.values() if r.d == M) >= FLOOR
        assert sum(1 for r in resm.values() if every_word(r.paths)) >= FLOOR


def test_brute_force_on_a_hand_made_case(case):
    """the stretch of the repeat lies at two x of the one path of graph 8 and counts it once; a segment of four graphs gives every path
    of the four"""
    rep_reads = [i for i, n in enumerate(case.names) if n == "repeat"]
    res, _ = case.rescued(1)
    last = case.index.view.n_paths - 1
    assert sum(1 for i in rep_reads if i in res and res[i].paths == (last,) and res[i].kept == 2 and res[i].multi_x) >= FLOOR
    a = [i for i, n in enumerate(case.names) if n == "segA" and i in res]
    assert len(a) >= FLOOR and all(res[i].paths == tuple(range(int(case.gpo[4]))) for i in a)


# ---- the device side -----------------------------------------------------------------------------------------------------------------------

def _open(case, M=1, on=True, ec=True, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    kw.setdefault("max_batch_reads", max(1024, case.batch.n))
    al = device.Aligner(case.index, threshold=THR, **kw)
    if ec:
        al.ec_enable()
    if M:
        al.rescue_enable(M)
    if on:
        al.rescue_ec_enable()
    return al


def _assert_device(al, want, passes=None):
    ecs, added, slow, mapped, mapped_slow = want
    got = dict(_dev_ecs(al))
    assert got == ecs, _first_diff(got, ecs)
    st, es = al.rescue_ec_stats(), al.ec_stats()
    print("rescue_ec", st, "ec", es)
    assert (st["reads"], st["slow_reads"]) == (added, slow), (st, added, slow)
    assert (es["reads"], es["distinct"], es["slow_reads"]) == (mapped + added, len(ecs), mapped_slow), (es, mapped, added, len(ecs), mapped_slow)
    # three kernels per pass behind rescue's (a pass that collect redoes launches them again, and they return at once in the pass that is not counted)
    assert st["launches"] % 3 == 0 and (passes is None or st["launches"] >= 3 * passes), (st, passes)
    return st


def _pieces(case, cuts):
    return [(_of_reads("piece %d" % i, case.reads[a:b]), range(a, b)) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_class_at_once(case, hip_lib, monkeypatch, M):
    _stage(monkeypatch, "path_first")
    al = _open(case, M)
    try:
        _feed(al, [case.batch])
        st = _assert_device(al, case.expect(M), passes=1)
        assert st["rows"] == max(1024, case.batch.n)                # (the byte budget holds more bitmaps than a batch has reads)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    _stage(monkeypatch, stage)
    al = _open(case, results_on_device=rod)
    try:
        _feed(al, [case.batch])
        _assert_device(al, case.expect(1), passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_forced_slow_mode(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every set in more than one graph goes through the bitmaps"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    al = _open(case)
    try:
        _feed(al, [case.batch])
        want = case.expect(1, max_segs=1)
        assert want[2] >= 4 * FLOOR
        _assert_device(al, want, passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_too_few_bitmaps_fail_the_batch(case, hip_lib, monkeypatch):
    """one bitmap fewer than the batch's slow rescued reads: GROOT_E_NOSPACE that names the knob; exactly as many: every read counted"""
    _stage(monkeypatch, "path_first")
    want = case.expect(1)
    assert want[2] >= 2 * FLOOR
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(want[2] - 1))
    al = _open(case)
    try:
        assert al.rescue_ec_stats()["rows"] == want[2] - 1
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "GROOT_TEST_RESCUE_EC_ROWS" in str(e.value), e.value      # GROOT_E_NOSPACE
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(want[2]))
    al = _open(case)
    try:
        _feed(al, [case.batch])
        assert _assert_device(al, want, passes=1)["rows"] == want[2]
    finally:
        al.close()


CUTS = [0, 700, 700, 701, 1100, 1500, 1900, None]


@pytest.mark.gpu
def test_table_growth_with_batches_in_flight(case, hip_lib, monkeypatch):
    """GROOT_TEST_EC_SLOTS small and three batches in flight: the table of classes grows between merges, the rescued sets among them"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "2")
    pieces = _pieces(case, CUTS[:-1] + [case.batch.n])
    al = _open(case, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        _assert_device(al, case.expect(1), passes=sum(1 for p, _ in pieces if p.n))
        assert al.ec_stats()["grows"] >= 1                      # (two slots hold no piece: the first reserve grows the table for certain)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case, hip_lib, monkeypatch, small):
    """the batch cut into seven, one piece empty and one of a single read, three in flight -- and the same with GROOT_TEST_SMALL_BUFFERS,
    where pieces are redone at collect and count once"""
    pieces = _pieces(case, CUTS[:-1] + [case.batch.n])
    assert [p.n for p, _ in pieces][1:3] == [0, 1]
    want = case.expect(1)
    if small:       # a piece of its own with more records than the small buffers hold: redone for certain; its reads are the batch's first 450
        texts, rng = path_texts(case.index), np.random.default_rng(16)
        clean = [texts[p][0][x:x + 64] for p, x in zip(rng.choice([0, 70, 134, 199, 329, 457], 300), rng.integers(1, 200, 300))]
        extra = _of_reads("mapped and not", clean + case.reads[:150])
        has = _has_record(extra, case.index)
        assert int(has.sum()) >= 280 and len(extra.want(case.index).alns) > 1000
        ecs = dict(want[0])
        for s in case.exact(extra).values():
            ecs[s] = ecs.get(s, 0) + 1
        res = rescued_sets(case.index, 1, _reads_of(extra), has)[0]
        for r in res.values():
            ecs[r.paths] = ecs.get(r.paths, 0) + 1
        n_slow = lambda sets: sum(case.graphs_of(s) > 4 for s in sets)
        want = (ecs, want[1] + len(res), want[2] + n_slow(r.paths for r in res.values()), want[3] + int(has.sum()), want[4] + n_slow(case.exact(extra).values()))
        pieces.insert(4, (extra, None))
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(case, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        st = _assert_device(al, want)
        n = sum(1 for p, _ in pieces if p.n)
        assert st["launches"] > 3 * n if small else st["launches"] >= 3 * n, st      # (a pass that was redone launched its kernels again, and counted once)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE adds nothing; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP counts whole (the bad
    read has no record and is no candidate)"""
    cut = 1100
    reads, ex = list(case.reads[cut:]), case.exact()
    mid = next(i for i in range(300, len(reads)) if len(reads[i]) >= 48 and cut + i in ex)
    reads[mid] = {"long": reads[mid] * 6, "short": reads[mid][:5], "lower": reads[mid].lower()}[kind]
    code = {"long": -6, "short": -7, "lower": -8}[kind]
    counted = list(range(cut)) + ([] if kind == "long" else [i for i in range(cut, case.batch.n) if i != cut + mid])
    _stage(monkeypatch, "path_first")
    al = _open(case)
    try:
        first = _feed(al, [_of_reads("good", case.reads[:cut])])
        b = _of_reads(kind, reads)
        al.submit(b.seq, b.off, first_read_id=first)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == code
        _assert_device(al, case.expect(1, counted))
    finally:
        al.close()


def _sum(a, b):
    ecs = dict(a)
    for k, v in b.items():
        ecs[k] = ecs.get(k, 0) + v
    return ecs


@pytest.mark.gpu
def test_two_ctxs_off_on_and_reset(case, hip_lib, monkeypatch):
    (a, ra), (b, rb) = _pieces(case, [0, 2000, case.batch.n])
    wa, wb, whole = case.expect(1, ra), case.expect(1, rb), case.expect(1)
    _stage(monkeypatch, "path_first")
    al, al2 = _open(case), _open(case)
    try:
        _feed(al, [b])
        al.ec_reset()                                           # the classes, the rescued reads in them and the stats start over
        assert _dev_ecs(al) == [] and al.rescue_ec_stats()["reads"] == 0
        _feed(al, [a])
        s1 = _assert_device(al, wa, passes=2)
        _feed(al2, [b])
        s2 = _assert_device(al2, wb, passes=1)
        assert _sum(dict(_dev_ecs(al)), dict(_dev_ecs(al2))) == whole[0]      # the merge of two ctxs is a sum by set
        assert s1["reads"] + s2["reads"] == whole[1] and s1["slow_reads"] + s2["slow_reads"] == whole[2]
        al.rescue_reset()                                       # the rescue tables start over, the classes stay
        al.rescue_enable(2); al.rescue_enable(1)                # another M and back: likewise
        _assert_device(al, wa, passes=2)
        al.rescue_ec_enable(False)                              # off: no launch, and the classes gain what today's code counts
        _feed(al, [b])
        off = case.expect(1, rb, on=False)
        st = al.rescue_ec_stats()
        assert st == dict(reads=0, slow_reads=0, rows=0, launches=s1["launches"]), st
        assert dict(_dev_ecs(al)) == _sum(wa[0], off[0])
        al.rescue_ec_enable()                                   # on again: the classes stay, the counts of the rescued start from zero
        _feed(al, [b])
        assert dict(_dev_ecs(al)) == _sum(_sum(wa[0], off[0]), wb[0])
        st = al.rescue_ec_stats()
        assert (st["reads"], st["slow_reads"]) == (wb[1], wb[2]) and st["launches"] >= s1["launches"] + 3 and st["launches"] % 3 == 0, st
        al.rescue_enable(0)                                     # rescue off takes it off too
        assert al.rescue_ec_stats()["rows"] == 0
        _feed(al, [b])
        assert dict(_dev_ecs(al)) == _sum(_sum(_sum(wa[0], off[0]), wb[0]), off[0]) and al.rescue_ec_stats()["launches"] == st["launches"]
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_feature_off_is_todays_code(case, hip_lib, monkeypatch):
    """with rescue and the classes on and the feature off, the classes are the records' and nothing is launched for it"""
    _stage(monkeypatch, "path_first")
    al = _open(case, on=False)
    try:
        _feed(al, [case.batch])
        assert dict(_dev_ecs(al)) == dict(ecs_of_alns(case.batch.want(case.index).alns))
        assert al.rescue_ec_stats() == dict(reads=0, slow_reads=0, rows=0, launches=0)
    finally:
        al.close()


def _refused(call, code, *words):
    with pytest.raises(host.GrootError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), e.value


@pytest.mark.gpu
def test_refusals_in_both_orders(case, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    al = _open(case, M=0, on=False, ec=False)
    try:
        _refused(al.rescue_ec_enable, -9, "rescue")             # GROOT_E_STATE: neither is on
        al.ec_enable()
        _refused(al.rescue_ec_enable, -9, "mismatch rescue")
        al.ec_enable(False); al.rescue_enable(1)
        _refused(al.rescue_ec_enable, -9, "equivalence classes are off")
        al.ec_enable()
        al.pairs_enable()                                       # pairing first
        _refused(al.rescue_ec_enable, -10, "paired")            # GROOT_E_UNSUPPORTED
        al.pairs_enable(False)
        al.acov_enable()                                        # assigned coverage first
        _refused(al.rescue_ec_enable, -10, "assigned coverage")
        al.acov_enable(False)
        al.rescue_ec_enable()                                   # the feature first
        _refused(al.pairs_enable, -10, "rescued reads")
        _refused(al.acov_enable, -10, "rescued read")
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        _refused(lambda: al.rescue_ec_enable(False), -9, "in flight")
        al.wait()
        _assert_device(al, case.expect(1), passes=1)            # none of the refusals left anything behind
        al.ec_enable(False)                                     # the classes off take it off too
        assert al.rescue_ec_stats()["rows"] == 0
        al.ec_enable()
        al.rescue_ec_enable()
        _feed(al, [case.batch])
        _assert_device(al, case.expect(1), passes=1 + 1)
    finally:
        al.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case, hip_lib, monkeypatch):
    """coverage, shared reads, the rescue tables, the gap tables, their stats and the records with the feature on == without it"""
    _stage(monkeypatch, "path_first")
    got = []
    for on in (False, True):
        al = _open(case, M=2, on=False)
        try:
            al.coverage_enable(); al.shared_enable(); al.gap_enable(3)
            if on:
                al.rescue_ec_enable()
            al.submit(case.batch.seq, case.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[f] for f in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.shared(), al.shared_stats(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(),
                        al.gap_stats()))
            if on:
                _assert_device(al, case.expect(2), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
