"""Rescued records on the device (groot_hip_rescue_rec_*, kernels_rescue_rec.hpp) at the shapes tests/test_rescue_records.py does not
reach, against the same brute force (tests/rescue_records_def.py); the index and the reads are in tests/rescue_records_shapes_case.py:

    the order       the list is in ascending (read, path, strand, pos) order, and rescue_rec_emit_kernel sorts every read's segment into it
                    with rescue_rec_before.  Reads of reverse-complement palindromic repeats have both strands on one path at interleaving
                    or equal pos: dozens of reads of the batch would come out differently under (read, path, pos, strand) order, which
                    no read of tests/rescue_records_case.py would;
    mismatch offsets  three 16-bit fields shifted into one 64-bit register, from 32 * word + bit / 2 over up to 16 words of rescue_diff:
                    reads of up to 512 bases with offsets on either side of every word edge from 256 upwards, 510 and 511 among them;
    segments        up to 108 records of one read (the insertion sort's longest run), four paths per read, a capacity that ends inside
                    such a segment;
    full buffers    max_batch_reads candidates of max_batch_bases bases with the last read rescued: n_kept[n_reads], rec_off[n_reads - 1]
                    and rec_d[n - 1] are all live; slots_per_batch exactly the total;
    forced slow     rescue_count_rec_kernel<*, true> beside the classes under GROOT_TEST_SHARED_SLOW;
    the batch's order  a read's segment does not depend on where the read stands in the batch.

Not covered: a path whose first Position is not 0 -- a GFA file cannot give one (tests/gap_shapes_case.py); the hand-worked cases of
tests/test_rescue_records_def.py keep the definition's X = first Position + offset.  Every comparison is exact."""
import numpy as np
import pytest

import rescue_records_shapes_case as shapes
from groot_amd import host
from rescue_records_def import plain
from rescue_records_shapes_case import OFFSETS
from test_abundance import _dev_ecs
from test_counter_edges import _feed
from test_coverage import STAGES, _stage
from test_rescue import _has_record, _plain
from test_rescue_records import _one_batch, _open, _pieces_pipelined, _same
from test_rescue_shapes import _candidates_only

FLOOR = 10
SLOTS = 1 << 17


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(rescue_records_shapes_case.RecordsShapes of the batch, {path name: global path}, {path name: text}, the sixth graph's spans)"""
    return shapes.build(tmp_path_factory)


def _on(c, M=2, slots=SLOTS, **kw):
    return _open(c, M, slots, max_read_len=512, **kw)


# ---- CPU: the definition alone --------------------------------------------------------------------------------------------------------------

def test_inputs_hold_every_class(case):
    """every class of record the device tests rely on occurs at least FLOOR times in the batch, by the brute force alone"""
    c, paths, T, spans = case
    k = {M: shapes.classes(c, paths, M) for M in (1, 2, 3)}
    for M in (1, 2, 3):
        print("M =", M, k[M])
    assert len(c.records(2)) < SLOTS
    for M in (1, 2, 3):
        # the order: reads whose segment differs between (path, strand, pos) and (path, pos, strand) order
        assert k[M]["order_sensitive_reads"] >= FLOOR, (M, k[M])
        # (read, path) pairs with both strands at different sets of pos, and (read, path, pos) on both strands
        assert k[M]["both_strands_other_pos"] >= FLOOR and k[M]["both_strands_one_pos"] >= FLOOR, (M, k[M])
        assert k[M]["reads_on_4_paths"] >= FLOOR and k[M]["of_long_reads"] >= FLOOR and k[M]["offset_256_up"] >= FLOOR, (M, k[M])
        assert k[M]["pos_0_long_path"] >= FLOOR and k[M]["last_base_long_path"] >= FLOOR and k[M]["on_textless_or_p11"] == 0, (M, k[M])
        for s in (0, 1):
            assert k[M]["offset_0_strand_%d" % s] >= FLOOR and k[M]["offset_last_strand_%d" % s] >= FLOOR, (M, s, k[M])
        for at in OFFSETS:
            assert k[M]["offset_%d" % at] >= FLOOR, (M, at, k[M])
    # both strands at different sets of pos: windows of the period-4 repeat that begin with C or T, and windows inside the palindrome off
    # its centre.  pal/edge cannot give it: its unique bases hold the read to the one placement it was cut from (see the case's text)
    for name in ("pal4", "palindrome/in"):
        assert k[2]["both_strands_other_pos_by_class"].get(name, 0) >= FLOOR, k[2]
    assert "pal/edge" not in k[2]["both_strands_other_pos_by_class"] and sum(n == "pal/edge" and c.per_read(2)[i] > 0 for i, n in enumerate(c.names)) >= FLOOR
    for name in ("pal4", "pal2", "palindrome/in"):
        assert k[2]["order_sensitive_by_class"].get(name, 0) >= FLOOR, k[2]
    # long segments: 64 and 100 records and more of one read (a read of 64 bases and more has fewer copies inside a repeat: none at M = 3)
    for M in (1, 2):
        assert k[M]["reads_64_records"] >= FLOOR and k[M]["reads_100_records"] >= FLOOR and k[M]["most_of_one_read"] >= 100, (M, k[M])
    assert k[3]["reads_64_records"] == 0 and k[3]["most_of_one_read"] >= 32, k[3]
    # every d up to M, and none above
    assert all(n >= FLOOR for n in k[1]["d"][:2]) and k[1]["d"][2:] == [0, 0], k[1]
    assert all(n >= FLOOR for n in k[2]["d"][:3]) and k[2]["d"][3] == 0, k[2]
    assert all(n >= FLOOR for n in k[3]["d"]), k[3]
    # the path of 46 bases: filled exactly at M = 1 (46 bases are too few for M = 2)
    assert k[1]["pos_0_p46"] >= FLOOR and k[1]["last_base_p46"] >= FLOOR, k[1]
    assert k[2]["pos_0_p46"] == k[2]["last_base_p46"] == k[3]["pos_0_p46"] == k[3]["last_base_p46"] == 0, (k[2], k[3])
    assert len({k[M]["records"] for M in (1, 2, 3)}) == 3


def test_the_other_order_differs(case):
    """what pins the comparator: sorted by (read, path, pos, strand) the definition's list is another list, on at least FLOOR reads, and
    so is the list in the order the kernel emits it before its sort (strand, then as found) wherever a read lies on two paths"""
    c = case[0]
    rec = c.records(2)
    other = shapes.sort_by(rec, ("read", "path", "pos", "strand"))
    assert sorted(plain(rec)) == sorted(plain(other)) and not np.array_equal(rec, other)
    assert len(np.unique(rec["read"][rec != other])) == len(shapes.order_sensitive(rec)) >= FLOOR
    by_strand = shapes.sort_by(rec, ("read", "strand", "path", "pos"))
    assert len(np.unique(rec["read"][rec != by_strand])) >= FLOOR


# ---- the device side -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_shape_at_once(case, hip_lib, monkeypatch, M):
    c = case[0]
    _stage(monkeypatch, "path_first")
    al = _on(c, M)
    try:
        want = c.records(M)
        _same(_one_batch(al, c.batch), want)
        st = al.rescue_rec_stats()
        print("rescued records", st)
        assert (st["records"], st["reads"], st["failed"], st["slots"]) == (len(want), len(np.unique(want["read"])), 0, SLOTS), st
        assert al.rescue_stats()["placements"] == len(want)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    c = case[0]
    _stage(monkeypatch, stage)
    al = _on(c, results_on_device=rod)
    try:
        _same(_one_batch(al, c.batch), c.records(2))
    finally:
        al.close()


@pytest.mark.gpu
def test_order_of_the_batch_does_not_matter(case, hip_lib, monkeypatch):
    """the batch, the batch reversed and one fixed permutation of it: every read has the same records but for `read` -- mapped back
    through the permutation and brought into the batch's order of reads, each list is the definition's list of the batch"""
    c = case[0]
    n = c.batch.n
    _stage(monkeypatch, "path_first")
    al = _on(c)
    try:
        for idx in (np.arange(n), np.arange(n)[::-1], np.random.default_rng(44).permutation(n)):
            b = c.pick(idx)
            assert np.array_equal(_has_record(b, c.index), c.has[idx])      # (a read's records do not depend on its batch)
            got = _one_batch(al, b)
            assert np.array_equal(got["read"], np.sort(got["read"]))
            back = got.copy()
            back["read"] = idx[got["read"]]
            _same(back[np.argsort(back["read"], kind="stable")], c.records(2))
            _same(got, c.records_for(2, idx))
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gap", [False, True])
def test_beside_classes_forced_slow(case, hip_lib, monkeypatch, gap):
    """rescue_count_rec_kernel<kGap, true> with every set in more than one graph forced into the slow path (GROOT_TEST_SHARED_SLOW): the
    list is the same, and the classes, the rescued reads in them and the gap tables are what they are without the records"""
    c = case[0]
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    got = []
    for slots in (0, SLOTS):
        al = _on(c, slots=slots)
        try:
            al.ec_enable()
            al.rescue_ec_enable()
            if gap:
                al.gap_enable(3, 1 << 12)
            if slots:
                _same(_one_batch(al, c.batch), c.records(2))
            else:
                _feed(al, [c.batch])
            st = al.rescue_ec_stats()
            assert st["slow_reads"] >= FLOOR, st
            got.append((al.rescue(), al.rescue_stats(), _dev_ecs(al), st["reads"], st["slow_reads"], al.gap() if gap else None))
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pieces_in_flight(case, hip_lib, monkeypatch, small):
    """five pieces, one of long reads only, three in flight: every piece hands out the batch's records of its reads with piece-relative
    `read` -- and with GROOT_TEST_SMALL_BUFFERS and a piece in front that is redone at collect for certain, which yields the records of
    its redo, once"""
    c = case[0]
    pieces = shapes.five_pieces(c)
    if small:
        pieces.insert(0, shapes.redone_piece(c))
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    want = [c.records_for(2, idx) for _, idx in pieces]
    assert all(len(w) for w in want) and sum(len(w) for w in want[small:]) == len(c.records(2))
    _stage(monkeypatch, "path_first")
    al = _on(c, pipeline_depth=3)
    try:
        got = _pieces_pipelined(al, [p for p, _ in pieces])
        assert [s for s, _ in got] == [0] * len(pieces)
        for (_, g), w in zip(got, want):
            _same(g, w)
        st = al.rescue_rec_stats()
        assert st["records"] == sum(len(w) for w in want) and st["failed"] == 0, st
        if small:
            assert st["launches"] > 2 * len(pieces), st          # (a pass was redone: its kernels ran again, and it counted once)
        else:
            assert st["launches"] >= 2 * len(pieces) and st["launches"] % 2 == 0, st
    finally:
        al.close()


@pytest.mark.gpu
def test_batch_that_fills_the_buffer(case, hip_lib, monkeypatch):
    """max_batch_reads candidates of exactly max_batch_bases bases, none with a record, the LAST one rescued: n_kept[n_reads] (zeroed and
    scanned, never written), rec_off[n_reads - 1] and rec_d[n - 1] are all in use -- with room to spare, and with exactly the total"""
    c, paths, T, spans = case
    n = 1024
    full, t = _candidates_only(c.index, T["l0"], n)
    f = c.of(full)
    idx = np.arange(n)
    last = int(np.flatnonzero(f.per_read(2))[-1])                # the last rescued read goes to the batch's end: the same reads, the same bases
    idx[[last, n - 1]] = idx[[n - 1, last]]
    b, want = f.pick(idx), f.records_for(2, idx)
    assert b.n == n and int(b.off[-1]) == int(full.off[-1]) and not _has_record(b, c.index).any()
    assert len(np.unique(want["read"])) == t.stats["rescued"] >= 100 and int(want["read"][-1]) == n - 1 and len(want) == t.stats["placements"]
    _stage(monkeypatch, "path_first")
    al = _on(f, max_batch_bases=int(b.off[-1]))
    try:
        assert al.params.max_batch_reads == n and al.params.max_batch_bases == int(np.diff(b.off.astype(np.int64)).sum())
        _same(_one_batch(al, b), want)
        assert al.rescue_stats()["candidates"] == n
        al.rescue_rec_enable(len(want))
        _same(_one_batch(al, b), want)
        st = al.rescue_rec_stats()
        assert (st["records"], st["reads"], st["failed"], st["slots"]) == (len(want), t.stats["rescued"], 0, len(want)), st
    finally:
        al.close()


@pytest.mark.gpu
def test_room_inside_a_long_segment(case, hip_lib, monkeypatch):
    """a capacity that ends strictly inside the segment of a read with 100 records and more, rescued reads in front of it and behind it:
    the batch fails with GROOT_E_NOSPACE and hands out no record, its other results stay readable, the next batch is clean; with
    exactly the room up to that segment's end and for the reads behind it -- the batch's total -- it passes"""
    c = case[0]
    want, per = c.records(2), c.per_read(2)
    off = np.r_[0, np.cumsum(per)]
    r = next(i for i in range(c.batch.n // 2, c.batch.n) if c.names[i] == "many" and per[i] >= 100)
    assert 0 < off[r] and off[r + 1] < len(want) and r < c.batch.n - 300 and int((per[r + 1:] > 0).sum()) >= 100
    inside = int(off[r] + per[r] // 2)
    assert off[r] < inside < off[r + 1] and int(off[r + 1]) + int(per[r + 1:].sum()) == len(want)
    small = c.piece(0, 500)
    _stage(monkeypatch, "path_first")
    al = _on(c, slots=len(want))
    try:
        _same(_one_batch(al, c.batch), want)
        n_travs = len(al.travs()[0])
        al.rescue_rec_enable(inside)
        al.submit(c.batch.seq, c.batch.off)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "slots_per_batch" in str(e.value) and str(inside) in str(e.value) and str(len(want)) in str(e.value), e.value
        assert len(al.rescue_records()) == 0
        assert len(al.travs()[0]) == n_travs > 0
        st = al.rescue_rec_stats()
        assert st["failed"] == 1 and st["records"] == 0 and st["slots"] == inside, st
        _same(_one_batch(al, small, first=c.batch.n), c.records_of(2, 0, 500))
        st = al.rescue_rec_stats()
        assert st["failed"] == 1 and st["records"] == len(c.records_of(2, 0, 500)) > 0, st
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_concatenate(case, hip_lib, monkeypatch):
    """two halves on two contexts: each hands out the batch's records of its half"""
    c = case[0]
    half = c.batch.n // 2
    _stage(monkeypatch, "path_first")
    al, al2 = _on(c), _on(c)
    try:
        a, b = _one_batch(al, c.piece(0, half)), _one_batch(al2, c.piece(half, c.batch.n), first=half)
        _same(a, c.records_of(2, 0, half))
        _same(b, c.records_of(2, half, c.batch.n))
        b["read"] += half
        _same(np.concatenate([a, b]), c.records(2))
        assert al.rescue_rec_stats()["records"] + al2.rescue_rec_stats()["records"] == len(c.records(2))
    finally:
        al.close()
        al2.close()
