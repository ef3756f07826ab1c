"""The hand-off from the seed stage to the align stage and inside the align stage (groot_hip.hip launch_seed_stage / launch_align_stage):
the processing-order sort (rocprim radix_sort_pairs with 256-thread kernels), the list of reads the first pass appends for align_kernel
(a ballot and one atomic per wavefront at the end of first_pass_body, kernels_lean.hpp) and align_kernel's work set: that list followed by the
slots of the processing order a first pass on a narrow grid did not reach (kernels_align.hpp).

Memo off.  Every batch is compared with a fresh oracle run of the same reads -- counters, seeds, every record field with its path set, the
call-count delta -- under each of the three stages (path pass, GROOT_LEAN=1, GROOT_NO_PATH_PASS=1).  What puts a batch on its path (reads
with seeds, reads the first pass must leave) is asserted from the oracle's seeds and the reads themselves before the device is asked."""
import numpy as np
import pytest

import test_batch_history as bh
from groot_amd import device, host, synth
from test_batch_history import HEUR, Mirror, _check, _finished, _open, need_gpu, stage  # noqa: F401  (fixtures)
from test_path_pass import _gfa

pytestmark = pytest.mark.gpu

# Which rocprim algorithm sorts a batch of n reads under OrderSortConfig (groot_hip.hip; a fresh ctx and every batch that is not one of reads with
# errors gets that configuration):
#   n <= SINGLE_SORT_ITEMS         the single-block sort, 256 threads x 4 items (rocprim's default for it)
#   n <= SORT_MERGE_LIMIT          rocprim's merge sort (GROOT_SORT_MERGE_LIMIT = 2 048; rocprim's own default would be 2^20)
#   above                          the onesweep the configuration is about: 256 threads x GROOT_SORT_ITEMS = 16 items per thread per workgroup
SINGLE_SORT_ITEMS = 256 * 4
SORT_MERGE_LIMIT = 2048
SORT_BLOCK_ITEMS = 256 * 16
SIZES = [1, 63, 64, 65, 255, 256, 257,                                            # wavefront and workgroup seams of the list (single-block sort)
         SINGLE_SORT_ITEMS, SINGLE_SORT_ITEMS + 1, SORT_MERGE_LIMIT,                 # last single-block size, first and last merge-sort size
         SORT_MERGE_LIMIT + 1,                                                        # first onesweep size: one partly filled workgroup
         SORT_BLOCK_ITEMS - 1, SORT_BLOCK_ITEMS, SORT_BLOCK_ITEMS + 1, 2 * SORT_BLOCK_ITEMS + 1]   # onesweep: a workgroup less an item, whole, one more; two and one

_N = ord("N")


def _register(name, seq, off):
    """an input of this module among test_batch_history's: made once, its oracle answer computed once and shared by the stages"""
    if name not in bh._INPUTS:
        bh._INPUTS[name] = (np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64))
    return bh._INPUTS[name]


def _seeded(index, name):
    """reads of the input that have a seed, by the oracle: the reads the align stage walks"""
    return np.unique(bh._oracle(index, name)["seeds"]["read_id"])


def _one(index, stage, name):
    """the input as the first batch of a fresh ctx"""
    seq, off = bh._input(index, name)
    al = _open(index, max(len(off) - 1, 1))
    try:
        b, _ = _check(al, index, name, np.zeros((0, index.view.n_windows), dtype=np.uint32), where=stage)
    finally:
        al.close()
    assert b["counts"]["walked_reads"] == len(_seeded(index, name)), (b["counts"], len(_seeded(index, name)))
    return b


def _single_path_rows(index, n, seed):
    """error-free 100-mers of graphs that hold one path whose text is all ACGT: no walk branches and no node or window holds an 'N' (a first
    pass leaves the reads of a window or node with an 'N' at staging), so a first pass finishes every one that has a seed"""
    cat, o, lens = synth.reference_sequences(index)
    gop, npg = bh._graph_of_path(index)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ok = np.array([p for p in np.flatnonzero((npg[gop] == 1) & (lens >= 100)) if np.isin(cat[int(o[p]):int(o[p]) + int(lens[p])], acgt).all()])
    rng = np.random.default_rng(seed)
    p = ok[rng.integers(0, len(ok), n)]
    st = (rng.random(n) * (lens[p] - 99)).astype(np.int64)
    return np.stack([cat[int(o[q]) + int(s):int(o[q]) + int(s) + 100] for q, s in zip(p, st)]).astype(np.uint8)


# ---- sizes at the seams ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_the_seams(argannot_index, stage, n):
    """n error-free reads; every third one carries an N on its last base, so the list the first pass leaves has entries at every size
    beyond 2.  The sizes (SIZES) are the list's seams -- one wavefront less a lane, a whole one, one more; one workgroup -- and the sort's: the last
    size of the single-block sort, the merge sort's first and last, then the onesweep (every size above SORT_MERGE_LIMIT): its first size, one
    workgroup's items less one, whole, one more, two workgroups and one"""
    index = argannot_index
    name = "oh_size_%d" % n
    if name not in bh._INPUTS:
        seq, off = bh._perfect(index, n, 20_000_000)
        rows = seq.reshape(-1, 100).copy()
        rows[2::3, 99] = _N
        _register(name, rows.reshape(-1), off)
    seeded = _seeded(index, name)
    with_n = np.arange(2, n, 3)
    assert n < 3 or np.isin(with_n, seeded).any(), "no read with an N has a seed: the list would be empty"
    b = _one(index, stage, name)
    if stage != "no_path":
        left = b["counts"]["walked_reads"] - _finished(stage, b)
        assert left >= int(np.isin(with_n, seeded).sum()), (left, b["counts"], b["pp"])


# ---- an empty list, a full one, a list of one ----------------------------------------------------------------------------------------

def test_empty_list(argannot_index, stage):
    """reads of one-path graphs: the first pass finishes every read that is walked and appends nothing"""
    index = argannot_index
    _register("oh_empty", _single_path_rows(index, 3000, 31).reshape(-1), np.arange(3001, dtype=np.uint64) * 100)
    assert len(_seeded(index, "oh_empty")) > 2000
    b = _one(index, stage, "oh_empty")
    if stage != "no_path":
        assert _finished(stage, b) == b["counts"]["walked_reads"], (b["pp"], b["counts"])


def test_full_list(argannot_index, stage):
    """every read carries one byte other than ACGT (an N on its first or last base): the first pass leaves every walked read"""
    index = argannot_index
    seq, off = _register("oh_full", *bh._edge_n(index, 5000, 21_000_000, 7))
    assert ((seq.reshape(-1, 100) == _N).sum(axis=1) >= 1).all()      # (a few reference stretches bring an N of their own)
    assert len(_seeded(index, "oh_full")) > 2500
    b = _one(index, stage, "oh_full")
    if stage != "no_path":
        assert _finished(stage, b) == 0 and b["counts"]["walked_reads"] > 2500, (b["pp"], b["counts"])


def _n_twin(index):
    """a read of a one-path graph and its copy with an N on the last base that keeps the read's seeds (so also its sort key): by the oracle"""
    rows = _single_path_rows(index, 64, 41)
    twins = rows.copy()
    twins[:, 99] = _N
    run = bh.oracle_check.oracle_run(index, np.concatenate([rows, twins]).reshape(-1), np.arange(129, dtype=np.uint64) * 100)
    s = run.seeds()
    for i in range(64):
        a, b = np.sort(s["window_id"][s["read_id"] == i]), np.sort(s["window_id"][s["read_id"] == 64 + i])
        if 0 < len(a) <= 4 and np.array_equal(a, b):
            return rows[i], twins[i]
    raise AssertionError("no read keeps its seeds with an N on its last base")


def test_one_left_read_in_the_last_lane(argannot_index, stage):
    """639 copies of one read of a one-path graph, then the same read with an N on its last base: equal sort keys, the sort is stable, so the
    read with the N takes slot 639 -- the last lane of the tenth wavefront, the last one that has work -- and is the one read left"""
    index = argannot_index
    if "oh_one_left" not in bh._INPUTS:
        read, twin = _n_twin(index)
        _register("oh_one_left", np.concatenate([np.tile(read, 639), twin]), np.arange(641, dtype=np.uint64) * 100)
    seeds = bh._oracle(index, "oh_one_left")["seeds"]
    assert len(_seeded(index, "oh_one_left")) == 640 and 640 % 64 == 0
    first = np.sort(seeds["window_id"][seeds["read_id"] == 0])
    assert all(np.array_equal(np.sort(seeds["window_id"][seeds["read_id"] == r]), first) for r in (1, 638, 639))
    b = _one(index, stage, "oh_one_left")
    if stage != "no_path":
        assert b["counts"]["walked_reads"] - _finished(stage, b) == 1, (b["pp"], b["counts"])


# ---- the list and the range behind it ------------------------------------------------------------------------------------------------

def test_list_and_range(argannot_index, stage):
    """3 % walked, then a dense batch: the first pass's grid (sized by the sparse batch) is narrower than the reads with seeds, so align_kernel
    takes the list of the reads left inside the grid (every fifth read carries an N) and then slots [grid, reads with seeds) of the processing order"""
    index = argannot_index
    n = 100_000
    if "oh_dense" not in bh._INPUTS:
        seq, off = bh._perfect(index, n, 22_000_000)
        rows = seq.reshape(-1, 100).copy()
        rows[4::5, 99] = _N
        _register("oh_dense", rows.reshape(-1), off)
    att = np.zeros((0, index.view.n_windows), dtype=np.uint32)
    mir = Mirror(stage)
    al = _open(index, n)
    try:
        b0, att = _check(al, index, "sparse3", att, where=(stage, 0))
        mir.update(b0)
        assert HEUR["no_first_pass"] <= mir.dfs < HEUR["sparse"], mir.dfs
        slots = mir.lean_slots(n)
        walked = len(_seeded(index, "oh_dense"))
        assert walked > slots and (walked - slots) % 64 != 0, ("the range behind the list is empty or whole wavefronts", walked, slots)
        b1, att = _check(al, index, "oh_dense", att, where=(stage, 1))
    finally:
        al.close()
    assert b1["counts"]["walked_reads"] == walked
    if stage != "no_path":
        fin = _finished(stage, b1)
        assert 0 < fin < slots - slots // 10, ("no read was left inside the grid", fin, slots)


# ---- one digit bin ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("unseeded", [False, True])
def test_one_bin(argannot_index, stage, unseeded):
    """20 000 copies of one read (above SORT_MERGE_LIMIT: the onesweep): every pass of the sort puts everything into one bin; `unseeded`: 20 000 random reads among them, which have
    no seed and whose keys are all ones -- two bins, and a processing order whose second half nobody walks"""
    index = argannot_index
    name = "oh_one_bin_%d" % unseeded
    read = _single_path_rows(index, 1, 51)[0]
    if name not in bh._INPUTS:
        rows = np.tile(read, (20_000, 1))
        if unseeded:
            rnd, _ = bh._random(20_000, 100, 52)
            rows = np.concatenate([rows, rnd.reshape(-1, 100)])
            np.random.default_rng(53).shuffle(rows, axis=0)
        _register(name, rows.reshape(-1), np.arange(len(rows) + 1, dtype=np.uint64) * 100)
    seq, _ = bh._input(index, name)
    copies = np.flatnonzero((seq.reshape(-1, 100) == read).all(axis=1))
    assert 20_000 > SORT_MERGE_LIMIT
    assert len(copies) == 20_000 and np.array_equal(_seeded(index, name), copies), "the copies have a seed, the random reads have none"
    b = _one(index, stage, name)
    assert b["counts"]["walked_reads"] == 20_000


# ---- an index of two windows: the sorted key range is shorter than one digit -----------------------------------------------------------

@pytest.fixture(scope="module")
def two_window_index(tmp_path_factory):
    """one path of 32 bases in windows of 30 at k = 7: two windows, so that end_bit - begin_bit of the sort is 7, less than a digit"""
    rng = np.random.default_rng(61)
    text = "".join(rng.choice(list("ACGT"), 32))
    f = _gfa(tmp_path_factory.mktemp("oh") / "tiny.gfa", {1: text[:20], 2: text[20:]}, [(1, 2)], [("p0", [1, 2])])
    return host.Index.from_gfa_files([f], host.index_params(k=7, s=10, w=30)), text


def test_small_index(two_window_index, stage):
    """5 000 reads (above SORT_MERGE_LIMIT: the onesweep) on an index of two windows: the sorted key range is 7 bits, one pass over less than a digit"""
    assert 5000 > SORT_MERGE_LIMIT
    index, text = two_window_index
    nw = index.view.n_windows
    win_bits = max(3, 2 + max(nw - 1, 0).bit_length())
    assert (win_bits - 2) + min(6, 32 - win_bits) < 8, ("the sorted bits fill a digit", nw)     # GROOT_SPAN_BITS = 6
    if "oh_tiny" not in bh._INPUTS:
        cat, o, lens = synth.reference_sequences(index)
        seq, off, _ = synth.reads_np(cat, o, lens, 5000, 28, seed=62)
        rows = seq.reshape(-1, 28).copy()
        rows[4::5, 27] = _N
        _register("oh_tiny", rows.reshape(-1), off)
    name = "oh_tiny"
    seq, off = bh._input(index, name)
    if name not in bh._ORACLE:
        run = bh.oracle_check.oracle_run(index, seq, off, 0.9)
        bh._ORACLE[name] = {"counts": run.counts(), "seeds": run.seeds().astype(device.SEED_DTYPE), "alns": run.alns().astype(device.ALN_DTYPE),
                            "attempts": run.attempts().copy()}
    assert len(_seeded(index, name)) > 500
    al = device.Aligner(index, threshold=0.9, max_batch_reads=5000, max_read_len=256, memo_budget_mb=device.MEMO_OFF)
    try:
        b, _ = _check(al, index, name, np.zeros((0, nw), dtype=np.uint32), where=stage)
    finally:
        al.close()
    assert b["counts"]["walked_reads"] == len(_seeded(index, name))
