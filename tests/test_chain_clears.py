"""The clears that left the batch's chain: the processing-order sort under the project's own launcher, whose one
scratch block is cleared once per batch behind the sort (order_sort.hpp, run_batch_async); the list counters of the seed stage and the work set's
overflow counts, which assign_q_rows_kernel leaves at zero; the work set's item counts, which order_ovf_kernel leaves at zero; the grids of
lsh_heavy_kernel and sort_seed_lists_kernel, sized by the lists of the latest finished batch; n_trav, which order_first_kernel writes.  All of it
is state that one batch leaves for the next, so every check here runs SEQUENCES of batches through one ctx that switch between

  all reads seeded / no read seeded / mixed lengths (75..150 bases: the list pass, the LSH-Forest branch and the long seed lists have entries,
  then none again) / a batch that follows one without seeds and is therefore ordered by stream compaction, not sorted / a batch below the
  sort's merge limit and batches above it, the second larger than the first (the scratch block grows)

-- pipelined at pipeline_depth 2 and 4 and one batch at a time, plain, under GROOT_TEST_SMALL_BUFFERS with one seed slot per read (every batch
with a read of two seeds is redone: the redo runs with the moved clears) and under GROOT_TEST_POISON.  Every batch is compared with the oracle's
answer for its reads (counters, every record field with its path set), the call counts over the sequence with the oracle's sum, and everything with
a ctx opened under GROOT_LIBRARY_SORT, which sorts every batch through rocprim::radix_sort_pairs as before: records and path sets bit for bit."""
import numpy as np
import pytest

import oracle_check
import test_batch_history as bh
from groot_amd import device, synth
from test_batch_history import need_gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SORT_MERGE_LIMIT = 2048          # GROOT_SORT_MERGE_LIMIT: batches above it take the onesweep (the project's launcher), batches up to it the library
ENV = ("GROOT_NO_PATH_PASS", "GROOT_LEAN", "GROOT_NO_SIG", "GROOT_NO_TEXT_TABLE", "GROOT_NO_OUTCOME_TABLE", "GROOT_TEST_SMALL_BUFFERS", "GROOT_TEST_POISON",
       "GROOT_LIBRARY_SORT", "GROOT_SERIAL_TAIL")
MODES = {"plain": {}, "small": {"GROOT_TEST_SMALL_BUFFERS": "1"}, "poison": {"GROOT_TEST_POISON": "1"}}
R = 9000                         # the largest batch
SEQUENCE = ["cc_seeded", "cc_mixed", "cc_seeded", "cc_none", "cc_seeded", "cc_mixed", "cc_small", "cc_big", "cc_none", "cc_mixed", "cc_big", "cc_small"]


def _make(index, name):
    cat, o, lens = synth.reference_sequences(index)
    if name == "cc_seeded":
        return bh._perfect(index, 5000, 30_000_000)
    if name == "cc_none":
        return bh._random(5000, 100, 81)
    if name == "cc_mixed":
        seq, off, _ = synth.reads_np(cat, o, lens, 4000, 150, first=31_000_000, min_len=75)
        return seq, off
    if name == "cc_small":
        return bh._perfect(index, 1500, 32_000_000)
    if name == "cc_big":
        return bh._perfect(index, R, 33_000_000)
    raise KeyError(name)


def _input(index, name):
    if name not in bh._INPUTS:
        seq, off = _make(index, name)
        bh._INPUTS[name] = (np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64))
    return bh._INPUTS[name]


def _env(monkeypatch, mode, library_sort=False):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    if library_sort:
        monkeypatch.setenv("GROOT_LIBRARY_SORT", "1")


def _open(index, mode, depth):
    # (small: one seed slot per read on top of the small buffers -- every batch that holds a read with two seeds is redone as a whole)
    return device.Aligner(index, max_batch_reads=R, max_read_len=256, pipeline_depth=depth, memo_budget_mb=device.MEMO_OFF,
                          max_seeds_per_read=1 if mode == "small" else 8)


def _preconditions(index):
    """what puts the batches on their paths, from the oracle and the reads themselves"""
    n = {name: len(_input(index, name)[1]) - 1 for name in set(SEQUENCE)}
    assert n["cc_small"] <= SORT_MERGE_LIMIT < n["cc_seeded"] < n["cc_big"] and n["cc_mixed"] > SORT_MERGE_LIMIT
    seeds = {name: bh._oracle(index, name)["seeds"] for name in set(SEQUENCE)}
    assert len(seeds["cc_none"]) == 0, "a random read has a seed"
    for name in ("cc_seeded", "cc_small", "cc_big"):
        assert len(np.unique(seeds[name]["read_id"])) > 0.9 * n[name], name
        assert np.bincount(seeds[name]["read_id"].astype(np.int64)).max() >= 2, (name, "no read has two seeds: nothing to redo with one seed slot per read")
    lens = np.diff(_input(index, "cc_mixed")[1].astype(np.int64))
    assert lens.min() < 100 < lens.max() and len(seeds["cc_mixed"]) > 0


def _pipelined(index, mode, depth):
    """SEQUENCE with `depth` batches in flight, collected oldest first"""
    firsts, first = [], 0
    for name in SEQUENCE:
        firsts.append(first)
        first += len(_input(index, name)[1]) - 1
    al = _open(index, mode, depth)
    got = []
    try:
        def take():
            r = al.collect()
            assert r["status"] == 0, r["status"]
            al.release(r["ticket"])
            got.append(r)

        for name, f in zip(SEQUENCE, firsts):
            al.submit(*_input(index, name), first_read_id=f)
            if al.in_flight()[0] == depth:
                take()
        while al.in_flight()[0]:
            take()
        att = al.attempts().copy()
    finally:
        al.close()
    assert [r["first_read_id"] for r in got] == firsts
    return got, att, firsts


def _against_oracle(index, got, att, firsts, where):
    oatt = np.zeros_like(att, dtype=np.int64)
    for i, (name, r) in enumerate(zip(SEQUENCE, got)):
        o = bh._oracle(index, name)
        for k in oracle_check.COUNTS:
            assert r["counts"][k] == o["counts"][k], (where, i, name, k, r["counts"][k], o["counts"][k])
        a = device.expand_alns(index, r["travs"], r["masks"])
        a["read_id"] -= firsts[i]
        assert len(a) == len(o["alns"]), (where, i, name, len(a), len(o["alns"]))
        for f in o["alns"].dtype.names:
            assert np.array_equal(a[f], o["alns"][f]), (where, i, name, f)
        oa = o["attempts"]
        oatt[: oa.shape[0]] += oa
    assert np.array_equal(att.astype(np.int64), oatt), (where, "call counts")


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_sequences_pipelined(argannot_index, need_gpu, monkeypatch, mode, depth):
    index = argannot_index
    _preconditions(index)
    _env(monkeypatch, mode)
    got, att, firsts = _pipelined(index, mode, depth)
    _against_oracle(index, got, att, firsts, (mode, depth, "own launcher"))
    _env(monkeypatch, mode, library_sort=True)
    ref, ratt, _ = _pipelined(index, mode, depth)
    _against_oracle(index, ref, ratt, firsts, (mode, depth, "library sort"))
    for i, (a, b) in enumerate(zip(got, ref)):
        for k in oracle_check.COUNTS:          # (the other counters say which kernel took a read: the launch choices of a pipelined run are timing)
            assert a["counts"][k] == b["counts"][k], (mode, depth, i, SEQUENCE[i], k)
        assert np.array_equal(a["travs"], b["travs"]) and np.array_equal(a["masks"], b["masks"]), (mode, depth, i, SEQUENCE[i])
    assert np.array_equal(att, ratt)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sequence_one_at_a_time(argannot_index, need_gpu, monkeypatch, mode):
    """every batch finishes before the next is submitted, so each is launched by the batch right before it: the batch behind the one without seeds is
    ordered by stream compaction (list mode, not sorted), the one behind that is sorted again; seeds and call-count deltas are compared too"""
    index = argannot_index
    _preconditions(index)
    _env(monkeypatch, mode)
    al = _open(index, mode, 2)
    att = np.zeros((0, index.view.n_windows), dtype=np.uint32)
    try:
        prev = None
        for i, name in enumerate(SEQUENCE):
            _input(index, name)
            b, att = bh._check(al, index, name, att, where=(mode, i))
            if prev == "cc_none":
                assert name != "cc_none" and b["counts"]["walked_reads"] > 0, "the batch in list mode walks no read: nothing is ordered"
            if name == "cc_none":
                assert b["counts"]["walked_reads"] == 0      # dfs_frac = 0: the next batch is launched in list mode
            if name == "cc_mixed":
                assert 0 < b["counts"]["full_sketch_reads"] < b["n"], "the signature kernel left no read to the list pass, or it did not run"
            prev = name
    finally:
        al.close()


@pytest.mark.parametrize("first", ["cc_seeded", "cc_none", "cc_mixed", "cc_small"])
@pytest.mark.parametrize("mode", ["plain", "small"])
def test_fresh_ctx_and_the_batch_behind_a_redo(argannot_index, need_gpu, monkeypatch, mode, first):
    """the first batch of a fresh ctx finds only what the allocation cleared; under `small` it is redone (cc_none apart: no seeds, nothing overflows), and
    the batch behind it is the first one that runs on what a redo left"""
    index = argannot_index
    _preconditions(index)
    _env(monkeypatch, mode)
    al = _open(index, mode, 2)
    att = np.zeros((0, index.view.n_windows), dtype=np.uint32)
    try:
        for i, name in enumerate([first, "cc_mixed", "cc_seeded"]):
            _input(index, name)
            _, att = bh._check(al, index, name, att, where=(mode, first, i))
    finally:
        al.close()
