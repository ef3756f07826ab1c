"""The case of tests/test_rescue_records_def.py and tests/test_rescue_records.py: the eight graphs and the batch of tests/test_rescue.py
(reads of 47 .. 150 bases in every class of mismatch rescue), with the definition's rescued records per M (tests/rescue_records_def.py).
Built once per process and shared by the two test files; the brute force's windows do not depend on M and are shared too."""
import numpy as np

from groot_amd import host
from rescue_def import Tables, path_texts
from rescue_records_def import records
from test_counter_edges import NP, SEGS, _graph, _of_reads
from test_path_pass import _seq
from test_rescue import _extra_graph, _has_record, _make_reads, _reads_of

_CASE = []


class RecordsCase:
    def __init__(self, tmp):
        rng = np.random.default_rng(13)
        shared = {name: _seq(rng, 45) for name, _ in SEGS}
        files = [_graph(rng, tmp / ("g%d.gfa" % g), g, shared)[0] for g in range(len(NP))] + [_extra_graph(rng, tmp / "g7.gfa")]
        self.index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=64))
        self.texts = path_texts(self.index)
        named = _make_reads(np.random.default_rng(14), self.texts)
        order = np.random.default_rng(15).permutation(len(named))
        self.names = [named[i][0] for i in order]
        self.batch = _of_reads("classes", [named[i][1] for i in order])
        self.reads = _reads_of(self.batch)
        self.has = _has_record(self.batch, self.index)
        self._win, self._rec = {}, {}

    def tables(self, M):
        t = Tables(self.index, M)
        t._win = self._win                 # (every window of every text: the same for every M)
        return t

    def records(self, M):
        """the definition's records of the whole batch under M"""
        if M not in self._rec:
            self._rec[M] = records(self.index, M, self.reads, self.has, self.tables(M))
        return self._rec[M]

    def records_of(self, M, lo, hi):
        """... of the piece [lo, hi) of the batch as a batch of its own: a read's records do not depend on its batch, `read` does"""
        rec = self.records(M)
        out = rec[(rec["read"] >= lo) & (rec["read"] < hi)].copy()
        out["read"] -= lo
        return out

    def piece(self, lo, hi):
        return _of_reads("reads %d..%d" % (lo, hi), self.reads[lo:hi])


def the_case(tmp_path_factory):
    if not _CASE:
        _CASE.append(RecordsCase(tmp_path_factory.mktemp("rescue_records")))
    return _CASE[0]
