"""The definition of the gap-placed reads in assigned coverage (include/groot_hip.h, "gap-placed reads in assigned coverage") as a brute
force, for tests/test_gap_calls_def.py, tests/test_gap_calls.py and tests/test_calls_gapped_cli.py:

    A kept gapped placement (p, strand, x, type, g, k*) of a gap-rescued read r of length len is, with X = first Position of p + x,
       type DEL:  TWO gapped records of r on p, covering [X, X + k* - 1] and [X + k* + g, X + len + g - 1]
       type INS:  ONE gapped record of r on p, covering [X, X + len - g - 1]
    The table of a run is the multiset of exact records, rescued records AND gapped records grouped by (e = EC of S++(r), p, Pos, last).

The gapped rows come from gap_def.Brute.placements and gap_def.keep alone (every (path, strand, x, type, g, k): no anchors, no tables, no
knowledge of the kernels); the exact and the rescued rows from rescue_calls_def; all are keyed by S++(r) of gap_sets_def.  numpy only."""
import numpy as np

from gap_def import DEL, keep
from gap_sets_def import ecs_plus3
from rescue_calls_def import exact_rows, rescued_records
from rescue_def import A, path_texts
from test_calls import Table, _group


def rows_of(kept, L, first):
    """the gapped records of the kept placements of a read of L bases -> int64[n, 3] rows (path, Pos, last), in the order of `kept`, a DEL's
    two rows one behind the other; first: path -> the first Position of its text"""
    out = []
    for p, strand, x, typ, g, d, k in kept:
        X = first(p) + x
        if typ == DEL:
            out += [(p, X, X + k - 1), (p, X + k + g, X + L + g - 1)]
        else:
            out.append((p, X, X + L - g - 1))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def kept_placements(case, M, G):
    """-> {read: kept placements [(p, strand, x, type, g, d, k*)]} of the gap-rescued reads of the case's batch: a candidate that mismatch
    rescue leaves unplaced (case.rescued's second result), long enough for a gap, with a kept gapped placement"""
    brute, out = case.placements(M, G), {}
    for i in case.rescued(M)[1]:
        if len(case.reads[i]) < A * (M + 3):
            continue
        e, kept = keep(brute(case.reads[i]), M, G)
        if e is not None:
            out[i] = kept
    return out


def gapped_records(case, M, G):
    """-> {read: int64[n, 3] rows (path, Pos, last)} of the gap-rescued reads of the case's batch"""
    firsts = [t[1] if t is not None else 0 for t in path_texts(case.index)]
    return {i: rows_of(kept, len(case.reads[i]), lambda p: firsts[p]) for i, kept in kept_placements(case, M, G).items()}


def table_of3(exact, ex_rows, rescued, res_records, gapped, gap_records, gap_kept=None, reads=None):
    """the table of the definition over `reads` (default: all): exact {read: S(r)}, ex_rows exact_rows(), rescued {read: Rescued} and
    res_records rescued_records() as for rescue_calls_def.table_of, gapped {read: Gapped} of gap_sets_def.gap_sets, gap_records
    gapped_records(), gap_kept kept_placements() (for the cross-check) -> test_calls.Table (ECs canonical, rows ascending)"""
    sel_reads = None if reads is None else set(reads)
    ecs = sorted(ecs_plus3(exact, rescued, gapped, None if reads is None else list(reads)).items())
    index = {ids: i for i, (ids, _) in enumerate(ecs)}
    rows = [np.zeros((0, 4), dtype=np.int64)]
    if len(ex_rows):
        sel = ex_rows if sel_reads is None else ex_rows[np.isin(ex_rows[:, 0], sorted(sel_reads))]
        e = np.array([index[exact[int(r)]] for r in sel[:, 0]], dtype=np.int64)
        rows.append(np.column_stack([e, sel[:, 1:]]).reshape(-1, 4))
    for i, rec in res_records.items():
        if sel_reads is not None and i not in sel_reads:
            continue
        assert tuple(np.unique(rec[:, 0]).tolist()) == rescued[i].paths and len(rec) == rescued[i].kept      # the two brute forces agree on R(r)
        rows.append(np.column_stack([np.full(len(rec), index[rescued[i].paths], dtype=np.int64), rec[:, :3]]))
    assert set(gap_records) == set(gapped)                                                                   # ... on who is gap-rescued
    for i, rec in gap_records.items():
        if sel_reads is not None and i not in sel_reads:
            continue
        assert tuple(np.unique(rec[:, 0]).tolist()) == gapped[i].paths                                       # ... on G(r)
        if gap_kept is not None:                                                                             # ... and on the number of kept placements
            assert len(gap_kept[i]) == gapped[i].kept and len(rec) == gapped[i].kept + sum(1 for pl in gap_kept[i] if pl[3] == DEL)
        rows.append(np.column_stack([np.full(len(rec), index[gapped[i].paths], dtype=np.int64), rec]))
    rows = np.concatenate(rows)
    return Table(ecs, *_group(rows, np.ones(len(rows), dtype=np.int64)))


class GapCalls:
    """the definition over tests/gap_ec_case.py's batch, each piece computed once per (M, G)"""

    def __init__(self, case):
        self.case = case
        self._ex_rows = None
        self._res_rec, self._kept, self._gap_rec, self._tables = {}, {}, {}, {}

    def ex_rows(self):
        if self._ex_rows is None:
            self._ex_rows = exact_rows(self.case.index, self.case.batch.want(self.case.index).alns, self.case.batch.off)
        return self._ex_rows

    def res_records(self, M):
        if M not in self._res_rec:
            c = self.case
            self._res_rec[M] = rescued_records(c.index, M, c.reads, c.has, c._tables)
        return self._res_rec[M]

    def kept(self, M, G):
        if (M, G) not in self._kept:
            self._kept[M, G] = kept_placements(self.case, M, G)
        return self._kept[M, G]

    def gap_records(self, M, G):
        if (M, G) not in self._gap_rec:
            self._gap_rec[M, G] = gapped_records(self.case, M, G)
        return self._gap_rec[M, G]

    def table(self, M=2, G=3, reads=None, gapped=True, rescued=True):
        """gapped off: the table of the rescued reads in assigned coverage alone; rescued off too: the exact records'"""
        key = (M, G, None if reads is None else tuple(reads), gapped, rescued)
        if key not in self._tables:
            c = self.case
            res = c.rescued(M)[0] if rescued else {}
            rec = self.res_records(M) if rescued else {}
            on = gapped and rescued
            self._tables[key] = table_of3(c.exact(), self.ex_rows(), res, rec, c.gapped(M, G)[0] if on else {}, self.gap_records(M, G) if on else {},
                                          self.kept(M, G) if on else None, reads)
        return self._tables[key]

    def counts(self, M=2, G=3, reads=None, max_segs=4):
        """what the stats of a run over `reads` say: gap-rescued reads, slow ones, their placements, records, records folded on the host;
        rescued records and those folded on the host"""
        c = self.case
        sel = range(c.batch.n) if reads is None else reads
        gap, res = c.gapped(M, G)[0], c.rescued(M)[0]
        kept, grec, rrec = self.kept(M, G), self.gap_records(M, G), self.res_records(M)
        g = [i for i in sel if i in gap]
        gs = [i for i in g if c.graphs_of(gap[i].paths) > max_segs]
        r = [i for i in sel if i in rrec]
        return dict(gap=len(g), gap_slow=len(gs), placements=sum(len(kept[i]) for i in g), records=sum(len(grec[i]) for i in g),
                    host_records=sum(len(grec[i]) for i in gs), host_entries_res=sum(len(rrec[i]) for i in r if c.graphs_of(res[i].paths) > max_segs),
                    res_records=sum(len(rrec[i]) for i in r), res_slow=sum(1 for i in r if c.graphs_of(res[i].paths) > max_segs))


_CALLS = {}


def gap_calls(case):
    """built once per session, for every test module"""
    if id(case) not in _CALLS:
        _CALLS[id(case)] = GapCalls(case)
    return _CALLS[id(case)]
