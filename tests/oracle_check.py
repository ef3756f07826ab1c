"""The device's results for one batch against the CPU oracle (oracle/oracle_py.Run) on the same batch, field by field: the counters,
the seeds, every field of the alignment records, the IncrementSubPath call counts and the f64 graph weights.  Shared by the parity
modules; a plain module, not a fixture file."""
import numpy as np

from groot_amd import device
from oracle import oracle_py as O

COUNTS = ("received", "mapped", "multimapped", "alignments", "seeds", "revcomp_panics")


def oracle_run(index, seq, off, threshold=0.99, no_align=False, first=0):
    run = O.Run(index, threshold, no_align)
    run.batch(seq, off, first_read_id=first)
    return run


def device_results(al, index):
    """what assert_same compares, taken from an open Aligner after wait() (so the Aligner can be closed before the comparison)"""
    att = al.attempts().copy()
    kf, kt = device.weights(index, att)
    return {"seeds": al.seeds(), "alns": al.alns(), "attempts": att, "kmer_freq": kf, "kmer_total": kt}


def assert_same(counts, res, run, where=""):
    """counts: the device's counters (Aligner.wait()); res: device_results(); run: the oracle on the same batch"""
    oc = run.counts()
    for k in COUNTS:
        assert counts[k] == oc[k], (where, k, counts[k], oc[k])
    assert np.array_equal(res["seeds"], run.seeds().astype(device.SEED_DTYPE)), (where, "seeds")
    got, exp = res["alns"], run.alns()
    assert len(got) == len(exp), (where, "alignments", len(got), len(exp))
    for f in exp.dtype.names:
        assert np.array_equal(got[f], exp[f]), (where, f, np.flatnonzero(got[f] != exp[f])[:8])
    att, oatt = res["attempts"], run.attempts()
    assert np.array_equal(att[: oatt.shape[0]], oatt) and not att[oatt.shape[0]:].any(), (where, "attempts")
    okf, okt = run.weights(order=1)
    assert np.array_equal(res["kmer_freq"], okf) and np.array_equal(res["kmer_total"], okt), (where, "weights")
    return got
