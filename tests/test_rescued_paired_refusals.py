"""What `groot-hip align` refuses of `--rescuedPaired` before it does anything, in the manner of tests/test_abundance_rescued_refusals.py:
one command line per refusal, run in a directory that holds nothing; the whole text of stdout and stderr and the exit status are pinned,
and a refusal leaves nothing behind.  The new checks come behind every earlier one (ORDER: the old texts byte for byte), and `report` does
not know the flag.  Behind them the library's own refusals (groot_hip_rescue_pairs_enable and the enables beside it), in both orders, with
code and text."""
import os
import subprocess

import numpy as np
import pytest

from groot_amd import host


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
R = AL + ["--abundance", "a.tsv", "--abundanceRescued"]
RP = R + ["--interleaved", "--rescuedPaired"]
FRAGS = "--abundanceRescued cannot be combined with %s yet: mates are rescued one by one, and a fragment's set has no rule for them\n"

REFUSED = [
    ("without_abundance_rescued", AL + ["--abundance", "a.tsv", "--interleaved", "--rescuedPaired"],
     "--rescuedPaired is the rule for the rescued mates of fragments: it needs --abundanceRescued\n"),
    ("without_fragments", R + ["--rescuedPaired"], "--rescuedPaired is the rule for the rescued mates of fragments: it needs --paired or --interleaved\n"),
    ("shared_reads", RP + ["--report", "r.tsv", "--sharedReads", "s.tsv"],
     "--rescuedPaired cannot be combined with --sharedReads: its pairs hold no rescued reads, and the fragments with a rescued mate would be missing from them\n"),
    ("calls_paired", RP + ["--calls", "c.tsv", "--callsRescued", "--callsPaired"],
     "--rescuedPaired cannot be combined with --calls: its pileup has no rule for a fragment with a rescued mate\n"),
    ("abundance_gapped", RP + ["--indels", "i.tsv", "--abundanceGapped"],
     "--rescuedPaired cannot be combined with --abundanceGapped: the rule for fragments knows exact and mismatch-rescued mates only\n"),
]
# an earlier check answers first, in the words it has today
ORDER = [
    ("paired_without_the_flag", R + ["-f", "r2.fq", "--paired"], FRAGS % "--paired"),
    ("interleaved_without_the_flag", R + ["--interleaved"], FRAGS % "--interleaved"),
    ("without_abundance", AL + ["--abundanceRescued", "--interleaved", "--rescuedPaired"],
     "--interleaved changes what --sharedReads and --abundance count, and nothing else: it needs one of them\n"),
    ("calls_first", RP + ["--calls", "c.tsv", "--callsPaired"], "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("calls_with_fragments_first", RP + ["--calls", "c.tsv", "--callsRescued"],
     "--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records "
     "outside the intersection have no weight rule\n"),
    ("assign_first", RP + ["--assignFrom", "f.tsv"],
     "--assignFrom cannot be combined with --abundance: it estimates from every ARG a read lies on, and an assigned read lies on one: run it as the first pass\n"),
    ("abundance_gapped_needs_indels_first", RP + ["--abundanceGapped"],
     "--abundanceGapped counts the reads gapped rescue places, which --indels switches on: it needs it\n"),
    ("paired_file_count_first", R + ["--paired", "--rescuedPaired"], "--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): 1 file(s) given\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in REFUSED + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    (tmp_path / "f.tsv").write_bytes(b"")
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == ["f.tsv"]        # no groot.log, no groot-graphs-*, none of the named files


def test_report_does_not_know_the_flag(cli, tmp_path):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--rescuedPaired"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and b"rescuedPaired" in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []


# ---- the library ---------------------------------------------------------------------------------------------------------------------------

def _refused(call, code, text):
    with pytest.raises(host.GrootError) as e:
        call()
    assert e.value.code == code and text in str(e.value), e.value


STATE, UNSUPPORTED = -9, -10
OLD_REC = "rescued reads in the equivalence classes with paired-end units are not supported: mates are rescued one by one"
OLD_PAIRS = "paired-end units with rescued reads in the equivalence classes are not supported: mates are rescued one by one (groot_hip_rescue_ec_enable)"


@pytest.mark.gpu
def test_library_refusals_in_both_orders(argannot_index, hip_lib):
    from groot_amd import device

    al = device.Aligner(argannot_index, max_batch_reads=1024, memo_budget_mb=device.MEMO_OFF)
    try:
        on = al.rescue_pairs_enable
        _refused(on, STATE, "rescued mates in paired-end units: mismatch rescue is off (groot_hip_rescue_enable)")
        assert al.rescue_pairs_stats()["launches"] == 0
        al.rescue_enable(1)
        # the old refusals, rule off, byte for byte
        al.ec_enable(); al.pairs_enable()
        _refused(al.rescue_ec_enable, UNSUPPORTED, OLD_REC)
        al.pairs_enable(False); al.rescue_ec_enable()
        _refused(al.pairs_enable, UNSUPPORTED, OLD_PAIRS)
        al.rescue_ec_enable(False)
        # the five features, each first
        al.shared_enable()
        _refused(on, UNSUPPORTED, "rescued mates in paired-end units with shared reads are not supported: the triangle has no rescued reads")
        al.shared_enable(False)
        al.acov_enable()
        _refused(on, UNSUPPORTED, "rescued mates in paired-end units with assigned coverage are not supported: a rescued mate has no record to weigh (groot_hip_acov_enable)")
        al.acov_enable(False)
        al.acov_pairs_enable()
        _refused(on, UNSUPPORTED, "rescued mates in paired-end units with assigned coverage over fragments are not supported")
        al.acov_pairs_enable(False); al.pairs_enable(False)
        al.gap_enable(3); al.rescue_ec_enable(); al.gap_ec_enable()
        _refused(on, UNSUPPORTED, "rescued mates in paired-end units with gap-placed reads in the equivalence classes are not supported")
        al.gap_ec_enable(False); al.rescue_ec_enable(False); al.ec_enable(False)
        al.rescue_enable(0)
        al.assign_enable(np.ones(argannot_index.view.n_paths))
        _refused(on, UNSUPPORTED, "rescued mates in paired-end units count S(r), which assignment collapses (groot_hip_assign_enable)")
        al.assign_enable(None)
        # the rule first: it brings the classes, pairing and the rescued classes, and each of the five is refused behind it
        al.rescue_enable(1); al.gap_enable(3)
        on()
        assert al.pairs_stats() == dict(joined=0, split=0, single=0) and al.rescue_ec_stats()["rows"] > 0 and al.ec_stats()["reads"] == 0
        on(); al.pairs_enable(); al.rescue_ec_enable()          # each of them again: no-ops, the rule is on
        _refused(al.shared_enable, UNSUPPORTED, "shared reads with rescued mates in paired-end units are not supported: the triangle has no rescued reads")
        _refused(al.acov_enable, UNSUPPORTED, "assigned coverage with paired-end units is not supported")
        _refused(al.acov_pairs_enable, UNSUPPORTED, "assigned coverage over fragments with rescued reads in the equivalence classes is not supported: mates are rescued one by one")
        _refused(al.gap_ec_enable, UNSUPPORTED, "gap-placed reads in the equivalence classes with rescued mates in paired-end units are not supported")
        _refused(lambda: al.assign_enable(np.ones(argannot_index.view.n_paths)), UNSUPPORTED, "assignment collapses S(r)")
        # every way out leaves no state with pairing and the rescued classes on and the rule off
        al.rescue_ec_enable(False)
        assert al.rescue_ec_stats()["rows"] == 0 and al.pairs_stats() == dict(joined=0, split=0, single=0)
        _refused(al.rescue_ec_enable, UNSUPPORTED, OLD_REC)
        on(); al.pairs_enable(False)
        assert al.rescue_ec_stats()["rows"] == 0
        with pytest.raises(host.GrootError):
            al.pairs_stats()
        on(); al.ec_enable(False)
        assert al.rescue_ec_stats()["rows"] == 0
        on(); al.rescue_enable(0)
        assert al.rescue_ec_stats()["rows"] == 0
        al.rescue_enable(1); on(); al.ec_reset()
        assert al.rescue_ec_stats()["rows"] > 0
        on(False)
        assert al.rescue_ec_stats()["rows"] == 0 and al.pairs_stats() == dict(joined=0, split=0, single=0) and al.ec_stats()["reads"] == 0
    finally:
        al.close()
