"""What `groot-hip align` refuses around --abundanceGapped before it does anything, as tests/test_abundance_rescued_refusals.py pins the
refusals of --abundanceRescued: one command line each, run in an empty directory against names that do not exist; the whole text of stderr
and the exit status are pinned, stdout stays empty, and nothing is left behind.  The new checks stand behind every older one, so a command
line that trips an older refusal too is answered by that one; `report` does not know the flag."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
AR = AL + ["--abundance", "a.tsv", "--abundanceRescued"]
ALL = AR + ["--indels", "i.tsv", "--abundanceGapped"]
NO_RESCUED = "--abundanceGapped adds the gap-placed reads to the classes beside the reads --abundanceRescued adds: it needs it\n"
NO_INDELS = "--abundanceGapped counts the reads gapped rescue places, which --indels switches on: it needs it\n"
CALLS = "--abundanceGapped cannot be combined with --calls%s: its pileup has no rule for a gapped record, and a deletion covers two intervals\n"

CASES = [
    ("alone", AL + ["--abundanceGapped"], NO_RESCUED),
    ("without_abundance_rescued", AL + ["--abundance", "a.tsv", "--indels", "i.tsv", "--abundanceGapped"], NO_RESCUED),
    ("without_indels", AR + ["--abundanceGapped"], NO_INDELS),
    ("without_indels_with_variants", AR + ["--variants", "v.tsv", "--abundanceGapped"], NO_INDELS),
    ("neither_rescued_first", AL + ["--abundance", "a.tsv", "--abundanceGapped"], NO_RESCUED),
    ("calls_rescued", ALL + ["--calls", "c.tsv", "--callsRescued"], CALLS % " --callsRescued"),
    # the older checks answer first
    ("calls_alone_is_abundance_rescueds", ALL + ["--calls", "c.tsv"], "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("abundance_first", AL + ["--abundanceRescued", "--indels", "i.tsv", "--abundanceGapped"],
     "--abundanceRescued adds the rescued reads to the classes --abundance estimates from: it needs --abundance\n"),
    ("noalign_first", ALL + ["--noAlign"], "--abundance needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("gap_range_first", ALL + ["--rescueGap", "9"], "--rescueGap allows a gap of 1 to 8 bases: 9\n"),
    ("rescue_gap_still_needs_indels", AR + ["--abundanceGapped", "--rescueGap", "2"], "--rescueGap and --gapEventSlots are the gap length and the table size of --indels: they need it\n"),
    ("paired_first", ALL + ["--interleaved"],
     "--abundanceRescued cannot be combined with --interleaved yet: mates are rescued one by one, and a fragment's set has no rule for them\n"),
    ("rescued_bam_gaps_first", ALL + ["--rescuedBamGaps", "--calls", "c.tsv", "--callsRescued"], "--rescuedBamGaps adds the gap-placed reads to the file of --rescuedBam: it needs it\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in CASES])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == []


def test_the_switch_is_accepted_with_both_flags(cli, tmp_path):
    """--abundance --abundanceRescued --indels --abundanceGapped --rescueGap passes the plan: the run then ends at its inputs, which do not exist"""
    r = subprocess.run([cli] + ALL + ["--rescueGap", "8", "--bootstraps", "5", "--rarefy", "r.tsv"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--abundanceGapped" not in r.stderr and b"no file found at r.fq" in r.stderr, r.stderr
    assert "a.tsv" not in os.listdir(str(tmp_path))


def test_report_does_not_know_the_flag(cli, tmp_path):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--abundanceGapped"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and b"abundanceGapped" in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []
