"""What `groot-hip align` refuses around --callsGapped before it does anything, as tests/test_abundance_gapped_refusals.py pins the refusals
of --abundanceGapped: one command line each, run in an empty directory against names that do not exist; the whole text of stderr and the
exit status are pinned, stdout stays empty, and nothing is left behind.  The new checks stand behind every older one, so a command line
that trips an older refusal too is answered by that one, and without the flag the older texts are what they were; `report` does not know
the flag."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
AR = AL + ["--abundance", "a.tsv", "--abundanceRescued"]
AG = AR + ["--indels", "i.tsv", "--abundanceGapped"]
ALL = AG + ["--calls", "c.tsv", "--callsRescued", "--callsGapped"]
NO_CALLS = "--callsGapped puts the reads --abundanceGapped adds to the classes into the pileup of --calls: it needs --calls\n"
NO_CALLS_RESCUED = "--callsGapped piles the gap-placed reads up beside the rescued reads' records: it needs --callsRescued\n"
NO_AB_GAPPED = "--callsGapped piles up the reads --abundanceGapped adds to the classes: it needs it\n"
OLD_CALLS = "--abundanceGapped cannot be combined with --calls%s: its pileup has no rule for a gapped record, and a deletion covers two intervals\n"

CASES = [
    ("alone", AL + ["--callsGapped"], NO_CALLS),
    ("without_calls", AG + ["--callsGapped"], NO_CALLS),
    ("without_calls_beside_abundance", AL + ["--abundance", "a.tsv", "--callsGapped"], NO_CALLS),
    ("without_calls_rescued", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--callsGapped"], NO_CALLS_RESCUED),
    ("without_abundance_gapped", AR + ["--calls", "c.tsv", "--callsRescued", "--callsGapped"], NO_AB_GAPPED),
    ("without_abundance_gapped_with_indels", AR + ["--indels", "i.tsv", "--calls", "c.tsv", "--callsRescued", "--callsGapped"], NO_AB_GAPPED),
    # the older checks answer first, in their words
    ("abundance_rescued_first", AG + ["--calls", "c.tsv", "--callsGapped"], "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("abundance_gapped_needs_indels_first", AR + ["--abundanceGapped", "--calls", "c.tsv", "--callsRescued", "--callsGapped"],
     "--abundanceGapped counts the reads gapped rescue places, which --indels switches on: it needs it\n"),
    ("calls_rescued_needs_first", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--callsRescued", "--callsGapped"],
     "--callsRescued puts the reads --abundanceRescued adds to the classes into the pileup of --calls: it needs both --calls and --abundanceRescued\n"),
    ("call_slots_range_first", ALL + ["--callSlots", "3"], "--callSlots is a number of table slots, a power of two up to 2^31: 3\n"),
    ("calls_needs_abundance_first", AL + ["--calls", "c.tsv", "--callsGapped"], "--calls has a line per line of the abundance file: it needs --abundance\n"),
    ("paired_first", ALL + ["--interleaved"],
     "--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records outside the intersection have no "
     "weight rule\n"),
    ("noalign_first", ALL + ["--noAlign"], "--abundance needs the exact alignments: it cannot be combined with --noAlign\n"),
    # without the flag the refusal of --abundanceGapped beside --calls keeps its bytes
    ("old_refusal_with_calls_rescued", AG + ["--calls", "c.tsv", "--callsRescued"], OLD_CALLS % " --callsRescued"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in CASES])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == []


def test_the_switch_lifts_the_refusal(cli, tmp_path):
    """--abundanceGapped beside --calls --callsRescued --callsGapped passes the plan: the run then ends at its inputs, which do not exist"""
    r = subprocess.run([cli] + ALL + ["--callSlots", "4096", "--rescueGap", "8", "--bootstraps", "5", "--callSupport", "--rarefy", "r.tsv", "--noBam"], cwd=str(tmp_path),
                       capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--callsGapped" not in r.stderr and b"--abundanceGapped" not in r.stderr and b"no file found at r.fq" in r.stderr, r.stderr
    assert "c.tsv" not in os.listdir(str(tmp_path)) and "a.tsv" not in os.listdir(str(tmp_path))


def test_report_does_not_know_the_flag(cli, tmp_path):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--calls", "c.tsv", "--callsGapped"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and b"callsGapped" in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []
