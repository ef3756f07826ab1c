"""What `groot-hip align` refuses around --rescuedBamGaps before it does anything, as tests/test_rescued_bam_refusals.py pins the refusals
of --rescuedBam: one command line each, run in an empty directory against names that do not exist; the whole text of stderr and the exit
status are pinned, stdout stays empty, and nothing is left behind.  The new checks stand behind every older one, so a command line that
trips an older refusal too is answered by that one."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
RB = AL + ["--rescuedBam", "r.bam"]
ALL = RB + ["--indels", "i.tsv", "--rescuedBamGaps"]
NO_BAM = "--rescuedBamGaps adds the gap-placed reads to the file of --rescuedBam: it needs it\n"
NO_INDELS = "--rescuedBamGaps writes the placements of gapped rescue, which --indels switches on: it needs it\n"
NO_SWITCH = "--gapRecordSlots is the room for the records of --rescuedBamGaps: it needs it\n"

CASES = [
    ("without_rescued_bam", AL + ["--indels", "i.tsv", "--rescuedBamGaps"], NO_BAM),
    ("alone", AL + ["--rescuedBamGaps"], NO_BAM),
    ("without_indels", RB + ["--rescuedBamGaps"], NO_INDELS),
    ("without_indels_with_variants", RB + ["--variants", "v.tsv", "--rescuedBamGaps"], NO_INDELS),
    ("slots_without_switch", RB + ["--indels", "i.tsv", "--gapRecordSlots", "100"], NO_SWITCH),
    ("slots_alone", AL + ["--gapRecordSlots", "100"], NO_SWITCH),
    ("slots_zero", ALL + ["--gapRecordSlots", "0"], "--gapRecordSlots is a number of records per batch, at least 1: 0\n"),
    ("slots_negative", ALL + ["--gapRecordSlots=-5"], "--gapRecordSlots is a number of records per batch, at least 1: -5\n"),
    ("slots_no_number", ALL + ["--gapRecordSlots", "many"], "--gapRecordSlots takes a number: many\n"),
    ("slots_no_value", ALL + ["--gapRecordSlots"], "flag needs an argument: --gapRecordSlots\n"),
    # the older checks answer first
    ("rescued_bam_noalign_first", ALL + ["--noAlign"], "--indels rescues the reads the exact alignments leave out: it cannot be combined with --noAlign\n"),
    ("rescued_bam_slots_first", ALL + ["--rescuedBamSlots", "0", "--gapRecordSlots", "0"], "--rescuedBamSlots is a number of records per batch, at least 1: 0\n"),
    ("gap_range_first", RB + ["--rescueGap", "9", "--indels", "i.tsv", "--gapRecordSlots", "5"], "--rescueGap allows a gap of 1 to 8 bases: 9\n"),
    ("same_file_first", AL + ["--rescuedBam", "r.bam", "--bam", "r.bam", "--rescuedBamGaps"], "--rescuedBam and --bam name the same file: r.bam\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in CASES])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == []


def test_the_switch_is_accepted_with_both_files(cli, tmp_path):
    """--rescuedBam --indels --rescuedBamGaps --gapRecordSlots passes the plan: the run then ends at its inputs, which do not exist"""
    r = subprocess.run([cli] + ALL + ["--gapRecordSlots", "1000", "--rescueGap", "8"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--rescuedBamGaps" not in r.stderr and b"--gapRecordSlots" not in r.stderr and b"no file found at r.fq" in r.stderr, r.stderr
    assert "r.bam" not in os.listdir(str(tmp_path))
