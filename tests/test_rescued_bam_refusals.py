"""What `groot-hip align` refuses around --rescuedBam before it does anything, as tests/test_cli_refusals.py pins the older refusals: one
command line each, run in an empty directory against names that do not exist; the whole text of stderr and the exit status are pinned,
stdout stays empty, and nothing is left behind -- no log, no BAM, no graph directory.  The new checks stand behind every older one, so a
command line that trips an older refusal too is answered by that one; and --rescue is accepted with --rescuedBam alone."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
RB = AL + ["--rescuedBam", "r.bam"]
NOALIGN = "--rescuedBam holds the reads the exact alignments leave out: it cannot be combined with --noAlign\n"

CASES = [
    ("noalign", RB + ["--noAlign"], NOALIGN),
    ("assign", RB + ["--assignFrom", "f.tsv"], None),      # (an older check answers first: the file of --assignFrom does not exist)
    ("slots_without_flag", AL + ["--rescuedBamSlots", "100"], "--rescuedBamSlots is the room for the records of --rescuedBam: it needs it\n"),
    ("slots_zero", RB + ["--rescuedBamSlots", "0"], "--rescuedBamSlots is a number of records per batch, at least 1: 0\n"),
    ("slots_negative", RB + ["--rescuedBamSlots=-5"], "--rescuedBamSlots is a number of records per batch, at least 1: -5\n"),
    ("slots_no_number", RB + ["--rescuedBamSlots", "many"], "--rescuedBamSlots takes a number: many\n"),
    ("same_file", RB + ["--bam", "r.bam"], "--rescuedBam and --bam name the same file: r.bam\n"),
    ("no_value", AL + ["--rescuedBam"], "flag needs an argument: --rescuedBam\n"),
    # the older checks answer first
    ("rescue_range_first", RB + ["--rescue", "4", "--noAlign"], "--rescue allows 1, 2 or 3 substitutions: 4\n"),
    ("variants_noalign_first", RB + ["--variants", "v.tsv", "--noAlign"], "--variants rescues the reads the exact alignments leave out: it cannot be combined with --noAlign\n"),
    ("nobam_first", RB + ["--noBam"], "--noBam without --report would leave no output of the alignments\n"),
    ("slots_behind_noalign", RB + ["--noAlign", "--rescuedBamSlots", "0"], NOALIGN),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in CASES])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err if err is not None else "--assignFrom: no file found at f.tsv\n")
    assert os.listdir(str(tmp_path)) == []


def test_refused_with_assignment(cli, tmp_path):
    """with a file for --assignFrom to find, the refusal is --rescuedBam's own (the plan reads no file)"""
    (tmp_path / "f.tsv").write_bytes(b"")
    r = subprocess.run([cli] + RB + ["--assignFrom", "f.tsv"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", "--rescuedBam cannot be combined with --assignFrom: assignment rewrites the records that tell which reads are unaligned\n")
    assert os.listdir(str(tmp_path)) == ["f.tsv"]


def test_rescue_is_accepted_with_the_flag_alone(cli, tmp_path):
    """--rescue 3 --rescuedBam passes the plan: the run then ends at its inputs, which do not exist -- through the log, as every run past the plan"""
    r = subprocess.run([cli] + RB + ["--rescue", "3", "--rescuedBamSlots", "1000"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--rescue" not in r.stderr and b"no file found at r.fq" in r.stderr, r.stderr
    assert "r.bam" not in os.listdir(str(tmp_path))
