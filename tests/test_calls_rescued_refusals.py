"""What `groot-hip align` refuses of `--callsRescued` and `--callSlots` before it does anything, in the manner of
tests/test_abundance_rescued_refusals.py: one command line per refusal, run in a directory that holds nothing, against names of an index
directory and a FASTQ file that do not exist.  The whole text of stdout and stderr and the exit status are pinned, and a refusal leaves
nothing behind.  The new checks come behind every earlier one (ORDER), the refusal of `--abundanceRescued --calls` without the new flag
keeps its text, and `report` does not know the flags."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
R = AL + ["--abundance", "a.tsv", "--abundanceRescued", "--calls", "c.tsv", "--callsRescued"]
BOTH = "--callsRescued puts the reads --abundanceRescued adds to the classes into the pileup of --calls: it needs both --calls and --abundanceRescued\n"
SLOTS = "--callSlots is a number of table slots, a power of two up to 2^31: %d\n"

# (id, arguments, stderr); stdout is empty for every one of them
REFUSED = [
    ("without_abundance_rescued", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--callsRescued"], BOTH),
    ("without_calls", AL + ["--abundance", "a.tsv", "--abundanceRescued", "--callsRescued"], BOTH),
    ("without_either", AL + ["--abundance", "a.tsv", "--callsRescued"], BOTH),
    ("slots_without_the_flag", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--callSlots", "1024"], "--callSlots is the size the table of --callsRescued starts with: it needs it\n"),
    ("slots_not_a_power_of_two", R + ["--callSlots", "12"], SLOTS % 12),
    ("slots_zero", R + ["--callSlots", "0"], SLOTS % 0),
    ("slots_too_many", R + ["--callSlots", "4294967296"], SLOTS % 4294967296),
    ("slots_not_a_number", R + ["--callSlots", "many"], "--callSlots takes a number: many\n"),
]
# an earlier check answers first, and the old refusal keeps its text where the new flag is absent
ORDER = [
    ("calls_without_the_flag", AL + ["--abundance", "a.tsv", "--abundanceRescued", "--calls", "c.tsv"],
     "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("calls_need_abundance_first", AL + ["--calls", "c.tsv", "--callsRescued"], "--calls has a line per line of the abundance file: it needs --abundance\n"),
    ("abundance_rescued_needs_abundance_first", AL + ["--abundanceRescued", "--callsRescued"],
     "--abundanceRescued adds the rescued reads to the classes --abundance estimates from: it needs --abundance\n"),
    ("rescue_range_first", R + ["--rescue", "4"], "--rescue allows 1, 2 or 3 substitutions: 4\n"),
    ("noalign_first", R + ["--noAlign"], "--abundance needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("interleaved_first", R + ["--interleaved"],
     "--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records outside the intersection have no "
     "weight rule\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in REFUSED + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == []               # no groot.log, no groot-graphs-*, none of the named files


@pytest.mark.parametrize("flag", [["--callsRescued"], ["--callSlots", "1024"]])
def test_report_does_not_know_the_flags(cli, tmp_path, flag):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--calls", "c.tsv"] + flag, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and flag[0][2:].encode() in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []
