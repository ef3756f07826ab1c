"""What `groot-hip align` refuses of `--callsRescuedPaired` before it does anything, in the manner of tests/test_rescued_paired_refusals.py:
one command line per refusal, run in a directory that holds nothing; the whole text of stdout and stderr and the exit status are pinned,
and a refusal leaves nothing behind.  The new checks come behind every earlier one (ORDER: the old texts byte for byte), the flag passes
over the one refusal that stood between --rescuedPaired and --calls and over nothing else, and `report` does not know the flag.  (The
library's own refusals are in tests/test_calls_rescued_paired.py.)"""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
R = AL + ["--abundance", "a.tsv", "--abundanceRescued"]
FLAG = ["--callsRescuedPaired"]
ALL = R + ["--interleaved", "--rescuedPaired", "--calls", "c.tsv", "--callsPaired", "--callsRescued"]

REFUSED = [
    ("without_calls", AL + ["--abundance", "a.tsv"] + FLAG, "--callsRescuedPaired piles up the fragments with rescued mates in the file of --calls: it needs --calls\n"),
    ("without_calls_paired", R + ["--calls", "c.tsv", "--callsRescued"] + FLAG,
     "--callsRescuedPaired extends the rule of --callsPaired to rescued mates: it needs --callsPaired\n"),
    # (told where --abundanceRescued meets fragments, the one place a missing --rescuedPaired can be seen; with the flag absent that check keeps its words)
    ("without_rescued_paired", R + ["--interleaved", "--calls", "c.tsv", "--callsPaired", "--callsRescued"] + FLAG,
     "--callsRescuedPaired piles up under the units of --rescuedPaired: it needs --rescuedPaired\n"),
    ("without_calls_rescued", AL + ["--abundance", "a.tsv", "--interleaved", "--calls", "c.tsv", "--callsPaired"] + FLAG,
     "--callsRescuedPaired piles up the placements --callsRescued counts, over fragments: it needs --callsRescued\n"),
]
# an earlier check answers first, in the words it has today -- with the flag and without it
ORDER = [
    ("fragments_without_either_flag", R + ["--interleaved", "--calls", "c.tsv", "--callsPaired", "--callsRescued"],
     "--abundanceRescued cannot be combined with --interleaved yet: mates are rescued one by one, and a fragment's set has no rule for them\n"),
    ("today_without_the_flag", ALL, "--rescuedPaired cannot be combined with --calls: its pileup has no rule for a fragment with a rescued mate\n"),
    ("without_abundance_rescued", AL + ["--abundance", "a.tsv", "--interleaved", "--calls", "c.tsv", "--callsPaired", "--callsRescued"] + FLAG,
     "--callsRescued puts the reads --abundanceRescued adds to the classes into the pileup of --calls: it needs both --calls and --abundanceRescued\n"),
    ("without_abundance", AL + ["--calls", "c.tsv"] + FLAG, "--calls has a line per line of the abundance file: it needs --abundance\n"),
    ("without_fragments", R + ["--rescuedPaired", "--calls", "c.tsv", "--callsPaired", "--callsRescued"] + FLAG,
     "--callsPaired is the rule for the records of fragments: it needs --paired or --interleaved\n"),
    ("calls_rescued_missing_beside_fragments", R + ["--interleaved", "--rescuedPaired", "--calls", "c.tsv", "--callsPaired"] + FLAG,
     "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("calls_paired_missing_beside_fragments", R + ["--interleaved", "--rescuedPaired", "--calls", "c.tsv", "--callsRescued"] + FLAG,
     "--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records "
     "outside the intersection have no weight rule\n"),
    ("shared_reads", ALL + FLAG + ["--report", "r.tsv", "--sharedReads", "s.tsv"],
     "--rescuedPaired cannot be combined with --sharedReads: its pairs hold no rescued reads, and the fragments with a rescued mate would be missing from them\n"),
    ("abundance_gapped", ALL + FLAG + ["--indels", "i.tsv", "--abundanceGapped", "--callsGapped"],
     "--rescuedPaired cannot be combined with --abundanceGapped: the rule for fragments knows exact and mismatch-rescued mates only\n"),
    ("assign_first", ALL + FLAG + ["--assignFrom", "f.tsv"],
     "--assignFrom cannot be combined with --abundance: it estimates from every ARG a read lies on, and an assigned read lies on one: run it as the first pass\n"),
    ("call_slots", ALL + FLAG + ["--callSlots", "3"], "--callSlots is a number of table slots, a power of two up to 2^31: 3\n"),
    ("no_align", ALL + FLAG + ["--noAlign"], "--abundance needs the exact alignments: it cannot be combined with --noAlign\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in REFUSED + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    (tmp_path / "f.tsv").write_bytes(b"")
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == ["f.tsv"]        # no groot.log, no groot-graphs-*, none of the named files


def test_the_whole_set_of_flags_passes_the_plan(cli, tmp_path):
    """every flag the rule needs, and the flag: no refusal of the plan is left -- the run ends at the first input file it cannot find"""
    r = subprocess.run([cli] + ALL + FLAG, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"no file found at r.fq\n"), r.stderr


def test_report_does_not_know_the_flag(cli, tmp_path):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--calls", "c.tsv", "--callsRescuedPaired"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and b"callsRescuedPaired" in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []
