"""What `groot-hip align` refuses around --callsPaired before it does anything, as tests/test_calls_gapped_refusals.py pins the refusals of
--callsGapped: one command line each, run in an empty directory against names that do not exist; the whole text of stderr and the exit
status are pinned, stdout stays empty, and nothing is left behind.  The new checks stand behind every older one, so a command line that
trips an older refusal too is answered by that one -- that is how --callsPaired beside --callsRescued, --abundanceRescued or --assignFrom is
refused, each in the words that refuse fragments there today -- and without the flag `--calls --paired` keeps its message byte for byte;
`report` does not know the flag."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r1.fq,r2.fq"]
AC = AL + ["--abundance", "a.tsv", "--calls", "c.tsv"]
NO_CALLS = "--callsPaired piles up the records of fragments in the file of --calls: it needs --calls\n"
NO_FRAGS = "--callsPaired is the rule for the records of fragments: it needs --paired or --interleaved\n"
TODAY = ("--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records outside the intersection have no "
         "weight rule\n")
RESCUED = "--abundanceRescued cannot be combined with %s yet: mates are rescued one by one, and a fragment's set has no rule for them\n"

CASES = [
    ("alone", AL + ["--callsPaired"], NO_CALLS),
    ("without_calls", AL + ["--abundance", "a.tsv", "--paired", "--callsPaired"], NO_CALLS),
    ("without_calls_interleaved", AL + ["--abundance", "a.tsv", "--interleaved", "--callsPaired"], NO_CALLS),
    ("without_fragments", AC + ["--callsPaired"], NO_FRAGS),
    ("without_fragments_with_support", AC + ["--bootstraps", "5", "--callSupport", "--callsPaired"], NO_FRAGS),
    # beside the rescued reads and assignment: the older checks answer, each with its reason
    ("abundance_rescued", AC + ["--paired", "--callsPaired", "--abundanceRescued", "--callsRescued"], RESCUED % "--paired"),
    ("abundance_rescued_interleaved", AC + ["--interleaved", "--callsPaired", "--abundanceRescued", "--callsRescued"], RESCUED % "--interleaved"),
    ("abundance_rescued_alone", AC + ["--paired", "--callsPaired", "--abundanceRescued"],
     "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("calls_rescued", AC + ["--paired", "--callsPaired", "--callsRescued"],
     "--callsRescued puts the reads --abundanceRescued adds to the classes into the pileup of --calls: it needs both --calls and --abundanceRescued\n"),
    ("assign_from", AC + ["--paired", "--callsPaired", "--assignFrom", "a0.tsv"],
     "--assignFrom cannot be combined with --abundance: it estimates from every ARG a read lies on, and an assigned read lies on one: run it as the first pass\n"),
    # older checks that stand in front
    ("calls_needs_abundance_first", AL + ["--calls", "c.tsv", "--paired", "--callsPaired"], "--calls has a line per line of the abundance file: it needs --abundance\n"),
    ("paired_and_interleaved_first", AC + ["--paired", "--interleaved", "--callsPaired"], "--paired and --interleaved contradict each other: the mates come in two files or in one\n"),
    ("odd_files_first", ["align", "-i", "idx", "-f", "r1.fq", "--abundance", "a.tsv", "--calls", "c.tsv", "--paired", "--callsPaired"],
     "--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): 1 file(s) given\n"),
    # without the switch: today's message, byte for byte
    ("today_paired", AC + ["--paired"], TODAY),
    ("today_interleaved", AC + ["--interleaved"], TODAY),
    ("today_with_support", AC + ["--paired", "--bootstraps", "5", "--callSupport"], TODAY),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in CASES])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("frags", ["--paired", "--interleaved"])
def test_the_switch_lifts_the_refusal(cli, tmp_path, frags):
    """--calls beside --paired / --interleaved and --callsPaired passes the plan, with the support columns and the curve too: the run then
    ends at its inputs, which do not exist"""
    r = subprocess.run([cli] + AC + [frags, "--callsPaired", "--bootstraps", "5", "--callSupport", "--rarefy", "r.tsv", "--noBam"], cwd=str(tmp_path), capture_output=True,
                       timeout=60)
    assert r.returncode == 1 and b"--callsPaired" not in r.stderr and b"weight rule" not in r.stderr and b"no file found at r1.fq" in r.stderr, r.stderr
    assert "c.tsv" not in os.listdir(str(tmp_path)) and "a.tsv" not in os.listdir(str(tmp_path))


def test_report_does_not_know_the_flag(cli, tmp_path):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--calls", "c.tsv", "--callsPaired"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and b"callsPaired" in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []
