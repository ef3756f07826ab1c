"""What `groot-hip align` refuses of `--abundanceRescued` before it does anything, in the manner of tests/test_variants_refusals.py: one
command line per refusal, run in a directory that holds nothing, against names of an index directory and a FASTQ file that do not exist.
The whole text of stdout and stderr and the exit status are pinned, and a refusal leaves nothing behind.  The new checks come behind every
earlier one (ORDER), and `report` does not know the flag."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
R = AL + ["--abundance", "a.tsv", "--abundanceRescued"]
FRAGS = "--abundanceRescued cannot be combined with %s yet: mates are rescued one by one, and a fragment's set has no rule for them\n"

# (id, arguments, stderr); stdout is empty for every one of them
REFUSED = [
    ("without_abundance", AL + ["--abundanceRescued"], "--abundanceRescued adds the rescued reads to the classes --abundance estimates from: it needs --abundance\n"),
    ("without_abundance_with_rescue", AL + ["--abundanceRescued", "--rescue", "2"],
     "--abundanceRescued adds the rescued reads to the classes --abundance estimates from: it needs --abundance\n"),
    ("calls", R + ["--calls", "c.tsv"], "--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none\n"),
    ("paired", R + ["-f", "r2.fq", "--paired"], FRAGS % "--paired"),
    ("interleaved", R + ["--interleaved"], FRAGS % "--interleaved"),
]
# an earlier check answers first, and the flags of --variants keep their rules beside it
ORDER = [
    ("abundance_noalign_first", R + ["--noAlign"], "--abundance needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("assign_first", R + ["--assignFrom", "f.tsv"],
     "--assignFrom cannot be combined with --abundance: it estimates from every ARG a read lies on, and an assigned read lies on one: run it as the first pass\n"),
    ("rescue_range_first", R + ["--calls", "c.tsv", "--rescue", "4"], "--rescue allows 1, 2 or 3 substitutions: 4\n"),
    ("variant_thresholds_still_need_variants", R + ["--variantMinReads", "3"], "--variantMinReads and --variantMinShare are the thresholds of --variants: they need it\n"),
    ("paired_file_count_first", R + ["--paired"], "--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): 1 file(s) given\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in REFUSED + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    (tmp_path / "f.tsv").write_bytes(b"")
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == ["f.tsv"]        # no groot.log, no groot-graphs-*, none of the named files


def test_report_does_not_know_the_flag(cli, tmp_path):
    r = subprocess.run([cli, "report", "--bamFile", "x.bam", "--abundance", "a.tsv", "--abundanceRescued"], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode != 0 and b"abundanceRescued" in r.stderr + r.stdout
    assert os.listdir(str(tmp_path)) == []
