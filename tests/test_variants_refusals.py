"""What `groot-hip align` refuses of `--variants` and its flags before it does anything, in the manner of tests/test_cli_refusals.py: one
command line per refusal, run in a directory that holds nothing (but the abundance file --assignFrom must find), against names of an index
directory and a FASTQ file that do not exist.  The whole text of stdout and stderr and the exit status are pinned, and a refusal leaves
nothing behind: no log file, no output file, no graph directory.  The new checks come behind every earlier one (ORDER)."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
V = AL + ["--variants", "v.tsv"]
NEEDS = "--variantMinReads and --variantMinShare are the thresholds of --variants: they need it\n"

# (id, arguments, stderr); stdout is empty for every one of them
REFUSED = [
    ("noalign", V + ["--noAlign"], "--variants rescues the reads the exact alignments leave out: it cannot be combined with --noAlign\n"),
    ("assign", V + ["--assignFrom", "f.tsv"],
     "--variants cannot be combined with --assignFrom: assignment rewrites the records that tell which reads are unaligned\n"),
    ("rescue_without_variants", AL + ["--rescue", "2"], "--rescue is the number of substitutions --variants allows: it needs it\n"),
    ("min_reads_without_variants", AL + ["--variantMinReads", "3"], NEEDS),
    ("min_share_without_variants", AL + ["--report", "r.tsv", "--variantMinShare=0.2"], NEEDS),
    ("rescue_0", V + ["--rescue", "0"], "--rescue allows 1, 2 or 3 substitutions: 0\n"),
    ("rescue_4", V + ["--rescue", "4"], "--rescue allows 1, 2 or 3 substitutions: 4\n"),
    ("rescue_negative", V + ["--rescue=-1"], "--rescue allows 1, 2 or 3 substitutions: -1\n"),
    ("rescue_no_number", V + ["--rescue", "two"], "--rescue takes a number: two\n"),
    ("min_reads_negative", V + ["--variantMinReads=-2"], "--variantMinReads is a number of reads: -2\n"),
    ("min_share_range", V + ["--variantMinShare", "1.5"], "--variantMinShare is a share: 1.5 is not in [0, 1]\n"),
    ("min_share_no_number", V + ["--variantMinShare", "half"], "--variantMinShare takes a number: half\n"),
    ("flag_without_value", AL + ["--variants"], "flag needs an argument: --variants\n"),
    # --noBam keeps its rule: the variants file is no output of the alignments
    ("nobam_with_variants_alone", V + ["--noBam"], "--noBam without --report would leave no output of the alignments\n"),
]
# an earlier check answers first
ORDER = [
    ("report_noalign_before_variants", V + ["--report", "r.tsv", "--noAlign"], "--report needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("assign_paired_before_variants", V + ["--assignFrom", "f.tsv", "--paired"],
     "--assignFrom cannot be combined with --paired: fragments are not assigned yet: the mates would be assigned one by one\n"),
    ("paired_alone_before_rescue", AL + ["--paired", "--rescue", "2"], "--paired changes what --sharedReads and --abundance count, and nothing else: it needs one of them\n"),
    ("noalign_before_rescue_range", V + ["--noAlign", "--rescue", "9"], REFUSED[0][2]),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in REFUSED + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    (tmp_path / "f.tsv").write_bytes(b"")
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == ["f.tsv"]        # no groot.log, no groot-graphs-*, none of the named files
