"""What `groot-hip align` refuses of `--indels` and its flags before it does anything, in the manner of tests/test_variants_refusals.py: one
command line per refusal, run in a directory that holds nothing (but the abundance file --assignFrom must find), against names of an index
directory and a FASTQ file that do not exist.  The whole text of stdout and stderr and the exit status are pinned, and a refusal leaves
nothing behind: no log file, no output file, no graph directory.  The new checks come behind every earlier one (ORDER); --rescue and
--variantMin* are accepted with --indels alone, and keep their own refusals there."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
I = AL + ["--indels", "i.tsv"]
NEEDS = "--rescueGap and --gapEventSlots are the gap length and the table size of --indels: they need it\n"

# (id, arguments, stderr); stdout is empty for every one of them
REFUSED = [
    ("noalign", I + ["--noAlign"], "--indels rescues the reads the exact alignments leave out: it cannot be combined with --noAlign\n"),
    ("assign", I + ["--assignFrom", "f.tsv"],
     "--indels cannot be combined with --assignFrom: assignment rewrites the records that tell which reads are unaligned\n"),
    ("gap_without_indels", AL + ["--rescueGap", "2"], NEEDS),
    ("gap_with_variants_alone", AL + ["--variants", "v.tsv", "--rescueGap", "2"], NEEDS),
    ("slots_without_indels", AL + ["--report", "r.tsv", "--gapEventSlots=1024"], NEEDS),
    ("gap_0", I + ["--rescueGap", "0"], "--rescueGap allows a gap of 1 to 8 bases: 0\n"),
    ("gap_9", I + ["--rescueGap", "9"], "--rescueGap allows a gap of 1 to 8 bases: 9\n"),
    ("gap_negative", I + ["--rescueGap=-1"], "--rescueGap allows a gap of 1 to 8 bases: -1\n"),
    ("gap_no_number", I + ["--rescueGap", "three"], "--rescueGap takes a number: three\n"),
    ("slots_no_power_of_two", I + ["--gapEventSlots", "1000"], "--gapEventSlots is a number of table slots, a power of two: 1000\n"),
    ("slots_0", I + ["--gapEventSlots", "0"], "--gapEventSlots is a number of table slots, a power of two: 0\n"),
    ("slots_negative", I + ["--gapEventSlots=-8"], "--gapEventSlots is a number of table slots, a power of two: -8\n"),
    ("slots_no_number", I + ["--gapEventSlots", "many"], "--gapEventSlots takes a number: many\n"),
    ("flag_without_value", AL + ["--indels"], "flag needs an argument: --indels\n"),
    # the thresholds and M of --variants are those of --indels too: their refusals, byte for byte
    ("rescue_4_with_indels", I + ["--rescue", "4"], "--rescue allows 1, 2 or 3 substitutions: 4\n"),
    ("min_reads_negative_with_indels", I + ["--variantMinReads=-2"], "--variantMinReads is a number of reads: -2\n"),
    ("min_share_range_with_indels", I + ["--variantMinShare", "1.5"], "--variantMinShare is a share: 1.5 is not in [0, 1]\n"),
    # --noBam keeps its rule: the indels file is no output of the alignments
    ("nobam_with_indels_alone", I + ["--noBam"], "--noBam without --report would leave no output of the alignments\n"),
]
# an earlier check answers first
ORDER = [
    ("report_noalign_before_indels", I + ["--report", "r.tsv", "--noAlign"], "--report needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("variants_noalign_before_indels", I + ["--variants", "v.tsv", "--noAlign"],
     "--variants rescues the reads the exact alignments leave out: it cannot be combined with --noAlign\n"),
    ("assign_paired_before_indels", I + ["--assignFrom", "f.tsv", "--paired"],
     "--assignFrom cannot be combined with --paired: fragments are not assigned yet: the mates would be assigned one by one\n"),
    ("rescue_range_before_indels_noalign", I + ["--noAlign", "--rescue", "9"], "--rescue allows 1, 2 or 3 substitutions: 9\n"),
    ("noalign_before_gap_range", I + ["--noAlign", "--rescueGap", "9"], REFUSED[0][2]),
    ("gap_range_before_slots", I + ["--rescueGap", "9", "--gapEventSlots", "7"], "--rescueGap allows a gap of 1 to 8 bases: 9\n"),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in REFUSED + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    (tmp_path / "f.tsv").write_bytes(b"")
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == ["f.tsv"]        # no groot.log, no groot-graphs-*, none of the named files
