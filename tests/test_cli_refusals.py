"""What `groot-hip align` (and `report`) refuse before they do anything: one command line per refusal, run in an empty directory against names
of an index directory and a FASTQ file that do not exist.  The whole text of stdout and stderr and the exit status are pinned, the first
failing check wins (ORDER trips two at once), and a refusal of `align` leaves nothing behind: no log file, no output file, no graph directory.
`report` checks most of its flags after it has opened its log, through the log's fatal path: the same text on stderr, and the log file exists."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


AL = ["align", "-i", "idx", "-f", "r.fq"]
ASSIGN = "--assignFrom cannot be combined with "
FRAGS = "fragments are not assigned yet: the mates would be assigned one by one\n"
COV = "supplied coverage cutoff exceeds 1.0 (100%): 1.5\n"
CALLS_PAIRED = ("--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records "
                "outside the intersection have no weight rule\n")

# (id, arguments, stderr); stdout is empty for every one of them
ALIGN = [
    ("fasta", AL + ["--fasta"], "--fasta is an experimental reference feature that is not supported\n"),
    ("report_noalign", AL + ["--report", "r.tsv", "--noAlign"], "--report needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("report_cutoff", AL + ["--report", "r.tsv", "--covCutoff", "1.5"], COV),
    ("shared_without_report", AL + ["--sharedReads", "s.tsv"], "--sharedReads lists pairs of reported ARGs: it needs --report\n"),
    ("abundance_noalign", AL + ["--abundance", "a.tsv", "--noAlign"], "--abundance needs the exact alignments: it cannot be combined with --noAlign\n"),
    ("bootstraps_without_abundance", AL + ["--bootstraps", "5"], "--bootstraps adds columns to the abundance file: it needs --abundance\n"),
    ("assign_rarefy", AL + ["--assignFrom", "f.tsv", "--rarefy", "c.tsv"],
     ASSIGN + "--rarefy: it redoes the estimate of --abundance on subsamples, and an assigned read lies on one ARG: run it with the first pass\n"),
    ("assign_shared", AL + ["--assignFrom", "f.tsv", "--report", "r.tsv", "--sharedReads", "s.tsv"],
     ASSIGN + "--sharedReads: it counts the reads two ARGs share, and an assigned read lies on one ARG\n"),
    ("assign_abundance", AL + ["--assignFrom", "f.tsv", "--abundance", "a.tsv"],
     ASSIGN + "--abundance: it estimates from every ARG a read lies on, and an assigned read lies on one: run it as the first pass\n"),
    ("assign_calls", AL + ["--assignFrom", "f.tsv", "--calls", "c.tsv"],
     ASSIGN + "--calls: it weighs every record of a read, and an assigned read keeps the records on one ARG\n"),
    ("assign_paired", AL + ["--assignFrom", "f.tsv", "--paired"], ASSIGN + "--paired: " + FRAGS),
    ("assign_interleaved", AL + ["--assignFrom", "f.tsv", "--interleaved"], ASSIGN + "--interleaved: " + FRAGS),
    ("assign_noalign", AL + ["--assignFrom", "f.tsv", "--noAlign"], ASSIGN + "--noAlign: assignment filters the exact alignments, which it leaves out\n"),
    ("assign_posterior_range", AL + ["--assignFrom", "f.tsv", "--minPosterior", "1.5"], "--minPosterior is a share: 1.5 is not in [0, 1]\n"),
    ("assign_posterior_negative", AL + ["--assignFrom", "f.tsv", "--minPosterior=-0.25"], "--minPosterior is a share: -0.25 is not in [0, 1]\n"),
    ("assign_no_file", AL + ["--assignFrom", "f.tsv"], "--assignFrom: no file found at f.tsv\n"),
    ("posterior_without_assign", AL + ["--minPosterior", "0.5"], "--minPosterior is the threshold of --assignFrom: it needs it\n"),
    ("posterior_no_number", AL + ["--minPosterior", "half"], "--minPosterior is a number in [0, 1]: half\n"),
    ("rarefy_without_abundance", AL + ["--rarefy", "c.tsv"], "--rarefy redoes the estimate of --abundance at every depth: it needs --abundance\n"),
    ("rarefy_no_steps", AL + ["--abundance", "a.tsv", "--rarefy", "c.tsv", "--rarefySteps", "0"], "--rarefySteps and --rarefyReps must be at least 1\n"),
    ("rarefy_no_reps", AL + ["--abundance", "a.tsv", "--rarefy", "c.tsv", "--rarefyReps", "0"], "--rarefySteps and --rarefyReps must be at least 1\n"),
    ("calls_without_abundance", AL + ["--calls", "c.tsv"], "--calls has a line per line of the abundance file: it needs --abundance\n"),
    ("calls_paired", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--paired"], CALLS_PAIRED),
    ("calls_interleaved", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--interleaved"], CALLS_PAIRED),
    ("support_without_calls", AL + ["--callSupport"], "--callSupport adds columns to the calls file: it needs --calls\n"),
    ("support_without_bootstraps", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--callSupport"],
     "--callSupport is computed from the bootstrap replicates: it needs --bootstraps\n"),
    ("calls_cutoff", AL + ["--abundance", "a.tsv", "--calls", "c.tsv", "--covCutoff", "1.5"], COV),
    ("nobam_alone", AL + ["--noBam"], "--noBam without --report would leave no output of the alignments\n"),
    ("nobam_and_bam", AL + ["--noBam", "--report", "r.tsv", "--bam", "o.bam"], "--noBam and --bam contradict each other\n"),
    ("paired_and_interleaved", AL + ["--abundance", "a.tsv", "--paired", "--interleaved"],
     "--paired and --interleaved contradict each other: the mates come in two files or in one\n"),
    ("paired_alone", AL + ["--paired"], "--paired changes what --sharedReads and --abundance count, and nothing else: it needs one of them\n"),
    ("interleaved_alone", AL + ["--interleaved"], "--interleaved changes what --sharedReads and --abundance count, and nothing else: it needs one of them\n"),
    ("paired_one_file", AL + ["--abundance", "a.tsv", "--paired"], "--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): 1 file(s) given\n"),
    ("paired_three_files", ["align", "-i", "idx", "-f", "a.fq,b.fq,c.fq", "--abundance", "a.tsv", "--paired"],
     "--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): 3 file(s) given\n"),
    ("paired_stdin", ["align", "-i", "idx", "--abundance", "a.tsv", "--paired"], "--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): 0 file(s) given\n"),
    ("flag_without_value", AL + ["--report"], "flag needs an argument: --report\n"),
]
# (`--calls` with `--noAlign` has a line of its own, but --calls needs --abundance, which --noAlign has refused before: no command line reaches it)

# two refusals at once: the earlier check answers
ORDER = [
    ("index_before_fasta", ["align", "-f", "r.fq", "--fasta"], None),
    ("fasta_before_report", AL + ["--fasta", "--report", "r.tsv", "--noAlign"], ALIGN[0][2]),
    ("report_noalign_before_cutoff", AL + ["--report", "r.tsv", "--noAlign", "--covCutoff", "1.5"], ALIGN[1][2]),
    ("shared_before_bootstraps", AL + ["--bootstraps", "5", "--sharedReads", "s.tsv"], ALIGN[3][2]),
    ("abundance_noalign_before_assign", AL + ["--assignFrom", "f.tsv", "--noAlign", "--abundance", "a.tsv"], ALIGN[4][2]),
    ("assign_rarefy_before_abundance", AL + ["--assignFrom", "f.tsv", "--abundance", "a.tsv", "--rarefy", "c.tsv"], ALIGN[6][2]),
    ("assign_calls_before_paired", AL + ["--assignFrom", "f.tsv", "--noAlign", "--paired", "--calls", "c.tsv"], ALIGN[9][2]),
    ("assign_paired_before_posterior", AL + ["--assignFrom", "f.tsv", "--minPosterior", "1.5", "--interleaved", "--paired"], ALIGN[10][2]),
    ("posterior_before_rarefy", AL + ["--rarefy", "c.tsv", "--minPosterior", "0.5"], ALIGN[16][2]),
    ("rarefy_before_calls", AL + ["--calls", "c.tsv", "--rarefy", "c.tsv"], ALIGN[18][2]),
    ("calls_before_support", AL + ["--calls", "c.tsv", "--callSupport"], ALIGN[21][2]),
    ("support_before_nobam", AL + ["--noBam", "--callSupport"], ALIGN[24][2]),
    ("nobam_before_pairs", AL + ["--noBam", "--bam", "o.bam", "--abundance", "a.tsv", "--paired", "--interleaved"], ALIGN[28][2]),
    ("contradiction_before_count", ["align", "-i", "idx", "--abundance", "a.tsv", "--paired", "--interleaved"], ALIGN[29][2]),
]


@pytest.mark.parametrize("args,err", [pytest.param(a, e, id=i) for i, a, e in ALIGN + ORDER])
def test_align_refuses_and_touches_nothing(cli, tmp_path, args, err):
    r = subprocess.run([cli] + args, cwd=str(tmp_path), capture_output=True, timeout=60)
    assert r.returncode == 1
    if err is None:      # cmd/align.go:56-60 prints this one, and only this one, on stdout
        assert (r.stdout, r.stderr) == (b"please specify a directory with the index files (--indexDir)\n", b"")
    else:
        assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert os.listdir(str(tmp_path)) == []          # no groot.log, no groot-graphs-*, none of the named files


RP = ["report", "--bamFile", "x.bam"]
# (id, arguments, stderr, the log file exists afterwards); x.bam does not exist, x.txt does
REPORT = [
    ("paired", RP + ["--paired"], "report cannot pair the records of a BAM: it carries no mate flags, and mates with equal QNAMEs cannot be told apart -- use "
                                  "`align --paired` (or --interleaved) with --sharedReads / --abundance\n", False),
    ("interleaved_before_support", RP + ["--interleaved", "--callSupport"],
     "report cannot pair the records of a BAM: it carries no mate flags, and mates with equal QNAMEs cannot be told apart -- use "
     "`align --paired` (or --interleaved) with --sharedReads / --abundance\n", False),
    ("support_without_calls", RP + ["--callSupport"], "--callSupport adds columns to the calls file: it needs --calls\n", True),
    ("support_without_bootstraps", RP + ["--abundance", "a.tsv", "--calls", "c.tsv", "--callSupport"],
     "--callSupport is computed from the bootstrap replicates: it needs --bootstraps\n", True),
    ("rarefy_without_abundance", RP + ["--rarefy", "c.tsv"], "--rarefy redoes the estimate of --abundance at every depth: it needs --abundance\n", True),
    ("rarefy_no_steps", RP + ["--abundance", "a.tsv", "--rarefy", "c.tsv", "--rarefySteps", "0"], "--rarefySteps and --rarefyReps must be at least 1\n", True),
    ("no_bam_file", RP, "BAM file does not exist: x.bam\n", True),
    ("rarefy_before_bam_file", RP + ["--rarefy", "c.tsv", "--bootstraps", "5"],
     "--rarefy redoes the estimate of --abundance at every depth: it needs --abundance\n", True),
    ("extension", ["report", "--bamFile", "x.txt"], "the BAM file does not have a `.bam` extension: x.txt\n", True),
    ("cutoff", ["report", "-c", "1.5"], COV, True),
    ("bam_file_before_cutoff", RP + ["-c", "1.5"], "BAM file does not exist: x.bam\n", True),
    ("bootstraps_without_abundance", ["report", "--bootstraps", "5"], "--bootstraps adds columns to the abundance file: it needs --abundance\n", True),
    ("calls_without_abundance", ["report", "--calls", "c.tsv"], "--calls has a line per line of the abundance file: it needs --abundance\n", True),
    ("bootstraps_before_calls", ["report", "--calls", "c.tsv", "--bootstraps", "5"], "--bootstraps adds columns to the abundance file: it needs --abundance\n", True),
]


@pytest.mark.parametrize("args,err,logs", [pytest.param(a, e, l, id=i) for i, a, e, l in REPORT])
def test_report_refuses_before_it_reads_a_bam(cli, tmp_path, args, err, logs):
    (tmp_path / "x.txt").write_bytes(b"")
    r = subprocess.run([cli] + args, cwd=str(tmp_path), stdin=subprocess.DEVNULL, capture_output=True, timeout=60)
    assert r.returncode == 1
    assert (r.stdout, r.stderr.decode()) == (b"", err)
    assert sorted(os.listdir(str(tmp_path))) == (["groot.log", "x.txt"] if logs else ["x.txt"])
    if logs:             # the refusal went through the log: its last line is the message behind Go's timestamp
        assert open(str(tmp_path / "groot.log")).read().splitlines()[-1].split(" ", 2)[2] == err[:-1]
