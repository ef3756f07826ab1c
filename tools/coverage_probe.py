"""tools/coverage_probe.py (GPU) -- what report coverage on the device (groot_hip_coverage_*, kernels_cov.hpp) costs.

1. The resident configs[2] rate (10 M x 100 bp reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline
   ctx) with coverage off and on, alternating, RUNS runs of each in one process.
2. `groot-hip align` wall time on a FASTQ of the same reads: (a) --bam x.bam, then `report --bamFile x.bam`; (b) --report r.tsv --bam
   x.bam; (c) --report r.tsv --noBam.  The reports of (a), (b) and (c) must be byte-identical.

    python tools/coverage_probe.py [--reads 10000000] [--runs 5] [--steps 10] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader, resident loop and FASTQ writer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cli-reads", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    from groot_amd import device, synth

    entry.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                        # (as it goes: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    index, _ = bench.load_index()
    dev = torch.device("cuda", 0)
    cat, off, lens = synth.reference_sequences(index)
    cat_t, off_t, lens_t = (torch.from_numpy(x).to(dev) for x in (cat, off, lens))
    R, L = args.reads, bench.READ_LEN
    d_seq = torch.zeros(R * L + 64, dtype=torch.uint8, device=dev)
    for c0 in range(0, R, 1_000_000):
        n = min(1_000_000, R - c0)
        p, _, _ = synth.reads_torch(cat_t, off_t, lens_t, n, L, first=c0)
        d_seq[c0 * L:(c0 + n) * L] = p[: n * L]
    d_off = torch.arange(0, R + 1, dtype=torch.int64, device=dev) * L
    torch.cuda.synchronize()

    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, results_on_device=True, pipeline_depth=2,
                        memo_budget_mb=device.MEMO_OFF)
    al.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    say(f"# resident configs[2]: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run, coverage off/on alternating")
    rates = {False: [], True: []}
    for i in range(args.runs):
        for on in (False, True):
            al.coverage_enable(on)
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[on].append(rate)
            say(f"run {i} coverage {'on ' if on else 'off'}: {rate:8.1f} Mreads/s  (alignments/batch {counts['alignments']}, travs/batch {counts['travs']})")
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    say(f"median off {med[False]:.1f} Mreads/s, on {med[True]:.1f} Mreads/s: on/off = {med[True] / med[False]:.3f}")
    al.coverage_enable(False)
    al.close()
    del d_seq
    torch.cuda.empty_cache()

    n = args.cli_reads
    say(f"# CLI wall time: {n} x {L} bp reads as a plain FASTQ, --batch 262144, -p {bench.usable_cpus()}")
    seq_host = synth.reads_np(cat, off, lens, n, L)[0]
    exe = entry.build_cli()
    with tempfile.TemporaryDirectory(dir=os.environ.get("GROOT_BENCH_TMP")) as td:
        idx_dir = os.path.join(td, "index")
        os.makedirs(idx_dir)
        index.save(os.path.join(idx_dir, "groot.gidx"))
        fq = os.path.join(td, "reads.fq")
        bench.write_fastq(fq, seq_host, n)
        base = [exe, "align", "-i", idx_dir, "-f", fq, "-g", os.path.join(td, "g"), "--log", os.path.join(td, "a.log"), "-p", str(bench.usable_cpus()),
                "--batch", "262144"]
        bam = os.path.join(td, "x.bam")

        def timed(cmd, out=None):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=open(out, "wb") if out else subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t0
            if p.returncode:
                raise SystemExit(f"{cmd[1]} failed: {p.stderr.decode()[-400:]}")
            return dt

        ta = timed(base + ["--bam", bam])
        bam_bytes = os.path.getsize(bam)
        tr = timed([exe, "report", "--bamFile", bam, "--log", os.path.join(td, "r.log")], out=os.path.join(td, "a.tsv"))
        say(f"(a) align --bam:               {ta:7.2f} s  (BAM {bam_bytes / 1e9:.2f} GB)")
        say(f"    report --bamFile:          {tr:7.2f} s  -> (a) total {ta + tr:7.2f} s")
        os.unlink(bam)
        tb = timed(base + ["--bam", bam, "--report", os.path.join(td, "b.tsv")])
        say(f"(b) align --report --bam:      {tb:7.2f} s")
        os.unlink(bam)
        tc = timed(base + ["--report", os.path.join(td, "c.tsv"), "--noBam"])
        say(f"(c) align --report --noBam:    {tc:7.2f} s")
        a, b, c = (open(os.path.join(td, f), "rb").read() for f in ("a.tsv", "b.tsv", "c.tsv"))
        n_args = a.count(b"\n")
        say(f"reports identical: {a == b == c} ({n_args} ARGs)")


if __name__ == "__main__":
    main()
