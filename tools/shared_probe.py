"""tools/shared_probe.py (GPU) -- what counting shared reads on the device (groot_hip_shared_*, kernels_shared.hpp) costs on top of
report coverage.

1. The resident configs[2] rate (10 M x 100 bp reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline
   ctx) with coverage alone and with coverage + shared reads, alternating, RUNS runs of each in one process.
2. `groot-hip align` wall time on a FASTQ of the same reads, alternating: (c) --report r.tsv --noBam; (d) --report r.tsv --sharedReads
   s.tsv --noBam.  Then `align --bam` + `report --bamFile --sharedReads`: its shared file must equal (d)'s byte for byte.

    python tools/shared_probe.py [--reads 10000000] [--runs 5] [--steps 10] [--cli-runs 3] [--out FILE]
    python tools/shared_probe.py --kernels-only      (a few batches with both on, for rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
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
    if args.kernels_only:
        al.coverage_enable(True)
        al.shared_enable(True)
        rate, _, _ = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 2)
        say(f"kernels-only: 3 batches with coverage + shared reads on, {rate:.1f} Mreads/s; {al.shared_stats()}")
        al.close()
        return
    say(f"# resident configs[2]: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run, coverage alone / "
        "coverage + shared reads alternating")
    rates = {False: [], True: []}
    al.coverage_enable(True)
    for i in range(args.runs):
        for on in (False, True):
            al.shared_enable(on)                       # (switched on: zeroed counters, so the stats below are this run's: warmup + steps batches)
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[on].append(rate)
            st = al.shared_stats() if on else None
            say(f"run {i} shared {'on ' if on else 'off'}: {rate:8.1f} Mreads/s  (alignments/batch {counts['alignments']}, travs/batch {counts['travs']})"
                + (f"  per batch: reads {st['reads'] // (args.steps + 2)}, distinct sets {st['distinct_sets'] // (args.steps + 2)}, "
                   f"slow-path reads {st['slow_reads'] // (args.steps + 2)}" if st else ""))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    say(f"median coverage alone {med[False]:.1f} Mreads/s, + shared {med[True]:.1f} Mreads/s: ratio {med[True] / med[False]:.3f}, "
        f"added {(R / med[True] - R / med[False]) / 1e3:.2f} ms per {R}-read batch")
    al.shared_enable(False)
    al.coverage_enable(False)
    al.close()
    del d_seq
    torch.cuda.empty_cache()

    n = args.cli_reads
    say(f"# CLI wall time: {n} x {L} bp reads as a plain FASTQ, --batch 262144, -p {bench.usable_cpus()}, alternating")
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

        tc, td_ = [], []
        for i in range(args.cli_runs):
            tc.append(timed(base + ["--report", os.path.join(td, "c.tsv"), "--noBam"]))
            td_.append(timed(base + ["--report", os.path.join(td, "d.tsv"), "--sharedReads", os.path.join(td, "d.shared"), "--noBam"]))
            say(f"run {i}: (c) align --report --noBam {tc[-1]:6.2f} s   (d) align --report --sharedReads --noBam {td_[-1]:6.2f} s")
        mc, md = sorted(tc)[len(tc) // 2], sorted(td_)[len(td_) // 2]
        say(f"median (c) {mc:.2f} s, (d) {md:.2f} s: added {md - mc:+.2f} s ({(md - mc) / mc * 100:+.1f} %; target within 10 %)")
        timed(base + ["--bam", bam])
        tr = timed([exe, "report", "--bamFile", bam, "--sharedReads", os.path.join(td, "a.shared"), "--log", os.path.join(td, "r.log")],
                   out=os.path.join(td, "a.tsv"))
        a, c, d = (open(os.path.join(td, f), "rb").read() for f in ("a.tsv", "c.tsv", "d.tsv"))
        sa, sd = (open(os.path.join(td, f), "rb").read() for f in ("a.shared", "d.shared"))
        n_args, n_lines = a.count(b"\n"), sd.count(b"\n")
        say(f"report --bamFile --sharedReads: {tr:.2f} s; reports identical: {a == c == d} ({n_args} ARGs); shared files identical: "
            f"{sa == sd} ({n_lines} lines)")


if __name__ == "__main__":
    main()
