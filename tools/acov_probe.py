"""tools/acov_probe.py (GPU) -- what the assigned-coverage table on the device (groot_hip_acov_*, kernels_acov.hpp) costs beside
equivalence-class counting, which it needs.

1. The resident configs[2] rate (10 M x 100 bp reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline
   ctx), alternating in one process: EC counting on; EC counting + assigned coverage.  Per run the distinct tuples, the records, the
   table's slots and the times it grew.
2. `groot-hip align` wall time on a FASTQ of the same reads, alternating: (e) --abundance a.tsv --noBam; (k) the same with --calls
   c.tsv.  Then `align --bam` + `report --bamFile --abundance --calls`: its file must equal (k)'s byte for byte.

    python tools/acov_probe.py [--reads 10000000] [--runs 3] [--steps 6] [--cli-runs 3] [--no-cli] [--out FILE]
    python tools/acov_probe.py --kernels-only      (a few batches with assigned coverage on, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import re
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--cli-reads", type=int, default=10_000_000)
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    from groot_amd import device, host, synth

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
        al.acov_enable(True)
        rate, _, _ = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 2)
        say(f"kernels-only: 3 + 2 batches with assigned coverage on, {rate:.1f} Mreads/s; {al.acov_stats()}")
        al.close()
        return
    say(f"# resident configs[2]: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run (+ 2 of warm-up, counted too); "
        "EC counting / EC counting + assigned coverage, alternating")
    modes = ("ec", "ec+acov")
    rates = {m: [] for m in modes}
    for i in range(args.runs):
        for m in modes:
            al.ec_enable(True)                         # (switched on: empty tables, so the stats below are this run's)
            al.acov_enable(m == "ec+acov")
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[m].append(rate)
            st = al.acov_stats() if m == "ec+acov" else None
            say(f"run {i} {m:8s}: {rate:8.1f} Mreads/s  (travs/batch {counts['travs']})"
                + (f"  distinct tuples {st['tuples']}, records {st['records']} ({st['records'] // (args.steps + 2)} per batch), slots {st['slots']}, "
                   f"grows {st['grows']}, records grouped on the host {st['slow_records']}" if st else ""))
            al.ec_enable(False)                        # (assigned coverage goes with it)
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    say(f"median ec+acov: {med['ec+acov']:.1f} Mreads/s ({min(rates['ec+acov']):.1f} .. {max(rates['ec+acov']):.1f}) vs ec {med['ec']:.1f} "
        f"({min(rates['ec']):.1f} .. {max(rates['ec']):.1f}): added {(R / med['ec+acov'] - R / med['ec']) / 1e3:.2f} ms per {R}-read batch")
    al.close()
    del d_seq
    torch.cuda.empty_cache()

    if args.no_cli:
        return
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
        base = [exe, "align", "-i", idx_dir, "-f", fq, "-g", os.path.join(td, "g"), "-p", str(bench.usable_cpus()), "--batch", "262144"]
        bam = os.path.join(td, "x.bam")

        def timed(cmd, out=None):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=open(out, "wb") if out else subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t0
            if p.returncode:
                raise SystemExit(f"{cmd[1]} failed: {p.stderr.decode()[-400:]}")
            return dt

        te, tk = [], []
        for i in range(args.cli_runs):
            te.append(timed(base + ["--abundance", os.path.join(td, "e.tsv"), "--noBam", "--log", os.path.join(td, "e.log")]))
            klog = os.path.join(td, "k.log")
            tk.append(timed(base + ["--abundance", os.path.join(td, "k.tsv"), "--calls", os.path.join(td, "kc.tsv"), "--noBam", "--log", klog]))
            m = re.search(r"calls: (\d+) tuple\(s\).*?(\d+) line\(s\), (\d+) called.*?in ([0-9.]+) s", open(klog).read())
            say(f"run {i}: (e) align --abundance --noBam {te[-1]:6.2f} s   (k) with --calls {tk[-1]:6.2f} s"
                + (f"  [{m.group(1)} tuples, {m.group(2)} lines, {m.group(3)} called, merge + file {m.group(4)} s]" if m else ""))
        me, mk = sorted(te)[len(te) // 2], sorted(tk)[len(tk) // 2]
        say(f"median (e) {me:.2f} s, (k) {mk:.2f} s: {mk - me:+.2f} s ({(mk - me) / me * 100:+.1f} %)")
        same_ab = open(os.path.join(td, "e.tsv"), "rb").read() == open(os.path.join(td, "k.tsv"), "rb").read()
        say(f"abundance file with and without --calls identical: {same_ab}")
        timed(base + ["--bam", bam, "--log", os.path.join(td, "b.log")])
        tr = timed([exe, "report", "--bamFile", bam, "--abundance", os.path.join(td, "r.tsv"), "--calls", os.path.join(td, "rc.tsv"), "--log", os.path.join(td, "r.log")])
        a, k = (open(os.path.join(td, f), "rb").read() for f in ("rc.tsv", "kc.tsv"))
        n_lines = k.count(b"\n")
        say(f"report --bamFile --abundance --calls: {tr:.2f} s; calls files identical: {a == k} ({n_lines} lines)")


if __name__ == "__main__":
    main()
