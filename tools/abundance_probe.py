"""tools/abundance_probe.py (GPU) -- what counting equivalence classes on the device (groot_hip_ec_*, kernels_ec.hpp) costs, and what
the EM over them costs.

1. The resident configs[2] rate (10 M x 100 bp reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline
   ctx), alternating in one process: EC counting off; on; on + coverage + shared reads.
2. `groot-hip align` wall time on a FASTQ of the same reads, alternating: (c) --report r.tsv --noBam; (e) --abundance a.tsv --noBam,
   with the EM's own time from the log.  Then `align --bam` + `report --bamFile --abundance`: its file must equal (e)'s byte for byte.

    python tools/abundance_probe.py [--reads 10000000] [--runs 5] [--steps 10] [--cli-runs 3] [--out FILE]
    python tools/abundance_probe.py --kernels-only      (a few batches with EC counting on, for rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
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
        al.ec_enable(True)
        rate, _, _ = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 2)
        say(f"kernels-only: 3 batches with EC counting on, {rate:.1f} Mreads/s; {al.ec_stats()}")
        al.close()
        return
    say(f"# resident configs[2]: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run; EC counting off / on / "
        "on + coverage + shared reads, alternating")
    modes = ("off", "ec", "ec+cov+shared")
    rates = {m: [] for m in modes}
    for i in range(args.runs):
        for m in modes:
            al.ec_enable(m != "off")                   # (switched on: an empty table, so the stats below are this run's)
            al.coverage_enable(m == "ec+cov+shared")
            al.shared_enable(m == "ec+cov+shared")
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[m].append(rate)
            st = al.ec_stats() if m != "off" else None
            say(f"run {i} {m:14s}: {rate:8.1f} Mreads/s  (travs/batch {counts['travs']})"
                + (f"  ECs {st['distinct']}, reads per batch {st['reads'] // (args.steps + 2)}, slow-path reads {st['slow_reads']}, grows {st['grows']}"
                   if st else ""))
            al.ec_enable(False)
            al.coverage_enable(False)
            al.shared_enable(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    for m in modes[1:]:
        say(f"median {m}: {med[m]:.1f} Mreads/s vs off {med['off']:.1f}: added {(R / med[m] - R / med['off']) / 1e3:.2f} ms per {R}-read batch")
    # the EM of these ECs
    al.ec_enable(True)
    bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 1, 0)
    e_off, e_ids, e_cnt = al.ecs()
    t0 = time.perf_counter()
    _, it = host.em(index.view.n_paths, e_off, e_ids, e_cnt)
    say(f"EM over {len(e_cnt)} ECs of one batch: {it} iterations, {time.perf_counter() - t0:.4f} s (host.em, target < 0.1 s)")
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
        base = [exe, "align", "-i", idx_dir, "-f", fq, "-g", os.path.join(td, "g"), "-p", str(bench.usable_cpus()), "--batch", "262144"]
        bam = os.path.join(td, "x.bam")

        def timed(cmd, out=None):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=open(out, "wb") if out else subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t0
            if p.returncode:
                raise SystemExit(f"{cmd[1]} failed: {p.stderr.decode()[-400:]}")
            return dt

        tc, te = [], []
        for i in range(args.cli_runs):
            tc.append(timed(base + ["--report", os.path.join(td, "c.tsv"), "--noBam", "--log", os.path.join(td, "c.log")]))
            elog = os.path.join(td, "e.log")
            te.append(timed(base + ["--abundance", os.path.join(td, "e.tsv"), "--noBam", "--log", elog]))
            m = re.search(r"abundance: (\d+) equivalence class\(es\), EM of (\d+) iteration\(s\) in ([0-9.]+) s", open(elog).read())
            say(f"run {i}: (c) align --report --noBam {tc[-1]:6.2f} s   (e) align --abundance --noBam {te[-1]:6.2f} s"
                + (f"  [{m.group(1)} ECs, EM {m.group(2)} iterations, {m.group(3)} s]" if m else ""))
        mc, me = sorted(tc)[len(tc) // 2], sorted(te)[len(te) // 2]
        say(f"median (c) {mc:.2f} s, (e) {me:.2f} s: {me - mc:+.2f} s ({(me - mc) / mc * 100:+.1f} %)")
        timed(base + ["--bam", bam, "--log", os.path.join(td, "b.log")])
        tr = timed([exe, "report", "--bamFile", bam, "--abundance", os.path.join(td, "r.tsv"), "--log", os.path.join(td, "r.log")])
        a, e = (open(os.path.join(td, f), "rb").read() for f in ("r.tsv", "e.tsv"))
        n_lines = e.count(b"\n")
        say(f"report --bamFile --abundance: {tr:.2f} s; abundance files identical: {a == e} ({n_lines} lines)")


if __name__ == "__main__":
    main()
