"""tools/assign_probe.py (GPU) -- what assignment (groot_hip_assign_*, kernels_assign.hpp) costs on the device and what it
saves behind it.

1. The resident configs[2] rate (10 M x 100 bp reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline
   ctx), alternating in one process: assignment off; assignment on with alpha from the same reads' own EM (one batch with
   equivalence classes on, groot_host_em over them).  Per run the share of traversals emptied and of records kept.
2. `groot-hip align` wall time on a FASTQ of the same reads, alternating: (b) --bam x.bam; (a) --assignFrom a.tsv --bam y.bam, with
   a.tsv from one `align --abundance a.tsv --noBam` run first.  Per run the BAM records, the BAM bytes and the writer's busy time
   (--stats).

    python tools/assign_probe.py [--reads 10000000] [--runs 3] [--steps 6] [--cli-runs 3] [--no-cli] [--no-build] [--out FILE]
    python tools/assign_probe.py --kernels-only      (a few batches with assignment on, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--cli-reads", type=int, default=10_000_000)
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-build", action="store_true", help="use build/ as it is")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    from groot_amd import device, host, synth

    if not args.no_build:
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
    # alpha: the EM over the ECs of one batch of these reads
    al.ec_enable(True)
    al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
    al.wait()
    e_off, e_ids, e_cnt = al.ecs()
    al.ec_enable(False)
    alpha, iters = host.em(index.view.n_paths, e_off, e_ids, e_cnt)
    say(f"# alpha: EM of {iters} iteration(s) over {len(e_cnt)} equivalence class(es) of one batch; {int((alpha > 0).sum())} of {len(alpha)} paths above 0")
    if args.kernels_only:
        al.assign_enable(alpha, 0.0)
        rate, _, _ = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 2)
        say(f"kernels-only: 3 + 2 batches with assignment on, {rate:.1f} Mreads/s; {al.assign_stats()}")
        al.close()
        return
    say(f"# resident configs[2]: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run (+ 2 of warm-up); "
        "assignment off / on, alternating")
    modes = ("off", "assign")
    rates = {m: [] for m in modes}
    for i in range(args.runs):
        for m in modes:
            al.assign_enable(alpha if m == "assign" else None, 0.0)
            if m == "assign":
                al.assign_reset()
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[m].append(rate)
            st = al.assign_stats() if m == "assign" else None
            say(f"run {i} {m:6s}: {rate:8.1f} Mreads/s  (travs/batch {counts['travs']}, alignments/batch {counts['alignments']})"
                + (f"  reads with records {st['reads']}, assigned {st['assigned']} (ties {st['ties']}), unassigned {st['unassigned']}; records kept "
                   f"{st['records_kept']} of {st['records_in']} ({100.0 * st['records_kept'] / max(st['records_in'], 1):.2f} %), traversals emptied "
                   f"{st['travs_emptied']} of {st['travs_emptied'] + st['records_kept']} "
                   f"({100.0 * st['travs_emptied'] / max(st['travs_emptied'] + st['records_kept'], 1):.2f} %)" if st else ""))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    say(f"median assign: {med['assign']:.1f} Mreads/s ({min(rates['assign']):.1f} .. {max(rates['assign']):.1f}) vs off {med['off']:.1f} "
        f"({min(rates['off']):.1f} .. {max(rates['off']):.1f}): added {(R / med['assign'] - R / med['off']) / 1e3:.2f} ms per {R}-read batch")
    al.close()
    del d_seq
    torch.cuda.empty_cache()

    if args.no_cli:
        return
    n = args.cli_reads
    say(f"# CLI wall time: {n} x {L} bp reads as a plain FASTQ, --batch 262144, -p {bench.usable_cpus()}, alternating")
    seq_host = synth.reads_np(cat, off, lens, n, L)[0]
    exe = entry.build_cli() if not args.no_build else os.path.join(REPO, "build", "groot-hip")
    with tempfile.TemporaryDirectory(dir=os.environ.get("GROOT_BENCH_TMP")) as td:
        idx_dir = os.path.join(td, "index")
        os.makedirs(idx_dir)
        index.save(os.path.join(idx_dir, "groot.gidx"))
        fq = os.path.join(td, "reads.fq")
        bench.write_fastq(fq, seq_host, n)
        base = [exe, "align", "-i", idx_dir, "-f", fq, "-g", os.path.join(td, "g"), "-p", str(bench.usable_cpus()), "--batch", "262144"]

        def timed(cmd):
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t0
            if p.returncode:
                raise SystemExit(f"{cmd[1]} failed: {p.stderr.decode()[-400:]}")
            return dt

        a_tsv = os.path.join(td, "a.tsv")
        t1 = timed(base + ["--abundance", a_tsv, "--noBam", "--log", os.path.join(td, "one.log")])
        say(f"pass one (align --abundance --noBam): {t1:.2f} s, {open(a_tsv).read().count(chr(10))} lines")
        tb, ta = [], []
        for i in range(args.cli_runs):
            row = []
            for tag, extra, acc in (("b", [], tb), ("a", ["--assignFrom", a_tsv], ta)):
                stats, log = os.path.join(td, tag + ".json"), os.path.join(td, tag + ".log")
                acc.append(timed(base + extra + ["--bam", os.path.join(td, tag + ".bam"), "--stats", stats, "--log", log]))
                s = json.load(open(stats))
                kept = next((ln.split("record(s) in, ")[1].split(" kept")[0] for ln in open(log) if "record(s) in, " in ln), None)
                row.append(f"({tag}) {acc[-1]:6.2f} s, BAM records {kept if kept is not None else s['alignments']}, BAM bytes {s['bam_bytes']}, writer busy {s['bam_busy_s']:.2f} s")
            say(f"run {i}: align --bam " + row[0] + "   with --assignFrom " + row[1])
        mb, ma = sorted(tb)[len(tb) // 2], sorted(ta)[len(ta) // 2]
        say(f"median (b) {mb:.2f} s, (a) {ma:.2f} s: {ma - mb:+.2f} s ({(ma - mb) / mb * 100:+.1f} %); both passes {t1 + ma:.2f} s")


if __name__ == "__main__":
    main()
