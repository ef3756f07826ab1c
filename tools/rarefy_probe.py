"""tools/rarefy_probe.py (GPU) -- what the rarefaction curve of `--abundance --rarefy` costs.

1. The ECs of one configs[2] batch (10 M x 100 bp reads of arg-annot.90): groot_hip_em_rarefy end to end (host clock around the call,
   it synchronises) against groot_host_em_rarefy on 16 threads at the depths of --rarefySteps D, alternating, warm, median of the runs.
   Both must return the same bits.
2. `groot-hip align --abundance a.tsv --noBam` with and without `--rarefy r.tsv` on a FASTQ of the same reads, alternating; the
   abundance file with must be the file without.

The libraries and the binary are used as built (python __graft_entry__.py builds them).

    python tools/rarefy_probe.py [--reads 10000000] [--reps 20] [--steps 10] [--runs 5] [--cli-runs 3] [--out FILE]
    python tools/rarefy_probe.py --kernels-only      (one device call, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader and FASTQ writer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry
    from groot_amd import device, host, synth

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                        # (as it goes: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    index, _ = bench.load_index()
    n_paths = index.view.n_paths
    cat, off, lens = synth.reference_sequences(index)
    N, L, R, D = args.reads, bench.READ_LEN, args.reps, args.steps
    seq, seq_off, _ = synth.reads_np(cat, off, lens, N, L)
    al = device.Aligner(index, max_batch_reads=N, max_read_len=256, memo_budget_mb=device.MEMO_OFF)
    al.ec_enable()
    al.submit(seq, seq_off)
    al.wait()
    e_off, e_ids, e_cnt = al.ecs()
    al.close()
    units = int(e_cnt.sum())
    depths = host.rarefy_depths(units, D)[:-1]
    depths = depths[depths > 0]
    say(f"# ECs of one batch of {N} x {L} bp reads: {len(e_cnt)} ECs over {n_paths} paths, {units} units, {len(e_ids)} listed IDs; "
        f"R = {R} replicates at the {len(depths)} drawn depths of D = {D}: {int(depths.sum()) * R} draws, {R * len(depths)} EMs")
    if args.kernels_only:
        _, _, its = device.em_rarefy(n_paths, e_off, e_ids, e_cnt, R, depths)
        say(f"kernels-only: iterations {int(its.min())} / {int(np.median(its))} / {int(its.max())}")
        return
    device.em_rarefy(n_paths, e_off, e_ids, e_cnt, 2, depths[:2])      # warm: the code object, the allocator
    td_, th_ = [], []
    for i in range(args.runs):
        t0 = time.perf_counter()
        d = device.em_rarefy(n_paths, e_off, e_ids, e_cnt, R, depths)
        td_.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h = host.em_rarefy(n_paths, e_off, e_ids, e_cnt, R, depths, threads=args.threads)
        th_.append(time.perf_counter() - t0)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(d, h))
        say(f"run {i}: device {td_[-1]:7.3f} s   host on {args.threads} threads {th_[-1]:7.3f} s   identical bits: {same}")
        if not same:
            raise SystemExit("the device and the host disagree")
    its = d[2]
    say(f"median device {sorted(td_)[len(td_) // 2]:.3f} s (range {min(td_):.3f} .. {max(td_):.3f}), host {sorted(th_)[len(th_) // 2]:.3f} s "
        f"(range {min(th_):.3f} .. {max(th_):.3f}); iterations of the EMs: smallest {int(its.min())}, median {int(np.median(its))}, largest {int(its.max())}")

    if not args.cli_runs:
        return
    say(f"# CLI wall time: {N} x {L} bp reads as a plain FASTQ, --batch 262144, -p {bench.usable_cpus()}, alternating")
    exe = entry.build_cli()
    with tempfile.TemporaryDirectory(dir=os.environ.get("GROOT_BENCH_TMP")) as td:
        idx_dir = os.path.join(td, "index")
        os.makedirs(idx_dir)
        index.save(os.path.join(idx_dir, "groot.gidx"))
        fq = os.path.join(td, "reads.fq")
        bench.write_fastq(fq, seq, N)

        def timed(tag, extra):
            log = os.path.join(td, tag + ".log")
            cmd = [exe, "align", "-i", idx_dir, "-f", fq, "-g", os.path.join(td, "g"), "-p", str(bench.usable_cpus()), "--batch", "262144",
                   "--abundance", os.path.join(td, tag + ".tsv"), "--noBam", "--log", log] + extra
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t0
            if p.returncode:
                raise SystemExit(f"{tag} failed: {p.stderr.decode()[-400:]}")
            return dt, open(log).read()

        modes = [("without", []), ("with", ["--rarefy", os.path.join(td, "r.tsv"), "--rarefyReps", str(R), "--rarefySteps", str(D)])]
        t = {m[0]: [] for m in modes}
        for i in range(args.cli_runs):
            row = []
            for tag, extra in modes:
                dt, log = timed(tag, extra)
                t[tag].append(dt)
                m = re.search(r"rarefaction: .*", log)
                row.append(f"{tag} {dt:6.2f} s" + (f" [{m.group(0).strip()}]" if m else ""))
            say(f"run {i}: " + "   ".join(row))
        for tag in t:
            say(f"{tag}: median {sorted(t[tag])[len(t[tag]) // 2]:.2f} s (range {min(t[tag]):.2f} .. {max(t[tag]):.2f})")
        without, with_ = (open(os.path.join(td, f + ".tsv"), "rb").read() for f in ("without", "with"))
        say(f"the abundance file with --rarefy is the file without: {with_ == without} ({without.count(10)} lines)")
        say("# the rarefaction file")
        for ln in open(os.path.join(td, "r.tsv")).read().splitlines():
            say(ln)


if __name__ == "__main__":
    main()
