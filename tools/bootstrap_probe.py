"""tools/bootstrap_probe.py (GPU) -- what the bootstrap replicates of `--abundance --bootstraps B` cost.

1. The ECs of one configs[2] batch (10 M x 100 bp reads of arg-annot.90): groot_hip_em_bootstrap end to end (host clock around the
   call, it synchronises) against groot_host_em_bootstrap on 16 threads, alternating, warm, with what the EM kernel's time depends
   on: the ECs per path and the replicates' iteration counts.  Both must return the same bits.
2. `groot-hip align --abundance a.tsv --noBam` with and without `--bootstraps B` on a FASTQ of the same reads, alternating; the first
   four columns of the file with must be the file without.  --parent-cli <groot-hip of the parent commit> adds that build's run
   without --bootstraps to the rotation and compares its bytes.

    python tools/bootstrap_probe.py [--reads 10000000] [--boot 100] [--runs 5] [--cli-runs 3] [--parent-cli PATH] [--out FILE]
    python tools/bootstrap_probe.py --kernels-only      (one device call, for rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--boot", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--parent-cli", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
    n_paths = index.view.n_paths
    cat, off, lens = synth.reference_sequences(index)
    R, L, B = args.reads, bench.READ_LEN, args.boot
    seq, seq_off, _ = synth.reads_np(cat, off, lens, R, L)
    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, memo_budget_mb=device.MEMO_OFF)
    al.ec_enable()
    al.submit(seq, seq_off)
    al.wait()
    e_off, e_ids, e_cnt = al.ecs()
    al.close()
    per_path = np.bincount(e_ids, minlength=n_paths)
    say(f"# ECs of one batch of {R} x {L} bp reads: {len(e_cnt)} ECs over {n_paths} paths, {int(e_cnt.sum())} reads, {len(e_ids)} listed IDs "
        f"({len(e_ids) / max(len(e_cnt), 1):.1f} per EC, largest EC {int(np.diff(e_off).max())}); ECs per path: mean {per_path.mean():.1f}, largest {int(per_path.max())}")
    if args.kernels_only:
        _, _, its = device.em_bootstrap(n_paths, e_off, e_ids, e_cnt, B)
        say(f"kernels-only: {B} replicates, iterations {int(its.min())} / {int(np.median(its))} / {int(its.max())}")
        return
    device.em_bootstrap(n_paths, e_off, e_ids, e_cnt, 2)                # warm: the code object, the allocator
    td_, th_ = [], []
    for i in range(args.runs):
        t0 = time.perf_counter()
        d = device.em_bootstrap(n_paths, e_off, e_ids, e_cnt, B)
        td_.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h = host.em_bootstrap(n_paths, e_off, e_ids, e_cnt, B, threads=args.threads)
        th_.append(time.perf_counter() - t0)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(d, h))
        say(f"run {i}: B = {B}: device {td_[-1]:7.3f} s   host on {args.threads} threads {th_[-1]:7.3f} s   identical bits: {same}")
        if not same:
            raise SystemExit("the device and the host disagree")
    its = d[2]
    say(f"median device {sorted(td_)[len(td_) // 2]:.3f} s (range {min(td_):.3f} .. {max(td_):.3f}), host {sorted(th_)[len(th_) // 2]:.3f} s "
        f"(range {min(th_):.3f} .. {max(th_):.3f}); iterations of the replicates: smallest {int(its.min())}, median {int(np.median(its))}, largest {int(its.max())}")
    t0 = time.perf_counter()
    device.em_bootstrap(n_paths, e_off, e_ids, e_cnt, 1, min_iter=1, max_iter=1)
    say(f"one replicate of one EM iteration (the draws of one replicate, the uploads, the allocations): {time.perf_counter() - t0:.3f} s")

    if not args.cli_runs:
        return
    say(f"# CLI wall time: {R} x {L} bp reads as a plain FASTQ, --batch 262144, -p {bench.usable_cpus()}, alternating")
    exe = entry.build_cli()
    with tempfile.TemporaryDirectory(dir=os.environ.get("GROOT_BENCH_TMP")) as td:
        idx_dir = os.path.join(td, "index")
        os.makedirs(idx_dir)
        index.save(os.path.join(idx_dir, "groot.gidx"))
        fq = os.path.join(td, "reads.fq")
        bench.write_fastq(fq, seq, R)

        def timed(cli, tag, extra):
            log = os.path.join(td, tag + ".log")
            cmd = [cli, "align", "-i", idx_dir, "-f", fq, "-g", os.path.join(td, "g"), "-p", str(bench.usable_cpus()), "--batch", "262144",
                   "--abundance", os.path.join(td, tag + ".tsv"), "--noBam", "--log", log] + extra
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t0
            if p.returncode:
                raise SystemExit(f"{tag} failed: {p.stderr.decode()[-400:]}")
            return dt, open(log).read()

        modes = [("without", exe, []), ("with", exe, ["--bootstraps", str(B)])] + ([("parent", args.parent_cli, [])] if args.parent_cli else [])
        t = {m[0]: [] for m in modes}
        for i in range(args.cli_runs):
            row = []
            for tag, cli, extra in modes:
                dt, log = timed(cli, tag, extra)
                t[tag].append(dt)
                m = re.search(r"bootstrap: .*", log)
                row.append(f"{tag} {dt:6.2f} s" + (f" [{m.group(0).strip()}]" if m else ""))
            say(f"run {i}: " + "   ".join(row))
        for tag in t:
            say(f"{tag}: median {sorted(t[tag])[len(t[tag]) // 2]:.2f} s (range {min(t[tag]):.2f} .. {max(t[tag]):.2f})")
        without, with_ = (open(os.path.join(td, f + ".tsv"), "rb").read() for f in ("without", "with"))
        first4 = b"".join(b"\t".join(ln.split(b"\t")[:4]) + b"\n" for ln in with_.splitlines())
        say(f"the first four columns with --bootstraps are the file without: {first4 == without} ({without.count(10)} lines)")
        if args.parent_cli:
            say(f"the file without --bootstraps is the parent's: {open(os.path.join(td, 'parent.tsv'), 'rb').read() == without}")


if __name__ == "__main__":
    main()
