"""tools/call_support_probe.py (GPU) -- what the per-replicate pileup of `--calls --callSupport` costs ("Bootstrap support").

The ECs and the assigned-coverage table of one resident configs[2] batch (10 M x 100 bp reads of arg-annot.90), B replicates from
groot_hip_em_bootstrap: groot_hip_call_support end to end (host clock around the call, it synchronises) against
groot_host_call_support on 16 threads, alternating, warm.  Both must return the same bits in every run.  The condition DESIGN states:
the device call's slowest run beats the host's fastest.

    python tools/call_support_probe.py [--reads 10000000] [--boot 100] [--runs 5] [--threads 16] [--out FILE]
    python tools/call_support_probe.py --kernels-only      (one device call, for rocprofv3 --kernel-trace --stats)

Uses the libraries as they are built (python -c 'import __graft_entry__ as g; g.build()' first).
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--boot", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--call-depth", type=float, default=1.0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
    lens = index.arrays["path_len"]
    cat, off, rlens = synth.reference_sequences(index)
    R, L, B = args.reads, bench.READ_LEN, args.boot
    seq, seq_off, _ = synth.reads_np(cat, off, rlens, R, L)
    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, memo_budget_mb=device.MEMO_OFF)
    al.acov_enable()
    al.submit(seq, seq_off)
    al.wait()
    e_off, e_ids, e_cnt, rows, tn = al.acov()
    al.close()
    pairs = np.unique(rows[:, :2], axis=0)
    per_path = np.bincount(pairs[:, 1], minlength=n_paths)
    alpha0, _ = host.em(n_paths, e_off, e_ids, e_cnt)
    sel = np.flatnonzero(alpha0 >= 1.0).astype(np.uint32)
    work = int(sum(int(lens[p]) for p in pairs[np.isin(pairs[:, 1], sel), 1]))
    say(f"# one batch of {R} x {L} bp reads: {len(e_cnt)} ECs, {len(e_ids)} listed IDs, {len(tn)} tuples of {int(tn.sum())} records, {len(pairs)} (EC, path) "
        f"with tuples (per path: mean {per_path.mean():.1f}, largest {int(per_path.max())}); {len(sel)} of {n_paths} paths with em_reads >= 1, "
        f"{int(lens[sel].sum())} bases, {work} multiply-adds per replicate")
    bc, alpha, _ = device.em_bootstrap(n_paths, e_off, e_ids, e_cnt, B)
    a = (n_paths, lens, e_off, e_ids, e_cnt, rows, tn, bc, alpha, sel)
    if args.kernels_only:
        cov = device.call_support(*a, call_depth=args.call_depth)
        say(f"kernels-only: {B} replicates, {device.call_support_info()}, covered bases {int(cov.sum())}")
        return
    device.call_support(n_paths, lens, e_off, e_ids, e_cnt, rows, tn, bc[:2], alpha[:2], sel, call_depth=args.call_depth)     # warm: the code object, the allocator
    info = device.call_support_info()
    td_, th_ = [], []
    for i in range(args.runs):
        t0 = time.perf_counter()
        d = device.call_support(*a, call_depth=args.call_depth)
        td_.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h = host.call_support(*a, call_depth=args.call_depth, threads=args.threads)
        th_.append(time.perf_counter() - t0)
        same = d.tobytes() == h.tobytes()
        say(f"run {i}: B = {B}: device {td_[-1]:7.3f} s   host on {args.threads} threads {th_[-1]:7.3f} s   identical bits: {same}")
        if not same:
            raise SystemExit("the device and the host disagree")
    called = (d.astype(np.float64) / np.maximum(lens[sel], 1)) >= 0.97
    say(f"rows {info['rows']} of u{8 * info['width']}, {info['chunks']} chunk(s) of paths; median device {sorted(td_)[len(td_) // 2]:.3f} s "
        f"(range {min(td_):.3f} .. {max(td_):.3f}), host {sorted(th_)[len(th_) // 2]:.3f} s (range {min(th_):.3f} .. {max(th_):.3f})")
    say(f"the device's slowest run beats the host's fastest: {max(td_) < min(th_)}")
    sup = called.sum(axis=0) / B
    say(f"support at callDepth {args.call_depth}, covCutoff 0.97: {int((sup == 0).sum())} paths at 0, {int((sup == 1).sum())} at 1, {int(((sup > 0) & (sup < 1)).sum())} between")


if __name__ == "__main__":
    main()
