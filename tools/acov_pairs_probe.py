"""tools/acov_pairs_probe.py (GPU) -- what the rule of assigned coverage over fragments (groot_hip_acov_pairs_*, the kPaired kernels of
kernels_acov.hpp) costs: the tail-stream kernels of one resident batch of fragments, in one of three modes per process, so that a
`rocprofv3 --kernel-trace --stats` run of it holds one mode's kernels alone:

    pairs         pairing + equivalence classes (what `align --paired --abundance` runs)
    calls_paired  assigned coverage over fragments (what `--calls --callsPaired` adds: ec_merge's serials, acov_serial_paired_kernel,
                  acov_count_kernel<false, true> and <true, true>)
    calls         assigned coverage of the same reads as unrelated reads (the unpaired `--calls`: acov_serial_kernel and the
                  kPaired = false instances; with GROOT_HIP_LIB set to an older library, that library's kernels)

and over two workloads of N fragments of arg-annot.90, 100-base mates, made on the host:

    mates   mate 1 at offset x of a path, mate 2 at x + d (20..400) of the same path on the other strand
    subset  every second fragment as above, the others with mate 2 from another path of the same graph at the same offsets: more fragments
            whose mates' sets intersect in a strict subset of both

Prints the wall-clock milliseconds of a resident batch and one batch's stats (fragments per class, records piled up and left out).  A
fourth mode, `describe`, times nothing: it reads one batch's traversal records back and prints the share of fragments joined on a strict
subset of both mates' sets.

    python tools/acov_pairs_probe.py --mode calls_paired --workload subset [--fragments 100000] [--steps 5] [--index groot.gidx] [--out FILE]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L = 100


def fragments(index, n, seed, cross):
    """the reads of n fragments, interleaved, as one uint8 array"""
    import numpy as np

    from groot_amd import synth

    cat, off, lens = synth.reference_sequences(index)
    gpo = index.arrays["graph_path_off"].astype(np.int64)
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGTN", b"TGCAN"):
        comp[a] = b
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(lens >= 3 * L)
    out = np.empty((2 * n, L), dtype=np.uint8)
    for i in range(n):
        p = int(rng.choice(ok))
        x = int(rng.integers(0, lens[p] - 2 * L))
        d = int(rng.integers(20, min(400, lens[p] - L - x) + 1))
        q = p
        if cross and i & 1:                 # another path of p's graph that is long enough, if there is one
            g = int(np.searchsorted(gpo, p, side="right")) - 1
            others = [c for c in range(int(gpo[g]), int(gpo[g + 1])) if c != p and lens[c] >= x + d + L]
            if others:
                q = int(rng.choice(others))
        out[2 * i] = cat[off[p] + x:off[p] + x + L]
        out[2 * i + 1] = comp[cat[off[q] + x + d:off[q] + x + d + L]][::-1]
    return out.reshape(-1)


def strict_share(trav, mask, n_frag):
    """the share of fragments whose mates' sets intersect in a strict subset of both, from the batch's traversal records"""
    sets = {}
    for r, g, m in zip(trav["read_id"].tolist(), trav["graph_id"].tolist(), mask.tolist()):
        s = sets.setdefault(r, {})
        s[g] = tuple(a | b for a, b in zip(s.get(g, (0,) * len(m)), m))
    k = 0
    for i in range(n_frag):
        a, b = sets.get(2 * i), sets.get(2 * i + 1)
        if not a or not b:
            continue
        u = {g: tuple(x & y for x, y in zip(a[g], b[g])) for g in a if g in b}
        u = {g: m for g, m in u.items() if any(m)}
        k += bool(u) and u != a and u != b
    return k / n_frag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["pairs", "calls_paired", "calls", "describe"], required=True)
    ap.add_argument("--workload", choices=["mates", "subset"], required=True)
    ap.add_argument("--fragments", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--index", default=None, help="a groot.gidx of arg-annot.90 (default: bench.py's cached one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from groot_amd import device, host

    if args.index:
        index = host.Index.load(args.index)
    else:
        import bench                        # (its index loader)

        index = bench.load_index()[0]
    dev = torch.device("cuda", 0)
    R = 2 * args.fragments
    seq = fragments(index, args.fragments, 7, args.workload == "subset")
    d_seq = torch.zeros(R * L + 64, dtype=torch.uint8, device=dev)
    d_seq[: R * L] = torch.from_numpy(seq).to(dev)
    d_off = torch.arange(0, R + 1, dtype=torch.int64, device=dev) * L
    torch.cuda.synchronize()
    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, results_on_device=args.mode != "describe", pipeline_depth=2,
                        memo_budget_mb=device.MEMO_OFF)
    al.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    if args.mode == "describe":
        al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
        al.wait()
        t, m = al.travs()
        line = f"{args.workload}: {args.fragments} fragments, {len(t)} traversal records, joined on a strict subset of both mates' sets: {strict_share(t, np.asarray(m), args.fragments):.3f}"
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        al.close()
        return
    if args.mode == "pairs":
        al.ec_enable()
        al.pairs_enable()
    elif args.mode == "calls_paired":
        al.acov_pairs_enable()
    else:
        al.acov_enable()
    ms = []
    for i in range(args.steps + 2):         # (two batches to warm up and to grow the tables: the fill is not what is compared)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
        counts = al.wait()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    line = f"{args.workload} {args.mode}: {args.fragments} fragments, batch wall-clock ms median {sorted(ms)[len(ms) // 2]:.2f} (min {min(ms):.2f}, max {max(ms):.2f}), mapped {counts['mapped']}"
    al.ec_reset()                           # one batch's stats
    al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
    al.wait()
    if args.mode != "calls":
        line += f", pairs {al.pairs_stats()}"
    if args.mode == "calls_paired":
        line += f", rule {al.acov_pairs_stats()}"
    if args.mode != "pairs":
        line += f", acov {al.acov_stats()}"
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    al.close()


if __name__ == "__main__":
    main()
