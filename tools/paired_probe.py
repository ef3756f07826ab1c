"""tools/paired_probe.py (GPU) -- what counting fragments instead of mates costs (groot_hip_pairs_enable: shared_gather_paired_kernel
and the kPaired kernels of kernels_shared.hpp / kernels_ec.hpp).

The resident configs[2] rate (10 M x 100 bp reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline ctx) with
EC counting on, alternating in one process: pairing off; pairing on.  Both ways the batch is the same reads ordered as (r, r) pairs --
read 2i and read 2i+1 are copies of one read, so every fragment with records is joined and its intersection is the read's own set: the
paired gather then does all of its work (both mates scanned, every common segment ANDed) and the tables see half as many units.

    python tools/paired_probe.py [--reads 10000000] [--runs 3] [--steps 10] [--out FILE]
    python tools/paired_probe.py --kernels-only off|on      (a few batches, for rocprofv3 --kernel-trace --stats)
    GROOT_HIP_LIB=build/parent/libgroot_hip.so python tools/paired_probe.py --unpaired-only
                                                            (one rate with EC counting on and the pairing calls never made: any library)
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader and resident loop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernels-only", choices=("off", "on"), default=None)
    ap.add_argument("--unpaired-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    from groot_amd import device, synth

    if not os.path.exists(os.environ.get("GROOT_HIP_LIB") or os.path.join(REPO, "build", "libgroot_hip.so")):
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
    R, L = args.reads & ~1, bench.READ_LEN
    d_seq = torch.zeros(R * L + 64, dtype=torch.uint8, device=dev)
    for c0 in range(0, R // 2, 500_000):            # R / 2 distinct reads, each twice in a row
        n = min(500_000, R // 2 - c0)
        p, _, _ = synth.reads_torch(cat_t, off_t, lens_t, n, L, first=c0)
        d_seq[2 * c0 * L:2 * (c0 + n) * L] = p[: n * L].view(n, 1, L).expand(n, 2, L).reshape(-1)
    d_off = torch.arange(0, R + 1, dtype=torch.int64, device=dev) * L
    torch.cuda.synchronize()

    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, results_on_device=True, pipeline_depth=2,
                        memo_budget_mb=device.MEMO_OFF)
    al.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    if args.unpaired_only:
        al.ec_enable(True)
        rate, _, _ = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
        say(f"unpaired-only {os.environ.get('GROOT_HIP_LIB', 'product')}: {rate:.1f} Mreads/s with EC counting on; {al.ec_stats()}")
        al.close()
        return
    if args.kernels_only:
        al.ec_enable(True)
        al.pairs_enable(args.kernels_only == "on")
        rate, _, _ = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 2)
        say(f"kernels-only, pairing {args.kernels_only}: 3 batches with EC counting on, {rate:.1f} Mreads/s; {al.ec_stats()}")
        al.close()
        return
    say(f"# resident configs[2]: {R} x {L} bp reads in HBM ordered as (r, r) pairs, memo off, 2 batches in flight, {args.steps} steps per run; "
        "EC counting on, pairing off / on, alternating")
    modes = ("off", "on")
    rates = {m: [] for m in modes}
    for i in range(args.runs):
        for m in modes:
            al.ec_enable(True)                          # (an empty table: the stats below are this run's)
            al.pairs_enable(m == "on")
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[m].append(rate)
            st = al.ec_stats()
            say(f"run {i} pairing {m:3s}: {rate:8.1f} Mreads/s  (travs/batch {counts['travs']})  ECs {st['distinct']}, units per batch "
                f"{st['reads'] // (args.steps + 2)}, slow-path units {st['slow_reads']}, grows {st['grows']}"
                + (f"  {al.pairs_stats()}" if m == "on" else ""))
            al.pairs_enable(False)
            al.ec_enable(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    say(f"median pairing on: {med['on']:.1f} Mreads/s vs off {med['off']:.1f} (range of off: {min(rates['off']):.1f} .. {max(rates['off']):.1f}): "
        f"added {(R / med['on'] - R / med['off']) / 1e3:+.2f} ms per {R}-read batch")
    al.close()


if __name__ == "__main__":
    main()
