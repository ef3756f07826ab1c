"""tools/gap_records_probe.py (GPU) -- what the gapped records on the device (groot_hip_gap_rec_*, kernels_gap_rec.hpp) cost on top of
gapped rescue.

The resident rate (reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline ctx) with gapped rescue alone and
with gapped rescue plus the records, alternating, RUNS runs of each in one process, over the three inputs of tools/rescued_bam_probe.py:
  configs2   error-free reads: nearly every read has a record, almost none is a gap candidate -- the price of the scan alone
  sub1       every base replaced with probability 0.01: the reads mismatch rescue leaves are gap candidates, few are gap-rescued
  random     uniformly random reads: nearly every read long enough is a gap candidate and almost no anchor hits
and the stats of one batch of each: records, gap-rescued reads, bytes copied out at collect.  The emit kernel walks sweep 2 once more,
and only for the gap candidates with an e*: the expectation is about one sweep of rescue_gap_kernel for those few reads.

    python tools/gap_records_probe.py [--reads 2000000] [--runs 5] [--steps 5] [--mismatch 2] [--gap 3] [--per-read 4] [--out FILE]

Per-kernel times: one run of its own under `rocprofv3 --kernel-trace --stats -- python tools/gap_records_probe.py --runs 1`.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader, resident loop and error model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mismatch", type=int, default=2)
    ap.add_argument("--gap", type=int, default=3)
    ap.add_argument("--per-read", type=int, default=4, help="slots_per_batch = this many records per read of the batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from groot_amd import device, synth

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
    g = torch.Generator(device=dev)
    g.manual_seed(0x67726F6F74)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    inputs = {"configs2": d_seq, "sub1": bench.substituted(d_seq, R, 0.01, g)}
    rnd = torch.zeros_like(d_seq)
    for c0 in range(0, R * L, 100_000_000):
        n = min(100_000_000, R * L - c0)
        rnd[c0:c0 + n] = acgt[torch.randint(0, 4, (n,), generator=g, device=dev)]
    inputs["random"] = rnd
    torch.cuda.synchronize()

    slots = args.per_read * R
    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, results_on_device=True, pipeline_depth=2,
                        memo_budget_mb=device.MEMO_OFF)
    al.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    al.rescue_enable(args.mismatch)
    al.gap_enable(args.gap)
    say(f"# resident: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run, gapped rescue (M = {args.mismatch}, G = {args.gap}) "
        f"alone / with records ({slots} slots per batch: {24 * slots / 2**20:.0f} MiB of HBM per pipeline slot) alternating")
    for name, seq in inputs.items():
        rates = {False: [], True: []}
        for i in range(args.runs):
            for on in (False, True):
                al.gap_rec_enable(slots if on else 0)
                rate, _, counts = bench.resident_rate(al, seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
                rates[on].append(rate)
                say(f"{name} run {i} records {'on ' if on else 'off'}: {rate:8.1f} Mreads/s  (mapped/batch {counts['mapped']})")
        med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        say(f"{name}: median gapped rescue alone {med[False]:.1f} (range {min(rates[False]):.1f} .. {max(rates[False]):.1f}), with records {med[True]:.1f} "
            f"(range {min(rates[True]):.1f} .. {max(rates[True]):.1f}) Mreads/s: with/alone = {med[True] / med[False]:.3f}")
        al.gap_rec_enable(0)                # the stats of one batch: from zero
        al.gap_rec_enable(slots)
        al.gap_reset()
        al.submit_device(seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
        al.wait()
        st, gs = al.gap_rec_stats(), al.gap_stats()
        say(f"{name}: one batch: {st}; gap candidates {gs['candidates']}, gap-rescued {gs['rescued']}: {st['records'] / max(st['reads'], 1):.1f} records per gap-rescued read, "
            f"{24 * st['records'] / 2**20:.3f} MiB copied out at collect")
        al.gap_rec_enable(0)
    say(f"launches since open: {al.gap_rec_stats()['launches']}")
    al.close()


if __name__ == "__main__":
    main()
