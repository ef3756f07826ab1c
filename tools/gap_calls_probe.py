"""tools/gap_calls_probe.py (GPU) -- what the gap-placed reads in assigned coverage (groot_hip_gap_acov_*, kernels_gap_acov.hpp) cost on
top of gapped rescue and the rescued reads in assigned coverage: tools/gap_ec_probe.py's twin.

The resident rate (reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline ctx) with assigned coverage, rescue,
gapped rescue and the rescued reads in assigned coverage on (what `align --abundance --abundanceRescued --calls --callsRescued --indels`
runs: the nearest thing without the feature, the gap reads piled up nowhere), the feature off and on, alternating, RUNS runs of each in one
process, over the three inputs of tools/rescue_probe.py (configs2: error-free reads; sub1: every base replaced with probability 0.01;
random: uniformly random reads), and per input the stats of one batch: the gapped placements and records piled up, the table's tuples
before and behind the batch.  The rate to compare with is the feature off, not the headline.

    python tools/gap_calls_probe.py [--reads 2000000] [--runs 5] [--steps 5] [--mismatch 2] [--gap 3] [--slots 16777216] [--only NAME] [--out FILE]
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
    ap.add_argument("--slots", type=int, default=1 << 24)
    ap.add_argument("--only", default=None)
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

    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, results_on_device=True, pipeline_depth=2,
                        memo_budget_mb=device.MEMO_OFF)
    al.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    al.acov_enable()
    al.rescue_enable(args.mismatch)
    al.gap_enable(args.gap)
    al.rescue_acov_enable(min_slots=args.slots)
    say(f"# resident: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run, ECs, rescue (M = {args.mismatch}), gapped rescue "
        f"(G = {args.gap}) and the rescued reads in assigned coverage on (table of {args.slots} slots at the start), gap-placed reads in assigned coverage off/on alternating")
    for name, seq in inputs.items():
        if args.only and name != args.only:
            continue
        rates = {False: [], True: []}
        for i in range(args.runs):
            for on in (False, True):
                al.gap_acov_enable(on)
                al.ec_reset()               # (the table starts empty in every run: its fill is not what is compared)
                rate, _, counts = bench.resident_rate(al, seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
                rates[on].append(rate)
                say(f"{name} run {i} gap-placed-in-calls {'on ' if on else 'off'}: {rate:8.1f} Mreads/s  (mapped/batch {counts['mapped']})")
        med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        say(f"{name}: median off {med[False]:.1f} (range {min(rates[False]):.1f} .. {max(rates[False]):.1f}), on {med[True]:.1f} "
            f"(range {min(rates[True]):.1f} .. {max(rates[True]):.1f}) Mreads/s: on/off = {med[True] / med[False]:.3f}")
        for on in (False, True):            # the stats of one batch, without the feature and with it
            al.gap_acov_enable(on)
            al.ec_reset()
            al.rescue_reset()
            al.gap_reset()
            al.submit_device(seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
            al.wait()
            say(f"{name}: one batch, feature {'on' if on else 'off'}: gap_acov {al.gap_acov_stats()} acov {al.acov_stats()} rescue_acov {al.rescue_acov_stats()} "
                f"gap_ec {al.gap_ec_stats()} gap {al.gap_stats()}")
        al.gap_acov_enable(False)
        al.ec_reset()
    say(f"launches since open: {al.gap_acov_stats()['launches']}")
    al.close()


if __name__ == "__main__":
    main()
