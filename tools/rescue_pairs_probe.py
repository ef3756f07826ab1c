"""tools/rescue_pairs_probe.py (GPU) -- what rescued mates in paired-end units (groot_hip_rescue_pairs_*, kernels_rescue_pairs.hpp) cost
on top of pairing, the classes and mismatch rescue.

Resident batches of mates of arg-annot.90 in HBM (memo off, two batches in flight: bench.py's headline ctx): mate 1 is a read of
bench.py's generator, mate 2 the READ_LEN bases that start `--insert` bases further along the same reference sequence (pulled back to
its end where it would hang over), on the other strand; then every base of both is replaced with probability 0.01.  Alternating in one
process, RUNS runs of each: pairing, equivalence classes and rescue on and the rule off (what `align --paired --abundance --variants` runs:
the baseline, not the headline); the same with the rule on.  Then the stats of one batch: the share of fragments by kind and the units that
took a bitmap.

    python tools/rescue_pairs_probe.py [--reads 4000000] [--runs 5] [--steps 5] [--mismatch 2] [--insert 150] [--out FILE]
    python tools/rescue_pairs_probe.py --kernels-only off|on      (a few batches, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader, resident loop and error model)


def mates(cat_t, off_t, lens_t, n_frag, L, insert, comp):
    """-> uint8 [2 n_frag * L + 64]: mate 1 of fragment i at read 2i, mate 2 at read 2i + 1"""
    import torch

    from groot_amd import synth

    dev = cat_t.device
    out = torch.zeros(2 * n_frag * L + 64, dtype=torch.uint8, device=dev)
    rows = out[: 2 * n_frag * L].view(n_frag, 2, L)
    within = torch.arange(L, dtype=torch.int64, device=dev).unsqueeze(0)
    for c0 in range(0, n_frag, 1_000_000):
        n = min(1_000_000, n_frag - c0)
        p, _, truth = synth.reads_torch(cat_t, off_t, lens_t, n, L, first=c0)
        rows[c0:c0 + n, 0] = p[: n * L].view(n, L)
        start2 = torch.minimum(truth["start"] + insert, lens_t[truth["seq"]] - L)
        other = 1 - truth["strand"]
        pos = torch.where(other.unsqueeze(1) == 0, within, L - 1 - within)
        b = cat_t[((off_t[truth["seq"]] + start2).unsqueeze(1) + pos).reshape(-1)].view(n, L)
        rows[c0:c0 + n, 1] = torch.where(other.unsqueeze(1) == 1, comp[b.long()], b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mismatch", type=int, default=2)
    ap.add_argument("--insert", type=int, default=150)
    ap.add_argument("--kernels-only", choices=("off", "on"), default=None)
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
    R, L = args.reads & ~1, bench.READ_LEN
    g = torch.Generator(device=dev)
    g.manual_seed(0x67726F6F74)
    clean = mates(cat_t, off_t.long(), lens_t.long(), R // 2, L, args.insert, torch.from_numpy(synth._COMP).to(dev))
    d_seq = bench.substituted(clean, R, 0.01, g)
    del clean
    d_off = torch.arange(0, R + 1, dtype=torch.int64, device=dev) * L
    torch.cuda.synchronize()

    al = device.Aligner(index, max_batch_reads=R, max_read_len=256, max_batch_bases=R * L + 64, results_on_device=True, pipeline_depth=2,
                        memo_budget_mb=device.MEMO_OFF)
    al.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    al.ec_enable()
    al.pairs_enable()
    al.rescue_enable(args.mismatch)

    def rule(on):
        al.rescue_pairs_enable(on)          # (off: the rule and the rescued classes go, pairing and the classes stay)

    if args.kernels_only:
        rule(args.kernels_only == "on")
        bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 1)
        al.close()
        return
    say(f"# resident: {R // 2} fragments of 2 x {L} bp in HBM, mate 2 {args.insert} bases along on the other strand, 1 % substitutions, memo off, 2 batches in "
        f"flight, {args.steps} steps per run; pairing, ECs and rescue (M = {args.mismatch}) on, the rule off/on alternating")
    rates = {False: [], True: []}
    for i in range(args.runs):
        for on in (False, True):
            rule(on)
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[on].append(rate)
            say(f"run {i} rule {'on ' if on else 'off'}: {rate:8.2f} Mreads/s  (mapped/batch {counts['mapped']})")
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    say(f"median off {med[False]:.2f} (range {min(rates[False]):.2f} .. {max(rates[False]):.2f}), on {med[True]:.2f} "
        f"(range {min(rates[True]):.2f} .. {max(rates[True]):.2f}) Mreads/s: on/off = {med[True] / med[False]:.3f}")
    for on in (False, True):                # the stats of one batch, the rule off and on
        rule(on)
        al.ec_reset()
        al.rescue_reset()
        al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
        al.wait()
        say(f"one batch, rule {'on' if on else 'off'}: pairs {al.pairs_stats()} ec {al.ec_stats()} rescue {al.rescue_stats()}")
        if on:
            st = al.rescue_pairs_stats()
            say(f"one batch, rule on: {st} rescue_ec {al.rescue_ec_stats()}")
            frag = R // 2
            say("share of the batch's fragments: " + ", ".join(f"{k} {100.0 * st[k] / frag:.2f} %" for k in list(st)[:6]) +
                f"; units that took a bitmap: {st['bitmap_units']}")
    al.close()


if __name__ == "__main__":
    main()
