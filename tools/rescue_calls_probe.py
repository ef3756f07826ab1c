"""tools/rescue_calls_probe.py (GPU) -- what the rescued reads in assigned coverage (groot_hip_rescue_acov_*, kernels_rescue_acov.hpp) cost
on top of the rescued reads in the equivalence classes.

The resident rate (reads of arg-annot.90 in HBM, memo off, two batches in flight: bench.py's headline ctx) with mismatch rescue on, in three
settings, alternating, RUNS runs of each in one process:
    classes   equivalence classes + the rescued reads in them           (align --abundance --abundanceRescued: the rate to compare with)
    calls     equivalence classes + assigned coverage, no rescued reads (align --abundance --calls --variants)
    rescued   classes, assigned coverage and the rescued reads in both  (align --abundance --abundanceRescued --calls --callsRescued)
over the three inputs of tools/rescue_probe.py (configs2: error-free reads; sub1: every base replaced with probability 0.01; random:
uniformly random reads), and per input the stats of one batch into an empty table: the rescued records, the distinct tuples with and
without them (their difference is the growth of the table's fill that --callSlots has to hold), and `dropped`.

    python tools/rescue_calls_probe.py [--reads 10000000] [--runs 5] [--steps 5] [--mismatch 2] [--slots 67108864] [--only NAME] [--out FILE]
    rocprofv3 --kernel-trace --stats -- python tools/rescue_calls_probe.py --kernels-only [--only sub1] [--reads N] [--steps K]
--kernels-only: K passes with the feature on over one input and nothing else, for a kernel trace of its own.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (its index loader, resident loop and error model)

MODES = ("classes", "calls", "rescued")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mismatch", type=int, default=2)
    ap.add_argument("--slots", type=int, default=1 << 26)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
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
    al.ec_enable()
    al.rescue_enable(args.mismatch)

    def mode(m):
        """everything off that the setting does not have (assigned coverage off takes the rescued records and classes with it), then on"""
        al.acov_enable(False)
        al.rescue_ec_enable(False)
        al.ec_reset()
        if m == "classes":
            al.rescue_ec_enable()
        else:
            al.acov_enable()
        if m == "rescued":
            al.rescue_acov_enable(min_slots=args.slots)

    def one_batch(seq):
        al.rescue_reset()
        al.submit_device(seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
        al.wait()

    if args.kernels_only:
        name = args.only or "sub1"
        mode("rescued")
        for _ in range(args.steps):
            one_batch(inputs[name])
        say(f"# {args.steps} passes of {R} {name} reads with the feature on: {al.rescue_acov_stats()}")
        al.close()
        return

    say(f"# resident: {R} x {L} bp reads in HBM, memo off, 2 batches in flight, {args.steps} steps per run, rescue (M = {args.mismatch}) on, table of the rescued setting "
        f"started at {args.slots} slots; settings alternating")
    for name, seq in inputs.items():
        if args.only and name != args.only:
            continue
        rates = {m: [] for m in MODES}
        for i in range(args.runs):
            for m in MODES:
                mode(m)
                rate, _, counts = bench.resident_rate(al, seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
                rates[m].append(rate)
                say(f"{name} run {i} {m:8s}: {rate:8.1f} Mreads/s  (mapped/batch {counts['mapped']})")
        med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        say(f"{name}: median " + ", ".join(f"{m} {med[m]:.1f} (range {min(rates[m]):.1f} .. {max(rates[m]):.1f})" for m in MODES)
            + f" Mreads/s: rescued/classes = {med['rescued'] / med['classes']:.3f}, rescued/calls = {med['rescued'] / med['calls']:.3f}")
        mode("calls")                       # one batch into an empty table, without and with the rescued records
        one_batch(seq)
        plain = al.acov_stats()
        mode("rescued")
        one_batch(seq)
        st, full = al.rescue_acov_stats(), al.acov_stats()
        say(f"{name}: one batch: {st} rescue {al.rescue_stats()} rescued-in-ECs {al.rescue_ec_stats()} acov {full} acov without the rescued records {plain}")
        say(f"{name}: one batch: {st['records']} rescued record(s), {full['tuples'] - plain['tuples']} distinct tuple(s) more than the {plain['tuples']} of the exact records, "
            f"{st['dropped']} dropped")
    say(f"launches since open: {al.rescue_acov_stats()['launches']}")
    al.close()


if __name__ == "__main__":
    main()
