"""tools/calls_rescued_pairs_probe.py (GPU) -- what the rescued mates in assigned coverage over fragments (groot_hip_rescue_acov_pairs_*,
kernels_rescue_acov_pairs.hpp) cost, against the two states they join.

The workload is tools/rescue_pairs_probe.py's: resident batches of mates of arg-annot.90 in HBM (memo off, two batches in flight), mate 2
`--insert` bases further along mate 1's reference sequence on the other strand, every base of both replaced with probability 0.01.
Alternating in one process, RUNS runs of each setting:
    rescued   pairing, the classes, rescue and the rescued mates' rule      (align --paired --abundance --abundanceRescued --rescuedPaired)
    paired    assigned coverage over fragments, rescue off                  (align --paired --abundance --calls --callsPaired)
    rule      the rule: both of the above and the pileup of the fragments with a rescued mate       (... --callsRescuedPaired)
The first two launch nothing this rule adds; with GROOT_HIP_LIB naming another build of the library (the parent commit's), `--settings
rescued,paired` measures them there.  Then one batch into an empty table under the rule: the record counts by kind and the growth of the
table's fill by that batch -- the largest a batch of this workload causes, since every later batch finds most of its tuples there.

    python tools/calls_rescued_pairs_probe.py [--reads 4000000] [--runs 5] [--steps 5] [--mismatch 2] [--insert 150] [--slots 67108864] [--out FILE]
    python tools/calls_rescued_pairs_probe.py --kernels-only rescued|paired|rule      (a few batches, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402  (its index loader, resident loop and error model)
from rescue_pairs_probe import mates  # noqa: E402

SETTINGS = ("rescued", "paired", "rule")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mismatch", type=int, default=2)
    ap.add_argument("--insert", type=int, default=150)
    ap.add_argument("--slots", type=int, default=1 << 26)
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--kernels-only", choices=SETTINGS, default=None)
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

    def setting(name):
        """from any of the three states to `name`, through everything off"""
        al.rescue_enable(0)                 # (the rescued classes, the rescued mates' rule and this rule go with it)
        al.acov_enable(False)
        al.pairs_enable(False)
        al.ec_enable(False)
        if name == "paired":
            al.acov_pairs_enable()
            return
        al.rescue_enable(args.mismatch)
        if name == "rescued":
            al.rescue_pairs_enable()
        else:
            al.rescue_acov_pairs_enable(min_slots=args.slots)

    if args.kernels_only:
        setting(args.kernels_only)
        bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, 3, 1)
        al.close()
        return
    names = [s for s in args.settings.split(",") if s in SETTINGS]
    say(f"# resident: {R // 2} fragments of 2 x {L} bp in HBM, mate 2 {args.insert} bases along on the other strand, 1 % substitutions, memo off, 2 batches in "
        f"flight, {args.steps} steps per run, M = {args.mismatch}; settings {', '.join(names)} alternating; library {os.environ.get('GROOT_HIP_LIB', 'this tree')}")
    rates = {n: [] for n in names}
    for i in range(args.runs):
        for n in names:
            setting(n)
            rate, _, counts = bench.resident_rate(al, d_seq.data_ptr(), d_off.data_ptr(), R, L, args.steps, 2)
            rates[n].append(rate)
            say(f"run {i} {n:8s}: {rate:8.2f} Mreads/s  (mapped/batch {counts['mapped']})")
    med = {n: sorted(v)[len(v) // 2] for n, v in rates.items()}
    for n in names:
        say(f"median {n:8s} {med[n]:8.2f} Mreads/s (range {min(rates[n]):.2f} .. {max(rates[n]):.2f})" +
            "".join(f", {n}/{b} = {med[n] / med[b]:.3f}" for b in names if n == "rule" and b != "rule"))
    if "rule" in names:                     # one batch into an empty table
        setting("rule")
        al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=L)
        al.wait()
        st, ast = al.rescue_acov_pairs_stats(), al.acov_stats()
        say(f"one batch, rule on: {st} acov {ast} acov_pairs {al.acov_pairs_stats()} rescue_pairs {al.rescue_pairs_stats()}")
        say(f"fill of the table after one batch from empty: {ast['tuples']} tuples in {ast['slots']} slots ({ast['grows']} growths), "
            f"{st['exact_records'] + st['rescued_records']} of {ast['records']} records piled up in one pass, dropped {st['dropped']}")
    al.close()


if __name__ == "__main__":
    main()
