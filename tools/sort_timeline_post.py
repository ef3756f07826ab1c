#!/usr/bin/env python3
"""Timeline of a traced kernel_path_probe run in the layout of profiles/r11_timeline.txt, plus what round 12 asks per batch:
`python tools/sort_timeline_post.py TRACE_DIR [passes]` after `rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o t -- python
tools/kernel_path_probe.py c2_nomemo 12`.

Per batch of the processing-order sort (the run of radix_sort_onesweep kernels on the seed stream; its last `passes` kernels, default 3, are the
onesweep iterations): the sort's span (first histogram start -> last iteration end), the end of its first iteration relative to the end of the
first pass (align_path_kernel) that was running when the sort started, the walk stream's gap between two first passes, and the period."""
import csv
import glob
import sys


def short(name):
    n = name.replace("void ", "").replace("groot::", "")
    if "radix_sort_onesweep" in n:
        return "radix_sort_onesweep"
    for k in ("partition", "lookback_scan", "init_lookback"):
        if k in n:
            return k
    return n.split("<")[0].split("(")[0][:46]


def main():
    d = sys.argv[1]
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if len(files) != 1:
        sys.exit("%s: %d kernel_trace.csv files, expected exactly one" % (d, len(files)))
    rows = list(csv.DictReader(open(files[0])))
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r.get("Stream_Id", "?"), short(r["Kernel_Name"])) for r in rows))
    fp = [k for k in ks if k[4] in ("align_path_kernel", "align_lean_kernel")]
    if len(fp) < 5:
        print("# fewer than five first passes in the trace")
        return
    t0, t1 = fp[-5][0], fp[-2][0] + 1_500_000
    ms = lambda t: (t - t0) / 1e6
    for s, e, q, st, n in ks:
        if t0 <= s < t1 and e - s >= 20_000:
            print("%9.3f %9.3f %7.3f q%s s%s %s" % (ms(s), ms(e), (e - s) / 1e6, q, st, n))
    # sorts: runs of onesweep kernels with less than 0.5 ms between one's end and the next one's start
    groups, cur = [], []
    for k in ks:
        if k[4] != "radix_sort_onesweep":
            continue
        if cur and k[0] - cur[-1][1] > 500_000:
            groups.append(cur)
            cur = []
        cur.append(k)
    if cur:
        groups.append(cur)
    print("# per batch (ms): the sort's span; end of its first iteration minus end of the first pass running at the sort's start; its iterations")
    for g in groups:
        if g[0][0] < t0 or g[0][0] >= t1 or len(g) < passes + 1:
            continue
        it = g[-passes:]
        beside = [p for p in fp if p[0] <= g[0][0] < p[1]]
        rel = "%7.3f" % ((it[0][1] - beside[0][1]) / 1e6) if beside else "  alone"
        print("#   sort at %7.3f: span %6.3f   first iteration end vs first pass end %s   iterations %s" % (
            ms(g[0][0]), (g[-1][1] - g[0][0]) / 1e6, rel, " ".join("%.3f" % ((e - s) / 1e6) for s, e, *_ in it)))
    print("# per batch (ms): the walk stream's gap between two first passes (end -> next start), and the period (start -> next start)")
    for a, b in zip(fp[-5:-1], fp[-4:]):
        print("#   first pass at %7.3f: dur %6.3f   gap %6.3f   period %6.3f" % (ms(a[0]), (a[1] - a[0]) / 1e6, (b[0] - a[1]) / 1e6, (b[0] - a[0]) / 1e6))


if __name__ == "__main__":
    main()
