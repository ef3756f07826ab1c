#!/bin/bash
# kernel timeline of one batch of a kernel_path_probe workload, per stream: start offset, duration, wait behind the previous kernel of the same queue (us)
#   tools/timeline_probe.sh WORKLOAD      (GPU box; rocprofv3 --kernel-trace)
set -u
W=${1:-c2_nomemo}
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
P=/tmp/tl_$W; rm -rf $P
rocprofv3 --kernel-trace --output-format csv -d $P -o t -- python tools/kernel_path_probe.py $W 4 > /dev/null 2>&1
python - "$P" <<'PY'
import csv, glob, sys
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
# the last align kernel but one starts the window shown: one whole batch period
al = [i for i, r in enumerate(rows) if "align_kernel" in r["Kernel_Name"]]
lo, hi = int(rows[al[-3]]["Start_Timestamp"]), int(rows[al[-2]]["Start_Timestamp"])
last_end = {}
for r in rows:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    q = r.get("Queue_Id", "?")
    if lo <= s < hi:
        name = r["Kernel_Name"].split("(")[0].replace("groot::", "").replace("void ", "")[:46]
        print("q%-3s +%8.1f us  dur %8.1f  behind-prev-on-queue %8.1f  %s" % (q, (s - lo) / 1e3, (e - s) / 1e3, (s - last_end.get(q, s)) / 1e3, name))
    last_end[q] = max(last_end.get(q, 0), e)
# the batch periods the trace holds (start to start of consecutive align kernels), the window shown last but one
print("# periods between align kernels (us):", " ".join("%.1f" % ((int(rows[b]["Start_Timestamp"]) - int(rows[a]["Start_Timestamp"])) / 1e3) for a, b in zip(al, al[1:])))
# end of the seed stage (last kernel on its queue before a first pass) -> start of that first pass
fp = [r for r in rows if "align_path_kernel" in r["Kernel_Name"] or "align_lean_kernel" in r["Kernel_Name"]]
seedq = next((r.get("Queue_Id") for r in rows if "assign_q_rows_kernel" in r["Kernel_Name"]), None)
gaps = []
for f in fp:
    s = int(f["Start_Timestamp"])
    before = [int(r["End_Timestamp"]) for r in rows if r.get("Queue_Id") == seedq and "fillBuffer" not in r["Kernel_Name"] and int(r["End_Timestamp"]) <= s]
    if before:
        gaps.append((s - max(before)) / 1e3)
print("# seed stage's last kernel -> first pass (us):", " ".join("%.1f" % g for g in gaps))
PY
