"""ICP time per frame from a rocprofv3 --kernel-trace CSV of a bench.py run: first half-iteration launch of a solve -> end
of its finish launch.

    python tools/icp_solve_profile.py <kernel_trace.csv>
"""
import csv, sys
rows = []
for r in csv.DictReader(open(sys.argv[1])):
    n = r["Kernel_Name"]
    if "gs_icp_" in n:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n))
rows.sort()
first, out = None, []
for s, e, n in rows:
    if first is None and "half_batch" in n:
        first = s
    if "finish" in n and first is not None:
        out.append((e - first) / 1e3)
        first = None
print("# frame: ICP us (first half-iteration launch -> end of the finish launch)")
for i, t in enumerate(out):
    print("%3d %8.1f" % (i + 1, t))
tt = out
print("# mean %.1f us over %d solves; mean of the last 20: %.1f" % (sum(tt) / len(tt), len(tt), sum(tt[-20:]) / len(tt[-20:])))
