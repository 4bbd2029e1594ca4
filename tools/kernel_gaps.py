"""Kernel durations and the idle gaps between consecutive kernels from a rocprofv3 --kernel-trace directory (csv):
where does the part of a bench step go that is not the fused kernel?
    python tools/kernel_gaps.py <trace_dir> [out.json]"""
import csv, glob, json, sys
from collections import defaultdict

d = sys.argv[1]
rows = [r for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f))]


def short(n):
    if n.startswith("void "): n = n[5:]
    return n.split("(")[0]


ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows)
dur, gap = defaultdict(list), defaultdict(list)
for i, (s, e, n) in enumerate(ks):
    dur[n].append(e - s)
    if i: gap[(ks[i - 1][2], n)].append(s - ks[i - 1][1])
med = lambda v: sorted(v)[len(v) // 2] / 1e3
res = {"durations_us": {}, "gaps_us": {}}
print("kernel durations (us): launches, median, min")
for n, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
    if len(v) < 5: continue
    print(f"  {n:60s} {len(v):6d} {med(v):9.2f} {min(v) / 1e3:9.2f}")
    res["durations_us"][n] = {"launches": len(v), "median": med(v), "min": min(v) / 1e3}
print("gaps end -> next start (us): pairs, median, min")
for (a, b), v in sorted(gap.items(), key=lambda kv: -len(kv[1])):
    if len(v) < 5: continue
    print(f"  {a:44s} -> {b:44s} {len(v):6d} {med(v):9.2f} {min(v) / 1e3:9.2f}")
    res["gaps_us"][f"{a} -> {b}"] = {"pairs": len(v), "median": med(v), "min": min(v) / 1e3}
if len(sys.argv) > 2:
    json.dump(res, open(sys.argv[2], "w"), indent=1)
