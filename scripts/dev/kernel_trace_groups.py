"""usage: kernel_trace_groups.py TRACE_DIR GROUP SKIP OUT.json
kernel_trace.csv of one rocprofv3 run -> per kernel-name family: count, mean, and the means of consecutive groups (spread)."""
import csv, glob, json, sys, re, collections
d, group, skip = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
fam = collections.defaultdict(list)
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        nm = r["Kernel_Name"]
        m = re.search(r"(od_augment_mosaic_k|od_augment_k|od_assign_match<[^>]*>|od_assign_encode<[^>]*>|od_assign_match|od_assign_encode)", nm)
        if m:
            fam[m.group(1)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
out = {}
for k, v in fam.items():
    v = v[skip:]
    groups = [v[i:i + group] for i in range(0, len(v) - group + 1, group)]
    gm = [sum(g) / len(g) for g in groups]
    out[k] = {"n": len(v), "mean_us": sum(v) / max(1, len(v)), "group_means_us": [round(x, 3) for x in gm],
              "min_us": min(v) if v else None, "max_us": max(v) if v else None}
print(json.dumps(out, indent=1))
open(sys.argv[4], "w").write(json.dumps(out, indent=1))
