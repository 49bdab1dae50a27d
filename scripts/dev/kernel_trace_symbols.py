"""usage: kernel_trace_symbols.py WARMUP TAIL PATTERN PARENT_TRACE NEW_TRACE [OUT.md]
Two builds under `rocprofv3 --kernel-trace` on the same bench command whose forward passes do NOT launch the same number of
kernels (kernel_trace_compare.py matches launches by position and needs that): per kernel symbol matching the regular
expression PATTERN, launches per pass and mean microseconds per launch over the timed passes of each build, and the launches
per pass of everything.  Passes are cut at od_stem_k as in kernel_trace_compare.py; template arguments are dropped from names."""
import collections
import csv
import re
import statistics
import sys


def passes(path, warmup, tail):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    streams = collections.defaultdict(list)
    for r in rows:
        m = re.search(r"(od_\w+)", r["Kernel_Name"])
        if m:
            streams[(r["Queue_Id"], r["Stream_Id"])].append(
                (m.group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Start_Timestamp"])))
    out = []
    for v in streams.values():
        cur = None
        for nm, us, t0 in v:
            if nm.startswith("od_stem_k"):
                cur = [t0, []]
                out.append(cur)
            if cur is not None:
                cur[1].append((nm, us))
    out.sort(key=lambda p: p[0])
    return [p[1] for p in out[warmup:len(out) - tail]]


def table(ps, pat):
    per = collections.defaultdict(list)  # symbol -> per pass: (launches, total us)
    for p in ps:
        acc = collections.defaultdict(lambda: [0, 0.0])
        for nm, us in p:
            if re.search(pat, nm):
                acc[nm][0] += 1
                acc[nm][1] += us
        for nm, (k, us) in acc.items():
            per[nm].append((k, us))
    return {nm: (statistics.fmean(k for k, _ in v), statistics.fmean(us / k for k, us in v)) for nm, v in per.items()}


def main():
    warmup, tail, pat = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    pp, pn = passes(sys.argv[4], warmup, tail), passes(sys.argv[5], warmup, tail)
    tp, tn = table(pp, pat), table(pn, pat)
    lines = [f"passes: parent {len(pp)}, new {len(pn)}; launches per pass: parent {statistics.fmean(len(p) for p in pp):.0f}, "
             f"new {statistics.fmean(len(p) for p in pn):.0f}", "",
             "| symbol | parent launches / pass | parent µs / launch | new launches / pass | new µs / launch |", "|---|---|---|---|---|"]
    tot = [0.0, 0.0]
    for nm in sorted(set(tp) | set(tn)):
        cells = []
        for i, t in enumerate((tp, tn)):
            if nm in t:
                cells += [f"{t[nm][0]:.0f}", f"{t[nm][1]:.1f}"]
                tot[i] += t[nm][0] * t[nm][1]
            else:
                cells += ["-", "-"]
        lines.append(f"| `{nm}` | " + " | ".join(cells) + " |")
    lines.append(f"| sum per pass | | {tot[0]:.1f} | | {tot[1]:.1f} |")
    txt = "\n".join(lines)
    print(txt)
    if len(sys.argv) > 6:
        open(sys.argv[6], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
