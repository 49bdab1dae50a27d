"""usage: kernel_trace_compare.py WARMUP TAIL GROUP PARENT_TRACE[,PARENT_TRACE..] NEW_TRACE[,NEW_TRACE..] [OUT.md]
Two builds of the library under `rocprofv3 --kernel-trace` on the same bench command -> one row per kernel symbol of the NEW
build, with the time the PARENT build spent on the SAME launches.

The symbols of two builds need not correspond one to one (a template argument added to a kernel splits one symbol into
several), but the plan does: the n-th launch of a forward pass is the same layer in both.  So every stream is cut into forward
passes at od_stem_k, the first WARMUP passes and the last TAIL (bench.py's one-op-at-a-time roofline passes) are dropped, and
launches are matched by their position in the pass.  spread = (max - min) / median of the per-launch mean over consecutive
groups of GROUP passes, the larger of the two builds: what one run says about its own repeatability for that symbol."""
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
        m = re.search(r"(od_\w+(<[^>]*>)?)", r["Kernel_Name"])
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
    out = [p[1] for p in out[warmup:len(out) - tail]]
    names = [tuple(n for n, _ in p) for p in out]
    assert len(set(names)) == 1, f"{path}: the timed passes do not launch the same kernels ({len(set(names))} sequences)"
    return list(names[0]), [[us for _, us in p] for p in out]


def load(paths, warmup, tail):
    names, durs = None, []
    for p in paths.split(","):
        n, d = passes(p, warmup, tail)
        assert names is None or names == n
        names = n
        durs += d
    return names, durs


def main():
    warmup, tail, group = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    pn, pd = load(sys.argv[4], warmup, tail)
    nn, nd = load(sys.argv[5], warmup, tail)
    assert len(pn) == len(nn), (len(pn), len(nn))
    pos = collections.defaultdict(list)
    for i, nm in enumerate(nn):
        pos[nm].append(i)

    def per_launch(durs, idx):  # per pass: mean over the launches of this symbol; -> overall mean, spread over groups
        v = [sum(d[i] for i in idx) / len(idx) for d in durs]
        g = [statistics.fmean(v[k:k + group]) for k in range(0, len(v) - group + 1, group)]
        return statistics.fmean(v), (max(g) - min(g)) / statistics.median(g)

    lines = [f"passes: parent {len(pd)}, new {len(nd)}; {len(nn)} launches per pass; groups of {group} passes", "",
             "| symbol (new build) | launches / pass | parent symbol | parent µs | new µs | new − parent | spread | |",
             "|---|---|---|---|---|---|---|---|"]
    tot_p = tot_n = 0.0
    for nm in sorted(pos, key=lambda k: -sum(statistics.fmean(d[i] for d in pd) for i in pos[k])):
        idx = pos[nm]
        a, sa = per_launch(pd, idx)
        b, sb = per_launch(nd, idx)
        tot_p += a * len(idx)
        tot_n += b * len(idx)
        rel, s = (b - a) / a, max(sa, sb)
        par = ", ".join(sorted({pn[i] for i in idx}))
        verdict = "slower" if rel > s else ("faster" if rel < -s else "within spread")
        lines.append(f"| `{nm}` | {len(idx)} | `{par}` | {a:.2f} | {b:.2f} | {rel * 100:+.1f} % | {s * 100:.1f} % | {verdict} |")
    lines.append(f"| sum over one pass | {len(nn)} | | {tot_p:.1f} | {tot_n:.1f} | {(tot_n - tot_p) / tot_p * 100:+.1f} % | | |")
    txt = "\n".join(lines)
    print(txt)
    if len(sys.argv) > 6:
        open(sys.argv[6], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
