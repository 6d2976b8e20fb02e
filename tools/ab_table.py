"""In-step A/B table: DIR holds the JSON lines of `python bench.py --gpus 1 --steps 20 --warmup 5` of two builds run interleaved in
separate processes, parent_N.json and cand_N.json (N = 1 .. 5): per event group the median and the spread (max - min) of each build's
own passes (the protocol of profiles/region_grid_probe.txt section 1).  usage: python tools/ab_table.py DIR"""
import glob
import json
import statistics
import sys

d = sys.argv[1]


def load(tag):
    out = []
    for p in sorted(glob.glob("%s/%s_[0-9].json" % (d, tag))):
        out.append(json.loads(open(p).read().strip().splitlines()[-1]))
    return out


def groups(j):
    for k, v in j.items():
        if isinstance(v, dict) and "hungarian_batch" in v and "pseudo_label" in v and "gbs" not in k:
            return k, v
    raise KeyError


P, C = load("parent"), load("cand")
key = groups(P[0])[0]
print("# group key:", key, " passes:", len(P), len(C))


def stat(vals):
    return statistics.median(vals), max(vals) - min(vals)


def line(name, pv, cv):
    (pm, ps), (cm, cs) = stat(pv), stat(cv)
    print("  %-28s parent median %.3f spread %.3f | new median %.3f spread %.3f | delta %+.3f" % (name, pm, ps, cm, cs, cm - pm))


print("parent  ms_per_step passes", ["%.3f" % j["ms_per_step"] for j in P])
print("new     ms_per_step passes", ["%.3f" % j["ms_per_step"] for j in C])
line("ms_per_step", [j["ms_per_step"] for j in P], [j["ms_per_step"] for j in C])
for g in sorted(P[0][key]):
    line(g, [j[key][g] for j in P], [j[key][g] for j in C])
line("hungarian_batch+pseudo_label", [j[key]["hungarian_batch"] + j[key]["pseudo_label"] for j in P],
     [j[key]["hungarian_batch"] + j[key]["pseudo_label"] for j in C])
