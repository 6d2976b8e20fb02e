"""Launch lists of the hungarian_batch / pseudo_label groups from a rocprofv3 kernel trace of the bench command.
Per timed call: every launch from the first one after the preceding MSDA / EMA kernel to the call's last kernel, with the launches that
are not ours (copies, concatenations, fills) counted and summed -- the glue around the matcher and the pseudo-label kernels
(profiles/native_chains_probe.txt).  The mask clone bench.py issues before the pseudo-label call shows as the first copy of that call.
usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 10 --warmup 3
       python tools/trace_groups.py DIR/*/*_kernel_trace.csv"""
import csv
import re
import statistics
import sys

OURS = ("match_cost_kernel", "lsap_kernel", "nms_prepare_kernel", "nms_class_kernel", "nms_topk_kernel", "pseudo_label_kernel",
        "transform_bboxes_kernel", "build_targets_kernel")


def short(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    m = re.match(r"[\w:]+", n)
    n = m.group(0) if m else n
    return n.split("::")[-1] if n.startswith("at::") else n


rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
ev = [(short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
is_ours = [any(e[0].startswith(o) for o in OURS) for e in ev]
is_msda = [("msda" in e[0] or "ema" in e[0]) for e in ev]
# units: the launches of one timed call -- closed by its last kernel (lsap / transform), or by the next msda / ema kernel
# (the trailing stack + read-back of the pseudo-label launch belong to it)
segs, cur = [], None
for i in range(len(ev)):
    if is_msda[i]:
        if cur is not None and any(is_ours[cur:i]):
            segs.append((cur, i))
        cur = None
        continue
    if cur is None:
        cur = i
    if ev[i][0].startswith(("lsap_kernel", "transform_bboxes_kernel")):
        segs.append((cur, i + 1))
        cur = None


def kind(seg):
    names = [ev[k][0] for k in range(*seg) if is_ours[k]]
    if "match_cost_kernel" in names:
        return "hungarian_batch"
    return "pseudo_label(launch)" if "nms_prepare_kernel" in names else "pseudo_label(finish)"


by = {}
for s in segs:
    by.setdefault(kind(s), []).append(s)
for k, ss in by.items():
    glue_between, glue_lead, n_glue = [], [], []
    for a, b in ss:
        ours = [x for x in range(a, b) if is_ours[x]]
        f, l = ours[0], ours[-1]
        glue_between.append(sum(ev[x][2] - ev[x][1] for x in range(f, l) if not is_ours[x]) / 1e3)
        glue_lead.append(sum(ev[x][2] - ev[x][1] for x in range(a, f)) / 1e3)
        n_glue.append(sum(1 for x in range(a, l) if not is_ours[x]))
    print("== %s: %d segments; non-ours launches up to the group's last kernel: count median %g, time between first and last "
          "of ours median %.2f us, time before the first of ours median %.2f us" %
          (k, len(ss), statistics.median(n_glue), statistics.median(glue_between), statistics.median(glue_lead)))
    print("   elapsed first launch start -> last launch end: median %.2f us" %
          statistics.median((ev[b - 1][2] - ev[a][1]) / 1e3 for a, b in ss))
    a, b = ss[-1]
    t0 = ev[a][1]
    for x in range(a, b):
        print("   %-46s %s start %8.2f us  dur %6.2f us" % (ev[x][0][:46], "ours" if is_ours[x] else "    ", (ev[x][1] - t0) / 1e3,
                                                          (ev[x][2] - ev[x][1]) / 1e3))
