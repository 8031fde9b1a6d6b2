#!/usr/bin/env python3
"""Compare the launches of two traced runs.  Each run is the output directory of
    rocprofv3 --kernel-trace --hip-runtime-trace --output-format csv -d DIR -o trace -- <program>
It is reduced to the ordered (kernel, grid, workgroup, LDS bytes) list per process and queue -- once for the library's own
kernels, once with the runtime's copy and fill kernels (__amd_rocclr_*) as well -- and to the count of every HIP call.
usage: tools/trace_launches.py DIR_A DIR_B   (profiles/r08, r09)"""
import collections
import csv
import glob
import os
import sys


def find(d, suffix):
    hits = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    assert hits, (d, suffix)
    return hits


def col(header, *names):
    low = {h.lower(): h for h in header}
    for n in names:
        if n.lower() in low:
            return low[n.lower()]
    raise KeyError((names, header))


def kernels(d):
    per_pid = collections.OrderedDict()
    for path in sorted(find(d, "kernel_trace.csv")):
        rows = list(csv.DictReader(open(path)))
        if not rows:
            continue
        h = rows[0].keys()
        name, q, disp = col(h, "Kernel_Name"), col(h, "Queue_Id"), col(h, "Dispatch_Id")
        grid = [col(h, "Grid_Size_" + a, "Grid_Size") for a in "XYZ"]
        wg = [col(h, "Workgroup_Size_" + a, "Workgroup_Size") for a in "XYZ"]
        lds = col(h, "LDS_Block_Size", "LDS_Block_Size_v", "Lds_Block_Size")
        rows.sort(key=lambda r: int(r[disp]))
        queues = collections.OrderedDict()
        for r in rows:
            queues.setdefault(r[q], []).append((r[name], tuple(r[g] for g in grid), tuple(r[w] for w in wg), r[lds]))
        per_pid[os.path.basename(path)] = list(queues.values())   # queues in order of first dispatch
    return per_pid


def hip_calls(d):
    c = collections.Counter()
    for path in sorted(find(d, "hip_api_trace.csv")):
        rows = csv.DictReader(open(path))
        f = None
        for r in rows:
            f = f or col(r.keys(), "Function")
            c[r[f]] += 1
    return c


def main():
    a, b = sys.argv[1], sys.argv[2]
    ka, kb = kernels(a), kernels(b)
    print("processes:", len(ka), len(kb))
    equal = len(ka) == len(kb)
    for (fa, qa), (fb, qb) in zip(ka.items(), kb.items()):
        print("queues:", [len(x) for x in qa], [len(x) for x in qb])
        if qa != qb:
            equal = False
            for i, (x, y) in enumerate(zip(qa, qb)):
                for j, (u, v) in enumerate(zip(x, y)):
                    if u != v:
                        print("first difference: queue", i, "launch", j, u, v)
                        break
    print("LAUNCH LISTS, runtime kernels included:", "EQUAL" if equal else "DIFFER")
    own = lambda per_pid: [[[k for k in q if not k[0].startswith("__amd_rocclr_")] for q in qs] for qs in per_pid.values()]
    oa, ob = own(ka), own(kb)
    print("own launches per queue:", [[len(q) for q in qs] for qs in oa], [[len(q) for q in qs] for qs in ob])
    print("LAUNCH LISTS, the library's own kernels:", "EQUAL" if oa == ob else "DIFFER")
    names = collections.Counter()
    for q in next(iter(ka.values())):
        for k in q:
            names[k[0].split("(")[0][-60:]] += 1
    for n, c in names.most_common():
        print("  %6d %s" % (c, n))
    ha, hb = hip_calls(a), hip_calls(b)
    print("HIP calls (A, B, B - A):")
    for f in sorted(set(ha) | set(hb)):
        print("  %-40s %8d %8d %+d" % (f, ha[f], hb[f], hb[f] - ha[f]))


if __name__ == "__main__":
    main()
