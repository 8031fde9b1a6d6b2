#!/usr/bin/env python3
"""Wall time of the command line for two builds of it: the README demo to consensus and a --batch of three samples, one warm-up
and ten runs per binary, the two binaries alternating; the first child that fails ends the run (profiles/r11/README.md).
usage: tools/cli_timing.py PARENT_BINARY NEW_BINARY"""
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEMO = ["sars_20000_twilight_dipper.panman", "isolate_R1.fastq.gz", "isolate_R2.fastq.gz"]
BIN = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2])}
work = tempfile.mkdtemp(prefix="cli_time_")
for f in DEMO:
    shutil.copy(os.path.join(GOLDEN, f), os.path.join(work, f))
open(os.path.join(work, "three.txt"), "w").write("isolate_R1.fastq.gz isolate_R2.fastq.gz out/paired\nisolate_R1.fastq.gz single_end\nisolate_R2.fastq.gz\n")
cases = {"demo": DEMO + ["-o", "x"], "batch3": [DEMO[0], "--batch", "three.txt"]}


def one(b, args):
    t0 = time.perf_counter()
    r = subprocess.run([BIN[b]] + args, cwd=work, capture_output=True, text=True, timeout=300)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stderr[-2000:])
        sys.exit("%s %s: exit %d; stopping" % (b, args, r.returncode))
    return dt


one("parent", DEMO + ["--stop", "index"])          # the index cache, outside the timing
for name, args in cases.items():
    one("parent", args)                              # one warm-up each
    one("new", args)
    t = {"parent": [], "new": []}
    for i in range(10):
        for b in ("parent", "new"):
            t[b].append(one(b, args))
    for b in t:
        v = t[b]
        print("%-7s %-6s mean %.3f min %.3f max %.3f  %s" % (name, b, sum(v) / len(v), min(v), max(v), " ".join("%.3f" % x for x in v)), flush=True)
shutil.rmtree(work, ignore_errors=True)
