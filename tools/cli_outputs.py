#!/usr/bin/env python3
"""Every output file and the stderr of a fixed list of `panmap` invocations, one directory per invocation under OUTDIR; the
`(…ms)` of the --batch lines is taken out of the stderr.  To compare two builds of the command line
(panmap_amd/csrc/cli/panmap_main.cpp), run it once per binary and `diff -r` the two directories (profiles/r11/README.md).
Every child runs under its own time limit; the first one that ends with a signal or at its limit ends the driver.
With NAMEs, only the invocations so named run, and the `rsv_index` they build on.
usage: tools/cli_outputs.py BINARY OUTDIR [NAME ...]"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEMO = ["sars_20000_twilight_dipper.panman", "isolate_R1.fastq.gz", "isolate_R2.fastq.gz"]


def fastq(path, prefix, seqs, mode="w"):
    with open(path, mode) as f:
        for i, s in enumerate(seqs):
            f.write("@%s%d\n%s\n+\n%s\n" % (prefix, i, s, "I" * len(s)))


def genome(name):
    return "".join(l.strip() for l in open(os.path.join(GOLDEN, name)) if not l.startswith(">")).upper()


def strided(g, n, L=150):
    """the first n reads of length L at the stride that spreads n of them over g (the sample of tests/test_cli.py)"""
    step = max(1, (len(g) - L) // n)
    return [g[i:i + L] for i in range(0, len(g) - L + 1, step)][:n]


def inputs(work):
    """the demo, the rsv tree with the 70 / 30 mixture and a small paired set, an HPC index of the rsv tree with long reads; for
    the --meta features the mixture with planted singletons, its amplicon table (tests/test_cli_amplicon.py) and the rsv
    tree's taxonomy table (tests/test_cli_taxa.py)"""
    import panmap_amd as pmx
    import hpc_checks as hc
    import taxa_checks as tc
    for f in DEMO:
        shutil.copy(os.path.join(GOLDEN, f), os.path.join(work, f))
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), os.path.join(work, "rsv.panman"))
    a, b = genome("MZ515733.1.fa"), genome("rsv_4K.panman.random.node_1330.fa")
    fastq(os.path.join(work, "mix.fastq"), "A", strided(a, 700))
    fastq(os.path.join(work, "mix.fastq"), "B", strided(b, 300), "a")
    mix = strided(a, 700) + strided(b, 300)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    planted = ["".join(flip.get(x, x) if i in (40, 110) else x for i, x in enumerate(r)) for r in mix[::25]]   # their changed k-min-mers occur once
    fastq(os.path.join(work, "planted.fastq"), "r", mix + planted)
    primer = [None if i % 7 == 3 else "amp%02d" % (i // 50) for i in range(len(mix))] + ["amp_planted"] * len(planted)
    with open(os.path.join(work, "depth.tsv"), "w") as f:            # 50 consecutive reads a primer, every 7th read unlisted
        f.write("".join("r%d\t%s\n" % (i, p) for i, p in enumerate(primer) if p is not None))
    stride = (len(b) - 250) // 200
    r1 = [b[i * stride:i * stride + 150] for i in range(200)]
    r2 = [b[i * stride + 100:i * stride + 250][::-1].translate(str.maketrans("ACGT", "TGCA")) for i in range(200)]
    fastq(os.path.join(work, "R1.fastq"), "p", r1)
    fastq(os.path.join(work, "R2.fastq"), "p", r2)
    fastq(os.path.join(work, "R2_short.fastq"), "p", r2[:-1])
    x, noise = 12345, []
    for _ in range(150):                           # one pseudo-random read (tests/test_cli.py)
        x = (1103515245 * x + 12345) % (1 << 31)
        noise.append("ACGT"[(x >> 16) & 3])
    fastq(os.path.join(work, "noise.fastq"), "n", ["".join(noise)])
    rsv = pmx.Panman(os.path.join(work, "rsv.panman"))
    pmx.Index.build(rsv, hpc=True).save(os.path.join(work, "hpc.idx"))
    oriented = pmx.Index.build(rsv, flank_mask=0, mode=0x100)
    parent = oriented.arrays()["parent"]
    tc.write_metadata(os.path.join(work, "taxa.tsv"), [oriented.node_id(v) for v in range(len(parent))], tc.label(parent, tc.RSV_T))
    g = rsv.genome(rsv.find_node("MZ515733.1"))
    rng = np.random.default_rng(2)
    long_reads = []
    for _ in range(200):
        n = int(rng.integers(500, 3000))
        st = int(rng.integers(0, len(g) - n))
        long_reads.append(hc.run_length_errors(rng, g[st:st + n]).decode())
    fastq(os.path.join(work, "long.fq"), "r", long_reads)
    with open(os.path.join(work, "three.txt"), "w") as f:
        f.write("# reads1 [reads2] [prefix]\nisolate_R1.fastq.gz isolate_R2.fastq.gz out/paired\n\nisolate_R1.fastq.gz single_end\nisolate_R2.fastq.gz\n")
    with open(os.path.join(work, "failing.txt"), "w") as f:
        f.write("R1.fastq R2.fastq first\nR1.fastq R2_short.fastq short\nR1.fastq R2.fastq third\nR1.fastq R2.fastq deep/er/fourth\nnoise.fastq noise\n")
    os.mkdir(os.path.join(work, "meet"))


def invocations(work):
    """(name, arguments, extra environment, time limit in seconds)"""
    two = dict(PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=os.path.join(work, "meet"))
    refine = ["--refine", "--refine-max-top-n", "4", "--refine-max-neighbor-n", "3"]
    rsv = ["rsv.panman", "-i", "rsv.idx"]       # (its own index file: hpc.idx must not be found as the cache of the same tree)
    assign = rsv + ["mix.fastq", "--meta", "--filter-and-assign", "-o", "x"]
    amplicons = rsv + ["planted.fastq", "--meta", "--amplicon-depth", "depth.tsv", "--mask-reads-relative-frequency", "0.05", "-o", "x"]
    return [("index", ["sars_20000_twilight_dipper.panman", "--stop", "index"], {}, 120),
            ("demo", DEMO + ["-o", "x"], {}, 240),
            ("annotate", DEMO + ["-o", "x", "--annotate-vcf"], {}, 240),
            ("stop_place", DEMO + ["-o", "x", "--stop", "place"], {}, 120),
            ("stop_align", DEMO + ["-o", "x", "--stop", "align"], {}, 240),
            ("stop_genotype", DEMO + ["-o", "x", "--stop", "genotype"], {}, 240),
            ("refine", DEMO + ["-o", "x", "--stop", "place"] + refine, {}, 240),
            ("dedup", DEMO + ["-o", "x", "--stop", "place", "--dedup"], {}, 120),
            ("min_seed_quality", DEMO + ["-o", "x", "--stop", "place", "--min-seed-quality", "20"], {}, 120),
            ("single_end", DEMO[:2] + ["-o", "x"], {}, 240),
            ("batch", [DEMO[0], "--batch", "three.txt"], {}, 600),
            ("gpus2_refine", DEMO + ["-o", "x", "--gpus", "2"] + refine, two, 600),
            ("gpus2_dedup", DEMO + ["-o", "x", "--gpus", "2", "--dedup"], two, 600),
            ("rsv_index", ["rsv.panman", "--index-out", "rsv.idx", "--stop", "index"], {}, 120),
            ("meta", rsv + ["mix.fastq", "--meta", "-o", "x"], {}, 300),
            ("meta_gpus2", rsv + ["mix.fastq", "--meta", "--gpus", "2", "-o", "x"], two, 300),
            ("meta_assign", assign, {}, 300),
            ("meta_assign_taxa", assign + ["--taxonomic-metadata", "taxa.tsv", "--maximum-taxon-number", "1"], {}, 300),
            ("meta_assign_breadth", assign + ["--breadth-ratio"], {}, 300),
            ("meta_mask_seeds", rsv + ["planted.fastq", "--meta", "--mask-seeds", "1", "-o", "x"], {}, 300),
            ("meta_amplicons", amplicons, {}, 300),
            ("meta_amplicons_gpus2", amplicons + ["--gpus", "2"], two, 300),
            ("hpc_place", ["rsv.panman", "long.fq", "-i", "hpc.idx", "--stop", "place", "-o", "x"], {}, 120),
            ("batch_failed_sample", rsv + ["--batch", "failing.txt", "--stop", "align"], {}, 240),
            ("batch_refine", rsv + ["--batch", "failing.txt", "--stop", "place", "--refine", "--refine-max-top-n", "3", "--refine-max-neighbor-n", "2"], {}, 240)]


def files(work):
    return {os.path.relpath(os.path.join(d, f), work) for d, _, fs in os.walk(work) for f in fs}


def main():
    binary, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    os.makedirs(out)
    work = tempfile.mkdtemp(prefix="cli_outputs_")
    try:
        inputs(work)
        only = set(sys.argv[3:])
        unknown = only - {name for name, _, _, _ in invocations(work)}
        if unknown:
            sys.exit("no such invocation: " + ", ".join(sorted(unknown)))
        for name, args, env, limit in invocations(work):
            if only and name not in only and name != "rsv_index":
                continue
            before = {f: os.stat(os.path.join(work, f)).st_mtime_ns for f in files(work)}
            try:
                r = subprocess.run([binary] + args, cwd=work, capture_output=True, text=True, timeout=limit, env=dict(os.environ, **env))
            except subprocess.TimeoutExpired:
                sys.exit("%s: not back within %d s; stopping" % (name, limit))
            dest = os.path.join(out, name)
            os.makedirs(dest)
            with open(os.path.join(dest, "stderr.txt"), "w") as f:
                f.write(re.sub(r" \(\d+ms\)", "", r.stderr))
                f.write("exit code %d\n" % r.returncode)
            written = sorted(f for f in files(work) if not f.endswith(".idx") and not f.startswith("meet/") and
                             before.get(f) != os.stat(os.path.join(work, f)).st_mtime_ns)
            for f in written:
                os.makedirs(os.path.dirname(os.path.join(dest, f)), exist_ok=True)
                shutil.move(os.path.join(work, f), os.path.join(dest, f))
            print("%-20s exit %d, %d files" % (name, r.returncode, len(written)), flush=True)
            if r.returncode < 0 or r.returncode > 128:   # (a rank that a signal ended: 128 + the signal, fork_ranks)
                sys.exit("%s: ended by a signal (code %d); stopping" % (name, r.returncode))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
