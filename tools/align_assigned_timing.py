#!/usr/bin/env python3
"""--meta --filter-and-assign --align-reads on rsv_4K: where a node's time goes, and the select kernel against its bound.
  align_assigned_timing.py [n_reads] [n_nodes]   reads at step 1 over two genomes of the tree (default 20,000), the n_nodes most
                                                 populated heads (default 64)
Prints one JSON line:
  spans_before / spans_after   meta_assign / meta_assign_emit of Meta.assign(0.6) run before and after the alignments (ms)
  per_node_ms                  medians over the nodes of the wall time of select + pack, set_reference, align, fetch, write_bam
  select                       one select of 2,000,000 picks: kernel ms (pmx_last_kernel_ms "select"), bytes moved (2 x the selected
                               bytes, 4 x with qualities) and GB/s, without and with qualities
  cli                          wall seconds of the command line without --align-reads, and with it at 1 and at 4 workers
                               (PMX_ALIGN_READS_STREAMS), --min-num-align set so that n_nodes heads qualify; after one run to warm
                               up, each twice, interleaved"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def rsv_reads(pmx, n):
    reads = []
    for g in (_fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))):
        reads += [g[i:i + 150].encode() for i in range(min(n // 2, len(g) - 149))]
    for i in range(0, len(reads), 3):
        reads[i] = pmx.reverse_complement(reads[i])
    return reads


def main():
    import panmap_amd as pmx
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    n_nodes = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    ctx = pmx.Context(0)
    meta = pmx.Meta.build(ctx, pm)
    reads = rsv_reads(pmx, n)
    quals = [b"I" * len(r) for r in reads]
    meta.set_reads(reads)
    ms = ctx.kernel_ms

    def assign():
        for rep in range(2):
            res = meta.assign(0.6)
        return res, dict(meta_assign=ms("meta_assign"), meta_assign_emit=ms("meta_assign_emit"))
    res, before = assign()
    by_node = res.by_node()
    counts = sorted((len(v) for v in by_node.values()), reverse=True)
    k = counts[min(n_nodes, len(counts)) - 1]
    todo = [h for h in sorted(by_node) if len(by_node[h]) >= k]
    out = dict(reads=len(reads), assigned=int((res.fastq_index >= 0).sum()), heads_with_reads=len(by_node), min_num_align=k, nodes=len(todo),
               reads_per_node_median=float(np.median([len(by_node[h]) for h in todo])), spans_before=before)
    order = np.nonzero(res.fastq_index >= 0)[0].tolist()
    assigned = [reads[i] for i in order]
    src = pmx.ReadSet(ctx, assigned, pack=False)
    src.set_qualities([quals[i] for i in order])
    names = [b"r%d" % i for i in order]
    steps = {s: [] for s in ("select_pack", "set_reference", "align", "fetch", "write_bam")}
    al, sel = None, None
    with tempfile.TemporaryDirectory() as tmp:
        for h in todo:
            idx = by_node[h]
            genome = pm.genome(h)
            mean_len = sum(len(assigned[i]) for i in idx) // len(idx)
            t = [time.perf_counter()]
            sel = src.select(idx, out=sel)
            ctx.synchronize()
            t.append(time.perf_counter())
            if al is None:
                al = pmx.Aligner(ctx, genome, mean_len)
            else:
                al.set_reference(genome, mean_len)
            ctx.synchronize()
            t.append(time.perf_counter())
            al.align_readset(sel, paired=False)
            ctx.synchronize()
            t.append(time.perf_counter())
            recs, cig = al.fetch()
            t.append(time.perf_counter())
            results = pmx.records_to_results(recs, cig, False)
            t0 = time.perf_counter()
            pmx.write_bam(os.path.join(tmp, "n.bam"), "n", len(genome), [assigned[i] for i in idx], [b"I" * len(assigned[i]) for i in idx], [names[i] for i in idx], results, False)
            t1 = time.perf_counter()
            for s, d in zip(steps, [t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t1 - t0]):
                steps[s].append(d * 1e3)
        out["per_node_ms"] = {s: float(np.median(v)) for s, v in steps.items()}
        _, out["spans_after"] = assign()
        # the select kernel alone
        picks = np.random.default_rng(1).integers(0, len(assigned), 2000000)
        out["select"] = {}
        for name, s in (("with_qualities", src), ("bases_only", pmx.ReadSet(ctx, assigned, pack=False))):
            big = None
            for rep in range(3):
                big = s.select(picks, pack=False, out=big)
                ctx.synchronize()
            moved = big.total_bases * (4 if name == "with_qualities" else 2)
            out["select"][name] = dict(kernel_ms=ms("select"), bytes_moved=moved, gb_per_s=moved / (ms("select") * 1e-3) / 1e9)
            big.close()
        # the command line
        fq = os.path.join(tmp, "reads.fastq")
        with open(fq, "w") as f:
            for i, r in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
        cli = os.path.join(ROOT, "panmap_amd", "bin", "panmap")
        base = [cli, os.path.join(GOLDEN, "rsv_4K.panman"), fq, "--meta", "--filter-and-assign", "--discard", "0.6", "-q"]
        out["cli"] = {}
        with_it = ["--align-reads", "--min-num-align", str(k)]
        for name, extra, workers in (("warm_up", [], None), ("without", [], None), ("workers_1", with_it, "1"), ("workers_4", with_it, "4"),
                                     ("without", [], None), ("workers_1", with_it, "1"), ("workers_4", with_it, "4")):
            env = dict(os.environ)
            if workers:
                env["PMX_ALIGN_READS_STREAMS"] = workers
            t0 = time.perf_counter()
            subprocess.run(base + extra + ["-o", os.path.join(tmp, name)], check=True, env=env, timeout=300)
            out["cli"].setdefault(name, []).append(time.perf_counter() - t0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
