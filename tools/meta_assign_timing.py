#!/usr/bin/env python3
"""--meta --filter-and-assign: device time of pmx_meta_assign (pmx_last_kernel_ms "meta_assign" + "meta_assign_emit") against
the only other route to the same answer, pmx_meta_score with EVERY node as a candidate ("meta_score": bit matrices + score
kernel; the download of the score matrix and a host argmax are not counted).  Each is run twice, the second run is reported
(the first one allocates inside the span).
With `taxonomy` as the last argument instead: the taxonomy filter.  Every node gets a taxon by the labelling of tests/taxa_checks.py
with 16 taxa (a leaf v with v % 7 != 3 and an internal node with v % 11 == 5 get (16 v) // n), at most one taxon a read.  Three
calls, each run twice: without a taxonomy, with it, and with it and --ambiguous-score-threshold-ratio 0.1; "meta_assign_taxa" is
the taxonomy pass (its kernels and the scan of the node counts, which "meta_assign" holds without a taxonomy).
With `breadth` as the last argument instead: --breadth-ratio.  Two calls, each run twice: without breadth and with it; "meta_breadth" is
the breadth pass (k_meta_breadth_rows per chunk and k_meta_breadth_count once), hit_matrix_bytes the matrix it keeps across the chunks.
With `best` as the last argument instead: the all-node pass of the read-score reports, pmx_meta_read_best, beside its yardstick
pmx_meta_assign on the same reads.  Three rounds, each two calls of assign and two of read_best; of every round the second call's
span ("meta_assign", "meta_read_best") and wall time; the three observations and their median.  A library without
pmx_meta_read_best (PMX_LIB_PATH pointing at an earlier build) gives the yardstick alone.
  meta_assign_timing.py rsv  [n_reads]   rsv_4K, reads at step 1 over two of its genomes (default 20,000)
  meta_assign_timing.py sars [n_reads]   SARS-CoV-2 20k tree, the 5-haplotype mixture of test_config5_sars_five_haplotypes (default 200,000)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def rsv_reads(pmx, n):
    rng = np.random.default_rng(1330)
    reads = []
    for g in (_fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))):
        reads += [g[i:i + 150].encode() for i in range(min(n // 2, len(g) - 149))]
    for i in range(0, len(reads), 3):
        reads[i] = pmx.reverse_complement(reads[i])
    for i in range(1, len(reads), 6):
        q = bytearray(reads[i])
        for p in rng.integers(0, len(q), 2):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4] if q[p] in b"ACGT" else q[p]
        reads[i] = bytes(q)
    concat, off = pmx.concat_reads(reads)
    return np.frombuffer(concat, np.uint8), off


def sars_reads(pmx, pm, n):
    golden = [x.rstrip("\n").split("\t") for x in open(os.path.join(GOLDEN, "example.mgsr.abundance.out"))]
    parts, offs, base = [], [np.zeros(1, np.int64)], 0
    for i, (name, share) in enumerate(zip([g[0] for g in golden[:5]], [0.50, 0.20, 0.15, 0.10, 0.05])):
        c, o = pmx.simulate_paired_reads(pm.genome(pm.find_node(name)), int(n * share) // 2, seed=10 + i)
        parts.append(c if isinstance(c, np.ndarray) else np.frombuffer(c, np.uint8))
        offs.append(np.asarray(o[1:], np.int64) + base)
        base += int(o[-1])
    return np.concatenate(parts), np.concatenate(offs)


def label(parent, n_taxa=16):
    n = len(parent)
    internal = np.zeros(n, bool)
    internal[np.asarray(parent[1:], np.int64)] = True
    v = np.arange(n)
    return np.where(np.where(internal, v % 11 == 5, v % 7 != 3), (v * n_taxa) // n, -1).astype(np.int32)


def taxonomy_mode(meta, ms, out):
    taxon = label(meta.index_oriented.arrays()["parent"])
    for name, with_taxonomy, ratio in (("plain", False, 0.0), ("taxa", True, 0.0), ("taxa_ratio_0.1", True, 0.1)):
        meta.set_taxonomy(taxon, 1) if with_taxonomy else meta.set_taxonomy(max_taxa=0)
        for rep in range(2):
            res = meta.assign(0.0, ambiguous_ratio=ratio)
            out[name] = dict(assign_ms=ms("meta_assign"), taxa_ms=ms("meta_assign_taxa"), emit_ms=ms("meta_assign_emit"),
                             assigned=int((res.state == 2).sum()), over=int((res.state == 3).sum()))


def breadth_mode(meta, ms, out):
    for name, on in (("off", False), ("on", True)):
        for rep in range(2):
            t0 = time.perf_counter()
            res = meta.assign(0.0, breadth=on)
            out[name] = dict(wall_s=time.perf_counter() - t0, assign_ms=ms("meta_assign"), emit_ms=ms("meta_assign_emit"), breadth_ms=ms("meta_breadth"),
                             assigned=int((res.state == 2).sum()))
    total, observed, depth = res.breadth
    out["hit_matrix_bytes"] = out["bit_matrix_bytes"] // 2
    out["nodes_with_hits"], out["observed_sum"], out["depth_sum"] = int((observed > 0).sum()), int(observed.sum()), int(depth.sum())


def best_mode(pmx, meta, ms, out):
    have = "pmx_meta_read_best" not in pmx._lib.MISSING
    seen = dict(assign_ms=[], assign_wall_s=[], read_best_ms=[], read_best_wall_s=[])
    for rnd in range(3):
        for rep in range(2):
            t0 = time.perf_counter()
            res = meta.assign(0.0)
            wall, span = time.perf_counter() - t0, ms("meta_assign")
        seen["assign_ms"].append(span)
        seen["assign_wall_s"].append(wall)
        for rep in range(2 if have else 0):
            t0 = time.perf_counter()
            mx, nb = meta.read_best()
            wall, span = time.perf_counter() - t0, ms("meta_read_best")
        if have:
            seen["read_best_ms"].append(span)
            seen["read_best_wall_s"].append(wall)
    for name, obs in seen.items():
        if obs:
            out[name], out[name + "_median"] = obs, float(np.median(obs))
    if have:
        merged_max = np.zeros(meta.n_reads, np.int64)
        merged_max[res.merged[res.merged >= 0]] = res.max[res.merged >= 0]
        out["max_equal"] = bool(np.array_equal(mx.astype(np.int64), merged_max))
        out["mapped_reads"], out["n_best_sum"], out["active_nodes"] = int((mx > 0).sum()), int(nb.sum()), int(meta.active_nodes().sum())


def main():
    import panmap_amd as pmx
    from panmap_amd._lib import lib
    taxonomy, breadth, best = sys.argv[-1] == "taxonomy", sys.argv[-1] == "breadth", sys.argv[-1] == "best"
    if taxonomy or breadth or best:
        sys.argv.pop()
    which = sys.argv[1] if len(sys.argv) > 1 else "rsv"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else (20000 if which == "rsv" else 200000)
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman" if which == "rsv" else "sars_20000_twilight_dipper.panman"))
    ctx = pmx.Context(0)
    meta = pmx.Meta.build(ctx, pm)
    concat, off = rsv_reads(pmx, n) if which == "rsv" else sars_reads(pmx, pm, n)
    meta.set_reads(concat=concat, offsets=off)
    n_nodes = meta.index.info.n_nodes
    ms = lambda name: float(lib.pmx_last_kernel_ms(ctx._h, name.encode()))
    out = dict(case=which, reads=len(off) - 1, distinct_reads=meta.n_reads, nodes=n_nodes)
    _, h, _ = meta.read_seedmers()
    words = ((n_nodes + 63) // 64 + 1) & ~1
    out["distinct_seedmers"] = int(len(np.unique(h)))
    out["bit_matrix_bytes"] = 2 * out["distinct_seedmers"] * words * 8     # (of all reads: split over chunks of at most 2 GiB)
    if taxonomy or breadth or best:
        taxonomy_mode(meta, ms, out) if taxonomy else breadth_mode(meta, ms, out) if breadth else best_mode(pmx, meta, ms, out)
        print(json.dumps(out))
        return
    for rep in range(2):
        t0 = time.perf_counter()
        res = meta.assign(0.0)
        out["assign_wall_s"] = time.perf_counter() - t0
        out["assign_ms"], out["assign_emit_ms"] = ms("meta_assign"), ms("meta_assign_emit")
    out["assigned_reads"] = int((res.state == 2).sum())
    out["assigned_nodes_total"] = int(lib.pmx_meta_assign_num_nodes(meta._h))
    every = np.arange(n_nodes, dtype=np.uint32)
    for rep in range(2):
        meta.score(candidates=every)
        out["score_all_nodes_ms"] = ms("meta_score")
    out["score_matrix_bytes"] = meta.n_reads * n_nodes * 2
    if which == "rsv":                                          # the two routes agree (the big case would download 7 GB)
        sc = meta.scores()
        merged_max = np.zeros(meta.n_reads, np.int64)
        merged_max[res.merged[res.merged >= 0]] = res.max[res.merged >= 0]
        out["max_equal"] = bool(np.array_equal(sc.max(axis=1).astype(np.int64), merged_max))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
