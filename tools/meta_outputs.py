#!/usr/bin/env python3
"""Every output of the --meta stage for three runs, one file per output under the directory argv[1]: the rsv 70 / 30 sample
without --dust and with --dust 20, and the `sars` sample of tests/dist_meta_worker.py (--dust 20 --discard 0.5); then two
masked runs, one run under amplicons with a relative mask and one --filter-and-assign run with taxonomy and breadth
(masked_and_assigned).  Doubles go out as bit patterns.  To compare two builds of the library, run it once per build, each selected with PMX_LIB_PATH, and
`diff -r` the two directories (profiles/r09/README.md)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out = sys.argv[1]
    tag = os.path.basename(os.path.normpath(out))
    os.makedirs(out, exist_ok=True)
    import panmap_amd as pmx
    from panmap_amd import _lib
    import dist_meta_worker as w
    ctx = pmx.Context(0)
    metas = {}
    for name, case, dust_override in (("rsv_nodust", "rsv", None), ("rsv_dust20", "rsv", 20.0), ("sars_dust20_discard05", "sars", None)):
        pm, reads, dust, discard = w.sample(pmx, case)
        if dust_override is not None:
            dust = dust_override
        if case not in metas:
            metas[case] = pmx.Meta.build(ctx, pm)
        meta = metas[case]
        meta.set_dust(dust)
        meta.set_reads(reads)
        meta.score(top_oc=1000)
        haps = meta.em(_lib.MetaParams(discard=discard))
        off, h, rev = meta.read_seedmers()
        ns, mult = meta.read_info()
        info = meta.em_info()
        arrays = dict(seedmer_off=off, seedmer_hash=h, seedmer_rev=rev, info_n=ns, info_mult=mult,
                      oc_bits=w.bits(meta.overlap_coefficients()), candidates=meta.candidates(), scores=meta.scores())
        for k, v in arrays.items():
            np.ascontiguousarray(v).tofile(os.path.join(out, "%s.%s.bin" % (name, k)))
        text = dict(haplotypes=[(n, int(w.bits(p)[0]), m) for n, p, m in haps],
                    em_info=[info["rounds"], info["iterations"], int(w.bits(info["log_likelihood"])[0])],
                    shapes={k: list(np.shape(v)) for k, v in arrays.items()})
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(text, f, sort_keys=True)
        print(tag, name, "reads", len(reads), "merged", meta.n_reads, "cands", len(meta.candidates()), "haps", len(haps), info, flush=True)
    masked_and_assigned(out, tag, metas["rsv"])


def dump(out, name, arrays, text):
    for k, v in arrays.items():
        np.ascontiguousarray(v).tofile(os.path.join(out, "%s.%s.bin" % (name, k)))
    text = dict(text, shapes={k: list(np.shape(v)) for k, v in arrays.items()})
    with open(os.path.join(out, name + ".json"), "w") as f:
        json.dump(text, f, sort_keys=True)


def masked_and_assigned(out, tag, meta):
    """the read family of tests/mask_checks.py under --mask-reads 1 and under --mask-seeds 2, the same family dealt into
    amplicons (tests/amplicon_checks.py) under --mask-reads-relative-frequency 0.05, and one --filter-and-assign run of the rsv
    reads of tests/assign_checks.py with the taxonomy of tests/taxa_checks.py and breadth: every array of each result"""
    import amplicon_checks as amp
    import assign_checks as ac
    import mask_checks as mc
    import taxa_checks as tc
    meta.set_dust(100.0)
    D = amp.family()
    for name, reads, masks, relative, groups in (("mask_reads1", mc.family().reads, (1, 0), (0.0, 0.0), None),
                                                 ("mask_seeds2", mc.family().reads, (0, 2), (0.0, 0.0), None),
                                                 ("amplicons_reads_rf005", D.reads, (0, 0), (0.05, 0.0), D.groups)):
        if groups is not None:
            meta.set_amplicons(groups, len(D.group_names))
        meta.set_masks(*masks)
        meta.set_relative_masks(*relative)
        try:
            meta.set_reads(reads)
        finally:
            meta.set_masks(0, 0)
            meta.set_relative_masks(0, 0)
            meta.set_amplicons(None)
        off, h, rev = meta.read_seedmers()
        ns, mult = meta.read_info()
        ch, cc = meta.mask_counts()
        arrays = dict(seedmer_off=off, seedmer_hash=h, seedmer_rev=rev, info_n=ns, info_mult=mult, raw_to_merged=meta.raw_to_merged(),
                      mask_count_hash=ch, mask_count=cc, oc_bits=_bits(meta.overlap_coefficients()))
        if groups is not None:
            g, gh, gc = meta.amplicon_counts()
            arrays.update(read_amplicons=meta.read_amplicons(), amplicon_count_group=g, amplicon_count_hash=gh, amplicon_count=gc,
                          **{"amplicon_" + k: v for k, v in meta.amplicon_info().items()})
        dump(out, name, arrays, dict(mask_info=meta.mask_info()))
        print(tag, name, "reads", len(reads), "merged", meta.n_reads, meta.mask_info(), flush=True)
    parent = meta.index_oriented.arrays()["parent"]
    meta.set_reads(ac.rsv_reads())
    meta.set_taxonomy(tc.label(parent, tc.RSV_T), 1)
    try:
        res = meta.assign(tc.RSV_DISCARD, breadth=True)
    finally:
        meta.set_taxonomy(max_taxa=0)
    arrays = dict(merged=res.merged, state=res.state, max=res.max, lca=res.lca, fastq_index=res.fastq_index, heads=res.heads, node_off=res._off,
                  nodes=res._nodes, read_n_taxa=res._read_taxa[0], read_taxa=res._read_taxa[1], breadth_total=res.breadth[0],
                  breadth_observed=res.breadth[1], breadth_depth=res.breadth[2])
    dump(out, "assign_taxa_breadth", arrays, {})
    print(tag, "assign_taxa_breadth", "reads", len(res.merged), "assigned", int((res.state == ac.ASSIGNED).sum()), "over", int((res.state == tc.OVER_TAXA).sum()), flush=True)


def _bits(x):
    return np.atleast_1d(np.asarray(x, np.float64)).copy().view(np.uint64)


if __name__ == "__main__":
    main()
