#!/usr/bin/env python3
"""Every output of the --meta stage for three runs, one file per output under the directory argv[1]: the rsv 70 / 30 sample
without --dust and with --dust 20, and the `sars` sample of tests/dist_meta_worker.py (--dust 20 --discard 0.5).  Doubles go
out as bit patterns.  To compare two builds of the library, run it once per build, each selected with PMX_LIB_PATH, and
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


if __name__ == "__main__":
    main()
