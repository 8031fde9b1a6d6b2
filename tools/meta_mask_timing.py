#!/usr/bin/env python3
"""Timings of --meta's low-coverage masks (pmx_meta_set_masks, csrc/meta_mask.hip) on the two samples of
tests/dist_meta_worker.py: `rsv` (the 70 / 30 mixture, 1,000 reads) and `sars` (30,000 reads of five haplotypes + 200
low-complexity reads).
  meta_mask_timing.py mask [runs]   per sample: the "meta_mask" span (device events) and the wall time of set_reads under
                                    mask_seeds 1, `runs` times after one warm-up; the share of merged reads on the sorted path
  meta_mask_timing.py wall [runs]   per sample: the wall time of set_reads with the masks OFF, `runs` times after one warm-up
                                    (works on a build without the masks too: run it once per build, PMX_LIB_PATH picks the build)
  --amplicons G (mask mode)         deal the reads round-robin into G amplicons (pmx_meta_set_amplicons, no read unlisted): the
                                    same spans with the (amplicon, hash) count key, plus "meta_mask_sort", the sort of the keys
One JSON line per sample."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import panmap_amd as pmx
    from dist_meta_worker import sample
    argv = sys.argv[1:]
    n_amplicons = 0
    if "--amplicons" in argv:
        at = argv.index("--amplicons")
        n_amplicons = int(argv[at + 1])
        del argv[at:at + 2]
    mode = argv[0] if len(argv) > 0 else "mask"
    runs = int(argv[1]) if len(argv) > 1 else 3
    ctx = pmx.Context(0)
    for case in ("rsv", "sars"):
        pm, reads, _, _ = sample(pmx, case)
        concat, offsets = pmx.concat_reads(reads)
        concat = np.frombuffer(concat, np.uint8)
        meta = pmx.Meta.build(ctx, pm)

        def set_reads():
            t0 = time.perf_counter()
            meta.set_reads(concat=concat, offsets=offsets)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        out = dict(mode=mode, case=case, lib=os.path.basename(os.path.dirname(pmx.LIB_PATH)), reads=len(reads))
        set_reads()                                                   # warm-up: code objects, buffers, rocprim's choices
        if mode == "mask":
            ns, _ = meta.read_info()
            out.update(merged_reads=int(len(ns)), seedmers=int(ns.sum()), share_on_sorted_path=float((ns > 1024).mean()))
            meta.set_masks(seeds=1)
            if n_amplicons > 0:
                meta.set_amplicons(np.arange(len(reads), dtype=np.int32) % n_amplicons, n_amplicons)
                out.update(amplicons=n_amplicons)
            set_reads()
            span, wall, sort = [], [], []
            for _ in range(runs):
                wall.append(set_reads())
                span.append(ctx.kernel_ms("meta_mask"))
                sort.append(ctx.kernel_ms("meta_mask_sort"))
            out.update(mask_info=meta.mask_info(), meta_mask_ms=span, meta_mask_ms_median=statistics.median(span), set_reads_ms=wall,
                       set_reads_ms_median=statistics.median(wall))
            if n_amplicons > 0:
                out.update(merged_reads_in_amplicons=int(meta.amplicon_info()["merged_before"].sum()), meta_mask_sort_ms=sort,
                           meta_mask_sort_ms_median=statistics.median(sort))
        else:
            wall = [set_reads() for _ in range(runs)]
            out.update(merged_reads=meta.n_reads, set_reads_ms=wall, set_reads_ms_median=statistics.median(wall))
        meta.close()
        print(json.dumps(out))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
