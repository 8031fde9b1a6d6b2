"""Worker of tests/test_meta_mask_dist_gpu.py: one rank of `--meta --mask-reads / --mask-seeds` over several GPUs through the C
ABI.  Launched like tests/dist_meta_worker.py (PMX_RANK / PMX_WORLD, the host-directory transport) and built from its pieces.
Every rank sets the same masks, runs the collective calls on ITS shard, then the whole sample through a Meta without a dist
under the same masks, and reports whether everything it holds equals that run bit for bit.  PMX_META_CASE: `rsv` or `shards`
(the cuts of dist_meta_worker.py); PMX_MASK_READS / PMX_MASK_SEEDS: the thresholds."""
import json
import os
import sys

import numpy as np

from dist_meta_worker import bits, cut, join, sample


def run(meta, reads, mask_reads, mask_seeds):
    meta.set_masks(mask_reads, mask_seeds)
    meta.set_reads(reads)
    meta.score(top_oc=1000)
    return meta.em()


def main():
    rank, world = int(os.environ["PMX_RANK"]), int(os.environ["PMX_WORLD"])
    case = os.environ.get("PMX_META_CASE", "rsv")
    mask_reads, mask_seeds = int(os.environ.get("PMX_MASK_READS", "0")), int(os.environ.get("PMX_MASK_SEEDS", "0"))
    import panmap_amd as pmx
    pm, reads, _, _ = sample(pmx, case)
    ctx = pmx.Context(0)
    dist = join(pmx, ctx, rank, world)
    dist.barrier()
    meta = pmx.Meta.build(ctx, pm)
    meta.attach_dist(dist)
    lo, hi = cut(case, len(reads), rank, world)
    haps = run(meta, reads[lo:hi], mask_reads, mask_seeds)
    info = meta.em_info()
    first, count = meta.row_range()
    got_scores = meta.scores()
    # the same sample on one rank, no dist, the same masks -- and without them, to see that the masks did something
    one = pmx.Meta(ctx, meta.index, meta.index_oriented)
    haps1 = run(one, reads, mask_reads, mask_seeds)
    info1 = one.em_info()
    o_off, o_h, o_rev = one.read_seedmers()
    d_off, d_h, d_rev = meta.read_seedmers()
    o_ns, o_mult = one.read_info()
    d_ns, d_mult = meta.read_info()
    want_scores = one.scores()
    o_ch, o_cc = one.mask_counts()
    d_ch, d_cc = meta.mask_counts()
    mask_info, mask_info1 = meta.mask_info(), one.mask_info()
    oc, oc1 = meta.overlap_coefficients(), one.overlap_coefficients()
    cands, cands1 = meta.candidates(), one.candidates()
    run(one, reads, 0, 0)
    out = dict(
        rank=rank, case=case, shard=[lo, hi], n_reads=meta.n_reads, n_reads_one=len(o_mult), n_seedmers=int(len(d_h)), row_range=[first, count],
        n_reads_unmasked=one.n_reads, n_seedmers_unmasked=int(len(one.read_seedmers()[1])),
        lists_equal=bool(np.array_equal(o_off, d_off) and np.array_equal(o_h, d_h) and np.array_equal(o_rev, d_rev)),
        info_equal=bool(np.array_equal(o_ns, d_ns) and np.array_equal(o_mult, d_mult)),
        counts_equal=bool(np.array_equal(o_ch, d_ch) and np.array_equal(o_cc, d_cc)),
        mask_info_equal=mask_info == mask_info1, mask_info=mask_info,
        oc_equal=bool(np.array_equal(bits(oc1), bits(oc))),
        candidates_equal=bool(np.array_equal(cands1, cands)), n_candidates=int(len(cands)),
        scores_shape=list(got_scores.shape),
        scores_equal=bool(got_scores.shape == (count, want_scores.shape[1]) and np.array_equal(got_scores, want_scores[first:first + count])),
        haplotypes_equal=[(n, int(bits(p)[0]), m) for n, p, m in haps] == [(n, int(bits(p)[0]), m) for n, p, m in haps1],
        n_haplotypes=len(haps),
        em_info_equal=info["rounds"] == info1["rounds"] and info["iterations"] == info1["iterations"]
        and int(bits(info["log_likelihood"])[0]) == int(bits(info1["log_likelihood"])[0]),
        em_info=info,
        top=[(meta.index.node_id(n), p) for n, p, _ in haps[:5]],
    )
    one.close()
    meta.close()
    dist.barrier()
    print("RESULT " + json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
