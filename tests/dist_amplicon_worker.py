"""Worker of tests/test_meta_amplicon_dist_gpu.py: one rank of `--meta --amplicon-depth` with a mask over several GPUs through
the C ABI.  Launched like tests/dist_mask_worker.py (PMX_RANK / PMX_WORLD, the host-directory transport).  Every rank passes
the amplicons of ITS shard, runs the collective calls, then the whole sample through a Meta without a dist under the same
setting, and reports whether everything it holds equals that run bit for bit.  PMX_AMP_SETTING: the four masking parameters,
comma-separated.  PMX_AMP_GROUPS_OFF=<rank>: that rank claims one group more than the others (the refusal).

The sample: the 70 / 30 rsv mixture, 50 consecutive reads an amplicon (every 7th read unlisted), plus 40 reads with two
substitutions each as one more amplicon.  Rank 0 takes reads [0, 525): amplicons 0..9 lie entirely on it, amplicon 10 (reads
500..549) is split across both ranks."""
import json
import os
import sys

import numpy as np

from dist_meta_worker import bits, join, sample

CUT = 525


def dealt(pmx):
    pm, reads, _, _ = sample(pmx, "rsv")
    rng = np.random.default_rng(70)
    planted = []
    for r in reads[::25]:
        q = bytearray(r)
        for p in rng.choice(len(q), 2, replace=False):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4] if q[p] in b"ACGT" else q[p]
        planted.append(bytes(q))
    n_groups = len(reads) // 50 + 1
    groups = [n_groups if i % 7 == 3 else i // 50 for i in range(len(reads))] + [n_groups - 1] * len(planted)
    return pm, reads + planted, np.array(groups, np.int32), n_groups


def run(meta, reads, groups, n_groups, setting):
    meta.set_amplicons(groups, n_groups)
    meta.set_masks(int(setting[0]), int(setting[1]))
    meta.set_relative_masks(setting[2], setting[3])
    meta.set_reads(reads)
    meta.score(top_oc=1000)
    return meta.em()


def same(a, b):
    return bool(all(np.array_equal(x, y) for x, y in zip(a, b)))


def main():
    rank, world = int(os.environ["PMX_RANK"]), int(os.environ["PMX_WORLD"])
    setting = [float(x) for x in os.environ["PMX_AMP_SETTING"].split(",")]
    import panmap_amd as pmx
    pm, reads, groups, n_groups = dealt(pmx)
    ctx = pmx.Context(0)
    dist = join(pmx, ctx, rank, world)
    dist.barrier()
    meta = pmx.Meta.build(ctx, pm)
    meta.attach_dist(dist)
    lo, hi = (0, CUT) if rank == 0 else (CUT, len(reads))
    if os.environ.get("PMX_AMP_GROUPS_OFF") is not None:               # the ranks disagree: every rank must come back with an error
        mine = n_groups + (1 if int(os.environ["PMX_AMP_GROUPS_OFF"]) == rank else 0)
        try:
            run(meta, reads[lo:hi], groups[lo:hi], mine, setting)
            refused = ""
        except pmx.PmxError as e:
            refused = str(e)
        print("RESULT " + json.dumps(dict(rank=rank, refused=refused)))
        sys.stdout.flush()
        return
    haps = run(meta, reads[lo:hi], groups[lo:hi], n_groups, setting)
    info = meta.em_info()
    first, count = meta.row_range()
    got_scores = meta.scores()
    one = pmx.Meta(ctx, meta.index, meta.index_oriented)
    haps1 = run(one, reads, groups, n_groups, setting)
    info1 = one.em_info()
    want_scores = one.scores()
    a_info, a_info1 = meta.amplicon_info(), one.amplicon_info()
    out = dict(
        rank=rank, n_reads=meta.n_reads, n_reads_one=one.n_reads, row_range=[first, count],
        lists_equal=same(meta.read_seedmers(), one.read_seedmers()), info_equal=same(meta.read_info(), one.read_info()),
        amplicons_equal=same([meta.read_amplicons()], [one.read_amplicons()]),
        triples_equal=same(meta.amplicon_counts(), one.amplicon_counts()), counts_equal=same(meta.mask_counts(), one.mask_counts()),
        amplicon_info_equal=same([a_info[k] for k in sorted(a_info)], [a_info1[k] for k in sorted(a_info1)]),
        mask_info_equal=meta.mask_info() == one.mask_info(), mask_info=meta.mask_info(),
        raw_reads=a_info["raw_reads"].tolist(), threshold=a_info["threshold"].tolist(), merged_before=a_info["merged_before"].tolist(),
        merged_left=a_info["merged_left"].tolist(),
        oc_equal=bool(np.array_equal(bits(one.overlap_coefficients()), bits(meta.overlap_coefficients()))),
        candidates_equal=bool(np.array_equal(one.candidates(), meta.candidates())),
        scores_shape=list(got_scores.shape),
        scores_equal=bool(got_scores.shape == (count, want_scores.shape[1]) and np.array_equal(got_scores, want_scores[first:first + count])),
        haplotypes_equal=[(n, int(bits(p)[0]), m) for n, p, m in haps] == [(n, int(bits(p)[0]), m) for n, p, m in haps1],
        n_haplotypes=len(haps),
        em_info_equal=info["rounds"] == info1["rounds"] and info["iterations"] == info1["iterations"]
        and int(bits(info["log_likelihood"])[0]) == int(bits(info1["log_likelihood"])[0]),
        em_info=info, top=[(meta.index.node_id(n), p) for n, p, _ in haps[:5]],
    )
    one.close()
    meta.close()
    dist.barrier()
    print("RESULT " + json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
