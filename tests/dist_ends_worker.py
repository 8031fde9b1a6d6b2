"""Worker of tests/test_meta_ends_dist_gpu.py: one rank of `--meta --mask-read-ends 5 --em-leaves-only` over several GPUs
through the C ABI.  As tests/dist_meta_worker.py (whose sample, cut, join and report it uses), with the two settings made on
both Metas: every rank trims its own shard, every rank chooses the candidates among the sampled genomes, and everything a
rank holds must equal the one-rank run over the whole sample bit for bit.  PMX_ENDS / PMX_LEAVES (defaults 5 and 1) set the
two; the one-rank Meta also runs on the reads trimmed in Python with the ends off, which must give the same again."""
import json
import os
import sys

import numpy as np

import dist_meta_worker as w


def configure(meta, ends, leaves):
    meta.set_mask_read_ends(ends)
    meta.set_em_leaves_only(leaves)


def main():
    rank, world = int(os.environ["PMX_RANK"]), int(os.environ["PMX_WORLD"])
    ends, leaves = int(os.environ.get("PMX_ENDS", "5")), bool(int(os.environ.get("PMX_LEAVES", "1")))
    case = os.environ.get("PMX_META_CASE", "rsv")
    import panmap_amd as pmx
    pm, reads, dust, discard = w.sample(pmx, case)
    ctx = pmx.Context(0)
    dist = w.join(pmx, ctx, rank, world)
    dist.barrier()
    meta = pmx.Meta.build(ctx, pm)
    meta.attach_dist(dist)
    configure(meta, ends, leaves)
    lo, hi = w.cut(case, len(reads), rank, world)
    haps = w.run(pmx, meta, reads[lo:hi], dust, discard)
    info = meta.em_info()
    first, count = meta.row_range()
    got_scores = meta.scores()
    # the same sample on one rank, no dist
    one = pmx.Meta(ctx, meta.index, meta.index_oriented)
    configure(one, ends, leaves)
    haps1 = w.run(pmx, one, reads, dust, discard)
    info1 = one.em_info()
    o_off, o_h, o_rev = one.read_seedmers()
    d_off, d_h, d_rev = meta.read_seedmers()
    o_ns, o_mult = one.read_info()
    d_ns, d_mult = meta.read_info()
    want_scores = one.scores()
    ids = [meta.index.node_id(int(v)) for v in meta.candidates()]
    out = dict(
        rank=rank, case=case, shard=[lo, hi], n_reads=meta.n_reads, n_reads_one=one.n_reads, row_range=[first, count],
        lists_equal=bool(np.array_equal(o_off, d_off) and np.array_equal(o_h, d_h) and np.array_equal(o_rev, d_rev)),
        info_equal=bool(np.array_equal(o_ns, d_ns) and np.array_equal(o_mult, d_mult)),
        oc_equal=bool(np.array_equal(w.bits(one.overlap_coefficients()), w.bits(meta.overlap_coefficients()))),
        candidates_equal=bool(np.array_equal(one.candidates(), meta.candidates())), n_candidates=int(len(meta.candidates())),
        n_sampled_candidates=sum(not x.startswith("node_") for x in ids),
        scores_shape=list(got_scores.shape),
        scores_equal=bool(got_scores.shape == (count, want_scores.shape[1]) and np.array_equal(got_scores, want_scores[first:first + count])),
        haplotypes_equal=[(n, int(w.bits(p)[0]), m) for n, p, m in haps] == [(n, int(w.bits(p)[0]), m) for n, p, m in haps1],
        n_haplotypes=len(haps),
        em_info_equal=info["rounds"] == info1["rounds"] and info["iterations"] == info1["iterations"]
        and int(w.bits(info["log_likelihood"])[0]) == int(w.bits(info1["log_likelihood"])[0]),
        em_info=info,
        top=[(meta.index.node_id(n), p) for n, p, _ in haps[:5]],
    )
    # ... and the one rank on the strings trimmed here, the ends off: the same merged reads and the same answer
    configure(one, 0, leaves)
    cut = [r[ends:len(r) - ends] if len(r) > 2 * ends else b"" for r in reads]
    haps2 = w.run(pmx, one, cut, dust, discard)
    c_off, c_h, c_rev = one.read_seedmers()
    out["trimmed_strings_equal"] = bool(np.array_equal(c_off, d_off) and np.array_equal(c_h, d_h) and np.array_equal(c_rev, d_rev) and
                                        [(n, int(w.bits(p)[0]), m) for n, p, m in haps2] == [(n, int(w.bits(p)[0]), m) for n, p, m in haps])
    # ... and the untrimmed sample is another one: the settings took effect
    configure(one, 0, False)
    w.run(pmx, one, reads, dust, discard)
    out["n_seedmers"], out["n_seedmers_untrimmed"] = int(len(d_h)), int(len(one.read_seedmers()[1]))
    out["n_candidates_all_nodes"] = int(len(one.candidates()))
    one.close()
    meta.close()
    dist.barrier()
    print("RESULT " + json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
