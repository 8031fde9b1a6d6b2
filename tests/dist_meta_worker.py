"""Worker of tests/test_meta_dist_gpu.py: one rank of `--meta` over several GPUs THROUGH THE C ABI (pmx_meta_attach_dist).
Launched once per rank as a plain subprocess (PMX_RANK / PMX_WORLD in the environment; two ranks share the one GPU of a box over
the library's host-directory test transport, PMX_DIST_HOST_DIR; with PMX_WORLD=1 and no directory the rank runs on a one-rank
RCCL group).  Every rank runs the collective calls on ITS shard of the sample, then the same sample through a Meta without a
dist, and reports whether everything it holds equals that run bit for bit.  PMX_META_CASE picks the sample and the cut:
  rsv     the 70 / 30 mixture of tests/test_meta_gpu.py (700 + 300 reads of rsv_4K), cut in two halves -- under 1,024 EM
          rows, so rank 1 owns no EM row and still joins every collective
  shards  the same mixture cut 70 / 30
  empty   the same mixture, rank 1 holds no read at all
  sars    30,000 reads of a five-haplotype SARS-CoV-2 mixture plus 200 low-complexity reads, --dust 20 --discard 0.5"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fasta(path):
    return "".join(l.strip() for l in open(path) if not l.startswith(">")).upper()


def _tile(g, n, L=150):
    step = max(1, (len(g) - L) // n)
    out, c, i = [], 0, 0
    while c < n and i + L <= len(g):
        out.append(g[i:i + L].encode())
        c += 1
        i += step
    return out


def sample(pmx, case):
    """-> (panman, reads as a list of bytes, dust threshold, discard)"""
    if case == "sars":
        pm = pmx.Panman(os.path.join(GOLDEN, "sars_20000_twilight_dipper.panman"))
        names = [l.split("\t")[0] for l in open(os.path.join(GOLDEN, "example.mgsr.abundance.out"))][:5]
        reads = []
        for i, (nm, sh) in enumerate(zip(names, [0.50, 0.20, 0.15, 0.10, 0.05])):
            c, o = pmx.simulate_paired_reads(pm.genome(pm.find_node(nm)), int(30000 * sh) // 2, seed=10 + i)
            c = np.asarray(c, np.uint8)
            reads += [bytes(c[o[k]:o[k + 1]]) for k in range(len(o) - 1)]
        for i in range(100):
            reads += [b"A" * 150, b"AC" * 75]
        return pm, reads, 20.0, 0.5
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    a, b = _fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    return pm, _tile(a, 700) + _tile(b, 300), 100.0, 0.0


def cut(case, n, rank, world):
    if case == "shards":
        c = n * 7 // 10
        return (0, c) if rank == 0 else (c, n)
    if case == "empty":
        return (0, n) if rank == 0 else (n, n)
    return n * rank // world, n * (rank + 1) // world


def join(pmx, ctx, rank, world):
    host_dir = os.environ.get("PMX_DIST_HOST_DIR")
    if world > 1:
        assert host_dir, "two ranks on one GPU: set PMX_DIST_HOST_DIR"
        uid_file = os.path.join(host_dir, "uid.meta")
        if rank == 0:
            uid = pmx.Dist.unique_id()
            with open(uid_file + ".part", "wb") as f:
                f.write(uid)
            os.rename(uid_file + ".part", uid_file)
        else:
            t0 = time.time()
            while not os.path.exists(uid_file):
                assert time.time() - t0 < 300, "rank 0 never published the id"
                time.sleep(0.01)
            uid = open(uid_file, "rb").read()
    else:
        uid = pmx.Dist.unique_id()
    return pmx.Dist(ctx, uid, rank, world)


def bits(x):
    """doubles as their bit patterns"""
    return np.atleast_1d(np.asarray(x, np.float64)).copy().view(np.uint64)


def run(pmx, meta, reads, dust, discard):
    from panmap_amd import _lib
    meta.set_dust(dust)
    meta.set_reads(reads)
    meta.score(top_oc=1000)
    haps = meta.em(_lib.MetaParams(discard=discard))
    return haps


def main():
    rank, world = int(os.environ["PMX_RANK"]), int(os.environ["PMX_WORLD"])
    case = os.environ.get("PMX_META_CASE", "rsv")
    import panmap_amd as pmx
    pm, reads, dust, discard = sample(pmx, case)
    ctx = pmx.Context(0)
    dist = join(pmx, ctx, rank, world)
    dist.barrier()
    meta = pmx.Meta.build(ctx, pm)
    meta.attach_dist(dist)
    lo, hi = cut(case, len(reads), rank, world)
    haps = run(pmx, meta, reads[lo:hi], dust, discard)
    info = meta.em_info()
    first, count = meta.row_range()
    got_scores = meta.scores()
    # the same sample on one rank, no dist
    one = pmx.Meta(ctx, meta.index, meta.index_oriented)
    haps1 = run(pmx, one, reads, dust, discard)
    info1 = one.em_info()
    o_off, o_h, o_rev = one.read_seedmers()
    d_off, d_h, d_rev = meta.read_seedmers()
    o_ns, o_mult = one.read_info()
    d_ns, d_mult = meta.read_info()
    want_scores = one.scores()
    out = dict(
        rank=rank, case=case, shard=[lo, hi], n_reads=meta.n_reads, n_reads_one=one.n_reads, row_range=[first, count],
        lists_equal=bool(np.array_equal(o_off, d_off) and np.array_equal(o_h, d_h) and np.array_equal(o_rev, d_rev)),
        info_equal=bool(np.array_equal(o_ns, d_ns) and np.array_equal(o_mult, d_mult)),
        multiplicity_total=int(d_mult.sum()),
        oc_equal=bool(np.array_equal(bits(one.overlap_coefficients()), bits(meta.overlap_coefficients()))),
        candidates_equal=bool(np.array_equal(one.candidates(), meta.candidates())), n_candidates=int(len(meta.candidates())),
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
