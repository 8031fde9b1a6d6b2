"""GPU parity of the align stage's distinct-pair map (align_pairs.hip readset_pair_map / k_pair_fanout): the compact tier and
the tail run one representative of every set of pairs with equal read records, and the copies take its results.  Every
case here is aligned with the map and without it (PMX_ALIGN_NO_DEDUP) and must come out equal by content: each record's
fields but its arena offset, and its CIGAR operations.  With the map, no two records may share arena words."""
import os

import numpy as np
import pytest

import align_checks as ac
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _map_at_any_depth(monkeypatch):
    """the map is used from 64 pairs per reference base by default; these sets are far shallower"""
    monkeypatch.setenv("PMX_ALIGN_DEDUP_DEPTH", "0")
    yield


FIELDS = ("rs", "re", "qs", "qe", "mapq", "rev", "proper_frag", "mapped", "n_cigar", "flags", "score")


def _ref_genome():
    return b"".join(l.strip() for l in open(os.path.join(GOLDEN, "isolate.ref.fa"), "rb") if not l.startswith(b">"))


def _pairs(pmx, genome, n, seed, **kw):
    concat, off = pmx.simulate_paired_reads(genome, n, seed=seed, **kw)
    reads = [bytes(concat[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    return [r if i % 2 == 0 else pmx.reverse_complement(r) for i, r in enumerate(reads)]


def _align(pmx, al, monkeypatch, dedup, revcomp_mate2=False, order_ahead=False, reads=None, concat=None, offsets=None):
    if dedup:
        monkeypatch.delenv("PMX_ALIGN_NO_DEDUP", raising=False)
        pmx.reload_options()
    else:
        monkeypatch.setenv("PMX_ALIGN_NO_DEDUP", "1")
    rs = pmx.ReadSet(al.ctx, reads) if reads is not None else pmx.ReadSet(al.ctx, concat=concat, offsets=offsets)
    if order_ahead:
        rs.order_pairs()     # the pair order and the map made on a side stream ahead of the align call
    al.align_readset(rs, paired=True, revcomp_mate2=revcomp_mate2)
    recs, cig = al.fetch()
    st = al.stats()
    rs.close()
    monkeypatch.delenv("PMX_ALIGN_NO_DEDUP", raising=False)
    pmx.reload_options()
    return recs, cig, st


def _content(recs, cig):
    fields = np.stack([recs[f].astype(np.int64) for f in FIELDS], axis=1)
    ops = [cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].tolist() for r in recs]
    return fields, ops


def _no_shared_words(recs):
    k = recs["n_cigar"].astype(np.int64)
    sel = k > 0
    off = recs["cigar_off"].astype(np.int64)[sel]
    k = k[sel]
    o = np.argsort(off, kind="stable")
    off, k = off[o], k[o]
    return bool(np.all(off[1:] >= off[:-1] + k[:-1]))


def _check_equal(pmx, al, monkeypatch, label, **kw):
    got = _align(pmx, al, monkeypatch, True, **kw)
    want = _align(pmx, al, monkeypatch, False, **kw)
    gf, go = _content(got[0], got[1])
    wf, wo = _content(want[0], want[1])
    assert gf.shape == wf.shape, label
    diff = np.nonzero(np.any(gf != wf, axis=1))[0]
    assert len(diff) == 0, (label, diff[:10], gf[diff[:3]], wf[diff[:3]])
    bad = [i for i in range(len(go)) if go[i] != wo[i]]
    assert not bad, (label, bad[:10])
    assert _no_shared_words(got[0]), label
    for k in ("n_items", "compact_tier_items"):
        assert got[2][k] == want[2][k], (label, k, got[2], want[2])
    return got


def test_dedup_bench_workload(pmx, sars, ctx, monkeypatch):
    """2M reads of the benchmark's generator against their source genome (a tenth of the pairs are copies), the
    map made by the align call itself and ahead of it on a side stream (pmx_readset_order_pairs: from a million pairs)"""
    from panmap_amd import synth
    src = sars.genome(synth.source_leaf_8d(np.array([sars.parent(i) if i else 0 for i in range(sars.num_nodes)]), 42))
    concat, off = synth.simulate_paired_reads_8d(src, 1 << 20)
    al = pmx.Aligner(ctx, src, 150)
    for ahead in (False, True):
        _check_equal(pmx, al, monkeypatch, "bench ahead=%s" % ahead, revcomp_mate2=True, order_ahead=ahead, concat=concat, offsets=off)
    al.close()


def test_dedup_example_reads(pmx, ctx, monkeypatch):
    g = _ref_genome()
    seqs, _, _ = pmx.read_fastq_paired(os.path.join(GOLDEN, "isolate_R1.fastq.gz"), os.path.join(GOLDEN, "isolate_R2.fastq.gz"))
    reads = seqs[:40000]
    al = pmx.Aligner(ctx, g, int(sum(len(r) for r in reads) / len(reads)))
    _check_equal(pmx, al, monkeypatch, "example", reads=reads)
    al.close()


def _crafted(pmx, g):
    base = _pairs(pmx, g, 3000, 71)
    noisy = _pairs(pmx, g, 600, 72, sub_rate=0.02)
    with_n = [r if i % 3 else r[:40] + b"NN" + r[42:] for i, r in enumerate(_pairs(pmx, g, 900, 73))]
    reads = list(base) + list(noisy) + list(with_n)
    for i in range(0, 600, 2):                       # five copies of some pairs, spread over the set
        reads += [reads[i], reads[i + 1]] * 4
    for i in range(len(base) + len(noisy), len(base) + len(noisy) + 600, 2):   # copies of pairs with an `N` (tail pairs)
        reads += [reads[i], reads[i + 1]] * 3
    for i in range(0, 200, 2):                       # pairs whose two mates are equal, twice each
        reads += [reads[i], reads[i]] * 2
    for i in range(200, 400, 2):                     # a read as mate 1 of one pair and mate 2 of another
        reads += [reads[i + 1], reads[i + 1], reads[i + 3], reads[i]]
    rng = np.random.default_rng(5)
    pairs = [(reads[2 * i], reads[2 * i + 1]) for i in range(len(reads) // 2)]
    order = rng.permutation(len(pairs))
    out = []
    for j in order:
        out += list(pairs[j])
    return out


def test_dedup_crafted(pmx, ctx, monkeypatch):
    g = _ref_genome()
    reads = _crafted(pmx, g)
    al = pmx.Aligner(ctx, g, 150)
    for n in (len(reads), len(reads) - 1, 2, 3, 129):   # odd counts: the trailing read is not aligned
        got = _check_equal(pmx, al, monkeypatch, "crafted n=%d" % n, reads=reads[:n])
        assert len(got[0]) == n
    al.close()


def test_dedup_arena_overflow(pmx, ctx, monkeypatch):
    """an arena far too small: the call is redone (without the map when a copy's representative overflowed) and the records
    come out equal, none flagged"""
    g = _ref_genome()
    reads = _crafted(pmx, g)
    al = pmx.Aligner(ctx, g, 150)
    monkeypatch.setenv("PMX_ALIGN_CIGAR_CAP", "64")
    got = _check_equal(pmx, al, monkeypatch, "overflow", reads=reads)
    assert not np.any(got[0]["flags"] & 1)
    al.close()


def test_dedup_edit_scores(pmx, ctx, monkeypatch):
    """score_reads (the edit counts --refine sums) with and without the map"""
    g = _ref_genome()
    reads = _crafted(pmx, g)
    al = pmx.Aligner(ctx, g, 150)
    rs = pmx.ReadSet(ctx, reads)
    with_map = al.score_reads(rs, True, False)
    monkeypatch.setenv("PMX_ALIGN_NO_DEDUP", "1")
    without = al.score_reads(rs, True, False)
    monkeypatch.delenv("PMX_ALIGN_NO_DEDUP", raising=False)
    rs.close()
    al.close()
    assert with_map == without


def test_dedup_direct_boundary(pmx, oracle, monkeypatch):
    """pmx_align_reads_direct (the reference's C-ABI boundary) with and without the map, and against the reference"""
    g = _ref_genome()
    reads = _crafted(pmx, g)[:6000]
    got = pmx.align_reads_direct(g, reads, True)
    monkeypatch.setenv("PMX_ALIGN_NO_DEDUP", "1")
    plain = pmx.align_reads_direct(g, reads, True)
    monkeypatch.delenv("PMX_ALIGN_NO_DEDUP", raising=False)
    assert got == plain
    want = oracle.ref_align_reads_direct(g, reads, True, 8)
    bad = ac.compare_results(got, want)
    assert not bad, bad[:5]
