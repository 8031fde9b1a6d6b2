"""Placement against homopolymer-compressed (HPC) indexes on the device.  The ground truth is the existing oracle run on reads
compressed in Python (tests/hpc_checks.py) -- the reference's own order of operations (src/placement.cpp:1143-1165 compresses
every read before anything else).  Every comparison is exact: bytes, integers, uint64 views of doubles."""
import os

import numpy as np
import pytest

import hpc_checks as hc
from conftest import GOLDEN
from place_tree_checks import assert_place_matches

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -7


def _as_reads(concat, off):
    return [bytes(concat[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def families():
    return hc.all_families()


@pytest.fixture(scope="module")
def sim_reads(pmx, sars):
    concat, off = pmx.simulate_paired_reads(sars.genome("node_5"), 1500, seed=3)
    return _as_reads(concat, off)


def _assert_compressed(got, reads, quals=None):
    concat, off, q = got
    if quals is None:
        want_r, want_q = hc.hpc_reads(reads), None
    else:
        want_r, want_q = hc.hpc_reads(reads, quals)
    want_off = np.cumsum([0] + [len(r) for r in want_r]).astype(np.int64)
    assert np.array_equal(off, want_off), "offsets differ"
    assert concat == b"".join(want_r), "bases differ"
    assert q == (None if want_q is None else b"".join(want_q)), "qualities differ"


# ---------------------------------------------------------------------------------------------- 1. compress, byte for byte
def test_compress_byte_for_byte(pmx, ctx, families):
    rs = pmx.ReadSet(ctx, families)
    c = rs.hpc_compress()
    assert c.is_hpc and not rs.is_hpc and c.n_reads == len(families)
    _assert_compressed(c.export(), families)
    assert ctx.kernel_ms("hpc") > 0
    # the source is untouched
    raw = rs.export()
    assert raw[0] == b"".join(families) and raw[2] is None
    # qualities follow in lockstep: the first base of a run gives the run's quality
    quals = hc.random_quals(np.random.default_rng(3), families)
    rs.set_qualities(quals)
    _assert_compressed(rs.hpc_compress(pack=False).export(), families, quals)
    # an empty read set, and a set of empty reads
    assert pmx.ReadSet(ctx, []).hpc_compress().export()[0] == b""
    _assert_compressed(pmx.ReadSet(ctx, [b"", b""]).hpc_compress().export(), [b"", b""])
    with pytest.raises(pmx.PmxError) as e:
        c.hpc_compress()
    assert e.value.code == ERR_ARG


def test_compress_a_wrapped_slice_and_reuse_the_target(pmx, ctx, families):
    import torch
    dev = torch.device("cuda", 0)
    concat, off = pmx.concat_reads(families)
    d_c = torch.from_numpy(np.frombuffer(concat, np.uint8).copy()).to(dev)
    d_o = torch.from_numpy(off).to(dev)
    n = len(families)
    r0, r1 = n // 3 + 1, n - 7
    assert off[r0] > 0 and off[r0] % 16 != 0
    # a slice [r0, r1] of the offsets array: its reads start at off[r0] of the same buffer
    sl = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr() + 8 * r0, r1 - r0, len(concat), 0, keepalive=(d_c, d_o))
    out = sl.hpc_compress()
    _assert_compressed(out.export(), families[r0:r1])
    raw = sl.export()
    assert raw[0] == b"".join(families[r0:r1]) and raw[1][0] == 0
    # the same target again with a smaller batch, then with a larger one
    small = pmx.ReadSet(ctx, families[5:400])
    again = small.hpc_compress(out=out)
    assert again is out and out.n_reads == 395
    _assert_compressed(out.export(), families[5:400])
    pmx.ReadSet(ctx, families).hpc_compress(out=out)
    _assert_compressed(out.export(), families)
    # a target whose buffers were wrapped is given buffers of its own: the wrapped ones are not written
    sl.rewrap_device(d_c.data_ptr(), d_o.data_ptr(), n, len(concat), 0, keepalive=(d_c, d_o))
    small.hpc_compress(out=sl)
    assert sl.is_hpc
    _assert_compressed(sl.export(), families[5:400])
    assert d_c.cpu().numpy().tobytes() == concat and np.array_equal(d_o.cpu().numpy(), off)
    # a call that fails leaves the target as it was: a wrapped target keeps the buffers it points at alive
    w = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), n, len(concat), 0, keepalive=(d_c, d_o))
    with pytest.raises(pmx.PmxError):
        out.hpc_compress(out=w)            # (the source is compressed already)
    assert w._keep == (d_c, d_o) and not w.is_hpc and w.export()[0] == concat


# ---------------------------------------------------------------------------------------------- 2. placement, bit-exact
def _place(pmx, ctx, index, reads, form, params, quals=None):
    """the placer after seeding `reads` in one of three forms: 'plain' (the placer compresses), 'compressed' (the caller does),
    'ranges' (add_reads_range of the plain set in three ranges)"""
    placer = pmx.Placer(ctx, index)
    placer.reset()
    rs = pmx.ReadSet(ctx, reads, pack=False)
    if quals is not None:
        rs.set_qualities(quals)
    if form == "plain":
        placer.add_reads(rs, params)
    elif form == "compressed":
        placer.add_reads(rs.hpc_compress(), params)
    else:
        n = len(reads)
        for a, b in ((0, n // 5), (n // 5, n // 5), (n // 5, n - 3), (n - 3, n)):
            placer.add_reads_range(rs, a, b, params)
    return placer


def _check_hpc_place(pmx, oracle, ctx, index, reads, forms, params=None, k=19, s=8, l=3, open_=False, t=0, quals=None):
    params = params or pmx.TraversalParams()
    if quals is None:
        creads, cquals = hc.hpc_reads(reads), None
    else:
        creads, cquals = hc.hpc_reads(reads, quals)
    want = oracle.place(creads, index.arrays(), k, s, l, open_, t, params.trimStart, params.trimEnd, params.seedMaskFraction,
                        params.minReadSupport, params.forceLeaf, params.dedupReads, cquals, params.minSeedQuality)
    assert len(want["hist_hash"]) > 100
    for form in forms:
        placer = _place(pmx, ctx, index, reads, form, params, quals)
        res = placer.score(params, len(reads))
        assert_place_matches(placer, res, want)
        placer.close()
    return want


@pytest.mark.parametrize("k,s,l,open_,t", [(19, 8, 3, False, 0), (15, 8, 1, False, 0), (19, 8, 2, True, 3)])
def test_place_hpc_bit_exact(pmx, oracle, ctx, sars, sim_reads, families, k, s, l, open_, t):
    """(19, 8, 3): the specialised kernel behind the read collapse when the compressed reads are short; (15, 8, 1) and the
    open-syncmer row: the generic kernel"""
    index = hc.hpc_index(oracle, sars.genome("node_5"), k, s, l, open_, t)
    reads = sim_reads + families
    want = _check_hpc_place(pmx, oracle, ctx, index, reads, ("plain", "compressed", "ranges"), None, k, s, l, open_, t)
    # the compression matters on these reads: the uncompressed reads seed differently
    hs, _ = oracle.histogram(reads, k, s, l, open_, t)
    assert not np.array_equal(hs, want["hist_hash"])


def test_place_hpc_short_reads_take_the_collapse_path(pmx, oracle, ctx, sars, sim_reads, families):
    """every compressed read is at most 160 bases: the derived set has records and k_collapse_reads runs on it"""
    index = hc.hpc_index(oracle, sars.genome("node_5"), 19, 8, 3, False, 0)
    reads = sim_reads + [r for r in families if len(r) <= 160]
    assert max(len(r) for r in hc.hpc_reads(reads)) <= 160
    _check_hpc_place(pmx, oracle, ctx, index, reads, ("plain", "compressed"))


def test_place_hpc_trims(pmx, oracle, ctx, sars, sim_reads, families):
    index = hc.hpc_index(oracle, sars.genome("node_5"), 19, 8, 3, False, 0)
    _check_hpc_place(pmx, oracle, ctx, index, sim_reads + families, ("plain", "compressed"), pmx.TraversalParams(trimStart=10, trimEnd=25))


def test_place_hpc_dedup_sees_the_compressed_reads(pmx, oracle, ctx, sars, sim_reads):
    index = hc.hpc_index(oracle, sars.genome("node_5"), 19, 8, 3, False, 0)
    rng = np.random.default_rng(9)
    twins = [hc.run_length_errors(rng, r, 0.5) for r in sim_reads[:800]]     # differ from their originals in run lengths only
    assert sum(a != b for a, b in zip(twins, sim_reads)) > 700
    reads = sim_reads + twins + sim_reads[:100]
    reads = [reads[int(i)] for i in rng.permutation(len(reads))]
    params = pmx.TraversalParams(dedupReads=True)
    want = _check_hpc_place(pmx, oracle, ctx, index, reads, ("plain", "compressed"), params)
    # a dedup over the raw bytes would count the twins twice
    raw_dedup = oracle.histogram(hc.hpc_reads(list(set(reads))), 19, 8, 3)
    assert not np.array_equal(raw_dedup[1], want["hist_count"])


def test_place_hpc_min_seed_quality(pmx, oracle, ctx, sars, sim_reads, families):
    index = hc.hpc_index(oracle, sars.genome("node_5"), 19, 8, 3, False, 0)
    reads = sim_reads + families[:600]
    rng = np.random.default_rng(12)
    quals = []
    for r in reads:
        q = rng.integers(2, 41, len(r)).astype(np.uint8) + 33
        if rng.random() < 0.5:
            q[:] = 73
        lo = int(rng.integers(0, max(1, len(r) - 30)))
        q[lo:lo + int(rng.integers(5, 40))] = 35
        quals.append(q.tobytes())
    _check_hpc_place(pmx, oracle, ctx, index, reads, ("plain", "compressed"), pmx.TraversalParams(minSeedQuality=20), quals=quals)


def test_place_hpc_long_reads_only(pmx, oracle, ctx, sars):
    """more than 160 bases after compression: no records, no collapse"""
    g = sars.genome("node_5")
    index = hc.hpc_index(oracle, g, 19, 8, 3, False, 0)
    rng = np.random.default_rng(21)
    reads = []
    for _ in range(300):
        n = int(rng.integers(400, 3000))
        st = int(rng.integers(0, len(g) - n))
        reads.append(hc.run_length_errors(rng, g[st:st + n]))
    assert min(len(r) for r in hc.hpc_reads(reads)) > 160
    _check_hpc_place(pmx, oracle, ctx, index, reads, ("plain", "compressed", "ranges"))


# ---------------------------------------------------------------------------------------------- 3. error cases
def test_mismatched_sets_and_indexes_are_refused(pmx, oracle, ctx, sars, sars_index, sim_reads):
    from panmap_amd._lib import lib
    g = sars.genome("node_5")
    rs = pmx.ReadSet(ctx, sim_reads[:200])
    comp = rs.hpc_compress()
    # a placer without HPC and a compressed set
    plain_placer = pmx.Placer(ctx, sars_index)
    with pytest.raises(pmx.PmxError) as e:
        plain_placer.add_reads(comp)
    assert e.value.code == ERR_ARG and "uncompressed read set" in str(e.value)
    with pytest.raises(pmx.PmxError) as e:
        plain_placer.add_reads_range(comp, 0, 10)
    assert e.value.code == ERR_ARG
    # the aligner and a compressed set
    al = pmx.Aligner(ctx, g, 150)
    with pytest.raises(pmx.PmxError) as e:
        al.align_readset(comp, True, True)
    assert e.value.code == ERR_ARG and "uncompressed reads" in str(e.value)
    # ... and what else works for the align and genotype stages: the pair order, and the pileup of an alignment of the raw set
    with pytest.raises(pmx.PmxError) as e:
        comp.order_pairs()
    assert e.value.code == ERR_ARG and "uncompressed read set" in str(e.value)
    al.align_readset(rs, True, True)
    pu = pmx.Pileup(ctx)
    with pytest.raises(pmx.PmxError) as e:
        pu.run(al, comp, len(g), True, True)
    assert e.value.code == ERR_ARG and "uncompressed read set" in str(e.value)
    pu.run(al, rs, len(g), True, True)
    # the dedup building blocks of an HPC placer hash the read bytes: a plain set is refused, the message says what to do
    hpc_placer = pmx.Placer(ctx, hc.hpc_index(oracle, g, 19, 8, 3, False, 0))
    assert lib.pmx_place_dedup_local(ctx._h, hpc_placer._h, rs._h, None, None, 0) == ERR_ARG
    assert b"compress first" in pmx.last_error() and b"pmx_readset_hpc_compress" in pmx.last_error()
    assert lib.pmx_place_dedup_local_count(ctx._h, hpc_placer._h, rs._h) == ERR_ARG
    assert lib.pmx_place_dedup_drop_seen(ctx._h, hpc_placer._h, rs._h, None, None, 0) == ERR_ARG
    # ... and the compressed set is taken: as many reads kept as there are distinct compressed reads
    assert lib.pmx_place_dedup_local(ctx._h, hpc_placer._h, comp._h, None, None, 0) == len(set(hc.hpc_reads(sim_reads[:200])))
    assert lib.pmx_place_dedup_local(ctx._h, plain_placer._h, comp._h, None, None, 0) == ERR_ARG


# ---------------------------------------------------------------------------------------------- 4. the raw reads stay raw
def test_aligning_the_plain_set_after_hpc_placement_is_unchanged(pmx, oracle, ctx, sars, sim_reads):
    g = sars.genome("node_5")
    reads = sim_reads[:1000]    # 500 pairs
    al = pmx.Aligner(ctx, g, 150)
    fresh = pmx.ReadSet(ctx, reads)
    al.align_readset(fresh, True, True)
    want = pmx.records_to_results(*al.fetch(), True)   # (records with their CIGARs: where a CIGAR lies in the arena varies from run to run)
    rs = pmx.ReadSet(ctx, reads)
    placer = pmx.Placer(ctx, hc.hpc_index(oracle, g, 19, 8, 3, False, 0))
    placer.reset()
    placer.add_reads(rs)
    assert placer.histogram_size() > 0 and not rs.is_hpc
    assert rs.export()[0] == b"".join(reads)
    al.align_readset(rs, True, True)
    recs, cig = al.fetch()
    assert len(recs) == 1000 and np.count_nonzero(recs["mapped"]) > 900
    assert pmx.records_to_results(recs, cig, True) == want


# ---------------------------------------------------------------------------------------------- 5. end to end on a real tree
def test_hpc_index_of_a_real_tree_places_long_noisy_reads(pmx, oracle, ctx):
    rsv = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    index = pmx.Index.build(rsv, hpc=True)       # reference defaults: k=19 s=8 l=3, flank mask 250
    assert index.hpc
    leaf = rsv.find_node("MZ515733.1")
    g = rsv.genome(leaf)
    rng = np.random.default_rng(33)
    reads = []
    for _ in range(300):
        n = int(rng.integers(2000, 5001))
        st = int(rng.integers(0, len(g) - n))
        reads.append(hc.run_length_errors(rng, g[st:st + n]))
    assert sum(a != b for a, b in zip(hc.hpc_reads(reads), reads)) == 300
    params = pmx.TraversalParams()
    placer = pmx.Placer(ctx, index)              # (PMX_ERR_UNSUPPORTED before the device learned HPC)
    placer.reset()
    placer.add_reads(pmx.ReadSet(ctx, reads, pack=False), params)
    res = placer.score(params, len(reads))
    want = oracle.place(hc.hpc_reads(reads), index.arrays(), 19, 8, 3)
    assert_place_matches(placer, res, want)
    for m in (0, 4):
        assert res.best_score[m] > 0
        assert leaf == res.best_index[m] or leaf in res.tied_indices[m].tolist(), (m, rsv.node_id(res.best_index[m]))
