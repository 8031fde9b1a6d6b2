"""GPU parity tests for the PLACE stage: HIP path (through the C ABI) vs the oracle, bit-exact."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from place_tree_checks import assert_place_matches

pytestmark = pytest.mark.gpu


def _as_reads(concat, off):
    return [bytes(concat[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def _check_place(pmx, oracle, ctx, index, reads, params=None, k=19, s=8, l=3, open_syncmer=False, t=0, quals=None):
    params = params or pmx.TraversalParams()
    placer = pmx.Placer(ctx, index)
    placer.reset()
    if reads:
        rs = pmx.ReadSet(ctx, reads)
        if quals is not None:
            rs.set_qualities(quals)
        placer.add_reads(rs, params)
    res = placer.score(params, len(reads))
    want = oracle.place(reads, index.arrays(), k, s, l, open_syncmer, t, params.trimStart, params.trimEnd, params.seedMaskFraction,
                        params.minReadSupport, params.forceLeaf, params.dedupReads, quals, params.minSeedQuality)
    assert_place_matches(placer, res, want)
    placer.close()
    return res


def test_log1p_device_restatement_is_exact(pmx, oracle, ctx, sars_index):
    # counts 1..N appear as read counts: build a histogram with count c for key c via merge()
    placer = pmx.Placer(ctx, sars_index)
    placer.reset()
    n = 200000
    keys = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761)
    counts = np.concatenate([np.arange(1, n // 2 + 1), np.random.default_rng(1).integers(1, 2 ** 40, n - n // 2)]).astype(np.int64)
    placer.merge(keys, counts)
    placer.score(pmx.TraversalParams(minReadSupport=1), 0)
    kh, kl = placer.kept_seeds()
    order = np.argsort(keys)
    assert np.array_equal(kh, keys[order])
    # the checker is glibc's log1p (through the oracle), NOT numpy's own log1p (differs in ~1% of inputs)
    wh, want, _ = oracle.finalize_reads(keys[order], counts[order], 19, 0.0, 1)
    assert np.array_equal(wh, kh)
    assert np.array_equal(kl.view(np.uint64), want.view(np.uint64))


def test_place_synthetic_pairs_bit_exact(pmx, oracle, ctx, sars, sars_index):
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 3000, seed=1)
    _check_place(pmx, oracle, ctx, sars_index, _as_reads(concat, off))


def test_place_edge_cases(pmx, oracle, ctx, sars, sars_index):
    g = sars.genome("node_100")
    rng = np.random.default_rng(2)
    reads = []
    for i in range(400):
        n = int(rng.integers(1, 400))
        st = int(rng.integers(0, len(g) - n))
        r = bytearray(g[st:st + n])
        if i % 5 == 0 and n > 3:
            r[int(rng.integers(0, n))] = ord("N")
        if i % 7 == 0:
            r = bytearray(bytes(r).lower())
        if i % 11 == 0 and n > 10:
            r[5:8] = b"RYK"
        reads.append(bytes(r))
    reads += [b"A" * 150, b"ACGT" * 40, b"", b"N" * 60, b"ACGTACGTACGTACGTACG"]   # homopolymer, periodic, empty, all-N, exactly k
    _check_place(pmx, oracle, ctx, sars_index, reads)
    _check_place(pmx, oracle, ctx, sars_index, reads, pmx.TraversalParams(trimStart=10, trimEnd=25, minReadSupport=1))
    _check_place(pmx, oracle, ctx, sars_index, [])                                  # no reads at all
    _check_place(pmx, oracle, ctx, sars_index, reads, pmx.TraversalParams(forceLeaf=True, seedMaskFraction=0.01))


def test_place_dedup(pmx, oracle, ctx, sars, sars_index):
    """--dedup (src/placement.cpp:1550-1620): every distinct read string counts once"""
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 1500, seed=5)
    reads = _as_reads(concat, off)
    rng = np.random.default_rng(8)
    dup = [reads[int(i)] for i in rng.integers(0, len(reads), 2000)]          # exact copies, some several times
    near = [r[:-1] + (b"A" if r[-1:] != b"A" else b"C") for r in reads[:200]]   # differ in the last base only
    case = [reads[0].lower(), reads[1][:100], reads[1][:100], b"", b""]         # case matters; prefixes; empties
    allr = reads + dup + near + case
    order = rng.permutation(len(allr))
    allr = [allr[int(i)] for i in order]
    _check_place(pmx, oracle, ctx, sars_index, allr, pmx.TraversalParams(dedupReads=True))
    _check_place(pmx, oracle, ctx, sars_index, allr, pmx.TraversalParams(dedupReads=False))


# (the three k=19, s=8, t=0 rows run the kernel specialised for the default k/s with the other l / open settings)
@pytest.mark.parametrize("k,s,l,open_syncmer,t", [(15, 8, 1, False, 0), (31, 6, 3, False, 0), (19, 8, 2, True, 3), (21, 10, 4, False, 2),
                                                  (19, 8, 1, False, 0), (19, 8, 3, True, 0), (19, 8, 5, False, 0)])
def test_place_other_parameters(pmx, oracle, ctx, sars, k, s, l, open_syncmer, t):
    # a small hand-made index over the real hashes keeps this fast: root = seeds of one genome
    g = sars.genome("node_5")
    hs, cn = oracle.histogram([g], k, s, l, open_syncmer, t)
    keep = cn < 30000
    hs, cn = hs[keep], cn[keep]
    half = len(hs) // 2
    parent = np.array([0, 0, 1], np.uint32)
    offsets = np.array([0, len(hs), len(hs) + half, len(hs) + half + 10], np.uint64)
    hash_ = np.concatenate([hs, hs[:half], hs[half:half + 10]])
    pc = np.concatenate([np.zeros(len(hs)), cn[:half], cn[half:half + 10]]).astype(np.int16)
    cc = np.concatenate([cn, cn[:half] + 1, np.zeros(10)]).astype(np.int16)
    index = pmx.Index.from_arrays(k, s, t, l, open_syncmer, parent, offsets, hash_, pc, cc)
    concat, off = pmx.simulate_paired_reads(g, 1500, seed=3)
    _check_place(pmx, oracle, ctx, index, _as_reads(concat, off), None, k, s, l, open_syncmer, t)


def test_place_min_seed_quality(pmx, oracle, ctx, sars, sars_index):
    """--min-seed-quality (src/placement.cpp:1386-1527): seeds whose k-mer averages below the Phred threshold are
    dropped, windows over the full syncmer list; restated in the oracle (no reference fixture exists for it)"""
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 1500, seed=6)
    reads = _as_reads(concat, off)
    rng = np.random.default_rng(12)
    quals = []
    for r in reads:
        q = rng.integers(2, 41, len(r)).astype(np.uint8) + 33
        if rng.random() < 0.5:
            q[:] = 73                                   # clean read
        lo = int(rng.integers(0, max(1, len(r) - 30)))
        q[lo:lo + int(rng.integers(5, 40))] = 35        # a low-quality stretch
        quals.append(q.tobytes())
    reads += [b"ACGT" * 10, b""]
    quals += [b"I" * 40, b""]
    for mq, ts, te in ((20, 0, 0), (30, 10, 20), (2, 0, 0)):
        _check_place(pmx, oracle, ctx, sars_index, reads, pmx.TraversalParams(minSeedQuality=mq, trimStart=ts, trimEnd=te, dedupReads=True),
                     quals=quals)
    # l = 1 index
    hs, cn = oracle.histogram([g], 15, 8, 1)
    keep = cn < 30000
    hs, cn = hs[keep], cn[keep]
    index = pmx.Index.from_arrays(15, 8, 0, 1, False, np.array([0], np.uint32), np.array([0, len(hs)], np.uint64), hs,
                                  np.zeros(len(hs), np.int16), cn.astype(np.int16))
    _check_place(pmx, oracle, ctx, index, reads, pmx.TraversalParams(minSeedQuality=25), 15, 8, 1, quals=quals)


def test_reference_e2e_fixtures_on_rsv_4k(pmx, oracle, ctx):
    """src/test/e2e/run_e2e.sh steps [2], [4], [6]: a leaf genome, an internal node's genome and a FASTQ of the leaf
    must place back on their own node with log_raw > 50 (rsv_4K has inverted blocks: from-scratch index producer);
    the HIP path must also equal the oracle bit for bit on these inputs"""
    rsv = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    index = pmx.Index.build(rsv)                      # reference defaults: k=19 s=8 l=3 closed syncmers, flank mask 250
    cases = [("MZ515733.1.fa", "MZ515733.1"), ("rsv_4K.panman.random.node_1330.fa", "node_1330"), ("MZ515733.1.fastq", "MZ515733.1")]
    for fname, node in cases:
        _, seqs, _ = pmx.read_fastx(os.path.join(GOLDEN, fname))
        res = _check_place(pmx, oracle, ctx, index, seqs)
        tsv = pmx.format_placement_tsv(res, rsv.node_id)
        assert node in tsv, (fname, tsv)
        log_raw = float([l for l in tsv.splitlines() if l.startswith("log_raw")][0].split("\t")[1])
        assert log_raw > 50, (fname, log_raw)


def test_golden_placement_tsv_on_gpu(pmx, ctx, sars, sars_index, tmp_path):
    """examples/check_examples.sh:52-70 through the HIP path: byte-exact isolate.placement.tsv."""
    placer = pmx.Placer(ctx, sars_index)
    out = tmp_path / "isolate.placement.tsv"
    res = pmx.place_lite(ctx, placer, os.path.join(GOLDEN, "isolate_R1.fastq.gz"), os.path.join(GOLDEN, "isolate_R2.fastq.gz"), str(out),
                         pmx.TraversalParams(), sars.node_id)
    assert out.read_text() == open(os.path.join(GOLDEN, "isolate.placement.tsv")).read()
    assert sars.node_id(res.bestLogContainmentNodeIndex) == "node_7618"
    assert res.n_reads == 102338 and res.n_unique_seeds == 317148 and res.readUniqueSeedCount == 117645


def test_native_fastq_ingest_feeds_the_device(pmx, ctx, sars_index):
    """FASTQ pair -> pmx_fastx_read_paired -> ReadSet.from_fastx (flat buffers, qualities attached) gives the same
    histogram and placement as the Python-list route (reverse-complementing mate 2 does not change canonical seeds, so
    the golden counts of the interleaved-as-read route hold here too)"""
    r1, r2 = os.path.join(GOLDEN, "isolate_R1.fastq.gz"), os.path.join(GOLDEN, "isolate_R2.fastq.gz")
    fx = pmx.read_fastq_paired_native(r1, r2)
    params = pmx.TraversalParams()
    out = []
    for rs in (pmx.ReadSet.from_fastx(ctx, fx, with_qualities=True), pmx.ReadSet(ctx, pmx.read_fastq_paired(r1, r2)[0])):
        placer = pmx.Placer(ctx, sars_index)
        placer.add_reads(rs, params)
        res = placer.score(params, rs.n_reads)
        out.append((placer.histogram_size(), res.n_unique_seeds, res.readUniqueSeedCount, tuple(res.best_index), tuple(res.best_score)))
    assert out[0] == out[1]
    assert out[0][1] == 317148 and out[0][2] == 117645


def test_histogram_shard_merge_equals_single_pass(pmx, ctx, sars, sars_index):
    """multi-GPU exchange step: per-shard histograms merged == one pass over all reads."""
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 4000, seed=5)
    reads = _as_reads(concat, off)
    a = pmx.Placer(ctx, sars_index); a.reset(); a.add_reads(pmx.ReadSet(ctx, reads))
    h_all, c_all = a.histogram()
    b = pmx.Placer(ctx, sars_index); b.reset(); b.add_reads(pmx.ReadSet(ctx, reads[:3000]))
    c = pmx.Placer(ctx, sars_index); c.reset(); c.add_reads(pmx.ReadSet(ctx, reads[3000:]))
    hb, cb = b.histogram()
    c.merge(hb, cb)
    h2, c2 = c.histogram()
    assert np.array_equal(h_all, h2) and np.array_equal(c_all, c2)
    ra = a.score(pmx.TraversalParams(), len(reads)); rc = c.score(pmx.TraversalParams(), len(reads))
    assert ra.best_score == rc.best_score and ra.best_index == rc.best_index


def test_histogram_parts_merge_on_device(pmx, ctx, sars, sars_index):
    """the exchange as bench.py runs it: the ranks' runs in one padded [world, 2, max] device buffer, merged in one call"""
    import torch
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 3000, seed=15)
    reads = _as_reads(concat, off)
    full = pmx.Placer(ctx, sars_index); full.reset(); full.add_reads(pmx.ReadSet(ctx, reads))
    h_all, c_all = full.histogram()
    shards = [reads[:1000], reads[1000:4400], reads[4400:]]
    placers, sizes = [], []
    for sh in shards:
        pl = pmx.Placer(ctx, sars_index); pl.reset(); pl.add_reads(pmx.ReadSet(ctx, sh))
        placers.append(pl); sizes.append(pl.histogram_size())
    mx = max(sizes)
    buf = torch.full((3, 2, mx), -1, dtype=torch.int64, device="cuda:0")
    for r, pl in enumerate(placers):
        pl.export_device(buf[r, 0].data_ptr(), buf[r, 1].data_ptr(), mx)
    torch.cuda.synchronize()
    for me in range(3):
        pl = pmx.Placer(ctx, sars_index); pl.reset(); pl.add_reads(pmx.ReadSet(ctx, shards[me]))
        pl.merge_device_parts(buf[0, 0].data_ptr(), buf[0, 1].data_ptr(), 2 * mx, sizes, me)
        h, c = pl.histogram()
        assert np.array_equal(h, h_all) and np.array_equal(c, c_all), me


def test_full_size_properties(pmx, ctx, sars, sars_index):
    """BASELINE config 2 size (1M reads): size-independent checks -- total seed frequency equals the number
    of emitted seeds, and doubling the read set doubles every count (linearity of the histogram)."""
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 500000, seed=42)
    rs = pmx.ReadSet(ctx, concat=concat, offsets=off)
    p = pmx.Placer(ctx, sars_index); p.reset(); p.add_reads(rs)
    h1, c1 = p.histogram()
    p.add_reads(rs)
    h2, c2 = p.histogram()
    assert np.array_equal(h1, h2) and np.array_equal(c2, 2 * c1)
    assert np.all(h1[1:] > h1[:-1])
    res = p.score(pmx.TraversalParams(), 2 * (len(off) - 1))
    assert sars.node_id(res.best_index[4]) in {sars.node_id(int(t)) for t in res.tied_indices[4]}
    assert "node_7618" in {sars.node_id(int(t)) for t in res.tied_indices[0]}


def test_streaming_read_sets_rewrap_on_the_device(pmx, ctx, sars, sars_index):
    """pmx_readset_rewrap_device: one read set object pointed at batch after batch in device memory (word offsets and the
    offset checks on the device, packed buffers reused) gives what fresh uploads give -- also for a slice of a larger offsets
    array and for ragged reads -- and refuses offsets that leave the buffer"""
    import torch
    g = sars.genome("node_7618")
    dev = torch.device("cuda", 0)

    def fresh_hist(reads):
        p = pmx.Placer(ctx, sars_index); p.reset(); p.add_reads(pmx.ReadSet(ctx, reads))
        out = p.histogram(); p.close()
        return out

    batches = []
    for seed, n in ((11, 3000), (12, 5000), (13, 1000)):
        concat, off = pmx.simulate_paired_reads(g, n, seed=seed)
        batches.append((concat, off))
    rag = [bytes(batches[0][0][i * 150:i * 150 + (i % 140) + 5]) for i in range(2000)] + [b"", b"ACGTN" * 7]     # ragged, empty, N
    rc, ro = pmx.concat_reads(rag)
    batches.append((np.frombuffer(rc, np.uint8).copy(), ro))
    rs = None
    for concat, off in batches:
        d_c = torch.from_numpy(concat).to(dev)
        d_o = torch.from_numpy(off).to(dev)
        n = len(off) - 1
        if rs is None:
            rs = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), n, int(concat.size), 0, keepalive=(d_c, d_o))
        else:
            rs.rewrap_device(d_c.data_ptr(), d_o.data_ptr(), n, int(concat.size), 0, keepalive=(d_c, d_o))
        rs.pack()
        p = pmx.Placer(ctx, sars_index); p.reset(); p.add_reads(rs)
        hh, hc = p.histogram(); p.close()
        wh, wc = fresh_hist(_as_reads(concat, off))
        assert np.array_equal(hh, wh) and np.array_equal(hc, wc)
        # a slice [r0, r1] of the same offsets array addresses its reads in the same buffer
        r0, r1 = n // 4 & ~1, n // 2 & ~1
        if r1 > r0:
            rs.rewrap_device(d_c.data_ptr(), d_o.data_ptr() + 8 * r0, r1 - r0, int(concat.size), 0, keepalive=(d_c, d_o))
            rs.pack()
            p = pmx.Placer(ctx, sars_index); p.reset(); p.add_reads(rs)
            hh, hc = p.histogram(); p.close()
            wh, wc = fresh_hist(_as_reads(concat, off)[r0:r1])
            assert np.array_equal(hh, wh) and np.array_equal(hc, wc)
    concat, off = batches[0]
    d_c = torch.from_numpy(concat).to(dev)
    bad = off.copy(); bad[-1] += 10
    d_o = torch.from_numpy(bad).to(dev)
    with pytest.raises(pmx.PmxError):
        rs.rewrap_device(d_c.data_ptr(), d_o.data_ptr(), len(off) - 1, int(concat.size), 0)
    bad = off.copy(); bad[5] = bad[7]
    bad[6] = bad[5] - 3
    d_o = torch.from_numpy(bad).to(dev)
    with pytest.raises(pmx.PmxError):
        rs.rewrap_device(d_c.data_ptr(), d_o.data_ptr(), len(off) - 1, int(concat.size), 0)
    with pytest.raises(pmx.PmxError):
        pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), len(off) - 1, int(concat.size), 0)
    rs.close()


def test_streaming_ranges_equal_whole_set(pmx, ctx, sars, sars_index):
    """pmx_readset_pack_range + pmx_place_add_reads_range (a batch packed and seeded range by range while its H2D copy is in
    flight): the histogram, the packed reads and the alignments equal those of the set packed and seeded as a whole -- ragged
    ranges, a range below the locality-sort threshold, an empty range; a range that was not packed is refused, so is --dedup
    on a sub-range; and two contexts run from two threads give the same results (each owns a hardware queue)"""
    import threading
    import torch
    g = sars.genome("node_7618")
    dev = torch.device("cuda", 0)
    concat, off = pmx.simulate_paired_reads(g, 30000, seed=21)
    n = len(off) - 1
    d_c = torch.from_numpy(concat).to(dev)
    d_o = torch.from_numpy(off).to(dev)
    whole = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), n, int(concat.size), 0, keepalive=(d_c, d_o))
    whole.pack()
    p = pmx.Placer(ctx, sars_index); p.reset(); p.add_reads(whole)
    wh, wc = p.histogram()
    al = pmx.Aligner(ctx, g, 150)
    al.align_readset(whole, paired=True, revcomp_mate2=True)
    w_recs, w_cig = al.fetch()

    def ops(recs, cig):
        return [tuple(cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]) for r in recs[:2000]]
    for bounds in ([0, 20000, 20002, 20002, 41000, n], [0, n], [0, 100, n]):
        rs = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), n, int(concat.size), 0, keepalive=(d_c, d_o))
        p.reset()
        with pytest.raises(pmx.PmxError):
            p.add_reads_range(rs, 0, bounds[1])                   # nothing packed yet
        for a, b in zip(bounds[:-1], bounds[1:]):
            rs.pack_range(a, b)
            p.add_reads_range(rs, a, b)
        hh, hc = p.histogram()
        assert np.array_equal(hh, wh) and np.array_equal(hc, wc)
        al.align_readset(rs, paired=True, revcomp_mate2=True)     # (the set counts as packed: the ranges cover it)
        recs, cig = al.fetch()
        for f in ("rs", "re", "qs", "qe", "mapq", "rev", "proper_frag", "mapped", "n_cigar", "flags", "score"):
            assert np.array_equal(recs[f], w_recs[f]), f
        assert ops(recs, cig) == ops(w_recs, w_cig)
        rs.close()
    rs = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), n, int(concat.size), 0, keepalive=(d_c, d_o))
    rs.pack_range(0, 1000)
    with pytest.raises(pmx.PmxError):
        al.align_readset(rs, paired=True, revcomp_mate2=True)     # not every read is packed
    with pytest.raises(pmx.PmxError):
        p.add_reads_range(rs, 0, 1000, pmx.TraversalParams(dedupReads=True))
    with pytest.raises(pmx.PmxError):
        rs.pack_range(10, n + 2)
    rs.close()
    # two contexts from two host threads
    out = {}

    def work(key):
        c2 = pmx.Context(0)
        r2 = pmx.ReadSet.wrap_device(c2, d_c.data_ptr(), d_o.data_ptr(), n, int(concat.size), 0)
        p2 = pmx.Placer(c2, sars_index)
        for _ in range(3):
            p2.reset()
            r2.pack()
            p2.add_reads(r2)
            out[key] = p2.histogram()
        p2.close(); r2.close()
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    for k in range(2):
        assert np.array_equal(out[k][0], wh) and np.array_equal(out[k][1], wc)
    p.close(); al.close(); whole.close()


def test_scoring_redone_with_level_kernels_when_the_persistent_launch_starves(pmx, oracle, ctx, sars, sars_index, monkeypatch):
    """the heavy-path scoring kernel spin-waits on flags and needs all of its workgroups resident; when a wave
    gives up (shared GPU) the call must not fail but redo the scoring with the level kernels -- the same bits"""
    g = sars.genome("node_7618")
    concat, off = pmx.simulate_paired_reads(g, 1500, seed=8)
    reads = _as_reads(concat, off)
    monkeypatch.setenv("PMX_PLACE_TEST_STARVED", "1")
    _check_place(pmx, oracle, ctx, sars_index, reads)


def test_read_collapse_keeps_the_histogram(pmx, oracle, ctx, sars, sars_index):
    """k_collapse_reads (src/placement.cpp:1550-1593: every distinct read seeded once with its multiplicity): deep coverage of a
    short region -- most reads are copies of one another -- with reads of several lengths up to 160 bases, `N`s, lower case,
    reads shorter than k, and copies spread over more than one 1,024-read block; fixed-length and ragged sets; with and
    without --dedup.  The histogram, the kept seeds and every node score equal the oracle's, which seeds read by read."""
    g = sars.genome("node_7618")[5000:5400]
    rng = np.random.default_rng(17)
    reads = []
    for i in range(16000):
        n = int(rng.choice([150, 150, 150, 151, 160, 100, 31, 19, 18, 5]))
        st = int(rng.integers(0, 24))
        r = bytearray(g[st:st + n])
        if rng.random() < 0.15:
            p = int(rng.integers(0, len(r)))
            r[p] = rng.choice(list(b"ACGTN"))
        if i % 50 == 0:
            r = bytearray(bytes(r).lower())
        reads.append(bytes(r))
    _check_place(pmx, oracle, ctx, sars_index, reads)
    _check_place(pmx, oracle, ctx, sars_index, reads, pmx.TraversalParams(dedupReads=True))
    fixed = [r for r in reads if len(r) == 150]
    assert len(fixed) > 4096
    _check_place(pmx, oracle, ctx, sars_index, fixed)


def test_seeding_redone_after_the_optimistic_table_overflows(pmx, oracle, ctx, sars, sars_index, monkeypatch, capfd):
    """PMX_SEED_BOUND_DIV=1048576 sizes the optimistic pass's table at its floor of 65,536 slots; 60,000 simulated reads carry
    115,522 distinct seeds, so inserts fail, the counters and the table are cleared and the pass is redone with the safe bound.
    The redo ran (the profile line reports failed inserts), the result equals the oracle's, and after reset() the same placer
    gives the same histogram and best nodes without the switch: nothing of the first pass's counters survives."""
    import re
    concat, off = pmx.simulate_paired_reads(sars.genome("node_7618"), 60000, seed=1)
    reads = _as_reads(concat, off)
    monkeypatch.setenv("PMX_SEED_BOUND_DIV", "1048576")
    monkeypatch.setenv("PMX_PLACE_PROF", "1")
    pmx.reload_options()
    capfd.readouterr()
    want = _check_place(pmx, oracle, ctx, sars_index, reads)
    lines = re.findall(r"\[pmx place\] seeding with bound 1/1048576: table (\d+) slots, (\d+) failed inserts", capfd.readouterr().err)
    assert lines and int(lines[0][1]) > 0, lines
    params = pmx.TraversalParams()
    placer = pmx.Placer(ctx, sars_index)
    placer.reset()
    rs = pmx.ReadSet(ctx, reads)
    placer.add_reads(rs, params)
    forced = placer.score(params, len(reads))
    forced_hist = placer.histogram()
    monkeypatch.delenv("PMX_SEED_BOUND_DIV")
    monkeypatch.delenv("PMX_PLACE_PROF")
    pmx.reload_options()
    placer.reset()
    placer.add_reads(rs, params)
    plain = placer.score(params, len(reads))
    plain_hist = placer.histogram()
    assert len(plain_hist[0]) > 65536
    for a, b in zip(forced_hist, plain_hist):
        assert np.array_equal(a, b)
    for res in (forced, plain):
        assert list(res.best_index) == list(want.best_index) and list(res.best_score) == list(want.best_score)
    rs.close()
    placer.close()
