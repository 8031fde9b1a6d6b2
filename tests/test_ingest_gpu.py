"""The read-ingest kernels against references of their own (tests/ingest_checks.py; the sets' claims are checked without a GPU
in tests/test_ingest_families.py).  Every comparison is exact.

  packed form     ReadSet.export_packed() -- 2-bit words, ambiguity words, word offsets, 64-byte records -- equals pack_reference:
                  fixed lengths at every byte offset of a wrapped buffer (k_pack_reads_fixed: every shift arm, every word count
                  and tail), ragged / skewed / alphabet sets (k_pack_reads: the read search), each through pack(), through
                  rewrap_device + pack() on one reused object (k_read_word_counts; stale records) and through pack_range
  histogram       Placer.histogram() equals oracle.histogram over kernel forms (specialised over tiles, specialised in place,
                  generic, quality mode), trims, --dedup and read sets
  read counts     around the 64-read tile, the 1,024-read collapse block and the 4,096-read locality order
  align stage     a fixed-length set wrapped at an odd byte offset aligns as the same reads uploaded
"""
import os

import numpy as np
import pytest

import align_checks as ac
import ingest_checks as ic
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_FIELDS = ("words", "amb", "woff", "records")


def _assert_packed(got, want, label):
    for f, g, w in zip(_FIELDS, got, want):
        if w is None or g is None:
            assert g is None and w is None, "%s: %s: records %s" % (label, f, "missing" if g is None else "not expected")
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (label, f, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i = tuple(int(x) for x in bad[0])
            raise AssertionError("%s: %s differs at %d places, first %s: got %#x, want %#x" % (label, f, len(bad), i, int(g[i]), int(w[i])))


_dev = {}


def _device_reads(name, j):
    """a named set in device memory, its first read ic.WRAP_PAD + j bytes behind a 16-byte boundary: (bases, absolute offsets,
    bytes of the buffer).  The spare bytes on both sides hold `T`, so a byte taken from outside a read shows in the words."""
    import torch
    if (name, j) not in _dev:
        concat, off = _concat(name)
        first = ic.WRAP_PAD + j
        buf = np.full(first + len(concat) + ic.WRAP_PAD + 16, ord("T"), np.uint8)
        buf[first:first + len(concat)] = concat
        d_c = torch.from_numpy(buf).to("cuda:0")
        d_o = torch.from_numpy(off + first).to("cuda:0")
        assert d_c.data_ptr() % 16 == 0 and d_o.data_ptr() % 8 == 0
        _dev[(name, j)] = (d_c, d_o, len(buf))
    return _dev[(name, j)]


def _concat(name):
    reads = ic.read_set(name)
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads), np.uint8), off


def _wrap(pmx, ctx, name, j):
    d_c, d_o, size = _device_reads(name, j)
    return pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), len(ic.read_set(name)), size, 0, keepalive=(d_c, d_o))


def _rewrap(rs, name, j, r0=0):
    d_c, d_o, size = _device_reads(name, j)
    rs.rewrap_device(d_c.data_ptr(), d_o.data_ptr() + 8 * r0, len(ic.read_set(name)) - r0, size, 0, keepalive=(d_c, d_o))


def _pack_ranges(pmx, rs, bounds):
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b == bounds[-1]:
            with pytest.raises(pmx.PmxError):
                rs.export_packed()                        # the ranges do not cover the set yet
        rs.pack_range(a, b)


# ------------------------------------------------------------------------------------------------ the packed form
@pytest.mark.parametrize("L", ic.FIXED_LENGTHS)
def test_fixed_length_sets_pack_to_the_reference_at_every_byte_offset(pmx, ctx, L):
    """gaps 1, 2 and 4 of the list in DESIGN: k_pack_reads_fixed at every sh = address & 15 (full and tail words; one to seven
    words per read; sets with and without records), whole sets and slices that start at an odd read, and the same buffers
    through pack_range (k_pack_reads on a fixed-length set: its own shift, address & 3)"""
    name = "fixed_%d_%d" % (L, ic.FIXED_SMALL)
    reads = ic.read_set(name)
    rs = pmx.ReadSet(ctx, reads, pack=False)
    with pytest.raises(pmx.PmxError):
        rs.export_packed()                                # not packed
    rs.pack()
    _assert_packed(rs.export_packed(), ic.packed(name), name + " uploaded")
    rs.close()
    sliced = None
    for j in ic.WRAP_OFFSETS:
        rs = _wrap(pmx, ctx, name, j)
        rs.pack()
        _assert_packed(rs.export_packed(), ic.packed(name), "%s wrapped at %d" % (name, j))
        rs.close()
        if sliced is None:
            sliced = _wrap(pmx, ctx, name, j)
        _rewrap(sliced, name, j, ic.SLICE_R0)
        sliced.pack()
        _assert_packed(sliced.export_packed(), ic.packed(name, ic.SLICE_R0), "%s slice from read %d, wrapped at %d" % (name, ic.SLICE_R0, j))
        rs = _wrap(pmx, ctx, name, j)
        _pack_ranges(pmx, rs, ic.range_bounds(name))
        _assert_packed(rs.export_packed(), ic.packed(name), "%s wrapped at %d, packed by ranges" % (name, j))
        rs.close()
    sliced.close()


NAMED = ic.RAGGED + ("alphabet", "skewed")


@pytest.mark.parametrize("name", NAMED)
def test_ragged_sets_pack_to_the_reference(pmx, ctx, name):
    """gaps 4 and 5: k_pack_reads on every length 0..200, every byte value, and a set whose words per read send the read search
    thousands of reads away from its first guess in both directions, next to runs of reads without a word; uploaded, wrapped at
    an odd byte offset, and packed by ranges whose bounds fall inside those runs"""
    rs = pmx.ReadSet(ctx, ic.read_set(name))
    _assert_packed(rs.export_packed(), ic.packed(name), name + " uploaded")
    rs.close()
    for j in (13, 2):
        rs = _wrap(pmx, ctx, name, j)
        rs.pack()
        _assert_packed(rs.export_packed(), ic.packed(name), "%s wrapped at %d" % (name, j))
        rs.close()
        rs = _wrap(pmx, ctx, name, j)
        _pack_ranges(pmx, rs, ic.range_bounds(name))
        _assert_packed(rs.export_packed(), ic.packed(name), "%s wrapped at %d, packed by ranges" % (name, j))
        rs.close()


def test_one_read_set_object_rewrapped_from_set_to_set(pmx, ctx):
    """gap 4, the device-side word offsets and the records of a REUSED object: ragged and fixed-length sets in turn (with and
    without records, fewer and shorter reads after more and longer ones), so every record slot the last batch left behind has
    to be gone -- k_collapse_reads compares records dword for dword"""
    rs = None
    for i, L in enumerate(ic.FIXED_LENGTHS):
        j = ic.WRAP_OFFSETS[i % len(ic.WRAP_OFFSETS)]
        for name in (NAMED[i % len(NAMED)], "fixed_%d_%d" % (L, ic.FIXED_SMALL)):
            if rs is None:
                rs = _wrap(pmx, ctx, name, j)
            else:
                _rewrap(rs, name, j)
            rs.pack()
            _assert_packed(rs.export_packed(), ic.packed(name), "%s rewrapped at %d (step %d)" % (name, j, i))
    # the slice form and the ranges on the reused object, after a set with records
    _rewrap(rs, "ragged_0_160_4200", 7, ic.SLICE_R0)
    rs.pack()
    _assert_packed(rs.export_packed(), ic.packed("ragged_0_160_4200", ic.SLICE_R0), "ragged slice rewrapped")
    for name in ("skewed", "fixed_19_%d" % ic.FIXED_SMALL, "ragged_0_160_4200"):
        _rewrap(rs, name, 15)
        _pack_ranges(pmx, rs, ic.range_bounds(name))
        _assert_packed(rs.export_packed(), ic.packed(name), name + " rewrapped, packed by ranges")
    rs.close()


# ------------------------------------------------------------------------------------------------ histograms
_placers, _sets = {}, {}


def _placer(pmx, oracle, ctx, params):
    """one placer per seed-parameter set, over a three-node index made by hand (as test_place_other_parameters)"""
    if params not in _placers:
        k, s, l, open_syncmer, t = params
        hs, cn = oracle.histogram([ic.genome()], k, s, l, open_syncmer, t)
        half = len(hs) // 2
        assert half > 10
        parent = np.array([0, 0, 1], np.uint32)
        offsets = np.array([0, len(hs), len(hs) + half, len(hs) + half + 10], np.uint64)
        hash_ = np.concatenate([hs, hs[:half], hs[half:half + 10]])
        pc = np.concatenate([np.zeros(len(hs)), cn[:half], cn[half:half + 10]]).astype(np.int16)
        cc = np.concatenate([cn, cn[:half] + 1, np.zeros(10)]).astype(np.int16)
        index = pmx.Index.from_arrays(k, s, t, l, open_syncmer, parent, offsets, hash_, pc, cc)
        _placers[params] = (pmx.Placer(ctx, index), index)
    return _placers[params][0]


def _read_set(pmx, ctx, name, with_qualities=False):
    if (name, with_qualities) not in _sets:
        rs = pmx.ReadSet(ctx, ic.read_set(name))
        if with_qualities:
            rs.set_qualities(ic.qualities(name))
        _sets[(name, with_qualities)] = rs
    return _sets[(name, with_qualities)]


def _assert_histogram(pmx, oracle, ctx, name, params, trim=(0, 0), dedup=False, min_q=0, rs=None):
    placer = _placer(pmx, oracle, ctx, params)
    placer.reset()
    placer.add_reads(rs or _read_set(pmx, ctx, name, min_q > 0),
                     pmx.TraversalParams(trimStart=trim[0], trimEnd=trim[1], dedupReads=dedup, minSeedQuality=min_q))
    hh, hc = placer.histogram()
    wh, wc = ic.want_histogram(oracle, name, params, trim, dedup, min_q)
    label = (name, params, trim, dedup, min_q)
    assert np.array_equal(hh, wh), ("seed set differs", label, len(hh), len(wh))
    assert np.array_equal(hc, wc), ("seed counts differ", label, int(hc.sum()), int(wc.sum()))
    return hh, hc


@pytest.mark.parametrize("dedup", (False, True), ids=("all", "dedup"))
@pytest.mark.parametrize("trim", ic.TRIMS, ids=lambda t: "trim%d_%d" % t)
@pytest.mark.parametrize("params", ic.SPECIALISED, ids=("l3", "l1"))
def test_histogram_of_the_specialised_kernel(pmx, oracle, ctx, params, trim, dedup):
    """gaps 2, 3 and 6: collapse + tiles (reads of up to 160 bases) and the in-place form (161, 200, the ragged set up to 200)
    against the oracle on every fixed length, 67 reads and 4,200 (locality order on, five collapse blocks), every ragged length,
    an N planted at the word and window edges, every byte value; with trims -- one leaves no k-mer -- and the --dedup mask"""
    for name in ic.SWEEP_FULL:
        hh, _ = _assert_histogram(pmx, oracle, ctx, name, params, trim, dedup)
        if trim == (0, 200):
            assert len(hh) == 0
    if trim == (0, 0):
        assert len(ic.want_histogram(oracle, "fixed_150_%d" % ic.FIXED_LARGE, params, trim, dedup)[0]) > 300


@pytest.mark.parametrize("dedup", (False, True), ids=("all", "dedup"))
@pytest.mark.parametrize("trim", ic.TRIMS, ids=lambda t: "trim%d_%d" % t)
@pytest.mark.parametrize("params", ic.GENERIC, ids=("k15", "k21_t2", "open_t3"))
def test_histogram_of_the_generic_kernel(pmx, oracle, ctx, params, trim, dedup):
    for name in ic.SWEEP_FEW:
        _assert_histogram(pmx, oracle, ctx, name, params, trim, dedup)


@pytest.mark.parametrize("params", (ic.SPECIALISED[0], ic.GENERIC[0]), ids=("k19", "k15"))
def test_histogram_in_quality_mode(pmx, oracle, ctx, params):
    """minSeedQuality with qualities attached: the generic kernel's quality mode, also for the default parameters (uploaded
    sets: the qualities share the reads' offsets, which start at 0)"""
    for name in ic.SWEEP_FEW:
        hq, _ = _assert_histogram(pmx, oracle, ctx, name, params, min_q=ic.MIN_Q)
        if name == "fixed_150_%d" % ic.FIXED_LARGE:
            assert 0 < len(hq) and not np.array_equal(hq, ic.want_histogram(oracle, name, params)[0])   # the threshold drops seeds
    _assert_histogram(pmx, oracle, ctx, "fixed_150_%d" % ic.FIXED_SMALL, params, trim=(10, 25), min_q=ic.MIN_Q)


def test_histogram_of_wrapped_and_range_packed_sets(pmx, oracle, ctx):
    """the seeding kernels on what the other pack paths left: a fixed-length set at an odd byte offset (collapse + tiles with
    fixed_len, and in place above 160 bases), a slice, and sets packed by ranges"""
    for params in (ic.SPECIALISED[0], ic.GENERIC[0]):
        for L in (33, 150, 151, 161):
            name = "fixed_%d_%d" % (L, ic.FIXED_LARGE)
            rs = _wrap(pmx, ctx, name, 13)
            rs.pack()
            _assert_histogram(pmx, oracle, ctx, name, params, rs=rs)
            _assert_histogram(pmx, oracle, ctx, name, params, dedup=True, rs=rs)
            rs.close()
        for name in ("skewed",) + ic.RAGGED:
            rs = _wrap(pmx, ctx, name, 7)
            _pack_ranges(pmx, rs, ic.range_bounds(name))
            _assert_histogram(pmx, oracle, ctx, name, params, rs=rs)
            rs.close()


# ------------------------------------------------------------------------------------------------ read-count edges
@pytest.mark.parametrize("n", ic.COUNT_EDGES)
def test_read_count_edges(pmx, oracle, ctx, n):
    """gap 6: n reads around the 64-read tile, the 1,024-read collapse block and the 4,096-read locality order, all copies of
    one read (one owner per block, multiplicities up to 1,024; every seed counted n times) and all different (every tile full)"""
    for params in ic.SPECIALISED:
        _, hc = _assert_histogram(pmx, oracle, ctx, "identical_%d" % n, params)
        assert len(hc) > 5 and np.all(hc == n)
        _, hc = _assert_histogram(pmx, oracle, ctx, "identical_%d" % n, params, dedup=True)
        assert np.all(hc == 1)
        _assert_histogram(pmx, oracle, ctx, "distinct_%d" % n, params)
        _assert_histogram(pmx, oracle, ctx, "distinct_%d" % n, params, trim=(10, 25), dedup=True)
    _assert_histogram(pmx, oracle, ctx, "distinct_%d" % n, ic.GENERIC[0])


def test_copies_spread_over_collapse_blocks(pmx, oracle, ctx):
    for params in ic.SPECIALISED:
        _, hc = _assert_histogram(pmx, oracle, ctx, "mixed_3x700", params)
        assert np.all(hc % 700 == 0)
        _assert_histogram(pmx, oracle, ctx, "mixed_3x700", params, dedup=True)


# ------------------------------------------------------------------------------------------------ the align stage
def test_wrapped_fixed_length_set_aligns_as_the_uploaded_one(pmx, oracle, ctx):
    """a fixed 151-base set wrapped at byte offset 13 (k_pack_reads_fixed, odd shifts) gives the align stage the packed words the
    uploaded reads give it: records and CIGARs of 400 pairs, path against path, and the uploaded path against the reference"""
    import torch
    g = b"".join(l.strip() for l in open(os.path.join(GOLDEN, "isolate.ref.fa"), "rb") if not l.startswith(b">"))
    concat, off = pmx.simulate_paired_reads(g, 400, read_len=151, seed=31)
    reads = [bytes(concat[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    al = pmx.Aligner(ctx, g, 151)
    up = pmx.ReadSet(ctx, reads)
    al.align_readset(up, paired=True, revcomp_mate2=True)
    u_recs, u_cig = al.fetch()
    first = ic.WRAP_PAD + 13
    buf = np.full(first + len(concat) + ic.WRAP_PAD + 16, ord("T"), np.uint8)
    buf[first:first + len(concat)] = concat
    d_c, d_o = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(off + first).to("cuda:0")
    assert d_c.data_ptr() % 16 == 0
    wr = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr(), len(reads), len(buf), 0, keepalive=(d_c, d_o))
    wr.pack()
    _assert_packed(wr.export_packed(), up.export_packed(), "wrapped against uploaded")
    _assert_packed(wr.export_packed(), ic.pack_reference(reads), "wrapped against the reference")
    al.align_readset(wr, paired=True, revcomp_mate2=True)
    w_recs, w_cig = al.fetch()
    assert len(u_recs) == len(w_recs) == len(reads)

    def ops(recs, cig):     # (a record's place in the CIGAR arena is the launch's affair)
        return [tuple(cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]) for r in recs]
    for f in ("rs", "re", "qs", "qe", "mapq", "rev", "proper_frag", "mapped", "n_cigar", "flags", "score"):
        assert np.array_equal(u_recs[f], w_recs[f]), f
    assert ops(u_recs, u_cig) == ops(w_recs, w_cig)
    host_rc = [r if i % 2 == 0 else pmx.reverse_complement(r) for i, r in enumerate(reads)]
    want = oracle.ref_align_reads_direct(g, host_rc, True, 8)
    bad = ac.compare_results(pmx.records_to_results(u_recs, u_cig, True), want)
    assert not bad, bad[:5]
    assert sum(w["mapped"] for w in want) > 350
    al.close(); up.close(); wr.close()
