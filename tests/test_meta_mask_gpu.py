"""--meta --mask-reads / --mask-seeds on the device (pmx_meta_set_masks, panmap_amd/csrc/meta_mask.hip) against the literal
restatement of the reference's loops (tests/mask_checks.py; src/mgsr.cpp:2049-2139), on the read family of that module: the
occurrence counts hash by hash, the surviving lists in their order, multiplicities, the raw -> merged map and the three numbers
the reference reports, at the default bound of the in-LDS counting path and with every read forced onto the sorted path; then
what runs on the survivors -- overlap coefficients, scores, EM."""
import os

import numpy as np
import pytest

import mask_checks as mc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsv_meta(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    ctx = pmx.Context(0)
    return pm, ctx, pmx.Meta.build(ctx, pm)


def _read_side(meta, reads, mask_reads, mask_seeds):
    """set_reads under the masks (cleared again: the module's Meta is shared) -> the read side by name"""
    meta.set_masks(mask_reads, mask_seeds)
    try:
        meta.set_reads(reads)
    finally:
        meta.set_masks(0, 0)
    out = dict(lists=meta.read_seedmers(), info=meta.read_info(), raw_to_merged=meta.raw_to_merged(), mask_info=meta.mask_info())
    if mask_reads or mask_seeds:
        out["counts"] = meta.mask_counts()
    return out


@pytest.fixture(scope="module")
def baseline(rsv_meta):
    """the family without masks: the merged lists the restatement starts from.  They equal the from-the-string restatement
    (as test_meta_gpu.py holds them), so nothing of the product is in what the masked runs are compared with."""
    got = _read_side(rsv_meta[2], mc.family().reads, 0, 0)
    off, h, rev, mult, raw_to_merged = mc.family_merged()
    assert np.array_equal(got["lists"][0], off) and np.array_equal(got["lists"][1], h) and np.array_equal(got["lists"][2], rev)
    assert np.array_equal(got["info"][1], mult) and np.array_equal(got["raw_to_merged"], raw_to_merged)
    assert got["mask_info"] == dict(reads_dropped=0, seeds_removed=0, reads_left=len(mult))
    return got


@pytest.fixture(scope="module")
def masked(rsv_meta, baseline):
    """the family under every mask of mc.MASKS at the default bound: computed once"""
    return {mk: _read_side(rsv_meta[2], mc.family().reads, *mk) for mk in mc.MASKS}


def _check_read_side(got, baseline, mask_reads, mask_seeds):
    off, h, rev = baseline["lists"]
    ns, mult = baseline["info"]
    w_off, w_h, w_rev, w_mult, to, n_dropped, n_removed, counts = mc.restate_masks(off, h, rev, mult, mask_reads, mask_seeds)
    ch, cc = got["counts"]
    assert np.array_equal(ch, np.array(sorted(counts), np.uint64))                       # every distinct hash before masking, ascending
    wrong = [int(x) for x, c in zip(ch.tolist(), cc.tolist()) if counts[x] != c]
    assert not wrong, (len(wrong), wrong[:5])
    g_off, g_h, g_rev = got["lists"]
    assert np.array_equal(g_off, w_off) and np.array_equal(g_h, w_h) and np.array_equal(g_rev, w_rev)
    assert np.array_equal(got["info"][0], np.diff(w_off)) and np.array_equal(got["info"][1], w_mult)
    base_raw = baseline["raw_to_merged"]
    assert np.array_equal(got["raw_to_merged"], np.where(base_raw >= 0, to[np.maximum(base_raw, 0)], -1))
    assert got["mask_info"] == dict(reads_dropped=n_dropped, seeds_removed=n_removed, reads_left=len(w_mult))


@pytest.mark.parametrize("mask", mc.MASKS)
def test_read_side_equals_the_restatement(masked, baseline, mask):
    got = masked[mask]
    _check_read_side(got, baseline, *mask)
    assert 0 < len(got["info"][1]) and (len(got["info"][1]) < len(baseline["info"][1]) or len(got["lists"][1]) < len(baseline["lists"][1]))


@pytest.mark.parametrize("mask", mc.MASKS)
def test_sorted_path_equals_the_default_bound(rsv_meta, masked, baseline, monkeypatch, mask):
    """PMX_META_MASK_LONG=1: every read with two seedmers or more is counted by the sorted path (at the default bound only the
    20 kb read is); the same counts, lists and numbers"""
    ns = baseline["info"][0]
    assert (ns > 1024).sum() == 1 and (ns > 1).sum() > 50 and (ns == 1).sum() >= 1
    monkeypatch.setenv("PMX_META_MASK_LONG", "1")
    got = _read_side(rsv_meta[2], mc.family().reads, *mask)
    _check_read_side(got, baseline, *mask)
    want = masked[mask]
    for name in ("lists", "info", "counts"):
        assert all(np.array_equal(g, w) for g, w in zip(got[name], want[name])), name
    assert np.array_equal(got["raw_to_merged"], want["raw_to_merged"]) and got["mask_info"] == want["mask_info"]


@pytest.mark.parametrize("mask", [(1, 0), (0, 1)])
def test_overlap_coefficients_and_scores_on_the_survivors(pmx, rsv_meta, baseline, mask):
    """the overlap coefficients' numerator set is the surviving hashes; every (read, candidate) score is of the masked lists"""
    from oracle import oracle_meta as om
    pm, ctx, meta = rsv_meta
    got = _read_side(meta, mc.family().reads, *mask)
    _check_read_side(got, baseline, *mask)
    off, h, rev = got["lists"]
    rng = np.random.default_rng(5)
    n_nodes = meta.index.info.n_nodes
    cands = np.unique(np.concatenate([rng.integers(0, n_nodes, 40), [0, n_nodes - 1, pm.find_node("MZ515733.1"), pm.find_node("node_1330")]])).astype(np.uint32)
    meta.score(candidates=cands)
    assert np.array_equal(meta.candidates(), cands)
    sc = meta.scores()
    assert sc.shape == (len(off) - 1, len(cands))
    read_hashes = set(h.tolist())
    assert read_hashes < set(baseline["lists"][1].tolist())                                # (hashes left the sample)
    o_arr, u_arr = meta.index_oriented.arrays(), meta.index.arrays()
    for j, node in enumerate(cands.tolist()):
        want = om.read_scores(om.node_seed_counts(o_arr, node, read_hashes), off, h, rev)
        assert np.array_equal(sc[:, j].astype(np.int64), want), (node, np.nonzero(sc[:, j] != want)[0][:5])
    assert sc.max() > 20
    oc =meta.overlap_coefficients()
    unmasked_hashes = set(baseline["lists"][1].tolist())
    differs = 0
    for node in cands.tolist()[::6] + [pm.find_node("node_1330")]:
        want = om.overlap_coefficient(u_arr, node, read_hashes)
        assert abs(oc[node] - want) < 1e-12, node
        differs += want != om.overlap_coefficient(u_arr, node, unmasked_hashes)
    assert differs > 0                                                                     # (the unmasked hash set would not have passed)


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def _tile(g, n, length=150):
    step = max(1, (len(g) - length) // n)
    return [g[i:i + length].encode() for i in range(0, len(g) - length + 1, step)][:n]


def _mixture_with_singletons():
    """the 70 / 30 mixture of test_meta_gpu.py plus 40 of its reads with two substitutions each: their changed k-min-mers
    occur once"""
    a, b = _fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    reads = _tile(a, 700) + _tile(b, 300)
    rng = np.random.default_rng(70)
    planted = []
    for r in reads[::25]:
        q = bytearray(r)
        for p in rng.choice(len(q), 2, replace=False):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4] if q[p] in b"ACGT" else q[p]
        planted.append(bytes(q))
    return reads + planted


def test_em_on_the_masked_rows(pmx, rsv_meta):
    """mask_seeds 1 on the mixture with planted singletons: the same nodes as the numpy restatement of the EM on the masked
    rows, every proportion within 1e-9 (the tolerance test_meta_gpu.py holds the unmasked EM to)"""
    from oracle import oracle_meta as om
    pm, ctx, meta = rsv_meta
    reads = _mixture_with_singletons()
    unmasked = _read_side(meta, reads, 0, 0)
    got = _read_side(meta, reads, 0, 1)
    _check_read_side(got, unmasked, 0, 1)
    assert got["mask_info"]["seeds_removed"] >= 40 and got["mask_info"]["reads_left"] == meta.n_reads
    meta.score(top_oc=50)
    haps = meta.em()
    sc = meta.scores().astype(np.int64)
    ns, mult = meta.read_info()
    assert np.array_equal(ns, np.diff(got["lists"][0]))
    cols, seen = [], {}
    for j in range(sc.shape[1]):                                      # equal score columns are one column (lowest candidate first)
        key = sc[:, j].tobytes()
        if key not in seen:
            seen[key] = j
            cols.append(j)
    rows = sc.max(axis=1) > 0
    kept, props = om.square_em(sc[rows][:, cols], ns[rows], mult[rows])
    cands = meta.candidates()
    want = sorted(((float(p), int(cands[cols[k]])) for k, p in zip(kept, props)), reverse=True)
    assert [n for _, n in want] == [n for n, _, _ in haps] and len(haps) >= 2
    assert np.allclose([p for p, _ in want], [p for _, p, _ in haps], rtol=0, atol=1e-9)


@pytest.mark.parametrize("mask", [(10 ** 9, 0), (0, 10 ** 9)])
def test_everything_masked(rsv_meta, baseline, mask):
    pm, ctx, meta = rsv_meta
    got = _read_side(meta, mc.family().reads, *mask)
    _check_read_side(got, baseline, *mask)
    n, n_entries = len(baseline["info"][1]), len(baseline["lists"][1])
    assert got["mask_info"] == dict(reads_dropped=n if mask[0] else 0, seeds_removed=0 if mask[0] else n_entries, reads_left=0)
    assert meta.n_reads == 0 and (got["raw_to_merged"] == -1).all() and got["lists"][0].tolist() == [0]
    assert not meta.overlap_coefficients().any()
    meta.score(top_oc=1000)
    assert meta.em() == [] and meta.haplotypes() == []
    info = meta.em_info()
    assert info["rounds"] == 0 and info["iterations"] == 0


def _bits(x):
    return np.atleast_1d(np.asarray(x, np.float64)).copy().view(np.uint64)


def _all_outputs(meta, reads):
    meta.set_reads(reads)
    meta.score(top_oc=1000)
    haps = meta.em()
    info = meta.em_info()
    return dict(lists=meta.read_seedmers(), info=meta.read_info(), raw=(meta.raw_to_merged(),), oc=(_bits(meta.overlap_coefficients()),),
                candidates=(meta.candidates(),), scores=(meta.scores(),), haplotypes=[(n, int(_bits(p)[0]), m) for n, p, m in haps],
                em_info=(info["rounds"], info["iterations"], int(_bits(info["log_likelihood"])[0])))


def test_one_meta_through_masks_on_off_on(pmx, rsv_meta, masked, baseline):
    """masks on, off, on again with another threshold, across two read sets: the masked legs equal the restatement, the
    unmasked leg equals a fresh Meta that never saw a mask, bit for bit"""
    pm, ctx, meta = rsv_meta
    family, mixture = mc.family().reads, _mixture_with_singletons()
    meta.set_masks(seeds=1)
    meta.set_reads(family)
    assert all(np.array_equal(g, w) for g, w in zip(meta.read_seedmers(), masked[(0, 1)]["lists"]))
    meta.set_masks(0, 0)
    got = _all_outputs(meta, mixture)
    assert meta.mask_info() == dict(reads_dropped=0, seeds_removed=0, reads_left=meta.n_reads)
    with pytest.raises(pmx.PmxError):
        meta.mask_counts()
    fresh = pmx.Meta(ctx, meta.index, meta.index_oriented)
    want = _all_outputs(fresh, mixture)
    fresh.close()
    assert got.keys() == want.keys() and len(want["haplotypes"]) == 2
    for name in want:
        if name in ("haplotypes", "em_info"):
            assert got[name] == want[name], name
        else:
            assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got[name], want[name])), name
    meta.set_masks(reads=2)
    meta.set_reads(family)
    meta.set_masks(0, 0)
    assert all(np.array_equal(g, w) for g, w in zip(meta.read_seedmers(), masked[(2, 0)]["lists"]))
    assert meta.mask_info() == masked[(2, 0)]["mask_info"]


_NOTHING_TO_MASK = {"no_reads": [], "no_seedmers": [b"ACGTTGCAAC", b"TTGACCATGA", b"GATTACAGTC"]}   # (10 bases: below k, no seedmer)


@pytest.mark.parametrize("reads", sorted(_NOTHING_TO_MASK))
@pytest.mark.parametrize("setting", [(1, 0), (0, 1), "amplicons"], ids=["mask_reads", "mask_seeds", "amplicons_relative"])
def test_a_sample_without_merged_reads(rsv_meta, masked, setting, reads):
    """set_reads of no reads, and of three reads that yield no seedmer, under a mask: the mask step ends before it allocates or
    launches anything.  No error, mask_info all zeros, no counts, no "meta_mask" span (the fixtures' masked runs left one), and
    the Meta is as good as before: the family under the same mask equals the fixture's result.  "amplicons": two amplicon
    groups (the reads alternate between the first one and the unlisted one) and --mask-reads-relative-frequency 0.5; the family
    then follows under mask_reads 1, without amplicons, which the fixture holds."""
    pm, ctx, meta = rsv_meta
    sample = _NOTHING_TO_MASK[reads]
    mask = (1, 0) if setting == "amplicons" else setting
    if setting == "amplicons":
        meta.set_amplicons(np.array([0, 2, 0][:len(sample)], np.int32), 2)
        meta.set_relative_masks(reads=0.5)
    else:
        meta.set_masks(*mask)
    try:
        meta.set_reads(sample)
    finally:
        meta.set_masks(0, 0)
        meta.set_relative_masks(0, 0)
        meta.set_amplicons(None)
    assert meta.n_reads == 0
    assert meta.mask_info() == dict(reads_dropped=0, seeds_removed=0, reads_left=0)
    ch, cc = meta.mask_counts()
    assert len(ch) == 0 and len(cc) == 0
    assert ctx.kernel_ms("meta_mask") < 0
    got, want = _read_side(meta, mc.family().reads, *mask), masked[mask]
    for name in ("lists", "info", "counts"):
        assert all(np.array_equal(g, w) for g, w in zip(got[name], want[name])), name
    assert np.array_equal(got["raw_to_merged"], want["raw_to_merged"]) and got["mask_info"] == want["mask_info"]
    assert ctx.kernel_ms("meta_mask") >= 0


def test_refusals(pmx, rsv_meta):
    pm, ctx, meta = rsv_meta
    with pytest.raises(pmx.PmxError, match="Only one masking parameter can be set at a time"):
        meta.set_masks(1, 1)
    for bad in ((-1, 0), (0, -1)):
        with pytest.raises(pmx.PmxError):
            meta.set_masks(*bad)
    meta.set_masks(seeds=1)
    try:
        meta.set_reads(mc.family().reads)
    finally:
        meta.set_masks(0, 0)
    with pytest.raises(pmx.PmxError, match="mask"):
        meta.assign()
    meta.set_reads(mc.family().tiles)                                 # without a mask the same Meta assigns again
    assert (meta.assign().state == 2).any()
