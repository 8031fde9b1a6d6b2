"""--meta --amplicon-depth and the relative-frequency masks on the device (pmx_meta_set_amplicons, pmx_meta_set_relative_masks;
panmap_amd/csrc/meta_mask.hip) against the restatement of tests/amplicon_checks.py, on the read family dealt into amplicons:
the (group, hash, count) triples, their per-hash sums, the surviving lists in the canonical order, multiplicities, the
amplicon of every merged read, the raw -> merged map, the per-group numbers and the three numbers the reference reports -- at
the default bound of the in-LDS counting path and with every read on the sorted path; then what runs on the survivors."""
import os

import numpy as np
import pytest

import amplicon_checks as amp
import mask_checks as mc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsv_meta(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    ctx = pmx.Context(0)
    return pm, ctx, pmx.Meta.build(ctx, pm)


def _read_side(meta, reads, groups, n_groups, setting):
    """set_reads under amplicons and the four parameters (all cleared again: the module's Meta is shared) -> the read side by name"""
    meta.set_amplicons(groups, n_groups)
    try:
        meta.set_masks(setting[0], setting[1])
        meta.set_relative_masks(setting[2], setting[3])
        meta.set_reads(reads)
    finally:
        meta.set_masks(0, 0)
        meta.set_relative_masks(0, 0)
        meta.set_amplicons(None)
    out = dict(lists=meta.read_seedmers(), info=meta.read_info(), raw_to_merged=meta.raw_to_merged(), mask_info=meta.mask_info(),
               amplicons=meta.read_amplicons(), amplicon_info=meta.amplicon_info())
    if any(setting):
        out["counts"] = meta.mask_counts()
        out["triples"] = meta.amplicon_counts()
    return out


def _check(got, merged, n_raw, where, setting):
    want = amp.restate_groups(merged, n_raw, *setting)
    if any(setting):
        g, h, c = got["triples"]
        assert g.dtype == np.int32 and h.dtype == np.uint64 and c.dtype == np.int64
        assert list(zip(g.tolist(), h.tolist(), c.tolist())) == want["triples"]
        ch, cc = got["counts"]
        assert np.array_equal(ch, np.array(sorted(want["counts"]), np.uint64))
        assert cc.tolist() == [want["counts"][x] for x in ch.tolist()]
        sums = {}
        for x, n in zip(h.tolist(), c.tolist()):
            sums[x] = sums.get(x, 0) + n
        assert sums == dict(zip(ch.tolist(), cc.tolist()))
    for g_arr, w_arr in zip(got["lists"], want["lists"]):
        assert np.array_equal(g_arr, w_arr)
    assert np.array_equal(got["info"][0], np.diff(want["lists"][0])) and np.array_equal(got["info"][1], want["mult"])
    assert np.array_equal(got["amplicons"], want["amplicons"])
    assert np.array_equal(got["raw_to_merged"], amp.raw_to_merged(where, want["old_to_new"]))
    info = got["amplicon_info"]
    assert list(zip(info["raw_reads"].tolist(), info["threshold"].tolist(), info["merged_before"].tolist(), info["merged_left"].tolist())) == want["info"]
    assert got["mask_info"] == dict(reads_dropped=want["reads_dropped"], seeds_removed=want["seeds_removed"], reads_left=len(want["mult"]))
    return want


@pytest.fixture(scope="module")
def dealt(rsv_meta):
    """the family under every setting of amp.SETTINGS at the default bound: computed once"""
    D = amp.family()
    return {s: _read_side(rsv_meta[2], D.reads, D.groups, len(D.group_names), s) for s in amp.SETTINGS}


@pytest.mark.parametrize("setting", amp.SETTINGS)
def test_read_side_equals_the_restatement(pmx, rsv_meta, dealt, setting):
    merged, n_raw, where = amp.family_merged()
    want = _check(dealt[setting], merged, n_raw, where, setting)
    assert len(want["mult"]) > 0


def test_groups_alone_run_no_mask_step(pmx, rsv_meta):
    pm, ctx, meta = rsv_meta
    D = amp.family()
    _read_side(meta, D.reads, D.groups, len(D.group_names), amp.SETTINGS[1])
    assert ctx.kernel_ms("meta_mask") > 0
    _read_side(meta, D.reads, D.groups, len(D.group_names), amp.SETTINGS[0])
    assert ctx.kernel_ms("meta_mask") < 0                             # no such span
    for getter in (meta.amplicon_counts, meta.mask_counts):
        with pytest.raises(pmx.PmxError):
            getter()


@pytest.mark.parametrize("setting", amp.SETTINGS[1:])
def test_sorted_path_equals_the_default_bound(rsv_meta, dealt, monkeypatch, setting):
    """PMX_META_MASK_LONG=1: every read with two seedmers or more is counted by the sorted path, on the pair ranks"""
    D = amp.family()
    merged, n_raw, where = amp.family_merged()
    monkeypatch.setenv("PMX_META_MASK_LONG", "1")
    got = _read_side(rsv_meta[2], D.reads, D.groups, len(D.group_names), setting)
    _check(got, merged, n_raw, where, setting)
    want = dealt[setting]
    for name in ("lists", "info", "counts", "triples"):
        assert all(np.array_equal(g, w) for g, w in zip(got[name], want[name])), name


def test_truncated_threshold(rsv_meta):
    D = amp.truncation_set()
    merged, n_raw, where = amp.merge_by_group(D.reads, D.groups, 1)
    setting = (0, 0, 0.29, 0.0)
    got = _read_side(rsv_meta[2], D.reads, D.groups, 1, setting)
    _check(got, merged, n_raw, where, setting)
    assert got["amplicon_info"]["threshold"].tolist() == [28, 0] and got["amplicon_info"]["raw_reads"].tolist() == [100, 1]
    assert sorted(got["info"][1].tolist()) == [1, 29, 43]


@pytest.mark.parametrize("setting", [(0, 0, 0.05, 0.0), (0, 0, 0.0, 0.05)])
def test_overlap_coefficients_and_scores_on_the_survivors(pmx, rsv_meta, setting):
    from oracle import oracle_meta as om
    pm, ctx, meta = rsv_meta
    D = amp.family()
    merged, n_raw, where = amp.family_merged()
    got = _read_side(meta, D.reads, D.groups, len(D.group_names), setting)
    _check(got, merged, n_raw, where, setting)
    off, h, rev = got["lists"]
    rng = np.random.default_rng(6)
    n_nodes = meta.index.info.n_nodes
    cands = np.unique(np.concatenate([rng.integers(0, n_nodes, 20), [0, n_nodes - 1, pm.find_node("MZ515733.1"), pm.find_node("node_1330")]])).astype(np.uint32)
    meta.score(candidates=cands)
    sc = meta.scores()
    assert sc.shape == (len(off) - 1, len(cands))
    read_hashes = set(h.tolist())
    unmasked_hashes = {int(x) for m in merged for x in m[1]}
    assert read_hashes < unmasked_hashes
    o_arr, u_arr = meta.index_oriented.arrays(), meta.index.arrays()
    for j, node in enumerate(cands.tolist()):
        want = om.read_scores(om.node_seed_counts(o_arr, node, read_hashes), off, h, rev)
        assert np.array_equal(sc[:, j].astype(np.int64), want), (node, np.nonzero(sc[:, j] != want)[0][:5])
    assert sc.max() > 20
    oc = meta.overlap_coefficients()
    for node in cands.tolist()[::6] + [pm.find_node("node_1330"), pm.find_node("MZ515733.1")]:
        assert abs(oc[node] - om.overlap_coefficient(u_arr, node, read_hashes)) < 1e-12, node


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def _tile(g, n, length=150):
    step = max(1, (len(g) - length) // n)
    return [g[i:i + length].encode() for i in range(0, len(g) - length + 1, step)][:n]


def _mixture_with_singletons():
    """the 70 / 30 mixture of test_meta_mask_gpu.py: 1,000 tiles of the two rsv genomes plus 40 of them with two substitutions
    each (their changed k-min-mers occur once)"""
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
    """mask_seeds 1 on the mixture dealt into three groups (reads [0, 400) and [400, 800) listed, the rest with the planted
    reads unlisted): the merged reads of the device equal the restatement, and the EM on them the numpy restatement of the EM,
    every proportion within 1e-9.  Consecutive tiles stay together, so within a group a k-min-mer keeps the coverage it has in
    the sample except at the ends of a block: both genomes stay covered and both haplotypes are found, as without groups."""
    from oracle import oracle_meta as om
    pm, ctx, meta = rsv_meta
    reads = _mixture_with_singletons()
    groups = np.minimum(np.arange(len(reads)) // 400, 2).astype(np.int32)
    merged, n_raw, where = amp.merge_by_group(reads, groups, 2)
    setting = (0, 1, 0.0, 0.0)
    got = _read_side(meta, reads, groups, 2, setting)
    _check(got, merged, n_raw, where, setting)
    assert got["mask_info"]["seeds_removed"] >= 40 and got["mask_info"]["reads_left"] == meta.n_reads
    meta.score(top_oc=50)
    haps = meta.em()
    sc = meta.scores().astype(np.int64)
    ns, mult = meta.read_info()
    cols, seen = [], {}
    for j in range(sc.shape[1]):
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


@pytest.mark.parametrize("setting", [(0, 0, 1e9, 0.0), (0, 0, 0.0, 1e9)])
def test_everything_masked_in_the_listed_groups(rsv_meta, setting):
    D = amp.family()
    merged, n_raw, where = amp.family_merged()
    got = _read_side(rsv_meta[2], D.reads, D.groups, len(D.group_names), setting)
    _check(got, merged, n_raw, where, setting)
    assert got["amplicon_info"]["merged_left"].tolist() == [0, 0, 0, 0, 6] and (got["amplicons"] == 4).all()
    assert got["amplicon_info"]["threshold"].tolist() == [40 * 10 ** 9, 48 * 10 ** 9, 3 * 10 ** 9, 0, 0]


def _bits(x):
    return np.atleast_1d(np.asarray(x, np.float64)).copy().view(np.uint64)


def _all_outputs(meta, reads):
    meta.set_reads(reads)
    meta.score(top_oc=1000)
    haps = meta.em()
    info = meta.em_info()
    out = dict(lists=meta.read_seedmers(), info=meta.read_info(), raw=(meta.raw_to_merged(),), oc=(_bits(meta.overlap_coefficients()),),
               candidates=(meta.candidates(),), scores=(meta.scores(),), haplotypes=[(n, int(_bits(p)[0]), m) for n, p, m in haps],
               em_info=(info["rounds"], info["iterations"], int(_bits(info["log_likelihood"])[0])), mask_info=meta.mask_info())
    if any(out["mask_info"][x] for x in ("reads_dropped", "seeds_removed")):
        out["counts"] = meta.mask_counts()
    return out


def _same(got, want):
    assert got.keys() == want.keys()
    for name in want:
        if name in ("haplotypes", "em_info", "mask_info"):
            assert got[name] == want[name], name
        else:
            assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got[name], want[name])), name


@pytest.mark.parametrize("mask_reads", [0, 1])
def test_one_unlisted_group_equals_no_amplicons(pmx, rsv_meta, mask_reads):
    """a table that lists none of the reads: one group, the unlisted one -- every array of the run without amplicons"""
    pm, ctx, meta = rsv_meta
    reads = mc.family().reads
    meta.set_masks(reads=mask_reads)
    try:
        want = _all_outputs(meta, reads)
        meta.set_amplicons(np.zeros(len(reads), np.int32), 0)
        got = _all_outputs(meta, reads)
        assert meta.read_amplicons().tolist() == [0] * meta.n_reads and meta.amplicon_info()["raw_reads"].tolist() == [len(reads)]
    finally:
        meta.set_masks(0, 0)
        meta.set_amplicons(None)
    assert want["scores"][0].size > 0 and want["scores"][0].max() > 20
    _same(got, want)


def test_one_meta_through_amplicons_on_off_on(pmx, rsv_meta, dealt):
    pm, ctx, meta = rsv_meta
    D = amp.family()
    mixture = _mixture_with_singletons()
    first = _read_side(meta, D.reads, D.groups, len(D.group_names), amp.SETTINGS[3])
    assert all(np.array_equal(g, w) for g, w in zip(first["lists"], dealt[amp.SETTINGS[3]]["lists"]))
    got = _all_outputs(meta, mixture)                                 # cleared: as a Meta that never saw amplicons
    with pytest.raises(pmx.PmxError):
        meta.read_amplicons()
    with pytest.raises(pmx.PmxError):
        meta.amplicon_info()
    fresh = pmx.Meta(ctx, meta.index, meta.index_oriented)
    want = _all_outputs(fresh, mixture)
    fresh.close()
    assert len(want["haplotypes"]) == 2
    _same(got, want)
    again = _read_side(meta, D.reads, D.groups, len(D.group_names), amp.SETTINGS[2])
    for name in ("lists", "info", "counts", "triples"):
        assert all(np.array_equal(g, w) for g, w in zip(again[name], dealt[amp.SETTINGS[2]][name])), name
    assert again["mask_info"] == dealt[amp.SETTINGS[2]]["mask_info"]


def test_refusals(pmx, rsv_meta):
    pm, ctx, meta = rsv_meta
    D = amp.family()
    try:
        with pytest.raises(pmx.PmxError):                             # a value out of range
            meta.set_amplicons(np.array([0, 5], np.int32), 4)
        with pytest.raises(pmx.PmxError):
            meta.set_amplicons(np.array([0, -1], np.int32), 4)
        meta.set_amplicons(D.groups[:-1], len(D.group_names))        # another number of reads
        with pytest.raises(pmx.PmxError, match="amplicons of 96"):
            meta.set_reads(D.reads)
        meta.set_amplicons(None)
        for bad in ((-0.1, 0), (0, -0.1)):
            with pytest.raises(pmx.PmxError):
                meta.set_relative_masks(*bad)
        meta.set_relative_masks(reads=0.05)                           # a relative parameter without amplicons
        with pytest.raises(pmx.PmxError, match="needs amplicons"):
            meta.set_reads(D.reads)
        for two in ((1, 0), (0, 1)):                                  # two parameters: whichever setter comes second
            with pytest.raises(pmx.PmxError, match="Only one masking parameter can be set at a time"):
                meta.set_masks(*two)
        with pytest.raises(pmx.PmxError, match="Only one masking parameter can be set at a time"):
            meta.set_relative_masks(0.05, 0.05)
        meta.set_relative_masks(0, 0)
        meta.set_masks(seeds=2)
        for two in ((0.1, 0), (0, 0.1)):
            with pytest.raises(pmx.PmxError, match="Only one masking parameter can be set at a time"):
                meta.set_relative_masks(*two)
        meta.set_masks(0, 0)
        meta.set_amplicons(D.groups, len(D.group_names))             # assign() on a read set with amplicons
        meta.set_reads(D.reads)
        with pytest.raises(pmx.PmxError, match="amplicons"):
            meta.assign()
    finally:
        meta.set_masks(0, 0)
        meta.set_relative_masks(0, 0)
        meta.set_amplicons(None)
    meta.set_reads(mc.family().tiles)                                 # cleared: the same Meta assigns again
    assert (meta.assign().state == 2).any()
