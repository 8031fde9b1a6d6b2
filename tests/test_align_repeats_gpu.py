"""GPU parity of the ALIGN stage on short pairs over repeat-bearing references (align_checks.repeat_reference): a mate with
several candidate loci, mapq below 60, real secondaries, pairing among several candidates per mate, improper pairs -- and the
capacity escalation of the wave tiers (compact layout -> general layout -> the "huge" layout with 16x the anchors in HBM,
AlignStage::wave_tiers), which exists only on the GPU.  HIP kernels through the C ABI against the reference's own aligner
(oracle/_ref), bit-exact on pos / rs / re / qs / qe / mapq / rev / proper_frag / CIGAR.  tests/test_align_repeat_families.py
shows that the reference takes its repeat paths on these inputs; tests/test_align_repeats_host.py runs them on the host build."""
import numpy as np
import pytest

import align_checks as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["default_tiers", "compact_off", "dp_service_forced", "wave_per_pair_only"])
def _tier_mode(request, monkeypatch):
    """the four tier modes of tests/test_align_gpu.py: the library's own tier choice, the compact tier off, the compact tier off
    and the DP service + replay rounds forced, every pair on the wave-per-pair kernels"""
    if request.param == "compact_off":
        monkeypatch.setenv("PMX_ALIGN_NO_COMPACT", "1")
    elif request.param == "dp_service_forced":
        monkeypatch.setenv("PMX_ALIGN_NO_COMPACT", "1")
        monkeypatch.setenv("PMX_ALIGN_TPP_MIN", "0")
    elif request.param == "wave_per_pair_only":
        monkeypatch.setenv("PMX_ALIGN_NO_TPP", "1")
    yield request.param


def _check(pmx, ctx, oracle, variant, name, paired=True, n=None):
    ref, reads = ac.repeat_reads(variant, name, n)
    want = ac.repeat_want(oracle, variant, name, n, paired)
    al = pmx.Aligner(ctx, ref, 150)
    try:
        got = al.align_reads(reads, paired=paired)
        st = al.stats()
    finally:
        al.close()
    flagged = [(i, x["flags"] & 3) for i, x in enumerate(got) if x["flags"] & 3]
    bad = ac.compare_results(got, want)
    print(variant, name, "paired" if paired else "single", "differing fields %d flagged %d" % (len(bad), len(flagged)), st)
    assert not bad, bad[:10]
    assert not flagged, flagged[:10]
    return st


@pytest.mark.parametrize("name", ac.REPEAT_FAMILIES)
def test_family_pairs_exact(pmx, oracle, ctx, name):
    """300 pairs over one repeat family (+- 250 bases) of the 24,830-base reference"""
    _check(pmx, ctx, oracle, "small", name)


@pytest.mark.parametrize("name", ["exact_dup", "tandem", "high_copy"])
def test_family_single_end_exact(pmx, oracle, ctx, name):
    _check(pmx, ctx, oracle, "small", name, paired=False)


def test_high_copy_reaches_the_huge_layout(pmx, oracle, ctx, _tier_mode):
    """30 copies of a 150-base unit at 1 % divergence (align_checks.HIGH_COPIES): on the host build 272 of these 300 pairs
    overflow the general layout (anchor scale 1), and on the GPU both the general and the huge launch of the wave tiers run.
    The two counters only show that the launches ran; they are not thresholds."""
    st = _check(pmx, ctx, oracle, "small", "high_copy")
    if _tier_mode in ("default_tiers", "wave_per_pair_only"):
        assert st["general_tier_items"] > 0, st
        assert st["huge_tier_items"] > 0, st


def test_mixed_set_exact(pmx, oracle, ctx, _tier_mode):
    """1,800 pairs over all six families and the base of the 41.5 kb reference (32-bit position words in the compact tier)"""
    st = _check(pmx, ctx, oracle, "large", "mixed")
    if _tier_mode == "default_tiers":
        assert st["compact_tier_items"] > 0, st


def test_mixed_set_fused_compact_kernels(pmx, oracle, ctx, monkeypatch):
    monkeypatch.setenv("PMX_ALIGN_COMPACT_FUSED", "1")
    _check(pmx, ctx, oracle, "large", "mixed")


def test_small_mixed_set_with_32_bit_position_words(pmx, oracle, ctx, monkeypatch):
    monkeypatch.setenv("PMX_ALIGN_COMPACT_POS32", "1")
    _check(pmx, ctx, oracle, "small", "mixed")


def test_mixed_set_edit_counts(pmx, oracle, ctx):
    """score_reads: the edit counts --refine sums, against score_reads_vs_reference of the reference"""
    ref, reads = ac.repeat_reads("large", "mixed")
    al = pmx.Aligner(ctx, ref, 150)
    rs = pmx.ReadSet(ctx, reads)
    try:
        got = al.score_reads(rs, True, False)
    finally:
        rs.close()
        al.close()
    assert got == oracle.ref_score_reads(ref, reads, True)


def test_distinct_pair_map_on_repeats(pmx, oracle, ctx, monkeypatch):
    """the distinct-pair path (align_pairs.hip): every pair of the small mixed set three times, in shuffled order -- one
    representative runs, the copies take its records; all must be the reference's"""
    monkeypatch.setenv("PMX_ALIGN_DEDUP_DEPTH", "0")
    ref, reads = ac.repeat_reads("small", "mixed")
    want1 = ac.repeat_want(oracle, "small", "mixed")
    order = np.random.Generator(np.random.PCG64(5)).permutation(np.repeat(np.arange(len(reads) // 2), 3))
    tripled = [reads[2 * int(p) + s] for p in order for s in (0, 1)]
    want = [want1[int(p)] for p in order]
    al = pmx.Aligner(ctx, ref, 150)
    try:
        got = al.align_reads(tripled, paired=True)
    finally:
        al.close()
    bad = ac.compare_results(got, want)
    assert not bad, bad[:10]
    assert all(x["flags"] & 3 == 0 for x in got)
    plain = oracle.ref_align_reads_direct(ref, tripled[:600], True, 8)      # (the reference on copies gives what it gives on one)
    assert plain == want[:300]


def test_lowcx_pairs_exact_or_withheld(pmx, oracle, ctx):
    """THE DELIBERATELY WEAKER CHECK of this module: 200 pairs over (AT)x100 and 200 over Ax80 (+- 250 bases).  Perfect
    dinucleotide and homopolymer runs give a mate more than 64 chains, beyond what the pipeline orders as the reference does
    (PMX_REC_UNSUPPORTED): the reference maps every one of these pairs, the product withholds those it flags.
    Asserted: every pair is exact or flagged with mapped == 0 and no CIGAR, and the drop-in boundary reports the flagged ones
    unmapped and says so.  There is NO cap on the flagged share: no statement about the reference alone bounds it.  The
    counts are printed (host build, anchor scale 16: 194 of 200 and 109 of 200)."""
    ref, reads = ac.repeat_reads("small", "lowcx")
    want = ac.repeat_want(oracle, "small", "lowcx")
    al = pmx.Aligner(ctx, ref, 150)
    try:
        got = al.align_reads(reads, paired=True)
    finally:
        al.close()
    for part, sl in (("(AT)x100", slice(0, 200)), ("Ax80", slice(200, 400))):
        fl = [x["flags"] & 3 for x in got[sl]]
        print("lowcx %s: %d of %d pairs flagged (OVERFLOW only %d, UNSUPPORTED only %d, both bits %d)" %
              (part, sum(1 for f in fl if f), len(fl), fl.count(1), fl.count(2), fl.count(3)))
    keep = [i for i, x in enumerate(got) if not (x["flags"] & 3)]
    for i, x in enumerate(got):
        if x["flags"] & 3:
            assert x["mapped"] == 0 and x["r1"]["cigar"] == [] and x["r2"]["cigar"] == [], i
    bad = ac.compare_results([got[i] for i in keep], [want[i] for i in keep])
    assert not bad, bad[:10]
    direct = pmx.align_reads_direct(ref, reads, True, 1)
    err = pmx.last_error()
    flagged = [i for i, x in enumerate(got) if x["flags"] & 3]
    assert flagged and b"withheld" in err, err
    for i in flagged:
        assert direct[i]["mapped"] == 0 and direct[i]["r1"]["cigar"] == [] and direct[i]["r1"]["pos"] == 2147483647, i
    assert not ac.compare_results([direct[i] for i in keep], [want[i] for i in keep])
