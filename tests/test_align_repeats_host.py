"""CPU tests of the ALIGN pipeline sources (tests/hostsim) on short pairs over repeat-bearing references
(align_checks.repeat_reference): mates with several candidate loci, secondaries, mapq below 60, pairing among candidates,
improper pairs -- what the SARS-CoV-2 inputs of tests/test_align_host.py never produce.  Every record the host build does not
flag must be the reference aligner's (oracle/_ref); tests/test_align_repeat_families.py shows that the reference itself
takes its repeat paths on these inputs, tests/test_align_repeats_gpu.py runs them through the HIP kernels."""
import ctypes as C
import os

import pytest

import align_checks as ac

SETS = [("small", f) for f in ac.REPEAT_FAMILIES] + [("large", "mixed")]
SITES = ("pair ends > 64", "pair logf", "chains > 64", "regions > 64", "mapq logf")


@pytest.fixture
def hs_env():
    """PMX_HS_* switches of the host build for the time of one test"""
    seen = []

    def set_(**kw):
        for k, v in kw.items():
            seen.append(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
    yield set_
    for k in seen:
        os.environ.pop(k, None)


def _unsupported_counts(reset=True):
    L = ac.hostsim(False)
    cnt = (C.c_longlong * len(SITES))()
    L.hs_unsupported_counts(cnt, int(reset))
    return dict(zip(SITES, [int(x) for x in cnt]))


@pytest.mark.parametrize("variant,name", SETS)
def test_wave_per_pair_form_at_the_huge_layouts_capacity(oracle, hs_env, variant, name):
    """anchor scale 16 (the wave tiers' last-resort layout): no pair flagged, every record the reference's"""
    ref, reads = ac.repeat_reads(variant, name)
    want = ac.repeat_want(oracle, variant, name)
    hs_env(PMX_HS_ANCHOR_SCALE=16)
    got = ac.hostsim_align(ref, reads, True)
    assert [i for i, x in enumerate(got) if x["flags"] & 3] == []
    bad = ac.compare_results(got, want)
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", ["exact_dup", "tandem", "high_copy"])
def test_single_end_at_the_huge_layouts_capacity(oracle, hs_env, name):
    ref, reads = ac.repeat_reads("small", name)
    want = ac.repeat_want(oracle, "small", name, paired=False)
    hs_env(PMX_HS_ANCHOR_SCALE=16)
    got = ac.hostsim_align(ref, reads, False)
    assert [i for i, x in enumerate(got) if x["flags"] & 3] == []
    bad = ac.compare_results(got, want)
    assert not bad, bad[:10]


def test_high_copy_overflows_one_general_layout(oracle, hs_env):
    """at anchor scale 1 (the general layout) pairs over the high-copy family come back PMX_REC_OVERFLOW: the family drives
    the capacity escalation of AlignStage::wave_tiers; what is not flagged is still exact"""
    ref, reads = ac.repeat_reads("small", "high_copy")
    want = ac.repeat_want(oracle, "small", "high_copy")
    hs_env(PMX_HS_ANCHOR_SCALE=1)
    got = ac.hostsim_align(ref, reads, True)
    over = [i for i, x in enumerate(got) if x["flags"] & 1]
    print("high_copy (%d copies) at anchor scale 1: %d of %d pairs OVERFLOW" % (ac.HIGH_COPIES, len(over), len(got)))
    assert len(over) >= 1
    keep = [i for i, x in enumerate(got) if not (x["flags"] & 3)]
    assert not ac.compare_results([got[i] for i in keep], [want[i] for i in keep])


@pytest.mark.parametrize("variant,name", SETS)
def test_thread_per_pair_dp_service_replay(oracle, variant, name):
    """the thread-per-pair control flow; pairs handed to the wave tiers (flag 0x8000) are excluded -- no floor on the share kept
    here: tandem and high-copy pairs are handed on nearly all the time"""
    ref, reads = ac.repeat_reads(variant, name)
    want = ac.repeat_want(oracle, variant, name)
    got = ac.hostsim_align(ref, reads, True, tpp=True)
    keep = [i for i, x in enumerate(got) if not (x["flags"] & 0x8000)]
    print(variant, name, "thread-per-pair form keeps %d of %d pairs" % (len(keep), len(got)))
    assert [i for i in keep if got[i]["flags"] & 3] == []
    bad = ac.compare_results([got[i] for i in keep], [want[i] for i in keep])
    assert not bad, bad[:10]


@pytest.mark.parametrize("form", ["first", "second", "first_split", "second_split", "first_pos32", "second_pos32", "second_split_pos32"])
@pytest.mark.parametrize("variant,name", SETS)
def test_compact_tier_forms(oracle, hs_env, variant, name, form):
    """every pair the compact tier finishes (first form, second form, fused and as two kernels, 16- and 32-bit position words)
    carries the reference's record; what it cannot decide it must hand on, not answer"""
    ref, reads = ac.repeat_reads(variant, name)
    want = ac.repeat_want(oracle, variant, name)
    hs_env(PMX_HS_COMPACT_MULTI="1" if form.startswith("second") else None, PMX_HS_COMPACT_SPLIT="1" if "split" in form else None,
           PMX_HS_COMPACT_POS32="1" if "pos32" in form else None)
    got, done = ac.hostsim_align_compact(ref, reads)
    idx = [i for i in range(len(want)) if done[i]]
    print(variant, name, form, "compact tier finishes %d of %d pairs" % (len(idx), len(want)))
    bad = ac.compare_results([got[i] for i in idx], [want[i] for i in idx])
    assert not bad, bad[:10]


def test_lowcx_pairs_exact_or_flagged(oracle, hs_env):
    """perfect dinucleotide and homopolymer runs reach PMX_REC_UNSUPPORTED (a mate with more than 64 chains, aln_hit.hpp gen_regs):
    a stated limit of the product, not a bug -- every pair is exact or flagged, and the sites that flag are
    counted.  20 pairs per run here (the host build takes 80 ms per such pair at anchor scale 16); with the 200 + 200 pairs of
    the GPU test it flags 194 of 200 over (AT)x100 (75 UNSUPPORTED only, 119 both bits) and 109 of 200 over Ax80 (46 and 63),
    every time at the `chains > 64` site."""
    ref, reads = ac.repeat_reads("small", "lowcx", 20)
    want = ac.repeat_want(oracle, "small", "lowcx", 20)
    assert all(w["mapped"] for w in want)
    hs_env(PMX_HS_ANCHOR_SCALE=16)
    _unsupported_counts()
    got = ac.hostsim_align(ref, reads, True, verbose=1)
    sites = _unsupported_counts()
    for part, sl in (("(AT)x100", slice(0, 20)), ("Ax80", slice(20, 40))):
        fl = [x["flags"] & 3 for x in got[sl]]
        print("lowcx %s: %d of %d pairs flagged (UNSUPPORTED only %d, OVERFLOW only %d, both %d)" %
              (part, sum(1 for f in fl if f), len(fl), fl.count(2), fl.count(1), fl.count(3)))
    print("lowcx: UNSUPPORTED set by", sites)
    keep = [i for i, x in enumerate(got) if not (x["flags"] & 3)]
    bad = ac.compare_results([got[i] for i in keep], [want[i] for i in keep])
    assert not bad, bad[:10]
    assert any(x["flags"] & 2 for x in got) and sites["chains > 64"] > 0      # (or DESIGN 7 item 8 is out of date again)
