"""GPU parity of the compact align tier's near class (k_compact_classes_near16/32 -> k_align_simple16/32; compact_near_class,
align/aln_compact_simple.hpp) on three families of tests/chain_near_cases.py -- overlaps of 1 .. 20 bases; the same with an
indel in every third read; overlaps of 15 .. 45 bases, where the junction rule goes both ways -- at 2,117 pairs each (one
2,048-position block of the class kernel and a second one that ends in a partial wave), through Aligner.align_readset, with
16- and with 32-bit position words, and against the same call without the class (PMX_ALIGN_NO_NEAR: the lists as the seeding
marks them).  Records and CIGAR operations in record order must be the reference's own aligner's (oracle/_ref) in both; the
compact tier must finish exactly as many pairs with the class as without it; the class's own counter must be positive with
it and zero without; and the counter of the pairs the seeding marks must not move."""
import pytest

import align_checks as ac
from chain_near_cases import GPU_FAMILIES, family_pairs

pytestmark = pytest.mark.gpu

N_PAIRS = 2117
FORMS = {"default": {}, "pos32": {"PMX_ALIGN_COMPACT_POS32": "1"}}

_cache = {}


def _family(sars, oracle, family):
    if family not in _cache:
        g = sars.genome("node_7618")
        reads = family_pairs(g, family, N_PAIRS)
        _cache[family] = (g, reads, oracle.ref_align_reads_direct(g, reads, True, 8))
    return _cache[family]


def _align(pmx, ctx, g, reads):
    al = pmx.Aligner(ctx, g, 150)
    rs = pmx.ReadSet(ctx, reads)
    al.align_readset(rs, paired=True, revcomp_mate2=False)
    recs, cig = al.fetch()
    st = al.stats()
    rs.close()
    al.close()
    return pmx.api.records_to_results(recs, cig, True), st


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("family", GPU_FAMILIES)
def test_near_class_equals_reference_and_the_tier_without_it(pmx, sars, oracle, ctx, family, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    g, reads, want = _family(sars, oracle, family)
    got, st = _align(pmx, ctx, g, reads)
    monkeypatch.setenv("PMX_ALIGN_NO_NEAR", "1")
    got_off, st_off = _align(pmx, ctx, g, reads)
    print("%s %s: compact_tier_items %d (without the class %d) of %d, near_chain_items %d, simple_chain_items %d (without the class %d)"
          % (family, form, st["compact_tier_items"], st_off["compact_tier_items"], st["n_items"], st["near_chain_items"],
             st["simple_chain_items"], st_off["simple_chain_items"]))
    for res in (got, got_off):
        bad = ac.compare_results(res, want)
        assert not bad, (family, form, bad[:5])
    assert st["n_items"] == N_PAIRS and st_off["n_items"] == N_PAIRS
    assert st["compact_tier_items"] == st_off["compact_tier_items"], (family, form, st, st_off)
    assert 0 < st["near_chain_items"] <= st["compact_tier_items"], (family, form, st)
    assert st_off["near_chain_items"] == 0, (family, form, st_off)
    assert st["simple_chain_items"] == st_off["simple_chain_items"], (family, form, st, st_off)
