"""GPU parity of the compact align tier's register-only chain kernel (k_align_simple16/32, align/aln_compact_simple.hpp) on
the first, third, fifth and seventh family of tests/chain_simple_cases.py -- mates apart; the same with an indel in every third
read; both classes in every wave; the junction beyond the chaining distance -- at 4,096 pairs each (64 waves), through
Aligner.align_readset, with 16- and with 32-bit position words, and against the same call without the kernel
(PMX_ALIGN_NO_SIMPLE: every pair through k_align_compact).  Records and CIGAR operations in record order must be the
reference's own aligner's (oracle/_ref) in both; the compact tier must finish exactly as many pairs with the kernel as
without it; and the kernel's own counter must be positive (every family has pairs whose mates lie apart) and zero without it.
The family whose mates all overlap keeps the counter at zero."""
import pytest

import align_checks as ac
from chain_simple_cases import GPU_FAMILIES, family_pairs

pytestmark = pytest.mark.gpu

N_PAIRS = 4096
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
def test_simple_kernel_equals_reference_and_the_tier_without_it(pmx, sars, oracle, ctx, family, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    g, reads, want = _family(sars, oracle, family)
    got, st = _align(pmx, ctx, g, reads)
    monkeypatch.setenv("PMX_ALIGN_NO_SIMPLE", "1")
    got_off, st_off = _align(pmx, ctx, g, reads)
    print("%s %s: compact_tier_items %d (without the kernel %d) of %d, simple_chain_items %d"
          % (family, form, st["compact_tier_items"], st_off["compact_tier_items"], st["n_items"], st["simple_chain_items"]))
    for res in (got, got_off):
        bad = ac.compare_results(res, want)
        assert not bad, (family, form, bad[:5])
        assert all(x["flags"] & 3 == 0 for x in res), (family, form)
    assert st["n_items"] == N_PAIRS and st_off["n_items"] == N_PAIRS
    assert st["compact_tier_items"] == st_off["compact_tier_items"], (family, form, st, st_off)
    assert 0 < st["simple_chain_items"] <= st["compact_tier_items"], (family, form, st)
    assert st_off["simple_chain_items"] == 0, (family, form, st_off)


def test_overlapping_mates_never_reach_the_simple_kernel(pmx, sars, oracle, ctx):
    g, reads, want = _family(sars, oracle, "overlap")
    got, st = _align(pmx, ctx, g, reads)
    bad = ac.compare_results(got, want)
    assert not bad, bad[:5]
    assert st["simple_chain_items"] == 0, st
