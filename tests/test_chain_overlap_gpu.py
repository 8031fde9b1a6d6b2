"""GPU parity of the chain fill's dominated tail (align/aln_compact.hpp) on read pairs whose mates overlap on the
reference: the three cases of tests/chain_overlap_cases.py at 4,096 pairs each (64 waves of the chain kernel: every mix of
lanes that end their predecessor loop early and lanes that do not), through Aligner.align_readset, in the default form of the
compact tier, the fused kernel, 32-bit position words and the first form alone (PMX_ALIGN_NO_MULTI).  Records and CIGAR
operations must be the reference's own aligner's (oracle/_ref), and the compact tier must finish exactly as many pairs as the
commit before the dominated tail did on the same input (PARENT_ITEMS: `compact_tier_items` of the parent's library, run on
the same MI355X beside this one): a closed form must not change which pairs the tier finishes."""
import pytest

import align_checks as ac
from chain_overlap_cases import CASES, overlap_pairs

pytestmark = pytest.mark.gpu

N_PAIRS = 4096
FORMS = {
    "default": {},
    "fused": {"PMX_ALIGN_COMPACT_FUSED": "1"},
    "pos32": {"PMX_ALIGN_COMPACT_POS32": "1"},
    "no_multi": {"PMX_ALIGN_NO_MULTI": "1"},
}
PARENT_ITEMS = {
    ("clean", "default"): 4096, ("clean", "fused"): 3585, ("clean", "pos32"): 4096, ("clean", "no_multi"): 3485,
    ("subs", "default"): 3946, ("subs", "fused"): 3053, ("subs", "pos32"): 3946, ("subs", "no_multi"): 3018,
    ("indel", "default"): 1391, ("indel", "fused"): 1203, ("indel", "pos32"): 1391, ("indel", "no_multi"): 1177,
}

_cache = {}


def _case(sars, oracle, case):
    if case not in _cache:
        g = sars.genome("node_7618")
        reads = overlap_pairs(g, case, N_PAIRS)
        _cache[case] = (g, reads, oracle.ref_align_reads_direct(g, reads, True, 8))
    return _cache[case]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("case", CASES)
def test_overlapping_mates_equal_reference_and_parent_items(pmx, sars, oracle, ctx, case, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    g, reads, want = _case(sars, oracle, case)
    al = pmx.Aligner(ctx, g, 150)
    rs = pmx.ReadSet(ctx, reads)
    al.align_readset(rs, paired=True, revcomp_mate2=False)
    recs, cig = al.fetch()
    st = al.stats()
    rs.close()
    al.close()
    print("%s %s: compact_tier_items %d of %d" % (case, form, st["compact_tier_items"], st["n_items"]))
    got = pmx.api.records_to_results(recs, cig, True)
    bad = ac.compare_results(got, want)
    assert not bad, (case, form, bad[:5])
    assert all(x["flags"] & 3 == 0 for x in got), (case, form)
    assert st["n_items"] == N_PAIRS
    assert st["compact_tier_items"] == PARENT_ITEMS[case, form], (case, form, st)
