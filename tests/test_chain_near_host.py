"""The compact align tier's near class -- mates whose extents overlap on the reference while their seeds do not, put on the
register-only chain path by the junction rule compact_near_class (align/aln_compact_simple.hpp) -- in the host build of the
kernel source (tests/hostsim/chain_near.cpp), CPU only: 2,048 pairs per family of tests/chain_near_cases.py.

compact_seed_pair -> the class as k_compact_classes_near16/32 decide it -> compact_chain_simple, beside the first and the second
form of the chain kernel.  For every pair the path finishes, the records, the CIGAR word and the edit counts must be
compact_chain_pair's (the first form, which must finish the pair too) and the reference's own aligner's (oracle/_ref).  For
every pair it bails on, the second form -- where such a pair goes -- must give the reference's record when it finishes it.  A
pair with a gapped read must bail, and mates that overlap by 50 bases and more (they share minimizers) are never classed.
So that the test cannot pass by bailing or by classing nothing: the error-free family with overlaps of 1 .. 20 bases must
finish at least 90 % of its pairs on the path (the first form alone finishes 2,026 of its 2,048, asserted below), and
CLASSED / DONE hold every family's counts, so that a change of the rule or of a bail condition shows."""
import numpy as np
import pytest

import align_checks as ac
from chain_near_cases import FAMILIES, family_pairs, host_chain_near

N_PAIRS = 2048
# per family: pairs the first form finishes / pairs classed near / pairs of the near class the path finishes
FIRST_DONE = {"near": 2026, "near_subs": 1984, "near_strands": 2024, "near_indel": 674, "edge": 2018, "deep": 1621}
CLASSED = {"near": 2009, "near_subs": 2029, "near_strands": 2017, "near_indel": 2027, "edge": 746, "deep": 0}
DONE = {"near": 2009, "near_subs": 1974, "near_strands": 2017, "near_indel": 671, "edge": 746, "deep": 0}
CASES = [(f, False, False) for f in FAMILIES] + [(f, True, False) for f in ("near", "near_strands", "edge")] + [("near_subs", False, True)]

_cache = {}


def _family(sars, oracle, family):
    if family not in _cache:
        g = sars.genome("node_7618")
        reads = family_pairs(g, family, N_PAIRS)
        _cache[family] = (g, reads, oracle.ref_align_reads_direct(g, reads, True, 8))
    return _cache[family]


@pytest.mark.parametrize("family,pos32,want_edits", CASES)
def test_near_class_equals_first_form_and_reference(sars, oracle, tmp_path_factory, family, pos32, want_edits):
    g, reads, want = _family(sars, oracle, family)
    cls, bound, forms = host_chain_near(tmp_path_factory.getbasetemp(), g, reads, pos32, want_edits)
    (r_s, d_s, e_s), (r_1, d_1, e_1), (r_2, d_2, e_2) = forms
    fin = [i for i in range(N_PAIRS) if cls[i] in (2, 4)]
    bailed = [i for i in range(N_PAIRS) if cls[i] in (3, 5)]
    n_near, n_done = int((cls >= 4).sum()), int((cls == 4).sum())
    print("%s pos32=%d edits=%d: seeding bailed %d, neither class %d, marked by the seeding %d (finished %d), near %d (finished %d); "
          "first form finished %d; extents overlap by less than k: %d"
          % (family, pos32, want_edits, int((cls == 0).sum()), int((cls == 1).sum()), int(((cls == 2) | (cls == 3)).sum()), int((cls == 2).sum()),
             n_near, n_done, int(d_1.sum()), int(bound.sum())))
    assert all(d_1[i] for i in fin), (family, [i for i in fin if not d_1[i]][:5])
    differ = [i for i in fin if r_s[i] != r_1[i] or e_s[2 * i] != e_1[2 * i] or e_s[2 * i + 1] != e_1[2 * i + 1]]
    assert not differ, (family, differ[:5])
    bad = ac.compare_results([r_s[i] for i in fin], [want[i] for i in fin])
    assert not bad, (family, bad[:5])
    if fin and not want_edits:   # (a pair the reference leaves unmapped counts its read lengths on both sides)
        sub = [reads[2 * i + s] for i in fin for s in (0, 1)]
        assert int(sum(int(e_s[2 * i]) + int(e_s[2 * i + 1]) for i in fin)) == -oracle.ref_score_reads(g, sub, True), family
    again = [i for i in bailed if d_2[i]]
    bad = ac.compare_results([r_2[i] for i in again], [want[i] for i in again])
    assert not bad, (family, bad[:5])
    if not want_edits:
        assert (int(d_1.sum()), n_near, n_done) == (FIRST_DONE[family], CLASSED[family], DONE[family]), family
    if family == "near":
        assert int(d_1.sum()) >= 0.9 * N_PAIRS   # (what the cap below may ask for)
        assert len(fin) >= 0.9 * N_PAIRS, (len(fin), n_done)
    if family == "near_indel":   # a pair with a gapped read must bail (every third READ carries an indel)
        gapped = {i // 2 for i in range(0, 2 * N_PAIRS, 3)}
        assert not [i for i in fin if i in gapped]
    if family == "deep":
        assert n_near == 0 and not fin and not bailed
