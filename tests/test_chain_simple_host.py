"""The compact align tier's register-only chain path for mates that do not overlap on the reference
(align/aln_compact_simple.hpp) in the host build of the kernel source (tests/hostsim/chain_simple.cpp), CPU only: 2,048 pairs
per family of tests/chain_simple_cases.py.

For every pair the path finishes, the records, the CIGAR word and the edit counts must be compact_chain_pair's (the first form
of the chain kernel, which must finish the pair too: the path may not widen the set of pairs the first form finishes) and the
reference's own aligner's (oracle/_ref; edit counts: the sum over the finished pairs against score_reads_vs_reference).  For
every pair it bails on, the second form -- where such a pair goes -- must give the reference's record when it finishes it.
So that the test cannot pass by bailing: in the two error-free families with mates apart ("clean", "strands") every pair the
first form finishes must be finished by the new path, and FIRST_DONE holds the number of pairs the first form finished at the
commit before this path existed (tests/hostsim with PMX_HS_COMPACT_SPLIT on the same reads).  The other families hold their
counts of finished pairs too (SIMPLE_DONE), so that a change of the class or of a bail condition shows."""
import numpy as np
import pytest

import align_checks as ac
from chain_simple_cases import FAMILIES, family_pairs, host_chain_simple

N_PAIRS = 2048
# pairs the first form finished before this path existed / pairs the new path finishes
FIRST_DONE = {"clean": 2010, "subs": 1998, "indel": 669, "strands": 2004, "mixed": 2013, "overlap": 1727, "far": 2012, "len160": 1743,
              "len75": 2048, "sparse": 2048, "ends": 2048}
SIMPLE_DONE = {"clean": 2010, "subs": 1998, "indel": 669, "strands": 2004, "mixed": 1018, "overlap": 0, "far": 2012, "len160": 1743,
               "len75": 2048, "sparse": 2048, "ends": 2048}
CASES = [(f, False, False) for f in FAMILIES] + [(f, True, False) for f in ("clean", "strands", "mixed", "far")] + [("subs", False, True)]

_cache = {}


def _family(sars, oracle, family):
    if family not in _cache:
        g = sars.genome("node_7618")
        reads = family_pairs(g, family, N_PAIRS)
        _cache[family] = (g, reads, oracle.ref_align_reads_direct(g, reads, True, 8))
    return _cache[family]


@pytest.mark.parametrize("family,pos32,want_edits", CASES)
def test_simple_path_equals_first_form_and_reference(sars, oracle, tmp_path_factory, family, pos32, want_edits):
    g, reads, want = _family(sars, oracle, family)
    cls, forms = host_chain_simple(tmp_path_factory.getbasetemp(), g, reads, pos32, want_edits)
    (r_s, d_s, e_s), (r_1, d_1, e_1), (r_2, d_2, e_2) = forms
    fin = [i for i in range(N_PAIRS) if cls[i] == 2]
    bailed = [i for i in range(N_PAIRS) if cls[i] == 3]
    print("%s pos32=%d edits=%d: seeding bailed %d, not simple %d, finished %d, bailed %d; first form finished %d"
          % (family, pos32, want_edits, int((cls == 0).sum()), int((cls == 1).sum()), len(fin), len(bailed), int(d_1.sum())))
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
        assert int(d_1.sum()) == FIRST_DONE[family]
        assert len(fin) == SIMPLE_DONE[family]
    if family in ("clean", "strands"):
        assert all(cls[i] == 2 for i in range(N_PAIRS) if d_1[i]), family
    if family == "indel":   # a pair with a gapped read must bail (every third READ carries an indel)
        gapped = {i // 2 for i in range(0, 2 * N_PAIRS, 3)}
        assert not [i for i in fin if i in gapped]
    if family == "overlap":
        assert not fin and not bailed
