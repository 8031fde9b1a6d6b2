"""The repeat families of tests/test_align_repeats_host.py and tests/test_align_repeats_gpu.py against the reference aligner alone
(no GPU, no product code): the inputs must make the reference itself take its repeat paths -- mates with several candidate
loci, mapping qualities below 60 and at 0, improper pairs, read 1 on both strands -- or the parity tests would pass on
inputs that exercise nothing.  The floors sit at about half of what the reference gave when the families were written
(seed 1), so a regenerated input survives them while one without repeats does not."""
import pytest

import align_checks as ac


def _mates(want):
    return [w[m] for w in want if w["mapped"] for m in ("r1", "r2")]


def test_reference_layout():
    """the generator is deterministic and gives the two variants their sizes (16-bit position words up to 32,767 bases)"""
    g = ac._isolate_genome()
    ref, fam = ac.repeat_variant("small")
    assert (ref, fam) == ac.repeat_reference(g, 1, 12000)
    assert len(ref) == 24830 and len(ac.repeat_variant("large")[0]) > 32767
    assert ref[:12000] == g[1000:13000]
    s, e = fam["exact_dup"][0]
    assert ref[s:e] == ref[2000:2800]
    assert [len(fam[k]) for k in ac.REPEAT_FAMILIES + ("lowcx",)] == [1, 1, 1, 1, 3, ac.HIGH_COPIES, 2]
    (s, e), (s2, e2) = fam["lowcx"]
    assert ref[s:e] == b"AT" * 100 and ref[s2:e2] == b"A" * 80
    assert ac.repeat_reads("small", "tandem")[1] == ac.pairs_over(ref, 300, 31 + 3, fam["tandem"][0][0] - 250, fam["tandem"][0][1] + 250)


@pytest.mark.parametrize("name", ac.REPEAT_FAMILIES + ("lowcx",))
def test_family_conditions(oracle, name):
    want = ac.repeat_want(oracle, "small", name)
    n = len(want)
    assert n == (400 if name == "lowcx" else 300)
    low = sum(1 for w in want if w["mapped"] and min(w["r1"]["mapq"], w["r2"]["mapq"]) < 60)
    rev1 = sum(1 for w in want if w["mapped"] and w["r1"]["rev"])
    print(name, "pairs %d mapped %d with a mate at mapq < 60: %d read 1 reverse: %d improper: %d" %
          (n, sum(w["mapped"] for w in want), low, rev1, sum(1 for w in want if w["mapped"] and not w["r1"]["proper_frag"])))
    assert all(w["mapped"] for w in want)        # the reference maps every pair of every family (lowcx included)
    if name in ("exact_dup", "tandem"):
        want200 = ac.repeat_want(oracle, "small", name, 200)
        low200 = sum(1 for w in want200 if w["mapped"] and min(w["r1"]["mapq"], w["r2"]["mapq"]) < 60)
        print(name, "200 pairs: with a mate at mapq < 60:", low200)
        assert 2 * low200 >= sum(w["mapped"] for w in want200)
    elif name != "lowcx":
        assert low >= 1
    if name == "inv_dup":
        assert 0 < rev1 < n


def test_mixed_set_conditions(oracle):
    want = ac.repeat_want(oracle, "large", "mixed")
    assert len(want) == 1800
    mates = _mates(want)
    mapq0 = sum(1 for m in mates if m["mapq"] == 0) / (2 * len(want))
    mid = sum(1 for m in mates if 0 < m["mapq"] < 60) / (2 * len(want))
    improper = sum(1 for w in want if w["mapped"] and not (w["r1"]["proper_frag"] and w["r2"]["proper_frag"])) / len(want)
    print("large mixed set: mates at mapq 0: %.3f, at 1..59: %.3f, improper mapped pairs: %.3f" % (mapq0, mid, improper))
    assert mapq0 >= 0.05
    assert mid >= 0.05
    assert improper >= 0.04
