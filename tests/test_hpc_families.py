"""Homopolymer compression on the CPU: the plain-Python restatement against the reference's pinned answers, the condition
every read family of tests/hpc_checks.py exists for, and -- with the oracle alone -- the property the mode is for: reads whose
only errors are run-length errors seed like the error-free reads."""
import numpy as np
import pytest

import hpc_checks as hc


def test_hpc_gives_the_reference_pinned_answers():
    """src/test/test_seeding.cpp:103-117"""
    assert hc.hpc(b"")[0] == b""
    assert hc.hpc(b"AAAA")[0] == b"A"
    assert hc.hpc(b"ACGT")[0] == b"ACGT"
    assert hc.hpc(b"AAACCCGGG")[0] == b"ACG"
    seq = b"AAACCCGGGT"
    c, m = hc.hpc(seq)
    assert c == b"ACGT" and len(m) == 4
    assert all(a < b for a, b in zip(m, m[1:]))
    assert all(seq[m[j]] == c[j] for j in range(4))
    # the comparison is on letters; the first character of a run gives its case
    assert hc.hpc(b"NNNN")[0] == b"N" and hc.hpc(b"RY")[0] == b"RY" and hc.hpc(b"aA")[0] == b"a" and hc.hpc(b"Aa")[0] == b"A"
    r, q = hc.hpc_reads([b"AAACCG", b"", b"TT"], [b"123456", b"", b"78"])
    assert r == [b"ACG", b"", b"T"] and q == [b"146", b"", b"7"]


@pytest.mark.parametrize("name", sorted(hc.FAMILIES))
def test_family_meets_its_condition(name):
    reads = hc.family(name)
    cond = hc.FAMILIES[name][1]
    assert cond.__doc__
    assert cond(reads), cond.__doc__
    assert reads == hc.family(name)   # reproducible


def test_families_together_are_about_3000_reads():
    assert 2500 <= len(hc.all_families()) <= 3500


def test_run_length_errors_vanish_under_hpc(oracle):
    rng = np.random.default_rng(4)
    clean = [hc.random_seq(rng, int(rng.integers(200, 3000))) for _ in range(60)]
    noisy = [hc.run_length_errors(rng, r) for r in clean]
    assert sum(a != b for a, b in zip(clean, noisy)) > 50
    assert all(hc.hpc(a)[0] == hc.hpc(b)[0] for a, b in zip(clean, noisy))
    for k, s, l in ((19, 8, 3), (15, 8, 1)):
        h0, c0 = oracle.histogram(hc.hpc_reads(clean), k, s, l)
        h1, c1 = oracle.histogram(hc.hpc_reads(noisy), k, s, l)
        assert len(h0) > 1000 and np.array_equal(h0, h1) and np.array_equal(c0, c1)
        # ... and they do not without the compression
        h2, _ = oracle.histogram(noisy, k, s, l)
        h3, _ = oracle.histogram(clean, k, s, l)
        assert not np.array_equal(h2, h3)
