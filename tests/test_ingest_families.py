"""The reference and the read sets of tests/test_ingest_gpu.py on their own (no GPU): pack_reference gives the hand-worked
words, unpacks to the reads it was given, and the sets reach the kernel edges they were built for -- computed here from
lengths and offsets alone -- or the GPU comparison would pass on sets that test nothing."""
import numpy as np
import pytest

import ingest_checks as ic

E4 = 0xE4E4E4E4E4E4E4E4     # ACGT x 8: codes 0 1 2 3 from the low bits up, 0xE4 per four bases


def _rec(words, amb, length):
    r = np.zeros(64, np.uint8)
    r.view(np.uint64)[:len(words)] = words
    r.view(np.uint32)[10:10 + len(amb)] = amb
    r.view(np.uint32)[15] = length
    return r


def test_pack_reference_on_hand_worked_reads():
    # 33 bases: two words; the N at base 32 is bit 0 of the second ambiguity word, its code 0
    w, a, woff, rec = ic.pack_reference([b"ACGT" * 8 + b"N"])
    assert w.dtype == np.uint64 and a.dtype == np.uint32 and woff.dtype == np.int64 and rec.dtype == np.uint8
    assert w.tolist() == [E4, 0] and a.tolist() == [0, 1] and woff.tolist() == [0, 2]
    assert np.array_equal(rec[0], _rec([E4, 0], [0, 1], 33))
    w, a, woff, rec = ic.pack_reference([b"ACGT" * 8 + b"G"])
    assert w.tolist() == [E4, 2] and a.tolist() == [0, 0]
    # an empty read: no word, a record of zeros
    w, a, woff, rec = ic.pack_reference([b""])
    assert len(w) == 0 and len(a) == 0 and woff.tolist() == [0, 0] and rec.shape == (1, 64) and not rec.any()
    # U keeps code 3 under its ambiguity bit, N code 0: 0 | 1 << 2 | 2 << 4 | 3 << 6 | 3 << 8
    w, a, woff, rec = ic.pack_reference([b"ACGTUN"])
    assert w.tolist() == [0x3E4] and a.tolist() == [0x30] and woff.tolist() == [0, 1]
    assert np.array_equal(rec[0], _rec([0x3E4], [0x30], 6))
    w, a, woff, rec = ic.pack_reference([b"acgtun"])
    assert w.tolist() == [0x3E4] and a.tolist() == [0x30]
    # several reads: each starts on a word; the records hold each read's own words
    w, a, woff, rec = ic.pack_reference([b"acgtn", b"", b"T" * 32, b"C" * 160])
    assert woff.tolist() == [0, 1, 1, 2, 7]
    assert w.tolist() == [0xE4, 0xFFFFFFFFFFFFFFFF] + [0x5555555555555555] * 5 and a.tolist() == [0x10, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(rec[0], _rec([0xE4], [0x10], 5)) and not rec[1].any()
    assert np.array_equal(rec[2], _rec([0xFFFFFFFFFFFFFFFF], [0], 32))
    assert np.array_equal(rec[3], _rec([0x5555555555555555] * 5, [0] * 5, 160))
    # one read longer than 160 bases: no records for the set
    assert ic.pack_reference([b"A" * 161, b"C"])[3] is None
    assert ic.pack_reference([])[3] is None


@pytest.mark.parametrize("name", ["alphabet", "ragged_0_200_4200", "skewed", "fixed_33_67", "planted_n_161"])
def test_unpacking_gives_the_reads_back(name):
    reads = ic.read_set(name)
    w, a, woff, _ = ic.packed(name)
    back = ic.unpack(w, a, woff, [len(r) for r in reads])
    assert back == [ic.kept_form(r) for r in reads]
    if name == "alphabet":
        every = back[0]
        assert len(every) == 256
        for c in range(256):
            want = chr(c).upper() if chr(c) in "ACGTacgtUu" else "N"
            assert chr(every[c]) == want, c
        assert back[0] == back[2] and back[1] == back[3]          # letter case does not reach the packed form
        r = ic.read_set("alphabet")[1]
        assert [chr(r[p]) for p in ic.ALPHABET_POS] == list("NnUuRNnU")
        assert [chr(back[1][p]) for p in ic.ALPHABET_POS] == list("NNUUNNNU")


def test_fixed_sets_reach_every_byte_shift():
    """k_pack_reads_fixed shifts its 48 loaded bytes down by sh = address & 15: over the lengths and byte offsets of the GPU test
    every sh occurs on a full word and on a tail word, whole sets and slices, and odd shifts load two and three 16-byte blocks"""
    full, tail, nq_odd, arms = set(), set(), set(), set()
    for L in ic.FIXED_LENGTHS:
        for j in (0,) + ic.WRAP_OFFSETS:
            for first in (0, ic.SLICE_R0):
                sh, nb, n_q = ic.fixed_shifts(L, ic.FIXED_SMALL - first, j + first * L)
                full |= set(sh[nb == 32].tolist())
                tail |= set(sh[nb < 32].tolist())
                nq_odd |= set(n_q[sh % 2 == 1].tolist())
                arms |= set(zip((sh >> 2).tolist(), ((sh & 3) * 8).tolist()))
                assert n_q.max() <= 3 and n_q.min() >= 1
    assert full == set(range(16)) and tail == set(range(16))
    assert nq_odd >= {2, 3}
    assert arms == {(sw, sb) for sw in range(4) for sb in (0, 8, 16, 24)}
    # the wrapped offsets alone (what an uploaded, aligned set never gives): odd shifts on reads of even length too
    sh, _, _ = ic.fixed_shifts(150, ic.FIXED_SMALL, 13)
    assert (sh % 2 == 1).all()
    # the suite's other fixed sets: 150-base reads in an aligned buffer, slices from even reads -- even shifts only
    sh, _, _ = ic.fixed_shifts(150, 3000, 0)
    assert not (sh % 2).any()
    # word counts 1..7 and a length that is a multiple of 32
    assert {(L + 31) // 32 for L in ic.FIXED_LENGTHS} == set(range(1, 8))
    assert any(L % 32 == 0 for L in ic.FIXED_LENGTHS) and any(L > ic.REC_MAX for L in ic.FIXED_LENGTHS)


def test_skewed_set_sends_the_read_search_far_both_ways():
    reads = ic.read_set("skewed")
    lens = np.array([len(r) for r in reads])
    assert len(reads) == 8506 and lens[0] == 0 and lens[1] == 20000 and lens[3002] == 9000 and lens[3503] == 40 and lens[-1] == 0
    assert lens[2:3002].max() == 3 and lens[2:3002].min() == 0 and not lens[3003:3503].any()
    assert not lens[3504:8504].any() and lens[8504] == 30000
    woff = ic.packed("skewed")[2]
    true, guess = ic.proportional_guess_error(woff)
    print("guess - true: max %d, true - guess: max %d" % ((guess - true).max(), (true - guess).max()))
    assert (guess - true).max() > 1000 and (true - guess).max() > 1000
    # the set's first read is empty, so the first read with a word is read 1: the backward gallop runs into its clamp at 0
    # and the bisection has to step over woff[0] == woff[1]; the last word belongs to the last read that has one
    assert true.min() == 1 and woff[0] == woff[1] == 0 and guess[true == 1].max() > 1000
    assert true[-1] == 8504 and true.max() == 8504 and guess[true == 8504].min() < 7000
    # the proportional guess is exact where the suite's other sets live
    t2, g2 = ic.proportional_guess_error(ic.packed("fixed_150_4200")[2])
    assert np.abs(t2 - g2).max() <= 1
    # the range bounds cut inside the runs of reads without a word
    b = ic.range_bounds("skewed")
    assert b[0] == 0 and b[-1] == len(reads) and all(x <= y for x, y in zip(b, b[1:]))
    assert any(3003 < x < 3503 for x in b) and any(3504 < x < 8504 for x in b) and any(x == y for x, y in zip(b, b[1:]))


def test_ragged_sets_hold_every_length():
    for name, hi in (("ragged_0_160_4200", 160), ("ragged_0_200_4200", 200)):
        reads = ic.read_set(name)
        assert len(reads) == 4200
        assert {len(r) for r in reads} == set(range(hi + 1))
        assert any(b"N" in r for r in reads) and any(r != r.upper() for r in reads)
    assert ic.packed("ragged_0_160_4200")[3] is not None and ic.packed("ragged_0_200_4200")[3] is None


def test_sets_sit_on_the_read_count_edges():
    assert ic.FIXED_LARGE >= 4096 and -(-ic.FIXED_LARGE // 1024) == 5
    assert {n - e for n in ic.COUNT_EDGES for e in (64, 1024, 4096)} >= {-1, 0, 1}
    assert len(set(ic.read_set("fixed_150_4200"))) < 3000            # copies for the collapse to find
    mixed = ic.read_set("mixed_3x700")
    assert len(mixed) == 2100 and len(set(mixed)) == 3
    for b in range(0, 2100, 1024):
        assert len(set(mixed[b:b + 1024])) == 3
    for L in ic.PLANTED:
        reads = ic.read_set("planted_n_%d" % L)
        assert [r.index(b"N") for r in reads] == list(ic.planted_positions(L)) and all(len(r) == L and r.count(b"N") == 1 for r in reads)
    for n in ic.COUNT_EDGES:
        assert len(ic.read_set("identical_%d" % n)) == n and len(set(ic.read_set("identical_%d" % n))) == 1
        assert len(set(ic.read_set("distinct_%d" % n))) == n


def test_oracle_histogram_keeps_its_own_rules(oracle):
    """what the GPU tests lean on: the histogram does not depend on the order of the reads, counts add up over copies, one
    copy of the repeated read gives every seed once, and the widest trim leaves nothing"""
    reads = ic.read_set("ragged_0_160_4200")
    for params in (ic.SPECIALISED[0], ic.GENERIC[1]):
        k, s, l, o, t = params
        h1, c1 = ic.want_histogram(oracle, "ragged_0_160_4200", params)
        assert len(h1) > 100 and np.all(h1[1:] > h1[:-1])
        order = np.random.default_rng(5).permutation(len(reads))
        h2, c2 = oracle.histogram([reads[int(i)] for i in order], k, s, l, o, t)
        assert np.array_equal(h1, h2) and np.array_equal(c1, c2)
        h3, c3 = oracle.histogram(reads + reads, k, s, l, o, t)
        assert np.array_equal(h1, h3) and np.array_equal(2 * c1, c3)
        hd, cd = oracle.histogram(reads + reads, k, s, l, o, t, dedup=True)
        hu, cu = oracle.histogram(sorted(set(reads)), k, s, l, o, t)
        assert np.array_equal(hd, hu) and np.array_equal(cd, cu)
        assert len(oracle.histogram(reads, k, s, l, o, t, 0, 200)[0]) == 0
    one = ic.read_set("identical_1")
    for params in ic.SPECIALISED:
        h, c = oracle.histogram(one, *params)
        assert len(h) > 5 and np.all(c == 1)
    # letter case and the kind of ambiguous byte do not reach the seeds: the alphabet set against its packed-and-unpacked form
    w, a, woff, _ = ic.packed("alphabet")
    back = ic.unpack(w, a, woff, [len(r) for r in ic.read_set("alphabet")])
    for params in ic.SPECIALISED + ic.GENERIC:
        ha, ca = oracle.histogram(ic.read_set("alphabet"), *params)
        hb, cb = oracle.histogram([r.replace(b"U", b"N") for r in back], *params)
        assert np.array_equal(ha, hb) and np.array_equal(ca, cb)
