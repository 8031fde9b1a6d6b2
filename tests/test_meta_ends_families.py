"""The read family of --mask-read-ends (tests/ends_checks.py) meets its own conditions, checked against plain Python and
oracle_meta alone: no device, no product code.  What the device tests then conclude from the family rests on these."""
import numpy as np
import pytest

import ends_checks as ec
from oracle import oracle_meta as om

K, S, L = ec.K, ec.S, ec.L


def test_trim_is_the_substring_rule():
    r = bytes(range(65, 75))                                    # ten distinct bytes
    assert ec.trim(r, 0) == r and ec.trim(r, 1) == r[1:9] and ec.trim(r, 4) == r[4:6]
    assert ec.trim(r, 5) == b"" and ec.trim(r, 6) == b"" and ec.trim(r, 10 ** 6) == b"" and ec.trim(b"", 3) == b""


@pytest.mark.parametrize("n", ec.NS)
def test_lengths_around_the_trim_and_around_k(n):
    F = ec.family(n)
    assert [len(r) for r in F.short] == [0, 1, 2 * n - 1, 2 * n, 2 * n + 1, 2 * n + K - 1, 2 * n + K, 2 * n + K + 1]
    assert [len(ec.trim(r, n)) for r in F.short] == [0, 0, 0, 0, 1, K - 1, K, K + 1]
    assert all(r in F.reads for r in F.short)
    # nothing shorter than l syncmers' worth of bases carries a seedmer
    assert all(len(om.seedmers(ec.trim(r, n), K, S, L)) == 0 for r in F.short[:6])


@pytest.mark.parametrize("n", ec.NS)
def test_trimmed_lengths_on_and_off_the_word_edges(n):
    F = ec.family(n)
    assert [len(ec.trim(r, n)) for r in F.edges] == [31, 32, 33, 63, 64, 65]
    assert [len(r) for r in F.edges] == [m + 2 * n for m in (31, 32, 33, 63, 64, 65)]
    assert all(r in F.reads for r in F.edges)
    # the reads are packed 32 bases a word: the trim starts inside a word, on its last base, or on the first of the next
    assert {n % 32 for n in ec.NS} >= {31, 0, 1}
    # ... and the longer three have seedmers to lose or keep
    assert all(len(om.seedmers(ec.trim(r, n), K, S, L)) > 0 for r in F.edges[3:])


@pytest.mark.parametrize("n", ec.NS)
def test_ambiguous_bases_beside_the_cut(n):
    F = ec.family(n)
    w, size = F.window, len(F.window)
    at = [n - 1, n, size - n - 1, size - n]
    for q, p in zip(F.with_n, at):
        assert len(q) == size and q[p] == ord("N") and q.count(b"N") == 1 and q[:p] + w[p:p + 1] + q[p + 1:] == w
    cut = [ec.trim(q, n) for q in F.with_n]
    assert cut[0] == cut[3] == ec.trim(w, n) and b"N" not in cut[0]          # the trim takes the N away
    assert cut[1][0] == ord("N") and cut[2][-1] == ord("N")                 # ... or leaves it as the first / last base
    full, first, last = (om.seedmers(x, K, S, L) for x in (cut[0], cut[1], cut[2]))
    # ... where it costs the k-mer that holds it, as one base fewer would
    assert len(full) > 0 and first == om.seedmers(cut[0][1:], K, S, L) and last == om.seedmers(cut[0][:-1], K, S, L)
    assert all(q in F.reads for q in F.with_n) and w in F.reads


@pytest.mark.parametrize("n", ec.NS)
def test_twins_differ_inside_the_trimmed_ends_only(n):
    F = ec.family(n)
    assert len(set(F.twins)) == 4 and len({ec.trim(r, n) for r in F.twins}) == 1
    t = F.twins[0]
    for r in F.twins[1:]:
        where = [i for i in range(len(t)) if r[i] != t[i]]
        assert where and all(i < n or i >= len(t) - n for i in where)
    assert len([i for i in range(len(t)) if F.twins[3][i] != t[i]]) == 2 * n      # every trimmed base differs
    assert len(om.seedmers(ec.trim(t, n), K, S, L)) > 0
    # so they are one merged read of multiplicity >= 4, and untrimmed they are not
    off, h, v, mult, raw = ec.family_expected(n)
    rows = {int(raw[F.reads.index(r)]) for r in F.twins}
    assert len(rows) == 1 and min(rows) >= 0 and mult[min(rows)] >= 4
    if n >= K:                                                  # (a few changed end bases may fall outside every syncmer)
        assert len({tuple(om.seedmers(r, K, S, L)) for r in F.twins}) > 1


@pytest.mark.parametrize("n", ec.NS)
def test_dust_reads_cross_the_threshold_both_ways(n):
    F = ec.family(n)
    T = ec.DUST_THRESHOLD
    assert om.get_dust(F.dust_down) > T >= om.get_dust(ec.trim(F.dust_down, n))
    assert om.get_dust(F.dust_up) <= T < om.get_dust(ec.trim(F.dust_up, n))
    assert F.dust_down in F.reads and F.dust_up in F.reads
    assert len(om.seedmers(ec.trim(F.dust_down, n), K, S, L)) > 0 and len(om.seedmers(F.dust_down, K, S, L)) > 0
    # the filter on the trimmed reads keeps `down` and drops `up`; on the raw reads it would be the other way round
    keep_cut = ec.kept_by_dust(ec.trimmed(F.reads, n), T)
    keep_raw = ec.kept_by_dust(F.reads, T)
    i, j = F.reads.index(F.dust_down), F.reads.index(F.dust_up)
    assert keep_cut[i] and not keep_cut[j] and not keep_raw[i] and keep_raw[j]
    # a read trimmed to nothing scores 0 and stays
    assert om.get_dust(b"") == 0.0 and all(keep_cut[F.reads.index(r)] for r in F.short[:4])
    # and the filter changes the sample: `down` is a merged read of its own only with the trimmed score
    assert ec.family_expected(n, T)[4][i] >= 0 and ec.merged_from_strings(F.reads, T)[4][i] == -1


@pytest.mark.parametrize("n", ec.NS)
def test_tiled_reads_give_scoring_and_the_em_something_to_do(n):
    F = ec.family(n)
    assert len(F.tiles) == 100 and all(len(r) == 150 for r in F.tiles) and all(r in F.reads for r in F.tiles)
    a, b = (set(h for h, _ in om.seedmers(g, K, S, L)) for g in ec.mc.genomes())
    from_a = from_b = 0
    for r in F.tiles:
        hs = {h for h, _ in om.seedmers(ec.trim(r, n), K, S, L)}
        assert hs <= (a | b) and (hs or not set(r) <= set(b"ACGT"))       # (a tile inside a stretch of N has none)
        from_a += bool(hs - b)
        from_b += bool(hs - a)
    assert from_a >= 10 and from_b >= 10                      # reads that tell the two genomes apart, both ways
    off, h, v, mult, raw = ec.family_expected(n)
    assert len(mult) >= 100 and int(mult.sum()) == int((raw >= 0).sum()) and (raw < 0).sum() >= 6
    assert len(F.reads) == 8 + 6 + 1 + 4 + 4 + 2 + 100


def test_the_trim_changes_the_lists():
    """the family tells trimming from not trimming: for every n the merged lists of the trimmed strings differ from those of
    the raw strings, and from those of the next n"""
    seen = []
    for n in ec.NS:
        F = ec.family(n)
        raw = ec.merged_from_strings(F.reads)
        cut = ec.family_expected(n)
        assert not (np.array_equal(raw[0], cut[0]) and np.array_equal(raw[1], cut[1]))
        assert not np.array_equal(ec.merged_from_strings(ec.trimmed(F.reads, n + 1))[1], cut[1])
        seen.append(len(cut[1]))
    assert seen[0] > seen[-1]                                   # more trimmed, fewer seedmers


def test_leaves_rule_restated_on_a_hand_example():
    oc = [0.9, 0.9, 0.8, 0.8, 0.7, 0.6, 0.5]
    ids = ["node_1", "A", "node_2", "node_3", "B", "node_4", "C"]
    heads = [0, 1, 2, 2, 4, 4, 6]                              # node_4 folds onto B's head: eligible through the fold
    assert list(ec.eligible_nodes(ids, heads)) == [False, True, False, False, True, True, True]
    assert list(ec.leaves_candidates(oc, ids, heads, 1)) == [1]
    assert list(ec.leaves_candidates(oc, ids, heads, 2)) == [1, 4]           # 0.8 is passed over: no rank for it
    assert list(ec.leaves_candidates(oc, ids, heads, 3)) == [1, 4, 5]
    assert list(ec.leaves_candidates(oc, ids, heads, 1000)) == [1, 4, 5, 6]
    assert list(ec.plain_candidates(oc, 2)) == [0, 1, 2, 3]
    assert len(ec.leaves_candidates(oc, ["node_%d" % i for i in range(7)], list(range(7)), 5)) == 0


def test_ocranks_text_restated_on_a_hand_example():
    text = ec.ocranks_text([0.5, 1.0, 0.5, 0.0, 1.0 / 3.0], ["a", "b", "c", "d", "e"])
    assert text == "b\t1.000000\t0\na\t0.500000\t1\nc\t0.500000\t1\ne\t0.333333\t2\nd\t0.000000\t3\n"


def test_small_tree_meets_its_conditions():
    tree, reads, ids = ec.small_tree()
    assert len(ids) == len(tree.parent) == 8 and len(reads) == 33
    heads = ec.ac.heads_np(tree.parent, tree.oriented["offsets"])
    assert list(heads) == [0, 1, 2, 3, 4, 5, 6, 6]                           # S_c folds onto node_5
    ok = ec.eligible_nodes(ids, heads)
    assert list(ok) == [False, False, True, False, True, False, True, True]
    assert not ec.is_sample(ids[6]) and ok[6]                                # eligible through the fold alone
    read_hashes = {h for r in reads for h, _ in om.seedmers(r, K, S, L)}
    oc = [om.overlap_coefficient(tree.plain, v, read_hashes) for v in range(8)]
    assert int(np.argmax(oc)) == 1 and not ok[1] and oc[1] > max(oc[v] for v in range(8) if ok[v])    # the best node is not eligible
    assert oc[6] == oc[7]
    ranks = sorted({oc[v] for v in range(8) if ok[v]}, reverse=True)
    assert len(ranks) == 3                                                   # S_a, S_b, node_5 = S_c: top_oc 1 and 2 cut between them
    got = [list(ec.leaves_candidates(oc, ids, heads, t)) for t in (1, 2, 3)]
    assert len(got[0]) < len(got[1]) < len(got[2]) == 4 and got[2] == [2, 4, 6, 7]
    assert list(ec.plain_candidates(oc, 1)) == [1]                           # without the switch the ineligible node is the one candidate
