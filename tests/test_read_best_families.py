"""The conditions the read-score tests rest on, from the restatement alone (tests/read_best_checks.py; no device): the crafted
trees of assign_checks and the edge family hold the cases k_meta_read_best can get wrong, and the restated file text is the
reference's (writeMetaReadScores, src/main.cpp:446-466) on a hand-written example."""
import numpy as np

import assign_checks as ac
import read_best_checks as rb


# the edge trees looked at here: of the three sizes around 8,192 columns the one that has a second lane round (the dense
# restatements of the other two cost as much again and hold the same cases one column short; the device tests run all three)
CASES = tuple((n, shape) for n, shape in rb.EDGE_CASES if n not in (8191, 8192))


def _all_bests():
    """(name, nodes, Best, of the edge family)"""
    for i, tree in enumerate(ac.crafted_trees()):
        yield tree.name, len(tree.parent), rb.crafted_best(i), False
    for n, shape in CASES:
        yield rb.edge_tree(n, shape).name, n, rb.edge_restated(n, shape), True


def test_every_tree_has_unmapped_single_and_wide_reads():
    """max 0 and n_best = 1 on every tree; n_best > 64 on every tree of the edge family that has the nodes for it (127 and
    more).  The crafted trees of assign_checks cannot give that: their seedmers are gained at one or two nodes and lost again
    below, and no read there has more than 10 best nodes."""
    for name, n, B, edge in _all_bests():
        assert (B.max == 0).any() and (B.max > 0).any(), name
        assert ((B.n_best == 0) == (B.max == 0)).all(), name          # a positive maximum is reached at an active node
        assert (B.n_best == 1).any(), name
        if edge and n >= 127:
            assert (B.n_best > 64).any() and ((B.n_best > 64) & (B.n_all > B.n_best)).any(), name
        assert B.active[0] and (B.n_best <= B.n_all).all(), name


def test_tie_sets_hold_inactive_nodes():
    """reads whose count over all nodes exceeds n_best: on every tree of the edge family but the single node, and on four of the
    six crafted trees (the single node has none to spare; the star's inactive leaves score as its root, where no read is best);
    over the families: an inactive node right after the first column of a tie set, inside one, and at its last column"""
    after_first = inside = last = crafted = 0
    for name, n, B, edge in _all_bests():
        if edge and n > 1:
            assert not B.active.all() and (B.n_all > B.n_best).any(), name
        crafted += (not edge) and (B.n_all > B.n_best).any()
        for m in np.nonzero(B.n_all > B.n_best)[0]:
            cols = np.nonzero(B.scores[m] == B.max[m])[0]
            assert B.active[cols[0]], (name, m)                       # (its nearest active ancestor would precede it)
            after_first += not B.active[cols[1]]
            inside += (~B.active[cols[1:-1]]).any()
            last += not B.active[cols[-1]]
    assert after_first and inside and last and crafted == 4


def test_the_plane_thresholds_are_in_the_crafted_reads():
    n = rb.crafted_best(0).n
    assert (n >= 128).any() and (n == 127).any() and (n < 127).any()


def test_the_long_read_of_the_edge_family_takes_it_to_sixteen_planes():
    """the reads of the edge family stay below 128 seedmers; the long read has 128 and more and holds all of theirs, so with
    it in the set the tie sets of the four reads go through the 16-plane kernels unchanged"""
    E = rb.edge_reads()
    hashes = lambda r: {h for h, _ in rb.om.seedmers(r, ac.K, ac.S, ac.L)}
    assert all(0 < len(rb.om.seedmers(r, ac.K, ac.S, ac.L)) < 127 for r in E.reads)
    assert len(rb.om.seedmers(E.long, ac.K, ac.S, ac.L)) >= 128
    assert all(hashes(r) <= hashes(E.long) for r in (E.one, E.spots, E.wide, E.marks))
    assert rb.LONG_CASES == ((8193, "path"), (8193, "star")) and set(rb.LONG_CASES) <= set(rb.EDGE_CASES)


def test_an_active_node_sits_at_bit_63_and_the_edge_columns_are_best():
    assert any(B.active[63::64].any() for _, _, B, _ in _all_bests())
    best_cols = set()
    for n, shape in CASES:
        tree, B = rb.edge_tree(n, shape), rb.edge_restated(n, shape)
        for m in np.nonzero(B.max > 0)[0]:
            cols = np.nonzero((B.scores[m] == B.max[m]) & B.active)[0]
            best_cols |= {int(c) for c in cols if c in (0, 63, 64, 127, 128, 8190, 8192) or c == n - 1}
        if n == 8193:                                                 # one tie set over two words, two lanes, two lane rounds
            m = int(B.merged[1])                                      # (raw read 1 is `spots`)
            spots = np.nonzero(B.scores[m] == B.max[m])[0]
            want = set(rb.SPOTS) | ({n - 1} if shape == "path" else set())
            assert set(spots.tolist()) == want, (tree.name, spots)
            assert B.n_best[m] == (4 if shape == "path" else 7) and B.n_all[m] == 7, tree.name
    assert {0, 63, 64, 127, 128, 8190, 8192} <= best_cols
    assert {n - 1 for n, _ in CASES} <= best_cols


def test_the_maximum_over_the_active_nodes_is_the_maximum_over_all():
    for name, _, B, _ in _all_bests():
        assert np.array_equal(B.scores[:, B.active].max(axis=1), B.max), name
    # ... and the restated scores are the tree-walking oracle's at sampled nodes of the edge family
    for n, shape in (CASES[2], CASES[5], CASES[-1]):
        tree = rb.edge_tree(n, shape)
        R = ac.restate(tree.oriented, rb.edge_reads().reads, 0.0)
        ac.check_against_oracle(tree.oriented, R, sorted({0, 1, n // 2, min(63, n - 1), min(64, n - 1), n - 1}))


def test_the_file_text_on_a_hand_written_example():
    """four merged reads: unmapped; below the threshold of --discard 0.5 (4 < int(10 * 0.5)); at a truncated threshold (4 >=
    int(9 * 0.5) = 4); a full score with three copies.  Raw read 6 was dropped, raw read 7 is the unmapped read."""
    n, mx, nb = [10, 10, 9, 7], [0, 4, 4, 7], [0, 3, 1, 70]
    raw = [1, 3, 2, 3, 3, 1, -1, 0]
    assert rb.scores_text(n, mx, nb, raw, 0.5, False) == (
        "ReadIndex\tNumDuplicates\tTotalScore\tMaxScore\tNumMaxScoreNodes\tRawReadsIndices\n"
        "1\t2\t10\t4\t3\t0,5\n"
        "2\t1\t9\t4\t1\t2\n"
        "3\t3\t7\t7\t70\t1,3,4\n")
    assert rb.scores_text(n, mx, nb, raw, 0.5, True) == (
        "ReadIndex\tNumDuplicates\tTotalScore\tMaxScore\tNumMaxScoreNodes\tOvermaximumTaxonNumber\tRawReadsIndices\n"
        "2\t1\t9\t4\t1\t0\t2\n"
        "3\t3\t7\t7\t70\t0\t1,3,4\n")
    assert rb.scores_text(n, mx, nb, raw, 0.0, True).count("\n") == 4
