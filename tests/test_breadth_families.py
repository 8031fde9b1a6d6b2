"""The input families of the --breadth-ratio tests (tests/breadth_checks.py) reach the cases the device path can get wrong --
judged on the restatement alone, no device: a union that matters (a seedmer hit by several reads of a node counts once), hits
that only the other orientation gives, reads that repeat a hash, merged reads of multiplicity > 1, weight sums beyond the
lowered flush bound; on rsv rows of more than 64 words, hits beyond column 4,096 and seedmers whose carriers fall into different
chunks.  On every crafted tree the matrix form of the computation equals the literal one, and the hand-written tree gives the
numbers worked out in its comment."""
import os

import numpy as np
import pytest

import assign_checks as ac
import breadth_checks as bc
from conftest import GOLDEN
from oracle import oracle_meta as om


def _assigned_merged(R):
    """{merged read: its assigned nodes} of the assigned merged reads"""
    return {int(R.merged[r]): R.nodes[r] for r in np.nonzero(R.state == ac.ASSIGNED)[0].tolist()}


def test_the_tandem_reads_repeat_hashes_and_the_copy_merges():
    reads = bc.reads()
    for read, n, distinct in ((reads[-3], 92, 49), (reads[-2], 85, 36)):
        s = om.seedmers(read, ac.K, ac.S, ac.L)
        assert (len(s), len({h for h, _ in s})) == (n, distinct)
    for i in range(len(ac.crafted_trees())):
        R = bc.crafted_restated(i)
        assert R.state[-3] == R.state[-2] == R.state[-1] == ac.ASSIGNED and R.merged[-1] == R.merged[-3], i


@pytest.mark.parametrize("tree_index", range(len(ac.crafted_trees())))
def test_crafted_family_reaches_every_case(tree_index):
    tree = ac.crafted_trees()[tree_index]
    R = bc.crafted_restated(tree_index)
    heads = ac.heads_np(tree.parent, tree.oriented["offsets"])
    total, observed, depth = bc.restate_breadth(tree.oriented, R, R.lists)
    # the matrix form equals the literal one
    obs2, dep2 = bc.closed_form(R)
    assert np.array_equal(observed, obs2) and np.array_equal(depth, dep2)
    # TotalRefSeeds against the PLAIN index of the same tree: its counts are the two orientations' added up
    plain, n = tree.plain, len(tree.parent)
    held = [dict() for _ in range(n)]
    for v in range(n):
        held[v] = dict(held[tree.parent[v]]) if v else {}
        for q in range(int(plain["offsets"][v]), int(plain["offsets"][v + 1])):
            held[v][int(plain["hash"][q])] = int(plain["child_count"][q])
    assert [sum(c > 0 for c in held[v].values()) for v in range(n)] == total.tolist()
    if tree.name == "one":
        return
    P = R.presence
    dup = bc.multiplicities(R.merged)
    per_read_hits = np.zeros(n, np.int64)
    other_only = repeats = 0
    weight = np.zeros(len(R.uniq), np.int64)                          # per seedmer: the multiplicities of its assigned carriers
    for m, nodes in _assigned_merged(R).items():
        u = np.searchsorted(R.uniq, np.array([h for h, _ in R.lists[m]], np.uint64))
        rv = np.array([int(v) for _, v in R.lists[m]])
        repeats += len(set(u.tolist())) < len(u)
        distinct = np.unique(u)
        weight[distinct] += dup[m]
        for v in nodes.tolist():
            per_read_hits[heads[v]] += int(P[distinct, v, :].any(axis=1).sum()) if heads[v] == v else 0
            other_only += int((~P[u, v, rv] & P[u, v, 1 - rv]).sum())
    is_head = heads == np.arange(n)
    assert (observed[is_head] < per_read_hits[is_head]).sum() >= 2   # the union matters
    assert other_only >= 1000
    assert repeats >= 2
    assert sum(dup[m] > 1 for m in _assigned_merged(R)) >= 10
    assert (weight > bc.FLUSH).any() and depth.max() > bc.FLUSH      # the lowered flush bound is crossed within one row


def test_three_nodes_by_hand():
    tree, reads, numbers = bc.three_nodes()
    R = ac.restate(tree.oriented, reads, 0.0)
    assert R.state.tolist() == [ac.ASSIGNED] * 4 and [x.tolist() for x in R.nodes] == [[0], [2], [0], [0]]
    assert R.merged[0] == R.merged[3] != R.merged[2]
    got = bc.restate_breadth(tree.oriented, R, R.lists)
    for g, w in zip(got, numbers):
        assert np.array_equal(g, w), (g, w)
    lines = bc.restate_text(got, np.arange(3), lambda v: "n%d" % v, True).split("\n")
    assert lines[0] == bc.HEADER and lines[1] == "n0\t10\t10\t1\t30\t3\t%g\t%g" % (1 - np.exp(-3.0), 1 / (1 - np.exp(-3.0)))
    assert lines[2] == "n1\t0\t0\t0\t0\t0\t0\t0" and len(lines) == 5 and lines[4] == ""
    assert bc.restate_text(got, np.arange(3), lambda v: "n%d" % v, False) == bc.HEADER + "\n"


def test_rsv_family_reaches_every_case(pmx):
    arrays = pmx.Index.build(pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")), flank_mask=0, mode=0x100).arrays()
    n = len(arrays["parent"])
    assert (n + 63) // 64 > 64                                       # more than one span of 64 words a row
    heads = ac.heads_np(arrays["parent"], arrays["offsets"])
    for discard in (0.0, 0.6):
        R = ac.rsv_restated(arrays, discard)
        total, observed, depth = bc.restate_breadth(arrays, R, R.lists)
        is_head = heads == np.arange(n)
        assert (observed[4096:][is_head[4096:]] > 0).sum() >= 50 and total.max() > 4096 and (depth >= observed).all()
        chunks = {7: {}, 64: {}}
        for m in _assigned_merged(R):
            for h in {h for h, _ in R.lists[m]}:
                for size, seen in chunks.items():
                    seen.setdefault(h, set()).add(m // size)
        for size, seen in chunks.items():
            assert sum(len(c) > 1 for c in seen.values()) >= 1000, (discard, size)
