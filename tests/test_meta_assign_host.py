"""The host-only helpers of --meta --filter-and-assign: pmx_index_node_heads and pmx_index_lca against the numpy restatement
(tests/assign_checks.py) on every crafted tree and on rsv_4K, and format_assigned on a hand-made result.  No device."""
import os

import numpy as np
import pytest

import assign_checks as ac
from conftest import GOLDEN


def _check_tree(plain, oriented, parent, offsets, rng):
    n = len(parent)
    assert np.array_equal(oriented.node_heads(), ac.heads_np(parent, offsets))
    pairs = [(0, 0), (0, n - 1), (n - 1, n - 1), (n - 1, n // 2)] + [tuple(rng.integers(0, n, 2).tolist()) for _ in range(200)]
    for a, b in pairs:
        assert plain.lca(a, b) == oriented.lca(b, a) == ac.lca_np(parent, a, b), (a, b)
    assert plain.lca(-1, 0) == -1 and plain.lca(0, n) == -1


def test_heads_and_lca_on_the_crafted_trees(pmx):
    rng = np.random.default_rng(11)
    for tree in ac.crafted_trees():
        plain, oriented = tree.indexes(pmx)
        _check_tree(plain, oriented, tree.parent, tree.oriented["offsets"], rng)
        with pytest.raises(pmx._lib.PmxError):
            plain.node_heads()                                       # the plain index does not tell identical nodes


def test_heads_and_lca_on_rsv(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    plain = pmx.Index.build(pm, flank_mask=0)
    oriented = pmx.Index.build(pm, flank_mask=0, mode=0x100)
    arrays = oriented.arrays()
    heads = oriented.node_heads()
    assert (heads != np.arange(len(heads))).any()
    _check_tree(plain, oriented, arrays["parent"], arrays["offsets"], np.random.default_rng(12))


def test_format_assigned_on_a_hand_made_result(pmx):
    # a tree of six nodes: 0 -> (1 -> (2, 3), 4 -> 5); nodes 3 and 5 carry no change: 3 folds into 1, 5 into 4
    heads = np.array([0, 1, 2, 1, 4, 4], np.uint32)
    # merged reads: 0 -> nodes {2, 3} (LCA 1), 1 -> {5} (LCA 5, head 4), 2 -> discarded, 3 -> {1, 3, 4} (LCA 0), 4 -> unmapped
    state = np.array([2, 2, 1, 2, 0], np.uint8)
    mx = np.array([7, 3, 1, 9, 0], np.uint16)
    lca = np.array([1, 5, 0xffffffff, 0, 0xffffffff], np.uint32)
    nodes = np.array([2, 3, 5, 1, 3, 4], np.uint32)
    off = np.array([0, 2, 3, 3, 6, 6], np.int64)
    merged = np.array([3, -1, 0, 2, 1, 0, 4, 3], np.int64)           # raw reads; FASTQ records: raw 0, 2, 4, 5, 7
    res = pmx.AssignResult(merged, state, mx, lca, off, nodes, heads)
    assert res.state.tolist() == [2, 0, 2, 1, 2, 2, 0, 2] and res.max.tolist() == [9, 0, 7, 1, 3, 7, 0, 9]
    assert res.fastq_index.tolist() == [0, -1, 1, -1, 2, 3, -1, 4] and res.lca.tolist() == [0, -1, 1, -1, 4, 1, -1, 0]
    assert res.nodes_of(0).tolist() == [1, 3, 4] and res.nodes_of(1).tolist() == [] and res.nodes_of(3).tolist() == []
    assert res.by_node() == {1: [0, 1, 3, 4], 2: [1, 3], 4: [0, 2, 4]} and res.by_lca() == {0: [0, 4], 1: [1, 3], 4: [2]}
    out, out_lca = pmx.format_assigned(res, lambda v: "n%d" % v, heads)
    assert out == "n1,n3\t.\t4\t0,1,3,4\nn2\t.\t2\t1,3\nn4,n5\t.\t3\t0,2,4\n"
    assert out_lca == "n0\t.\t2\t0,4\nn1,n3\t.\t2\t1,3\nn4,n5\t.\t1\t2\n"
    empty = pmx.AssignResult(np.array([-1, -1], np.int64), state[:0], mx[:0], lca[:0], np.zeros(1, np.int64), nodes[:0], heads)
    assert pmx.format_assigned(empty, str) == ("", "") and empty.state.tolist() == [0, 0]
