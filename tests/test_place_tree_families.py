"""The crafted trees of tests/test_place_trees_gpu.py against the oracle alone (no GPU): the generator keeps its own rules, the
shapes reach the edges of the scoring kernels they were built for, and the bit-equal comparison would notice additions in
another order -- or the GPU comparison would pass on trees that test nothing."""
import numpy as np
import pytest

import place_tree_checks as tc

BIG = [s for s in tc.SHAPES if len(tc.shape_parent(s)[0]) > 100]


@pytest.mark.parametrize("name", tc.SHAPES)
def test_shape_is_consistent_and_scores_are_sane(oracle, name):
    t, d = tc.tree(name), tc.decomposition(name)
    tc.check_consistent(t)
    same = np.mean(t.parent_count == t.child_count) if t.n_changes else 0.0
    assert same <= 0.06, same                                       # a small share of entries both sides skip
    if t.n_changes > 50000:                                          # (the small spines touch most hashes once)
        assert same >= 0.01, same
        assert set(np.unique(t.child_count).tolist()) >= {0, 1, 2, 3, 1000, 32767}
        hs, first = np.unique(t.hash, return_index=True)
        assert len(hs) < t.n_changes / 2                            # the same hash changes again and again
        in_a = np.isin(hs, tc.histogram("A")[0]).mean()
        assert 0.4 <= in_a <= 0.6, in_a                             # half the change hashes are read seeds
    for hist in ("A", "T"):
        w = tc.want(name, hist)
        assert w["counts"].min() >= 0
        assert np.all(np.isfinite(w["scores"])) and np.all(np.isfinite(w["metrics"]))
        assert w["state"].n_kept > 3000
    print(name, "nodes %d changes %d root list %d n_chains %d max_chain_len %d n_levels %d" %
          (t.n_nodes, t.n_changes, int(t.offsets[1]), d["n_chains"], d["max_chain_len"], d["n_levels"]))


def test_shapes_reach_the_edges_of_the_chains_kernel():
    d = {s: tc.decomposition(s) for s in tc.SHAPES}
    t = {s: tc.tree(s) for s in tc.SHAPES}
    # chains shorter than, equal to and longer than the prefetch depth PMX_CHAIN_AHEAD + 2 = 5
    assert {len(c) for c in d["broom"]["chains"]} >= set(range(1, 9))
    # publishing nodes per chain around one and two batches of PMX_CHAIN_FLUSH = 8; the spine is chain 0 whole
    for p in tc.PUBLISHERS:
        for v, tail in (("end", 1), ("tail", 5)):
            dd = d["spine_%d_%s" % (p, v)]
            spine = dd["chains"][0]
            assert spine == list(range(p + tail)), (p, v, spine)
            pub = np.flatnonzero(dd["publish"][spine])
            assert len(pub) == p and pub[-1] == len(spine) - 1 - tail
            assert dd["n_chains"] == p + 1
    assert {int(d[s]["publish"][d[s]["chains"][0]].sum()) for s in tc.SHAPES} >= {0, 1, 7, 8, 9, 15, 16, 17, 1999}
    # one chain, nothing published, a level per node; every spine node of the caterpillar publishes
    assert d["path"]["n_chains"] == 1 and d["path"]["n_levels"] == 2000 and not d["path"]["publish"].any()
    assert d["caterpillar"]["chains"][0][:2000] == list(range(2000)) and d["caterpillar"]["publish"][:1999].all()
    assert d["caterpillar"]["n_chains"] == 2000
    # zero-change nodes inside a chain, two in a row
    for s in ("path", "caterpillar", "random", "spine_17_tail"):
        own = np.diff(t[s].offsets.astype(np.int64))
        assert any(np.any((own[c][:-1] == 0) & (own[c][1:] == 0)) for c in d[s]["chains"] if len(c) > 2), s
    # every tail of the unrolled add loop, inside chains and at chain heads
    for s in ("path", "star", "binary", "random"):
        own = np.diff(t[s].offsets.astype(np.int64))
        assert set(tc.CYCLE) <= set(own.tolist()), s
    # more chains than three times the waves of a 256-CU grid: waves take a second, third and fourth chain
    assert d["star"]["n_chains"] >= 4100 and d["random"]["n_chains"] >= 4100
    assert d["binary"]["n_levels"] == 12 and d["binary"]["n_chains"] == 2048
    # root lists around the 1,024-wide tiles of the denominator kernel
    assert {int(t[s].offsets[1]) for s in tc.SHAPES} >= {0, 1, 1023, 1024, 1025, 2049}
    assert t["single_empty"].n_changes == 0 and t["single_300"].n_changes == 300


@pytest.mark.parametrize("name", BIG)
def test_reversed_change_lists_change_the_bits(oracle, name):
    share = tc.order_sensitive_share(name)
    print(name, "order-sensitive nodes: %.3f" % share)
    assert share >= 0.5


@pytest.mark.parametrize("name", BIG)
def test_tie_lists_longer_than_one(oracle, name):
    """histogram T: the best score is shared by many nodes -- and, where the shape has more than one leaf, by many leaves"""
    w = tc.want(name, "T")
    print(name, [len(x) for x in w["ties"]], [len(x) for x in tc.want(name, "T", force_leaf=True)["ties"]])
    assert max(len(x) for x in w["ties"]) > 1
    if name != "path":
        assert max(len(x) for x in tc.want(name, "T", force_leaf=True)["ties"]) > 1
