"""The two input families of the --filter-and-assign tests (tests/assign_checks.py) reach the cases the device path can get
wrong -- judged on the restatement alone, no device: reads with many assigned nodes, an LCA outside the assigned set, discarded
and unmapped reads, folded nodes, maxima beyond the first word of columns, reads exactly at and one below the --discard
threshold.  The restatement itself is checked against oracle_meta's tree-walking one on sampled nodes."""
import os

import numpy as np

import assign_checks as ac
from conftest import GOLDEN
from oracle import oracle_meta as om


_check_against_oracle = ac.check_against_oracle


def test_crafted_family_reaches_every_case():
    rng = np.random.default_rng(3)
    reads = ac.crafted_reads()[0]
    mapped = multi = lca_out = discarded = unmapped = assigned = folded = total = 0
    beyond = at_threshold = below_threshold = False
    planes = set()
    for i, tree in enumerate(ac.crafted_trees()):
        R = ac.crafted_restated(i)
        n_nodes = len(tree.parent)
        _check_against_oracle(tree.oriented, R, np.unique(np.concatenate([[0, n_nodes - 1], rng.integers(0, n_nodes, 6)])))
        heads = ac.heads_np(tree.parent, tree.oriented["offsets"])
        thr = (R.n.astype(np.float64) * 0.5).astype(np.int64)
        for r in range(len(reads)):
            total += 1
            unmapped += R.state[r] == ac.UNMAPPED
            discarded += R.state[r] == ac.DISCARDED
            if R.max[r] > 0:
                mapped += 1
                nodes = np.nonzero(R.scores[R.merged[r]] == R.max[r])[0]
                multi += len(nodes) > 1
                beyond |= bool(nodes.max() >= 64)
                at_threshold |= bool(R.max[r] == thr[r] and R.state[r] == ac.ASSIGNED)
                below_threshold |= bool(R.max[r] == thr[r] - 1 and R.state[r] == ac.DISCARDED)
            if R.state[r] == ac.ASSIGNED:
                assigned += 1
                lca_out += R.lca[r] not in R.nodes[r]
                folded += bool((heads[R.nodes[r]] != R.nodes[r]).any())
        planes |= {7 if R.n.max() < 128 else 16}
    assert planes == {16} and {127, 128} <= set(R.n.tolist()) and (R.merged < 0).any()
    assert multi >= 0.30 * mapped, (multi, mapped)
    assert lca_out >= 0.10 * mapped, (lca_out, mapped)
    assert discarded >= 0.10 * total, (discarded, total)
    assert unmapped >= 0.05 * total, (unmapped, total)
    assert folded >= 0.20 * assigned, (folded, assigned)
    assert beyond and at_threshold and below_threshold, (beyond, at_threshold, below_threshold)
    assert any((ac.heads_np(t.parent, t.oriented["offsets"]) != np.arange(len(t.parent))).any() for t in ac.crafted_trees())


def test_rsv_family_has_wide_assigned_sets(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    arrays = pmx.Index.build(pm, flank_mask=0, mode=0x100).arrays()
    R = ac.rsv_restated(arrays, 0.0)
    n_nodes = len(arrays["parent"])
    rng = np.random.default_rng(4)
    _check_against_oracle(arrays, R, np.unique(np.concatenate([[0, n_nodes - 1], rng.integers(0, n_nodes, 4)])))
    mapped = R.max > 0
    wide = np.array([len(x) > 64 for x in R.nodes])
    assert (wide & mapped).sum() >= 0.5 * mapped.sum(), ((wide & mapped).sum(), mapped.sum())
    assert len(R.state) == 780 and (R.state == ac.UNMAPPED).sum() >= 60
