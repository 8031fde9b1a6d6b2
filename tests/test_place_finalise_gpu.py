"""The place stage between seeding and the tree, at every boundary (tests/finalise_checks.py): the seed table's merge, rehash,
shrink and compaction against np.unique, and the read filters, the canonical sums, the probe table of the kept seeds and the
weighted-containment denominator against the oracle, bit for bit.  tests/test_place_finalise_families.py shows on the CPU that
the cases reach what they are named for."""
import numpy as np
import pytest

import finalise_checks as fc
import place_tree_checks as tc

pytestmark = pytest.mark.gpu

_indexes = {}


def _placer(pmx, ctx, tree_name):
    if tree_name not in _indexes:
        _indexes[tree_name] = fc.tree(tree_name).index(pmx)
    return pmx.Placer(ctx, _indexes[tree_name])


def _run_steps(pmx, placer, case):
    """reset, then the case's steps; every histogram() step against np.unique (summed counts) of the merges since the last reset"""
    placer.reset()
    merged, n_checked = [], 0
    for st in case.steps:
        if st[0] == "merge":
            placer.merge(st[1], st[2])
            merged.append(st[1:])
        elif st[0] == "reset":
            placer.reset()
            merged = []
        elif st[0] == "score":
            placer.score(pmx.TraversalParams(), 0)
        else:
            keys, counts = fc.unique_sum(merged)
            hh, hc = placer.histogram()
            assert len(hh) == len(keys) == placer.histogram_size(), "%s: %d seeds, expected %d" % (case.name, len(hh), len(keys))
            assert np.array_equal(hh, keys), case.name + ": seed set differs"
            assert np.array_equal(hc, counts), case.name + ": seed counts differ"
            n_checked += 1
    return n_checked


def _score_and_check(pmx, placer, name, tree_name=None):
    case = fc.cases()[name]
    _run_steps(pmx, placer, case)
    res = placer.score(case.traversal_params(pmx), 0)
    want = fc.want(name, tree_name)
    st = want["state"]
    print(name, "seeds %d alive %d kept %d support %d" % (len(want["hist_hash"]), st.n_unique_in, st.n_kept, st.min_support))
    print("  readMagnitude %r / %r  logContainmentDenominator %r / %r  weightedContainmentDenominator %r / %r" %
          (res.readMagnitude, st.log_magnitude, res.logContainmentDenominator, st.log_cont_den, res.weightedContainmentDenominator, want["wc_den"]))
    assert placer.score_info()["redone"] == 0
    tc.assert_place_matches(placer, res, want)
    return res, want


@pytest.mark.parametrize("name", fc.names("A"))
def test_seed_table(pmx, ctx, name):
    case = fc.cases()[name]
    placer = _placer(pmx, ctx, "default")
    assert _run_steps(pmx, placer, case) == sum(st[0] == "histogram" for st in case.steps) >= 1
    placer.close()


@pytest.mark.parametrize("name", fc.names("B"))
def test_read_filters(pmx, oracle, ctx, name):
    placer = _placer(pmx, ctx, "default")
    res, want = _score_and_check(pmx, placer, name)
    e = fc.cases()[name].expect
    if "support" in e:
        assert res.min_support == e["support"]
    if "n_mask" in e:
        assert res.n_unique_seeds == e["alive"] - e["n_mask"]
    if "n_kept" in e:
        assert res.readUniqueSeedCount == e["n_kept"]
    placer.close()


@pytest.mark.parametrize("n", fc.SUM_SIZES)
def test_canonical_sums(pmx, oracle, ctx, n):
    placer = _placer(pmx, ctx, "default")
    res, want = _score_and_check(pmx, placer, "C_sum_%d" % n)
    assert res.readUniqueSeedCount == n
    placer.close()


@pytest.mark.parametrize("name", fc.names("D"))
def test_probe_table_and_wc_denominator(pmx, oracle, ctx, name):
    case = fc.cases()[name]
    placer = _placer(pmx, ctx, case.tree)
    res, want = _score_and_check(pmx, placer, name)
    assert res.readUniqueSeedCount == case.expect["n_kept"] and res.weightedContainmentDenominator > 0
    placer.close()


def test_one_placer_across_families(pmx, oracle, ctx):
    """one placer through a B case, a C case, an empty histogram and a D case, twice: the buffers sized by the histogram (dead
    marks, scan, kept seeds, block sums, probe table) move between calls, and the seed table shrinks and grows"""
    placer = _placer(pmx, ctx, "clusters")
    for name in ("B_mask_70000_ties", "C_sum_%d" % (65 * 1024 + 9), "empty", "D_clusters", "B_auto_nine1_one4", "C_sum_1025", "empty",
                 "B_homopolymer_mask_0.01", "D_clusters"):
        res, want = _score_and_check(pmx, placer, name, "clusters")
        if name == "empty":
            assert res.readUniqueSeedCount == 0 and res.n_unique_seeds == 0 and not want["scores"].any()
    placer.close()
