"""The inputs of the crafted --meta scoring and EM tests (tests/em_checks.py) reach the cases the device path can get wrong --
judged on the restatement alone, no device: every word-edge case of the mask ranges, reads that fill the 7-plane counter and
reads that need 16 planes, every (columns, rows) pair at an unroll, chunk, block or LDS edge, both branches of the SQUAREM
choice with margins far from rounding, and the properties of the small whole-run mixtures.  The restatement itself is checked
against oracle_meta's tree-walking one on sampled nodes, the float64 EM restatement against the longdouble one."""
import numpy as np
import pytest

import assign_checks as ac
import em_checks as ec
from oracle import oracle_meta as om


def test_wide_restatement_equals_the_oracle():
    tree, R = ec.wide_family()
    n_nodes = len(tree.parent)
    rng = np.random.default_rng(6)
    ac.check_against_oracle(tree.oriented, R, np.unique(np.concatenate([[0, n_nodes - 1], rng.integers(0, n_nodes, 6)])))
    assert len(ec.distinct_columns(R.scores)) >= ec.WIDE_DISTINCT
    n = np.array([len(x) for x in R.lists])
    random_rows = R.scores.max(axis=1) == 0                          # the random reads match nothing ...
    assert random_rows.sum() >= 0.05 * len(n) and (R.scores[~random_rows].min(axis=1) < n[~random_rows]).all()
    assert np.array_equal(R.scores[~random_rows, 0], n[~random_rows])    # ... and the root holds every seedmer the others carry
    assert (~random_rows & (n <= ec.EM_MAX_SEEDMERS)).sum() >= 2100 and (R.merged < 0).any()


def test_candidate_sets_reach_every_word_edge():
    """the mask events of every candidate set of the scoring tests, enumerated: all classes of the range arithmetic occur"""
    seen = {}
    for i, tree in enumerate(ac.crafted_trees()):
        R = ac.crafted_restated(i)
        for cands in ec.crafted_candidate_sets(len(tree.parent), i):
            for name, hit in ec.event_classes(ec.mask_events(tree.oriented, cands, R.uniq)).items():
                seen[name] = seen.get(name, False) or hit
    assert all(seen.values()), seen                                  # (the crafted trees alone reach all of them)
    tree, R = ec.wide_family()
    for count in ec.WIDE_CANDIDATE_COUNTS:
        cands = ec.wide_candidate_set(len(tree.parent), count)
        assert len(cands) == count
        got = ec.event_classes(ec.mask_events(tree.oriented, cands, R.uniq))
        assert got["empty"] and got["both_orientations"] and got["bump"], (count, got)
        if count % 64 == 0:                                          # the root's range ends on the last word's last bit
            assert got["hi_on_word"], count
        if count >= 129:
            assert got["three_words"], count


def test_read_sets_fill_the_planes():
    tree, R = ec.wide_family()
    long_reads, short_reads, _ = ec.wide_reads()
    full, edge, short = (ec.capped_sample(R, long_reads, ec.READ_CAPS[p]) for p in ("planes16", "planes16_at_128", "planes7"))
    assert short.reads == short_reads and len(short.rows) == len(edge.rows) - 1 and len(edge.rows) < len(full.rows)
    assert short.mult.max() >= 2
    for count in ec.WIDE_CANDIDATE_COUNTS:
        cands = ec.wide_candidate_set(len(tree.parent), count)
        assert short.n.max() == 127 and short.scores(R, cands).max() == 127          # the 7-plane counter is full
        assert edge.n.max() == 128 and edge.scores(R, cands).max() == 128            # one more: 16 planes, or it wraps to 0
        sc = full.scores(R, cands)
        assert full.n.max() >= 128 and (sc[full.n == 128] == 128).any() and sc.max() > 255
    for i in range(len(ac.crafted_trees())):
        Rc = ac.crafted_restated(i)
        assert [ec.capped_sample(Rc, ac.crafted_reads()[0], ec.READ_CAPS[p]).n.max() > 255 if ec.READ_CAPS[p] is None else
                ec.capped_sample(Rc, ac.crafted_reads()[0], ec.READ_CAPS[p]).n.max() == ec.READ_CAPS[p] for p in ec.READ_CAPS] == [True] * 3


@pytest.mark.parametrize("n_cols,n_rows,discard", ec.FIXED_CASES)
def test_pick_case_meets_the_pair(n_cols, n_rows, discard):
    tree, R = ec.wide_family()
    cands, sample, sc, n, w = ec.fixed_case(n_cols, n_rows, discard)
    assert len(cands) == n_cols and np.all(np.diff(cands.astype(np.int64)) > 0)
    whole = sample.scores(R, cands)
    assert len(ec.distinct_columns(whole)) == n_cols
    keep = om.discard_rows(whole.max(axis=1), sample.n, discard)
    assert keep.sum() == n_rows == len(sc) and sc.shape[1] == n_cols
    assert w.max() >= 2 and n.max() <= ec.EM_MAX_SEEDMERS and len(sample.rows) > n_rows        # rows without weight are in the sample


def test_cut_is_the_shorter_run():
    _, _, sc, n, w = ec.fixed_case(65, 255, 0.0)
    whole = ec.fixed_restated(65, 255, 0.0, "float64")
    for it in ec.FIXED_ITERATIONS:
        res = ec.em_restated(sc, n, w, ec.EmParams(em_max_iterations=it, em_max_rounds=1, prop_threshold=0.0))
        part = ec.cut(whole, it)
        assert res.iterations == part.iterations == it and res.rounds == 1 and res.llh == part.llh
        assert np.array_equal(res.props, part.props) and np.array_equal(res.cols, part.cols)


def test_restatement_equals_square_em():
    """with the default parameters em_restated is oracle_meta.square_em: same columns, proportions to 1e-12"""
    for name, case in ec.small_cases().items():
        p = case.params
        _, _, sc, n, w = case.inputs()
        cols, props = om.square_em(sc, n, w, p.error_rate, p.em_convergence, p.em_delta_threshold, p.em_max_iterations, p.em_max_rounds, p.prop_threshold)
        res = case.restated()
        assert np.array_equal(cols, res.cols) and np.allclose(props, res.props, rtol=0, atol=1e-12), name


def test_small_mixtures_show_their_properties():
    for name, case in ec.small_cases().items():
        cols = case.inputs()[0]
        assert 6 <= len(cols) <= 40 and case.sample.mult.max() >= 2, name
        case.expect(case.restated())


@pytest.mark.skipif(not ec.HAVE_LONGDOUBLE, reason=ec.LONGDOUBLE_REASON)
def test_fixed_iterations_do_not_hang_on_rounding():
    """per fixed-iteration case: every choice between the extrapolated point and p2 has a margin beyond 1e-6 max(1, |llh2|),
    float64 and longdouble restatements agree far below the device tolerance (d <= 1e-11 on every proportion, 1e-13 relative
    on the log-likelihood), the iteration cap is reached, and over all cases both branches are taken.
    The three cases of em_checks.STOP_EARLY cannot reach the cap: one column, two columns and one read sit at their fixed
    point after an iteration or two, the log-likelihood stops moving and the run ends by the default convergence rule, the
    margin then being the convergence threshold itself, 1e-5.  There the run must end by that rule before the cap, and the
    margin must stay beyond 1e-6 absolute: a million times the rounding of a log-likelihood of a few hundred.  With one
    column the extrapolated point is NaN, so is the margin, and p2 is taken."""
    took = set()
    for case in ec.FIXED_CASES:
        lo, hi = ec.fixed_restated(*case, "float64"), ec.fixed_restated(*case, "longdouble")
        assert lo.iterations == hi.iterations and lo.rounds == hi.rounds == 1
        if case in ec.STOP_EARLY:
            assert 2 <= hi.iterations <= 3                       # N = 1 ends at the cap, N = 3 and 17 by the convergence rule
        else:
            assert hi.iterations == max(ec.FIXED_ITERATIONS)     # the cap is reached
        d = rel = 0.0
        smallest = np.inf
        for a, b in zip(lo.trace[0], hi.trace[0]):
            assert a["took_sq"] == b["took_sq"]
            took.add(b["took_sq"])
            if case[0] == 1:
                assert np.isnan(b["margin"]) and not b["took_sq"]
            else:
                bound = 1e-6 if case in ec.STOP_EARLY else 1e-6 * max(1.0, abs(b["llh2"]))
                assert abs(b["margin"]) > bound, (case, float(b["margin"]), float(b["llh2"]))
                smallest = min(smallest, float(abs(b["margin"])))
            d = max(d, float(np.abs(a["props"] - b["props"]).max()))
            rel = max(rel, float(abs(a["llh"] - b["llh"]) / abs(b["llh"])))
        print("case %5d x %4d: d = %.2e, llh rel = %.2e, smallest |margin| = %.3g" % (case[0], case[1], d, rel, smallest))
        assert d <= 1e-11 and rel <= 1e-13, (case, d, rel)
    assert took == {True, False}
