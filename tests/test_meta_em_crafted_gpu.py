"""--meta scoring and EM on the device (pmx_meta_score / pmx_meta_em, panmap_amd/csrc/api_meta.hip) on the crafted inputs of
tests/em_checks.py, at every edge of the kernels:
  * scores, candidates and the merged reads against the all-node restatement, exactly: the crafted trees and the wide tree
    with candidate sets at the word edges of k_meta_mask_events, with reads that fill the 7-plane counter of k_meta_scores
    and with reads that need 16 planes; overlap coefficients and the top_oc rule with ties;
  * the EM after 1, 3 and 17 iterations against the longdouble restatement at 1e-9 on every proportion: column counts at
    the wave and unroll edges of k_meta_denoms, row counts at the chunk and block edges of k_meta_colsum / k_meta_fold /
    k_meta_sum_blocks, and column counts on the three paths of EmRound (LDS, raised LDS limit, scratch vector);
  * whole runs on small mixtures against the float64 restatement, each showing a property of the round loop.
tests/test_meta_em_families.py shows, without a device, that the inputs reach these cases and that no choice of the
restatement hangs on rounding.  Parity with the reference's own run stays unpinned (oracle/oracle_meta.py)."""
import numpy as np
import pytest

import assign_checks as ac
import em_checks as ec
from oracle import oracle_meta as om

pytestmark = pytest.mark.gpu

TOL = 1e-9                    # the EM tolerance of test_meta_gpu.test_em_equals_the_restatement


@pytest.fixture(scope="module")
def ctx(pmx):
    return pmx.Context(0)


@pytest.fixture(scope="module")
def metas(pmx, ctx):
    """family -> (tree, Meta): "wide" and the crafted trees by index"""
    out = {}
    for key, tree in [("wide", ec.wide_family()[0])] + list(enumerate(ac.crafted_trees())):
        plain, oriented = tree.indexes(pmx)
        out[key] = (tree, pmx.Meta(ctx, plain, oriented))
    yield out
    for _, meta in out.values():
        meta.close()


def _set_reads(meta, sample):
    """the sample to the device; its merged reads come back as the restatement lists them, in its order"""
    meta.set_reads(sample.reads)
    off, h, rev = meta.read_seedmers()
    ns, mult = meta.read_info()
    want_off, want_h, want_rev = ac.flat(sample.lists)
    assert np.array_equal(off, want_off) and np.array_equal(h, want_h) and np.array_equal(rev, want_rev)
    assert np.array_equal(ns, sample.n) and np.array_equal(mult, sample.mult)


def _check_scores(meta, R, sample, cands):
    meta.score(candidates=cands)
    assert np.array_equal(meta.candidates(), cands)
    got, want = meta.scores(), sample.scores(R, cands)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]


# ------------------------------------------------------------------------------------------------ a. scores and candidates
def _crafted_sample(i, cap):
    R = ac.crafted_restated(i)
    return R, ec.capped_sample(R, ac.crafted_reads()[0], cap)


def _longest_is(ns, cap):
    return ns.max() > 255 if cap is None else ns.max() == cap


@pytest.mark.parametrize("planes", ec.READ_CAPS)
@pytest.mark.parametrize("tree_index", range(len(ac.crafted_trees())))
def test_scores_on_the_crafted_trees(metas, tree_index, planes):
    tree, meta = metas[tree_index]
    R, sample = _crafted_sample(tree_index, ec.READ_CAPS[planes])
    _set_reads(meta, sample)
    assert _longest_is(meta.read_info()[0], ec.READ_CAPS[planes])
    for cands in ec.crafted_candidate_sets(len(tree.parent), tree_index):
        _check_scores(meta, R, sample, cands)


@pytest.mark.parametrize("planes", ec.READ_CAPS)
def test_scores_on_the_wide_tree(metas, planes):
    tree, meta = metas["wide"]
    R = ec.wide_family()[1]
    sample = ec.capped_sample(R, ec.wide_reads()[0], ec.READ_CAPS[planes])
    _set_reads(meta, sample)
    ns = meta.read_info()[0]
    assert _longest_is(ns, ec.READ_CAPS[planes])
    for count in ec.WIDE_CANDIDATE_COUNTS:
        cands = ec.wide_candidate_set(len(tree.parent), count)
        _check_scores(meta, R, sample, cands)
        assert meta.scores().max() == ns.max()                   # the counter is filled: a read with all of its seedmers present


@pytest.mark.parametrize("tree_index", range(len(ac.crafted_trees())))
def test_overlap_coefficients_and_top_oc(metas, tree_index):
    """no override: the coefficients of every node equal the restatement, and the candidates are the nodes whose
    coefficient is among the top_oc largest distinct values (folded nodes tie with their heads)"""
    tree, meta = metas[tree_index]
    R, sample = _crafted_sample(tree_index, None)
    meta.set_reads(sample.reads)
    oc = meta.overlap_coefficients()
    read_hashes = set(R.uniq.tolist())
    n_nodes = len(tree.parent)
    for v in range(n_nodes):
        assert abs(oc[v] - om.overlap_coefficient(tree.plain, v, read_hashes)) < 1e-12, v
    values = np.unique(oc)[::-1]
    assert len(values) < n_nodes or n_nodes <= 3                 # ties
    for top_oc in sorted({1, 2, len(values), len(values) + 1}):
        meta.score(top_oc=top_oc)
        want = np.nonzero(np.isin(oc, values[:top_oc]))[0]
        assert np.array_equal(meta.candidates(), want), top_oc
        assert np.array_equal(meta.scores(), sample.scores(R, want)), top_oc


# ------------------------------------------------------------------------------------------------ b. and c.: the EM
def _check_em(meta, haps, nodes, want, members=None):
    """the device's result against a restated run `want` over columns whose representatives are `nodes` (ascending)"""
    info = meta.em_info()
    assert info["rounds"] == want.rounds and info["iterations"] == want.iterations, (info, want.rounds, want.iterations)
    assert abs(info["log_likelihood"] - float(want.llh)) <= TOL * abs(float(want.llh)), (info, float(want.llh))
    want_nodes, want_props = np.asarray(nodes)[want.cols], want.props.astype(np.float64)
    got_nodes, got_props = np.array([h[0] for h in haps], np.int64), np.array([h[1] for h in haps])
    assert len(got_nodes) == len(want_nodes) and np.array_equal(np.sort(got_nodes), want_nodes)
    by_node = got_props[np.argsort(got_nodes)]
    assert np.abs(by_node - want_props).max() <= TOL, np.abs(by_node - want_props).max()
    # the order: by proportion, descending, equal proportions in candidate order -- on the device's own numbers, and node
    # for node the restatement's order wherever its neighbours are further than twice the tolerance away
    assert np.array_equal(got_nodes, want_nodes[np.argsort(-by_node, kind="stable")])
    order = want.order()
    p = want_props[order]
    apart = np.concatenate([[True], p[:-1] - p[1:] > 2 * TOL]) & np.concatenate([p[:-1] - p[1:] > 2 * TOL, [True]])
    assert np.array_equal(got_nodes[apart], want_nodes[order][apart])
    if members is not None:
        assert {h[0]: h[2] for h in haps} == {int(want_nodes[i]): members[want.cols[i]] for i in range(len(want_nodes))}


@pytest.mark.skipif(not ec.HAVE_LONGDOUBLE, reason=ec.LONGDOUBLE_REASON)
@pytest.mark.parametrize("n_cols,n_rows,discard", ec.FIXED_CASES)
def test_em_after_fixed_iterations(metas, n_cols, n_rows, discard):
    """em_max_iterations = 1, 3, 17 in one round with nothing dropped: what a reduction got wrong is still there.  Every
    proportion against the longdouble restatement at 1e-9, rounds == 1, iterations == the cap -- except in the three cases of
    em_checks.STOP_EARLY (one column, two columns, one read), which sit at their fixed point after an iteration or two and end
    by the default convergence rule after 2 or 3 iterations whatever the cap: there the iterations equal the restatement's"""
    from panmap_amd import _lib
    _, meta = metas["wide"]
    R = ec.wide_family()[1]
    cands, sample, sc, n, w = ec.fixed_case(n_cols, n_rows, discard)
    assert sc.shape == (n_rows, n_cols) and w.max() >= 2
    _set_reads(meta, sample)
    _check_scores(meta, R, sample, cands)
    whole = ec.fixed_restated(n_cols, n_rows, discard, "longdouble")
    for iterations in ec.FIXED_ITERATIONS:
        want = ec.cut(whole, iterations)
        assert want.iterations == iterations or ((n_cols, n_rows, discard) in ec.STOP_EARLY and iterations > 1)
        haps = meta.em(_lib.MetaParams(em_max_iterations=iterations, em_max_rounds=1, prop_threshold=0.0, discard=discard))
        assert len(haps) == n_cols and not any(h[2] for h in haps)
        _check_em(meta, haps, cands, want)


@pytest.mark.parametrize("name", ["drop_then_none", "one_round_with_a_drop", "delta_threshold", "duplicate_columns", "discard_half", "one_column"])
def test_whole_runs_on_small_mixtures(metas, name):
    from panmap_amd import _lib
    case = ec.small_cases()[name]
    want = case.restated()
    case.expect(want)                                            # the restatement shows the property the case is there for
    _, meta = metas[case.family]
    cols, members, _, _, _ = case.inputs()
    _set_reads(meta, case.sample)
    _check_scores(meta, case.R, case.sample, case.cands)
    haps = meta.em(_lib.MetaParams(**vars(case.params)))
    _check_em(meta, haps, np.asarray(case.cands, np.int64)[cols], want, members)
    props = [h[1] for h in haps]
    if name == "one_round_with_a_drop":
        assert props == [1.0 / len(haps)] * len(haps)            # exactly uniform, in candidate order
        assert [h[0] for h in haps] == sorted(h[0] for h in haps)
    if name == "duplicate_columns":
        grouped = {h[0]: h[2] for h in haps if h[2]}
        assert sum(len(m) for m in grouped.values()) == 3 and all(node < min(m) for node, m in grouped.items())
    if name == "one_column":
        assert len(haps) == 1 and props == [1.0] and np.isfinite(meta.em_info()["log_likelihood"])
