"""The taxonomy filter of --meta --filter-and-assign on the device (Meta.set_taxonomy / Meta.assign; k_meta_assign_near and
k_meta_assign_taxa of panmap_amd/csrc/meta_assign.hip) against the LITERAL restatement of tests/taxa_checks.py, read by read:
state, best score, nodes, LCA head and taxa, on every leg of taxa_checks.LEGS (tests/test_taxa_families.py shows that each
has reads of both fates) and on rsv_4K, whose rows span two 64-word steps.  Chunk sizes of 1, 7 and 64 reads give the same
answers; clearing the taxonomy restores the results without one; the two refusals."""
import os

import numpy as np
import pytest

import assign_checks as ac
import taxa_checks as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
UNSUPPORTED = -7


@pytest.fixture(scope="module")
def crafted(pmx):
    """{tree name: (Meta with the crafted reads set, heads)}"""
    ctx = pmx.Context(0)
    out = {}
    for tree in ac.crafted_trees():
        plain, oriented = tree.indexes(pmx)
        meta = pmx.Meta(ctx, plain, oriented)
        meta.set_reads(ac.crafted_reads()[0])
        out[tree.name] = (meta, ac.heads_np(tree.parent, tree.oriented["offsets"]))
    return out


def _run(crafted, case):
    """one case of taxa_checks.LEGS through the device: (result, restatement, heads)"""
    name, discard, A, ratio, T, M = case
    meta, heads = crafted[name]
    _, taxon, want = tc.crafted_leg(*case)
    meta.set_taxonomy(taxon, M)
    try:
        return meta.assign(discard, ambiguous=A, ambiguous_ratio=ratio), want, heads
    finally:
        meta.set_taxonomy(max_taxa=0)


@pytest.mark.parametrize("leg", list(tc.LEGS))
def test_legs_equal_the_literal_restatement(crafted, leg):
    for case in tc.LEGS[leg]:
        res, want, heads = _run(crafted, case)
        tc.check_taxa_result(res, want, heads, str(case))
        assert (res.state == tc.OVER_TAXA).sum() == (want.state == tc.OVER_TAXA).sum()
        assert (res.fastq_index[res.state == tc.OVER_TAXA] == -1).all()


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_results_do_not_depend_on_the_chunking(crafted, monkeypatch, chunk):
    monkeypatch.setenv("PMX_META_ASSIGN_CHUNK", str(chunk))
    for case in (tc.LEGS["absolute"][2], tc.LEGS["default"][2]):
        assert case[0] in ("random300", "binary129")
        res, want, heads = _run(crafted, case)
        tc.check_taxa_result(res, want, heads, "chunk %d %s" % (chunk, case))


def test_the_16_plane_reads_go_through_the_near_kernel(crafted):
    """the 1,200-base read and its prefixes of 127 and 128 seedmers are part of the ratio leg: assigned or over, not skipped"""
    case = tc.LEGS["ratio"][0]
    res, want, _ = _run(crafted, case)
    n = ac.crafted_restated(tc.TREES[case[0]]).n
    assert sorted(n[n >= 127].tolist())[:2] == [127, 128] and (n > 128).sum() == 1
    assert np.isin(res.state[n >= 127], (ac.ASSIGNED, tc.OVER_TAXA)).all() and np.array_equal(res.state[n >= 127], want.state[n >= 127])


def test_clearing_the_taxonomy_restores_the_results(pmx, crafted):
    meta, heads = crafted["random300"]
    tree = ac.crafted_trees()[tc.TREES["random300"]]
    before = meta.assign(0.5)
    assert meta.ctx.kernel_ms("meta_assign") > 0 and meta.ctx.kernel_ms("meta_assign_taxa") < 0
    res, want, _ = _run(crafted, tc.LEGS["default"][3])
    assert meta.ctx.kernel_ms("meta_assign_taxa") > 0 and (res.state == tc.OVER_TAXA).any()
    after = meta.assign(0.5, ambiguous=3, ambiguous_ratio=0.5)        # (without a taxonomy the thresholds act on nothing)
    assert meta.ctx.kernel_ms("meta_assign_taxa") < 0
    ac.check_result(after, ac.crafted_restated(tc.TREES["random300"]), tree.parent, heads, "cleared")
    for a, b in ((before.state, after.state), (before.max, after.max), (before.lca, after.lca), (before._nodes, after._nodes), (before._off, after._off)):
        assert np.array_equal(a, b)
    assert all(len(after.taxa_of(r)) == 0 for r in range(len(after.state))) and len(after.node_taxa(0)) == 0


def test_refusals(pmx, crafted):
    meta, _ = crafted["path3"]
    taxon = tc.label(ac.crafted_trees()[tc.TREES["path3"]].parent, 16)
    try:
        with pytest.raises(pmx._lib.PmxError) as err:
            meta.set_taxonomy(taxon, 17)
        assert err.value.code == UNSUPPORTED
        meta.set_taxonomy(taxon, 16)
        for kw in (dict(ambiguous=1), dict(ambiguous_ratio=0.1)):
            with pytest.raises(pmx._lib.PmxError) as err:
                meta.assign(0.5, **kw)
            assert err.value.code == UNSUPPORTED
        assert (meta.assign(0.0, ambiguous=1).state == ac.ASSIGNED).any() and (meta.assign(0.5).state == ac.ASSIGNED).any()
    finally:
        meta.set_taxonomy(max_taxa=0)


def test_rsv_equals_the_literal_restatement(pmx):
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    arrays = meta.index_oriented.arrays()
    meta.set_reads(ac.rsv_reads())
    meta.set_taxonomy(tc.label(arrays["parent"], tc.RSV_T), 1)
    want = tc.rsv_leg(arrays)
    tc.check_taxa_result(meta.assign(tc.RSV_DISCARD), want, ac.heads_np(arrays["parent"], arrays["offsets"]), "rsv")
    assert min(tc.counts(want)) >= 20
    meta.close()
