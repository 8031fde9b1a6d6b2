"""--em-leaves-only on the device path (pmx_meta_set_em_leaves_only; select_candidates, panmap_amd/csrc/api_meta.hip) against
the rule restated in tests/ends_checks.py from the overlap coefficients, the node ids and the heads: on rsv_4K, and on a
hand-written tree of eight nodes given through Index.from_arrays with ids."""
import os

import numpy as np
import pytest

import assign_checks as ac
import ends_checks as ec
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOP_OCS = (1, 2, 5, 1000)


@pytest.fixture(scope="module")
def params(pmx):
    from panmap_amd import _lib
    return _lib.MetaParams()


@pytest.fixture(scope="module")
def rsv(pmx):
    """(Meta with the rsv family's reads set, ids, heads, overlap coefficients)"""
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    meta = pmx.Meta.build(pmx.Context(0), pm)
    meta.set_reads(ac.rsv_reads())
    n = meta.index.info.n_nodes
    return meta, [meta.index.node_id(v) for v in range(n)], meta.index_oriented.node_heads(), meta.overlap_coefficients()


def _scored(meta, params, top_oc=1000, candidates=None):
    meta.score(top_oc=top_oc, candidates=candidates)
    return meta.candidates(), meta.scores(), [(node, int(ec.bits(p)[0]), members) for node, p, members in meta.em(params)]


@pytest.mark.parametrize("top_oc", TOP_OCS)
def test_candidates_equal_the_rule_restated(rsv, params, top_oc):
    meta, ids, heads, oc = rsv
    want = ec.leaves_candidates(oc, ids, heads, top_oc)
    meta.set_em_leaves_only(True)
    cands, scores, haps = _scored(meta, params, top_oc)
    meta.set_em_leaves_only(False)
    assert len(want) > 0 and np.array_equal(cands, want)
    assert ec.eligible_nodes(ids, heads)[cands].all()
    # exactly these nodes given as an override, the switch off: the same columns, so the same scores and the same haplotypes
    cands2, scores2, haps2 = _scored(meta, params, top_oc, candidates=want)
    assert np.array_equal(cands2, want) and np.array_equal(scores2, scores) and haps2 == haps and len(haps) > 0
    # every line of the report names a sequence that exists
    for node, _, members in haps:
        assert any(ec.is_sample(ids[v]) for v in [node] + members), (node, members)
    # and without the switch the candidates are what they were
    plain, _, _ = _scored(meta, params, top_oc)
    assert np.array_equal(plain, ec.plain_candidates(oc, top_oc))


def test_leaves_only_narrows_the_candidates(rsv, params):
    meta, ids, heads, oc = rsv
    assert not ec.eligible_nodes(ids, heads).all() and ec.eligible_nodes(ids, heads).any()
    # a strict subset of the run without the switch, for some top_oc (at a given top_oc it need not be a subset at all:
    # passing over a rank lets a later one in; with more ranks than the tree has values it is one)
    strict = [t for t in TOP_OCS + (len(oc),)
              if set(ec.leaves_candidates(oc, ids, heads, t).tolist()) < set(ec.plain_candidates(oc, t).tolist())]
    assert strict
    meta.set_em_leaves_only(True)
    got = _scored(meta, params, strict[0])[0]
    meta.set_em_leaves_only(False)
    assert set(got.tolist()) < set(_scored(meta, params, strict[0])[0].tolist())


def test_an_override_ignores_the_switch(rsv, params):
    meta, ids, heads, oc = rsv
    barred = np.nonzero(~ec.eligible_nodes(ids, heads))[0][:7].astype(np.uint32)
    assert len(barred) == 7
    meta.set_em_leaves_only(True)
    cands = _scored(meta, params, 1, candidates=barred)[0]
    meta.set_em_leaves_only(False)
    assert np.array_equal(cands, barred)


@pytest.fixture(scope="module")
def small(pmx):
    tree, reads, ids = ec.small_tree()
    plain, oriented = ec.small_indexes(pmx, ids)
    meta = pmx.Meta(pmx.Context(0), plain, oriented)
    meta.set_reads(reads)
    return meta, tree, reads, ids


def test_small_tree_ranks_shift_fold_and_cut(small, params):
    meta, tree, reads, ids = small
    assert [meta.index.node_id(v) for v in range(8)] == ids
    heads = meta.index_oriented.node_heads()
    assert list(heads) == [0, 1, 2, 3, 4, 5, 6, 6]
    oc = meta.overlap_coefficients()
    ok = ec.eligible_nodes(ids, heads)
    assert int(np.argmax(oc)) == 1 and not ok[1]                # the best coefficient is an inferred ancestor's: the ranks shift
    assert not ec.is_sample(ids[6]) and ok[6] and oc[6] == oc[7]    # node_5 is eligible through the fold alone
    meta.set_em_leaves_only(True)
    got = {t: _scored(meta, params, t) for t in (1, 2, 3, 1000)}
    meta.set_em_leaves_only(False)
    for t, (cands, _, haps) in got.items():
        assert np.array_equal(cands, ec.leaves_candidates(oc, ids, heads, t)), t
        assert 1 not in cands and 0 not in cands and 3 not in cands and 5 not in cands
        assert haps and all(any(ec.is_sample(ids[v]) for v in [node] + members) for node, _, members in haps)
    sizes = [len(got[t][0]) for t in (1, 2, 3)]
    assert sizes[0] < sizes[1] < sizes[2] == 4                 # top_oc cuts between the eligible ranks
    assert list(got[3][0]) == [2, 4, 6, 7] and np.array_equal(got[1000][0], got[3][0])
    assert list(_scored(meta, params, 1)[0]) == [1]            # without the switch: the ancestor alone


def test_a_tree_without_a_sample_is_refused(pmx, small, params):
    tree, reads = small[1], small[2]
    plain, oriented = ec.small_indexes(pmx, ["node_%d" % v for v in range(8)])
    meta = pmx.Meta(pmx.Context(0), plain, oriented)
    meta.set_reads(reads)
    meta.set_em_leaves_only(True)
    with pytest.raises(pmx._lib.PmxError) as e:
        meta.score(top_oc=1000)
    assert e.value.code == -1 and "em-leaves-only" in str(e.value)
    meta.score(top_oc=1000, candidates=np.array([1, 2], np.uint32))          # an override is still taken
    assert list(meta.candidates()) == [1, 2]
    meta.set_em_leaves_only(False)
    meta.score(top_oc=1000)
    assert len(meta.candidates()) == 8
