"""--meta --filter-and-assign --breadth-ratio on the device (Meta.assign(breadth=True); k_meta_breadth_rows and
k_meta_breadth_count of panmap_amd/csrc/meta_assign.hip) against the LITERAL restatement of tests/breadth_checks.py: TotalRefSeeds,
ObservedBreadthCount and TotalDepth bit-equal at every node, folded nodes equal to their heads -- on the crafted trees with the
tandem reads, on the hand-written tree, on rsv_4K (rows of two 64-word spans); in chunks of 1, 7 and 64 merged reads and with
the counters' flush bound lowered; with a taxonomy (reads spanning too many taxa contribute nothing); across read sets and
breadth on / off / on on one Meta; and the text of the file.  tests/test_breadth_families.py shows what the families reach.
Parity with the reference's own run is unpinned, as for the rest of --meta."""
import os

import numpy as np
import pytest

import assign_checks as ac
import breadth_checks as bc
import taxa_checks as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ERR_ARG = -1
_want = {}


def _crafted_want(i):
    """(assignment, numbers) of crafted tree i with the family's reads: computed once"""
    if i not in _want:
        R = bc.crafted_restated(i)
        _want[i] = (R, bc.restate_breadth(ac.crafted_trees()[i].oriented, R, R.lists))
    return _want[i]


def _rsv_want(arrays, discard):
    if ("rsv", discard) not in _want:
        R = ac.rsv_restated(arrays, discard)
        _want["rsv", discard] = (R, bc.restate_breadth(arrays, R, R.lists))
    return _want["rsv", discard]


@pytest.fixture(scope="module")
def crafted(pmx):
    """[(tree, Meta with the family's reads set, heads)]"""
    ctx = pmx.Context(0)
    out = []
    for tree in ac.crafted_trees():
        plain, oriented = tree.indexes(pmx)
        meta = pmx.Meta(ctx, plain, oriented)
        meta.set_reads(bc.reads())
        out.append((tree, meta, ac.heads_np(tree.parent, tree.oriented["offsets"])))
    return out


@pytest.fixture(scope="module")
def three(pmx):
    tree, reads, numbers = bc.three_nodes()
    plain, oriented = tree.indexes(pmx)
    meta = pmx.Meta(pmx.Context(0), plain, oriented)
    meta.set_reads(reads)
    return tree, meta, reads, numbers


@pytest.fixture(scope="module")
def rsv(pmx):
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    arrays = meta.index_oriented.arrays()
    meta.set_reads(ac.rsv_reads())
    return meta, arrays, ac.heads_np(arrays["parent"], arrays["offsets"])


def _check_crafted(crafted):
    for i, (tree, meta, heads) in enumerate(crafted):
        R, numbers = _crafted_want(i)
        res = meta.assign(bc.DISCARD, breadth=True)
        ac.check_result(res, R, tree.parent, heads, tree.name)
        bc.check_numbers(res.breadth, numbers, heads, tree.name)


def _check_three(three):
    tree, meta, reads, numbers = three
    res = meta.assign(0.0, breadth=True)
    R = ac.restate(tree.oriented, reads, 0.0)
    ac.check_result(res, R, tree.parent, np.arange(3), "three")
    bc.check_numbers(res.breadth, numbers, np.arange(3), "three, by hand")
    bc.check_numbers(res.breadth, bc.restate_breadth(tree.oriented, R, R.lists), np.arange(3), "three")


def _check_rsv(rsv, discards=(0.0, 0.6)):
    meta, arrays, heads = rsv
    for discard in discards:
        R, numbers = _rsv_want(arrays, discard)
        res = meta.assign(discard, breadth=True)
        ac.check_result(res, R, arrays["parent"], heads, "rsv %g" % discard)
        bc.check_numbers(res.breadth, numbers, heads, "rsv %g" % discard)


def test_crafted_trees_equal_the_restatement(crafted):
    _check_crafted(crafted)
    tree, meta, _ = crafted[-1]
    assert meta.ctx.kernel_ms("meta_breadth") > 0
    assert meta.read_info()[1].max() >= 2 and _crafted_want(len(crafted) - 1)[1][2].max() > 100


def test_three_nodes_equal_the_numbers_worked_out_by_hand(three):
    _check_three(three)


@pytest.mark.parametrize("discard", [0.0, 0.6])
def test_rsv_equals_the_restatement(rsv, discard):
    _check_rsv(rsv, (discard,))
    observed = _rsv_want(rsv[1], discard)[1][1]
    assert (observed[4096:] > 0).any() and len(observed) > 64 * 64


@pytest.mark.parametrize("chunk,flush", [(1, None), (7, None), (64, None), (None, bc.FLUSH), (7, 1)])
def test_results_do_not_depend_on_the_chunking_or_the_flush_bound(crafted, three, rsv, monkeypatch, chunk, flush):
    if chunk is not None:
        monkeypatch.setenv("PMX_META_ASSIGN_CHUNK", str(chunk))
    if flush is not None:
        monkeypatch.setenv("PMX_META_BREADTH_FLUSH", str(flush))
    _check_crafted(crafted)
    _check_three(three)
    _check_rsv(rsv)


@pytest.mark.parametrize("case", tc.LEGS["default"])
def test_reads_over_the_taxon_limit_contribute_nothing(crafted, case):
    """the labelling of taxa_checks with at most one taxon a read, on the reads of assign_checks (the restatement of that leg is
    shared with the taxonomy tests): the breadth is that of the FILTERED assignment"""
    i = tc.TREES[case[0]]
    tree, meta, heads = crafted[i]
    _, taxon, want = tc.crafted_leg(*case)
    base = ac.crafted_restated(i)
    numbers = bc.restate_breadth(tree.oriented, want, base.lists)
    unfiltered = bc.restate_breadth(tree.oriented, base, base.lists)
    assert tc.counts(want)[0] > 0 and (numbers[2] < unfiltered[2]).any() and np.array_equal(numbers[0], unfiltered[0])
    try:
        meta.set_reads(ac.crafted_reads()[0])
        meta.set_taxonomy(taxon, case[5])
        res = meta.assign(case[1], breadth=True)
        tc.check_taxa_result(res, want, heads, str(case))
        bc.check_numbers(res.breadth, numbers, heads, str(case))
    finally:
        meta.set_taxonomy(max_taxa=0)
        meta.set_reads(bc.reads())


def test_one_meta_across_read_sets_and_breadth_on_off_on(pmx, crafted):
    lib = pmx._lib.lib
    tree, meta, heads = crafted[-1]
    n = len(tree.parent)
    R, numbers = _crafted_want(len(crafted) - 1)
    out = [np.zeros(n, np.uint64) for _ in range(3)]
    fetch = lambda: lib.pmx_meta_breadth(meta._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, n)
    try:
        on = meta.assign(bc.DISCARD, breadth=True)
        bc.check_numbers(on.breadth, numbers, heads, "on")
        assert fetch() == 0 and lib.pmx_meta_breadth(meta._h, None, None, None, n - 1) == ERR_ARG
        off = meta.assign(bc.DISCARD)                                      # breadth off: today's result, and nothing to fetch
        assert off.breadth is None and fetch() == ERR_ARG and meta.ctx.kernel_ms("meta_breadth") < 0
        ac.check_result(off, R, tree.parent, heads, "off")
        for a, b in ((on.state, off.state), (on.max, off.max), (on.lca, off.lca), (on._nodes, off._nodes), (on._off, off._off)):
            assert np.array_equal(a, b)
        with pytest.raises(ValueError):
            pmx.format_breadths(off, str)
        subset = bc.reads()[40:90]                                         # another read set: its own numbers; set_reads empties the result
        meta.assign(bc.DISCARD, breadth=True)
        meta.set_reads(subset)
        assert fetch() == ERR_ARG
        want = ac.restate(tree.oriented, subset, bc.DISCARD)
        res = meta.assign(bc.DISCARD, breadth=True)
        ac.check_result(res, want, tree.parent, heads, "subset")
        bc.check_numbers(res.breadth, bc.restate_breadth(tree.oriented, want, want.lists), heads, "subset")
        assert fetch() == 0 and np.array_equal(out[2].astype(np.int64), res.breadth[2])
        meta.set_reads(bc.reads())
        bc.check_numbers(meta.assign(bc.DISCARD, breadth=True).breadth, numbers, heads, "on again")
    finally:
        meta.set_reads(bc.reads())


def test_no_assigned_read_gives_zeros_and_the_header_alone(pmx, crafted):
    tree, meta, heads = crafted[1]
    try:
        meta.set_reads(sorted(ac.crafted_reads()[2])[:5])                  # random reads: they match nothing
        res = meta.assign(bc.DISCARD, breadth=True)
        assert not (res.state == ac.ASSIGNED).any() and not res.breadth[1].any() and not res.breadth[2].any()
        assert np.array_equal(res.breadth[0], _crafted_want(1)[1][0])
        assert pmx.format_breadths(res, str) == bc.HEADER + "\n"
    finally:
        meta.set_reads(bc.reads())


def test_format_breadths_equals_the_restated_text(pmx, crafted, three, rsv):
    for i, (tree, meta, heads) in enumerate(crafted):
        node_id = lambda v: "node_%d" % v
        res = meta.assign(bc.DISCARD, breadth=True)
        text = pmx.format_breadths(res, node_id)
        assert text == bc.restate_text(_crafted_want(i)[1], heads, node_id, True), tree.name
        assert len(text.splitlines()) == 1 + int((heads == np.arange(len(heads))).sum())
    tree, meta, reads, numbers = three
    assert pmx.format_breadths(meta.assign(0.0, breadth=True), str) == bc.restate_text(numbers, np.arange(3), str, True)
    meta, arrays, heads = rsv
    text = pmx.format_breadths(meta.assign(0.6, breadth=True), meta.index.node_id)
    assert text == bc.restate_text(_rsv_want(arrays, 0.6)[1], heads, meta.index.node_id, True)
    assert any("," in line.split("\t")[0] for line in text.splitlines()[1:])    # folded nodes on their head's line
