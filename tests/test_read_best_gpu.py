"""Meta.read_best / Meta.active_nodes on the device (pmx_meta_read_best, k_meta_active_nodes and k_meta_read_best of
panmap_amd/csrc/meta_assign.hip) against the restatement of tests/read_best_checks.py: the active nodes, and per merged read
its best score over all nodes and the number of active nodes that reach it -- on the crafted trees, in chunks of 1, 7 and 64
merged reads, on the edge family, on rsv_4K beside Meta.assign, on reads set with a mask and with masked ends, and across
several read sets on one Meta.  Parity with the reference's own run is unpinned, as for --meta (oracle/oracle_meta.py)."""
import os

import numpy as np
import pytest

import assign_checks as ac
import ends_checks as ec
import mask_checks as mc
import read_best_checks as rb
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted(pmx):
    """[(tree, Meta)] with the crafted reads set"""
    ctx = pmx.Context(0)
    out = []
    for tree in ac.crafted_trees():
        plain, oriented = tree.indexes(pmx)
        meta = pmx.Meta(ctx, plain, oriented)
        meta.set_reads(ac.crafted_reads()[0])
        out.append((tree, meta))
    return out


@pytest.fixture(scope="module")
def rsv(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    meta = pmx.Meta.build(pmx.Context(0), pm)
    arrays = meta.index_oriented.arrays()
    meta.set_reads(ac.rsv_reads())
    return meta, arrays


@pytest.fixture(scope="module")
def rsv_best(rsv):
    return rb.restate_best(rsv[1], ac.rsv_reads())


def _check_crafted(crafted):
    for i, (tree, meta) in enumerate(crafted):
        rb.check_best(meta, rb.crafted_best(i), tree.name)


def test_crafted_family_equals_the_restatement(crafted):
    _check_crafted(crafted)
    ns, mult = crafted[-1][1].read_info()
    assert ns.max() >= 128 and (ns == 127).any() and mult.max() >= 2     # both plane counts ran; copies were merged


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_results_do_not_depend_on_the_chunking(crafted, monkeypatch, chunk):
    monkeypatch.setenv("PMX_META_ASSIGN_CHUNK", str(chunk))
    _check_crafted(crafted)


@pytest.mark.parametrize("n,shape", rb.EDGE_CASES, ids=["%s%d" % (shape, n) for n, shape in rb.EDGE_CASES])
def test_edge_family_is_exact(pmx, ctx, n, shape):
    tree = rb.edge_tree(n, shape)
    plain, oriented = tree.indexes(pmx)
    meta = pmx.Meta(ctx, plain, oriented)
    meta.set_reads(rb.edge_reads().reads)
    rb.check_best(meta, rb.edge_restated(n, shape), tree.name)
    meta.close()


def _stored_assignment(pmx, meta):
    """what the handle holds of its last pmx_meta_assign, fetched without running it again"""
    lib, n = pmx._lib.lib, meta.n_reads
    state, mx = np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    lca, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert lib.pmx_meta_assign_reads(meta._h, state.ctypes.data, mx.ctypes.data, lca.ctypes.data, cnt.ctypes.data, n) == 0
    off, nodes = np.zeros(n + 1, np.int64), np.zeros(max(int(lib.pmx_meta_assign_num_nodes(meta._h)), 1), np.uint32)
    assert lib.pmx_meta_assign_nodes(meta._h, off.ctypes.data, nodes.ctypes.data, len(nodes)) == 0
    return state, mx, lca, cnt, off, nodes[:off[-1]]


def _stored_best(pmx, meta):
    """what the handle holds of its last pmx_meta_read_best, fetched without running it again"""
    lib, n = pmx._lib.lib, meta.n_reads
    mx, nb = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    act = np.zeros(meta.index_oriented.info.n_nodes, np.uint8)
    assert lib.pmx_meta_read_best_get(meta._h, mx.ctypes.data, nb.ctypes.data, n) == 0
    assert lib.pmx_meta_active_nodes(meta._h, act.ctypes.data, len(act)) == 0
    return mx, nb, act


@pytest.mark.parametrize("n,shape", rb.LONG_CASES, ids=["%s%d" % (shape, n) for n, shape in rb.LONG_CASES])
def test_edge_family_through_sixteen_planes(pmx, ctx, n, shape):
    tree, E = rb.edge_tree(n, shape), rb.edge_reads()
    plain, oriented = tree.indexes(pmx)
    meta = pmx.Meta(ctx, plain, oriented)
    meta.set_reads(E.reads + [E.long])
    assert meta.read_info()[0].max() >= 128
    rb.check_best(meta, rb.edge_restated_long(n, shape), tree.name + " with the long read")
    meta.close()


def test_rsv_equals_the_restatement_and_agrees_with_assign(pmx, rsv, rsv_best):
    meta, _ = rsv
    before = meta.assign(0.0)
    stored = _stored_assignment(pmx, meta)
    assert stored[4][-1] > 0 and (stored[0] == ac.ASSIGNED).any()
    rb.check_best(meta, rsv_best, "rsv")
    mx, nb = meta.read_best()                                              # (a second call: the active nodes are kept)
    active = meta.active_nodes()
    # read_best left the stored assignment as it was ...
    for a, b in zip(stored, _stored_assignment(pmx, meta)):
        assert a.shape == b.shape and np.array_equal(a, b)
    # ... and an assign (with another threshold: other states and lists) leaves the stored read_best results as they were
    held = _stored_best(pmx, meta)
    assert np.array_equal(held[0], mx) and np.array_equal(held[1], nb) and np.array_equal(held[2].astype(bool), active)
    meta.assign(0.6)
    for a, b in zip(held, _stored_best(pmx, meta)):
        assert np.array_equal(a, b)
    rb.check_best(meta, rsv_best, "rsv, after an assign")
    merged = before.merged
    first = {int(m): r for r, m in reversed(list(enumerate(merged))) if m >= 0}      # a raw read of every merged read
    assert sorted(first) == list(range(len(mx)))
    for m, r in first.items():
        assert before.max[r] == mx[m], m
        assert int(active[before.nodes_of(r)].sum()) == nb[m], m
    assert (nb > 64).any() and (mx == 0).any() and not active.all()
    assert any(len(before.nodes_of(r)) > nb[m] > 0 for m, r in first.items())      # inactive nodes inside a tie set


def test_masked_seeds_run_where_assign_refuses(pmx, rsv):
    meta, arrays = rsv
    reads = mc.family().reads
    off, h, v, mult, raw = mc.family_merged()
    threshold = 2
    n_off, n_h, n_v, _, old_to_new, _, removed, _ = mc.restate_masks(off, h, v, mult, 0, threshold)
    assert removed > 0 and (old_to_new < 0).any()
    want = rb.best_of_lists(arrays, n_off, n_h, n_v, np.where(raw >= 0, old_to_new[np.maximum(raw, 0)], -1))
    try:
        meta.set_masks(seeds=threshold)
        meta.set_reads(reads)
        with pytest.raises(pmx._lib.PmxError) as err:
            meta.assign(0.0)
        assert err.value.code == -7
        rb.check_best(meta, want, "mask-seeds")
        assert (want.max > 0).any()
    finally:
        meta.set_masks()
        meta.set_reads(ac.rsv_reads())


def test_masked_read_ends_run_where_assign_refuses(pmx, rsv):
    meta, arrays = rsv
    n = 5
    reads = ec.family(n).reads
    want = rb.restate_best(arrays, ec.trimmed(reads, n))
    try:
        meta.set_mask_read_ends(n)
        meta.set_reads(reads)
        with pytest.raises(pmx._lib.PmxError) as err:
            meta.assign(0.0)
        assert err.value.code == -7
        rb.check_best(meta, want, "mask-read-ends")
        assert (want.max > 0).any() and (want.merged < 0).any()
    finally:
        meta.set_mask_read_ends(0)
        meta.set_reads(ac.rsv_reads())


def _code(call):
    try:
        call()
    except Exception as err:                                              # PmxError
        return err.code
    return 0


def test_set_reads_empties_the_results(pmx, crafted):
    tree, meta = crafted[1]
    lib = pmx._lib.lib
    n = meta.n_reads
    mx, nb = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    act = np.zeros(len(tree.parent), np.uint8)
    meta.read_best()
    assert lib.pmx_meta_read_best_get(meta._h, mx.ctypes.data, nb.ctypes.data, n) == 0
    assert lib.pmx_meta_read_best_get(meta._h, None, None, n) == 0 and lib.pmx_meta_read_best_get(meta._h, None, None, n - 1) == -1
    assert lib.pmx_meta_active_nodes(meta._h, act.ctypes.data, len(act)) == 0
    meta.set_reads(ac.crafted_reads()[0])
    assert lib.pmx_meta_read_best_get(meta._h, mx.ctypes.data, nb.ctypes.data, n) == -1       # PMX_ERR_ARG
    assert lib.pmx_meta_active_nodes(meta._h, act.ctypes.data, len(act)) == -1
    rb.check_best(meta, rb.crafted_best(1), tree.name)


def test_before_set_reads_and_with_an_attached_dist(pmx, monkeypatch, tmp_path):
    monkeypatch.setenv("PMX_DIST_HOST_DIR", str(tmp_path))
    ctx = pmx.Context(0)
    plain, oriented = ac.crafted_trees()[1].indexes(pmx)
    meta = pmx.Meta(ctx, plain, oriented)
    early = _code(meta.read_best)
    dist = pmx.Dist(ctx, pmx.Dist.unique_id(), 0, 1)
    meta.attach_dist(dist)
    meta.set_reads(ac.crafted_reads()[0][:20])
    code = _code(meta.read_best)
    meta.close()                                                         # (in this order: each is freed on its live context)
    dist.close()
    assert early == -1 and code == -7                                    # PMX_ERR_ARG, PMX_ERR_UNSUPPORTED


def test_one_meta_across_read_sets_equals_fresh_handles(pmx, rsv):
    meta, arrays = rsv
    reads = ac.rsv_reads()
    ctx = pmx.Context(0)
    try:
        for subset in (reads[:50], reads[100:700], reads[700:707]):
            meta.set_reads(subset)
            got = meta.read_best() + (meta.active_nodes(),)
            fresh = pmx.Meta(ctx, meta.index, meta.index_oriented)
            fresh.set_reads(subset)
            want = fresh.read_best() + (fresh.active_nodes(),)
            fresh.close()
            for a, b in zip(got, want):
                assert np.array_equal(a, b), len(subset)
            rb.check_best(meta, rb.restate_best(arrays, subset), "subset of %d" % len(subset))
    finally:
        meta.set_reads(reads)
