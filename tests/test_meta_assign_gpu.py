"""--meta --filter-and-assign on the device (pmx_meta_assign, panmap_amd/csrc/meta_assign.hip) against the restatement of
tests/assign_checks.py: for every raw read its state, best score, assigned nodes, LCA head and merged read, on the crafted
trees (given through Index.from_arrays) and on rsv_4K -- whole, in chunks of 1, 7 and 64 merged reads, with DUST, and across
several read sets on one Meta.  Parity with the reference's own run is unpinned, as for --meta (oracle/oracle_meta.py)."""
import os

import numpy as np
import pytest

import assign_checks as ac
from conftest import GOLDEN
from oracle import oracle_meta as om

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted(pmx):
    """[(tree, Meta, heads)] with the crafted reads set"""
    ctx = pmx.Context(0)
    out = []
    for tree in ac.crafted_trees():
        plain, oriented = tree.indexes(pmx)
        meta = pmx.Meta(ctx, plain, oriented)
        meta.set_reads(ac.crafted_reads()[0])
        out.append((tree, meta, ac.heads_np(tree.parent, tree.oriented["offsets"])))
    return out


@pytest.fixture(scope="module")
def rsv(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    meta = pmx.Meta.build(pmx.Context(0), pm)
    arrays = meta.index_oriented.arrays()
    meta.set_reads(ac.rsv_reads())
    return meta, arrays, ac.heads_np(arrays["parent"], arrays["offsets"])


def _check_crafted(crafted):
    for i, (tree, meta, heads) in enumerate(crafted):
        ac.check_result(meta.assign(0.5), ac.crafted_restated(i), tree.parent, heads, tree.name)


def _check_rsv(rsv):
    meta, arrays, heads = rsv
    for discard in ac.RSV_DISCARDS:
        ac.check_result(meta.assign(discard), ac.rsv_restated(arrays, discard), arrays["parent"], heads, "rsv %g" % discard)


def test_crafted_family_equals_the_restatement(crafted):
    _check_crafted(crafted)
    tree, meta, _ = crafted[-1]
    ns, mult = meta.read_info()
    assert ns.max() >= 128 and mult.max() >= 2                          # the 16-plane kernel ran; copies were merged


def test_rsv_family_equals_the_restatement(rsv):
    _check_rsv(rsv)
    res = rsv[0].assign(0.0)
    assert (res.state == ac.ASSIGNED).sum() > 600 and max(len(res.nodes_of(r)) for r in range(0, 780, 7)) > 64


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_results_do_not_depend_on_the_chunking(crafted, rsv, monkeypatch, chunk):
    monkeypatch.setenv("PMX_META_ASSIGN_CHUNK", str(chunk))
    _check_crafted(crafted)
    _check_rsv(rsv)


def test_one_meta_across_read_sets_then_score_and_em(pmx, rsv):
    """three set_reads / assign calls of different sizes on one Meta, then the abundance path still gives the reference's e2e
    expectation (src/test/e2e/run_e2e.sh:182-204: 700 + 300 tiled reads -> MZ515733.1 in (0.55, 0.82), node_1330 in (0.18, 0.45))"""
    meta, arrays, heads = rsv
    reads = ac.rsv_reads()
    try:
        for subset in (reads[:50], reads[100:700], reads[700:707]):
            meta.set_reads(subset)
            ac.check_result(meta.assign(0.6), ac.restate(arrays, subset, 0.6), arrays["parent"], heads, "subset of %d" % len(subset))
        a, b = ac._fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), ac._fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
        meta.set_reads(ac._tile(a, 700) + ac._tile(b, 300))
        meta.assign(0.0)
        meta.score(top_oc=1000)
        got = {meta.index.node_id(node): p for node, p, _ in meta.em()}
        assert len(got) == 2 and 0.55 < got["MZ515733.1"] < 0.82 and 0.18 < got["node_1330"] < 0.45 and 0.99 < sum(got.values()) < 1.01
    finally:
        meta.set_reads(reads)


def test_dust_drops_reads_before_the_assignment(rsv):
    meta, arrays, heads = rsv
    reads = ac.rsv_reads()
    threshold = float(np.median([om.get_dust(r) for r in reads]))
    want = ac.restate(arrays, reads, 0.0, dust=threshold)
    assert 100 < (want.merged < 0).sum() < 700
    try:
        meta.set_dust(threshold)
        meta.set_reads(reads)
        ac.check_result(meta.assign(0.0), want, arrays["parent"], heads, "dust %g" % threshold)
    finally:
        meta.set_dust(100.0)
        meta.set_reads(reads)


def test_an_attached_dist_is_refused(pmx, monkeypatch, tmp_path):
    monkeypatch.setenv("PMX_DIST_HOST_DIR", str(tmp_path))
    ctx = pmx.Context(0)
    plain, oriented = ac.crafted_trees()[1].indexes(pmx)
    meta = pmx.Meta(ctx, plain, oriented)
    dist = pmx.Dist(ctx, pmx.Dist.unique_id(), 0, 1)
    meta.attach_dist(dist)
    meta.set_reads(ac.crafted_reads()[0][:20])
    code = 0
    try:
        meta.assign(0.0)
    except pmx._lib.PmxError as err:
        code = err.code
    meta.close()                                                         # (in this order: each is freed on its live context)
    dist.close()
    assert code == -7                                                    # PMX_ERR_UNSUPPORTED
