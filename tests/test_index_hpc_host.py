"""The HPC index producer (pmx_index_build_ex with PMX_INDEX_HPC) on rsv_4K: node n contributes the seeds of
hpc(genome(n)), the flank mask judged at the uncompressed coordinate of a k-mer's first base.  The checker is the oracle on
genomes compressed in Python (tests/hpc_checks.py)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from hpc_checks import hpc


@pytest.fixture(scope="module")
def rsv(pmx):
    return pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))


def _path_to_root(parent, nd):
    path = [nd]
    while nd != 0:
        nd = int(parent[nd])
        path.append(nd)
    return path[::-1]


def _reconstruct(a, off, nd):
    """the node's seed multiset from the count changes along its root path (the idiom of test_host_stage.py)"""
    counts = {}
    for p in _path_to_root(a["parent"], nd):
        sl = slice(off[p], off[p + 1])
        for hh, pc, cc in zip(a["hash"][sl].tolist(), a["parent_count"][sl].tolist(), a["child_count"][sl].tolist()):
            assert counts.get(hh, 0) == pc
            if cc:
                counts[hh] = cc
            else:
                counts.pop(hh, None)
    return counts


def _want(oracle, genome, k, s, l):
    hs, cn = oracle.histogram([hpc(genome)[0]], k, s, l)
    return dict(zip(hs.tolist(), cn.tolist()))


def _spread(n, count):
    return sorted(set([0] + np.linspace(1, n - 1, count).astype(int).tolist()))


def test_hpc_index_nodes_hold_the_seeds_of_their_compressed_genomes(pmx, oracle, rsv, monkeypatch):
    index = pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=0)
    assert index.hpc and index.info.hpc == 1
    a = index.arrays()
    off = a["offsets"].astype(np.int64)
    n = len(off) - 1
    assert n == rsv.num_nodes and off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(a["hash"])
    assert np.all(a["parent_count"] != a["child_count"])
    for nd in _spread(n, 40):
        assert _reconstruct(a, off, nd) == _want(oracle, rsv.genome(nd), 15, 8, 1), nd
    # it differs from the plain index (the compression is not a no-op on this tree)
    plain = pmx.Index.build(rsv, k=15, s=8, l=1, flank_mask=0, mode=1, max_nodes=60)
    m = int(plain.arrays()["offsets"][60])
    assert not plain.hpc and m > 0 and not np.array_equal(plain.arrays()["hash"][:m], a["hash"][:m])
    # parallel = serial: chunks of the pre-order, each replaying its root path, give the arrays of the serial walk
    # (on the first 1,500 nodes: nine chunks for five workers, and a serial walk of a few seconds)
    monkeypatch.setenv("PMX_INDEX_THREADS", "1")
    serial = pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=0, max_nodes=1500).arrays()
    monkeypatch.setenv("PMX_INDEX_THREADS", "5")
    par = pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=0, max_nodes=1500).arrays()
    m = int(serial["offsets"][1500])
    assert m > 0 and np.array_equal(serial["hash"][:m], a["hash"][:m]) and np.array_equal(serial["offsets"][:1501], a["offsets"][:1501])
    for key in serial:
        assert np.array_equal(serial[key], par[key]), key
    # mode 1 with the bit is the same producer; max_nodes stops it
    part = pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=0, mode=1, max_nodes=50).arrays()
    m = int(part["offsets"][50])
    assert np.array_equal(part["hash"][:m], a["hash"][:m]) and np.all(part["offsets"][50:] == m)


def test_hpc_index_with_kminmers(pmx, oracle, rsv):
    a = pmx.Index.build(rsv, hpc=True, k=19, s=8, l=3, flank_mask=0).arrays()
    off = a["offsets"].astype(np.int64)
    for nd in _spread(len(off) - 1, 10):
        assert _reconstruct(a, off, nd) == _want(oracle, rsv.genome(nd), 19, 8, 3), nd


def test_hpc_index_flank_mask_uses_uncompressed_coordinates(pmx, oracle, rsv):
    """the first genome of the tree: a syncmer of the compressed genome is masked iff the UNCOMPRESSED position i of its first base has i < flank - 1 or
    i > n - flank, n the uncompressed length (today's rule of the plain producer with i := mapping[i])"""
    flank = 250
    a = pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=flank, max_nodes=2).arrays()
    assert len(rsv.genome(0)) == 0 and a["offsets"][1] == 0   # (the root of this tree has no bases: its only child stands for it)
    g = rsv.genome(1)
    c, mapping = hpc(g)
    mapping = np.asarray(mapping, np.int64)
    syn = [(h, p) for h, _, is_syn, p in oracle.rolling_syncmers(c, 15, 8, False, 0, True) if is_syn]
    pos = mapping[np.array([p for _, p in syn], np.int64)]
    keep = ~((pos < flank - 1) | (pos > len(g) - flank))
    assert 0 < np.count_nonzero(~keep) < len(syn)
    # (the same rule at the compressed coordinates would keep another set)
    cpos = np.array([p for _, p in syn], np.int64)
    assert not np.array_equal(keep, ~((cpos < flank - 1) | (cpos > len(c) - flank)))
    want = {}
    for (h, _), kp in zip(syn, keep.tolist()):
        if kp:
            want[h] = want.get(h, 0) + 1
    assert _reconstruct(a, a["offsets"].astype(np.int64), 1) == want


def test_hpc_flag_survives_save_and_load(pmx, rsv, tmp_path):
    index = pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=0, max_nodes=200)
    for name, unc in (("z.idx", False), ("raw.idx", True)):
        path = str(tmp_path / name)
        index.save(path, uncompressed=unc)
        hdr = pmx.Index.read_header(path)
        assert hdr["hpc"] is True and (hdr["k"], hdr["s"], hdr["l"]) == (15, 8, 1)
        back = pmx.Index.load(path)
        assert back.hpc
        a, b = index.arrays(), back.arrays()
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    plain = pmx.Index.build(rsv, k=15, s=8, l=1, flank_mask=0, max_nodes=5)
    plain.save(str(tmp_path / "p.idx"))
    assert pmx.Index.read_header(str(tmp_path / "p.idx"))["hpc"] is False
    ix = pmx.Index.from_arrays(15, 8, 0, 1, False, [0], [0, 1], [7], [0], [1], hpc=True)
    assert ix.hpc and not pmx.Index.from_arrays(15, 8, 0, 1, False, [0], [0, 1], [7], [0], [1]).hpc


def test_hpc_bit_is_refused_where_it_has_no_meaning(pmx, rsv):
    with pytest.raises(pmx.PmxError) as e:
        pmx.Index.build(rsv, hpc=True, k=15, s=8, l=1, flank_mask=0, mode=2)
    assert e.value.code == -7 and "incremental" in str(e.value)
    with pytest.raises(pmx.PmxError) as e:
        pmx.Index.build(rsv, hpc=True, k=19, s=8, l=3, flank_mask=0, mode=0x100)
    assert e.value.code == -7 and "oriented" in str(e.value)
