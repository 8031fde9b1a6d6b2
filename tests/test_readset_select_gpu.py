"""ReadSet.select (pmx_readset_select, panmap_amd/csrc/readset_select.hip): a read set gathered on the device from a subset of
another equals, byte for byte, the set uploaded from the same reads -- bases, offsets, qualities -- for every index list of
tests/align_assigned_checks.py, into fresh and reused targets, from packed, unpacked, wrapped and compressed sources; and once
packed it seeds and aligns like the uploaded set."""
import ctypes as C
import os

import numpy as np
import pytest

import align_assigned_checks as aa
import assign_checks as ac
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def _uploaded(pmx, ctx, reads, quals=None):
    rs = pmx.ReadSet(ctx, reads, pack=False)
    if quals is not None:
        rs.set_qualities(quals)
    return rs


def _assert_same(got, want, label=""):
    assert np.array_equal(got[1], want[1]), (label, "offsets")
    assert got[0] == want[0], (label, "bases")
    assert got[2] == want[2], (label, "qualities")


@pytest.fixture(scope="module")
def sources(pmx, ctx):
    reads, quals = aa.select_family()
    plain = pmx.ReadSet(ctx, reads)
    with_q = pmx.ReadSet(ctx, reads)
    with_q.set_qualities(quals)
    return plain, with_q


@pytest.mark.parametrize("with_quals", [False, True])
@pytest.mark.parametrize("name", sorted(aa.select_index_lists()))
def test_select_equals_the_uploaded_subset(pmx, ctx, sources, name, with_quals):
    reads, quals = aa.select_family()
    idx = aa.select_index_lists()[name]
    src = sources[1 if with_quals else 0]
    got = src.select(idx, pack=False)
    assert got.n_reads == len(idx) and got.total_bases == sum(len(reads[i]) for i in idx) and not got.is_hpc
    want = _uploaded(pmx, ctx, [reads[i] for i in idx], [quals[i] for i in idx] if with_quals else None)
    _assert_same(got.export(), want.export(), name)
    assert (got.export()[2] is not None) == with_quals
    # the source is untouched
    _assert_same(src.export(), _uploaded(pmx, ctx, reads, quals if with_quals else None).export(), "source")
    if got.total_bases:
        assert ctx.kernel_ms("select") > 0


def test_reuse_of_the_target(pmx, ctx, sources):
    reads, quals = aa.select_family()
    lists = aa.select_index_lists()
    src = sources[1]

    def want(idx):
        return _uploaded(pmx, ctx, [reads[i] for i in idx], [quals[i] for i in idx]).export()
    out = src.select(lists["random_1000"])
    _assert_same(out.export(), want(lists["random_1000"]), "first")
    for name in ("repeated", "all", "empty", "last_alone", "random_1000", "zero_length_alone", "reversed"):   # smaller, larger, ...
        again = src.select(lists[name], out=out, pack=(name != "all"))
        assert again is out and out.n_reads == len(lists[name])
        _assert_same(out.export(), want(lists[name]), name)
    # a target made from a source without qualities has none afterwards, whatever it held before
    src_plain = sources[0]
    src_plain.select(lists["repeated"], out=out)
    assert out.export()[2] is None
    with pytest.raises(pmx.PmxError) as e:
        src.select([0], out=src)
    assert e.value.code == ERR_ARG


def test_unpacked_wrapped_and_compressed_sources(pmx, ctx):
    import torch
    reads, quals = aa.select_family()
    lists = aa.select_index_lists()
    unpacked = _uploaded(pmx, ctx, reads, quals)
    _assert_same(unpacked.select(lists["reversed"], pack=False).export(),
                 _uploaded(pmx, ctx, reads[::-1], quals[::-1]).export(), "unpacked")
    # a slice [r0, r1] of a device offsets array: its reads start at off[r0] != 0 of the same buffer
    dev = torch.device("cuda", 0)
    concat, off = pmx.concat_reads(reads)
    d_c = torch.from_numpy(np.frombuffer(concat, np.uint8).copy()).to(dev)
    d_o = torch.from_numpy(off).to(dev)
    r0, r1 = 2, len(reads)
    assert off[r0] > 0 and off[r0] % 16 != 0
    sl = pmx.ReadSet.wrap_device(ctx, d_c.data_ptr(), d_o.data_ptr() + 8 * r0, r1 - r0, len(concat), 0, keepalive=(d_c, d_o))
    for name, idx in (("all", list(range(r1 - r0))), ("picks", [10, 0, 3, 3, 7, 1, 10])):
        _assert_same(sl.select(idx).export(), _uploaded(pmx, ctx, [reads[r0 + i] for i in idx]).export(), "wrapped " + name)
    # a wrapped TARGET is given buffers of its own: the wrapped ones are not written
    unpacked.select([1, 2, 3], out=sl)
    _assert_same(sl.export(), _uploaded(pmx, ctx, reads[1:4], quals[1:4]).export(), "wrapped target")
    assert d_c.cpu().numpy().tobytes() == concat and np.array_equal(d_o.cpu().numpy(), off)
    # a compressed source: the subset of the compressed reads, still marked
    comp = unpacked.hpc_compress()
    c_concat, c_off, c_q = comp.export()
    c_reads = [c_concat[c_off[i]:c_off[i + 1]] for i in range(len(reads))]
    c_quals = [c_q[c_off[i]:c_off[i + 1]] for i in range(len(reads))]
    sel = comp.select(lists["repeated"])
    assert sel.is_hpc
    _assert_same(sel.export(), _uploaded(pmx, ctx, [c_reads[i] for i in lists["repeated"]], [c_quals[i] for i in lists["repeated"]]).export(), "hpc")


def test_bad_arguments_launch_nothing_and_leave_the_next_call_working(pmx, ctx, sources):
    from panmap_amd import _lib
    reads, _ = aa.select_family()
    src = sources[0]
    for idx in ([len(reads)], [0, -1], [2, 1 << 40]):
        with pytest.raises(pmx.PmxError) as e:
            src.select(idx)
        assert e.value.code == ERR_ARG and b"pmx_readset_select" in pmx.last_error()
    one = np.array([1], np.int64)
    h = C.c_void_p()
    assert _lib.lib.pmx_readset_select(ctx._h, src._h, one.ctypes.data, -1, C.byref(h)) == ERR_ARG and not h
    assert _lib.lib.pmx_readset_select(ctx._h, None, one.ctypes.data, 1, C.byref(h)) == ERR_ARG and not h
    assert _lib.lib.pmx_readset_select(ctx._h, src._h, None, 1, C.byref(h)) == ERR_ARG and not h
    assert _lib.lib.pmx_readset_select(ctx._h, src._h, one.ctypes.data, 1, None) == ERR_ARG
    # a failed call with a target leaves the target as it was
    out = src.select([5, 6])
    before = out.export()
    with pytest.raises(pmx.PmxError):
        src.select([99], out=out)
    _assert_same(out.export(), before, "target after a refused call")
    _assert_same(src.select([12, 0, 5]).export(), _uploaded(pmx, ctx, [reads[12], reads[0], reads[5]]).export(), "after the refusals")


def test_a_packed_selection_seeds_and_aligns_like_the_uploaded_set(pmx, ctx):
    """the packed words, ambiguity bits and 64-byte records of a selected set: the placer's histogram and the aligner's records"""
    reads = ac.rsv_reads()
    quals = [bytes(33 + (3 * i + j) % 40 for j in range(len(r))) for i, r in enumerate(reads)]
    idx = np.random.default_rng(11).permutation(len(reads))[:200].tolist()
    src = _uploaded(pmx, ctx, reads, quals)
    sel = src.select(idx)
    up = pmx.ReadSet(ctx, [reads[i] for i in idx])
    index = pmx.Index.build(pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    hist = []
    for rs in (sel, up):
        placer = pmx.Placer(ctx, index)
        placer.reset()
        placer.add_reads(rs)
        hist.append(placer.histogram())
        placer.close()
    assert len(hist[0][0]) > 1000 and np.array_equal(hist[0][0], hist[1][0]) and np.array_equal(hist[0][1], hist[1][1])
    genome = ac._fasta(os.path.join(GOLDEN, "MZ515733.1.fa")).encode()
    al = pmx.Aligner(ctx, genome, 150)
    got = []
    for rs in (sel, up):
        al.align_readset(rs, paired=False)
        recs, cig = al.fetch()
        got.append(pmx.records_to_results(recs, cig, False))       # (with the flags; without the arena offsets)
    assert len(got[0]) == 200 and sum(x["mapped"] for x in got[0]) > 50
    assert got[0] == got[1]
