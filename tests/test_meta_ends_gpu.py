"""--mask-read-ends on the device (pmx_meta_set_mask_read_ends, panmap_amd/csrc/api_meta.hip): the seeding kernels' per-end trim
against trimming the strings.  On one Meta over rsv_4K and one over a crafted tree of assign_checks, for every n of
ends_checks.NS, the family set with set_mask_read_ends(n) and the family trimmed in Python set with 0 must give the same
seedmer lists, multiplicities, raw -> merged map, overlap coefficients, candidates, scores, haplotypes and EM numbers --
exactly: downstream of the lists the two runs are the same deterministic code.  The lists must also be oracle_meta's seedmers of
the trimmed strings, or the two runs could be wrong together.  The list mode of k_seed_histogram and the place stage's
kernels behind the overlap coefficients run with a non-zero trim here and nowhere else in the suite."""
import os

import numpy as np
import pytest

import assign_checks as ac
import ends_checks as ec
import mask_checks as mc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CRAFTED_TREE = 4                                                # binary129: more than two words of 64 nodes


@pytest.fixture(scope="module")
def params(pmx):
    from panmap_amd import _lib
    return _lib.MetaParams()


@pytest.fixture(scope="module")
def rsv(pmx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    return pmx.Meta.build(pmx.Context(0), pm)


@pytest.fixture(scope="module")
def crafted(pmx):
    plain, oriented = ac.crafted_trees()[CRAFTED_TREE].indexes(pmx)
    return pmx.Meta(pmx.Context(0), plain, oriented)


def _both(meta, reads, n, params, **kw):
    """(in the kernel, on the strings)"""
    return ec.run(meta, reads, n, params, **kw), ec.run(meta, ec.trimmed(reads, n), 0, params, **kw)


@pytest.mark.parametrize("n", ec.NS)
def test_trim_in_the_kernel_equals_trimming_the_strings_rsv(rsv, params, n):
    got, want = _both(rsv, ec.family(n).reads, n, params)
    ec.assert_same(got, want, "rsv n=%d" % n)
    ec.assert_lists(got, ec.family_expected(n), "rsv n=%d against the oracle" % n)
    assert len(got["haplotypes"]) >= 2 and got["em_info"][1] >= 2 and got["scores"].max() > 0       # scoring and the EM had something to do
    assert (got["oc"] != 0).any()


@pytest.mark.parametrize("n", ec.NS)
def test_trim_in_the_kernel_equals_trimming_the_strings_crafted_tree(crafted, params, n):
    reads = ec.crafted_sample(n)
    got, want = _both(crafted, reads, n, params)
    ec.assert_same(got, want, "crafted n=%d" % n)
    ec.assert_lists(got, ec.family_expected(n, crafted=True), "crafted n=%d against the oracle" % n)
    assert len(got["haplotypes"]) >= 1 and got["scores"].max() > 0


@pytest.mark.parametrize("n", ec.NS)
def test_dust_sees_the_trimmed_read(rsv, params, n):
    F = ec.family(n)
    T = ec.DUST_THRESHOLD
    got, want = _both(rsv, F.reads, n, params, dust=T)
    ec.assert_same(got, want, "dust n=%d" % n)
    ec.assert_lists(got, ec.family_expected(n, T), "dust n=%d against the oracle" % n)
    # the read above the threshold before trimming only is kept, the one above it after trimming only is dropped
    assert got["raw_to_merged"][F.reads.index(F.dust_down)] >= 0 and got["raw_to_merged"][F.reads.index(F.dust_up)] == -1


@pytest.mark.parametrize("n", (5, 32))
def test_dust_sees_the_trimmed_read_crafted_tree(crafted, params, n):
    got, want = _both(crafted, ec.crafted_sample(n), n, params, dust=ec.DUST_THRESHOLD)
    ec.assert_same(got, want, "crafted dust n=%d" % n)
    ec.assert_lists(got, ec.family_expected(n, ec.DUST_THRESHOLD, crafted=True), "crafted dust n=%d against the oracle" % n)


@pytest.mark.parametrize("n", ec.NS)
def test_low_coverage_mask_counts_the_trimmed_reads(rsv, params, n):
    got, want = _both(rsv, ec.family(n).reads, n, params, mask_reads=2)
    ec.assert_same(got, want, "mask n=%d" % n)
    # ... and both are the mask restated on the oracle's lists of the trimmed strings
    off, h, v, mult, raw = ec.family_expected(n)
    m_off, m_h, m_v, m_mult, old_to_new = mc.restate_masks(off, h, v, mult, 2, 0)[:5]
    assert np.array_equal(got["seedmers"][0], m_off) and np.array_equal(got["seedmers"][1], m_h) and np.array_equal(got["seedmers"][2], m_v)
    assert np.array_equal(got["info"][1], m_mult)
    assert 0 < len(m_mult) < len(mult)
    rsv.set_masks()


def test_on_off_on_on_one_meta(rsv, params):
    reads = ec.family(5).reads
    on = ec.run(rsv, reads, 5, params)
    off = ec.run(rsv, reads, 0, params)
    again = ec.run(rsv, reads, 5, params)
    ec.assert_same(again, on, "on again")
    ec.assert_lists(off, ec.merged_from_strings(reads), "off")
    ec.assert_lists(on, ec.family_expected(5), "on")
    assert not np.array_equal(on["seedmers"][1], off["seedmers"][1])
    rsv.set_mask_read_ends(0)


def test_every_read_trimmed_to_nothing(rsv, params):
    """n = 10**6: a sample without seedmers -- no merged read, every read -1, every overlap coefficient 0, every node a candidate
    of the one rank, no score, no haplotype -- exactly what the same number of reads too short for a k-mer gives"""
    reads = ec.family(5).reads
    got = ec.run(rsv, reads, 10 ** 6, params)
    want = ec.run(rsv, [b"A"] * len(reads), 0, params)
    ec.assert_same(got, want, "all empty")
    assert rsv.n_reads == 0 and len(got["seedmers"][1]) == 0 and (got["raw_to_merged"] == -1).all() and len(got["raw_to_merged"]) == len(reads)
    assert not got["oc"].any() and got["haplotypes"] == [] and got["em_info"][:2] == (0, 0) and got["scores"].size == 0
    assert len(got["candidates"]) == rsv.index.info.n_nodes
    # ... and with DUST on: an empty read scores 0 and is kept, so nothing changes
    ec.assert_same(ec.run(rsv, reads, 10 ** 6, params, dust=ec.DUST_THRESHOLD), want, "all empty, dust")
    big = ec.run(rsv, reads, 2 ** 31 - 1, params)
    ec.assert_same(big, want, "the largest n")
    rsv.set_mask_read_ends(0)


def test_assign_after_masked_ends_is_refused(pmx, crafted):
    reads = ec.crafted_sample(5)
    crafted.set_mask_read_ends(5)
    crafted.set_reads(reads)
    with pytest.raises(pmx._lib.PmxError) as e:
        crafted.assign(0.5)
    assert e.value.code == -7 and "pmx_meta_set_mask_read_ends" in str(e.value)
    # the value is of the read set: lowering it without setting the reads again changes nothing, setting them again does
    crafted.set_mask_read_ends(0)
    with pytest.raises(pmx._lib.PmxError) as e:
        crafted.assign(0.5)
    assert e.value.code == -7
    crafted.set_reads(reads)
    res = crafted.assign(0.5)
    assert (res.state == ac.ASSIGNED).any()


def test_bad_values_are_refused(pmx, crafted):
    for n in (-1, 2 ** 31, -2 ** 40):
        with pytest.raises(pmx._lib.PmxError) as e:
            crafted.set_mask_read_ends(n)
        assert e.value.code == -1, n
    crafted.set_mask_read_ends(2 ** 31 - 1)
    crafted.set_mask_read_ends(0)
