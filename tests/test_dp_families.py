"""The request families of tests/test_dp_wave_gpu.py against the reference DP alone (no GPU): they must reach what the device kernels
get wrong most easily -- bands that cut the matrix, Z-drops that fire, every call shape -- and keep the reference's CIGARs within
what a served request can hold, or the GPU comparison would pass on requests nobody serves."""
import pytest

import dp_checks as dc

NAMES = ("boundary_table", "random_requests", "long_boundary_table", "long_random_requests")


@pytest.mark.parametrize("preset", sorted(dc.PRESETS))
@pytest.mark.parametrize("name", NAMES)
def test_family_conditions(oracle, name, preset):
    fam, want = dc.family(name, preset), dc.reference(name, preset)
    n = len(fam)
    long_cigar = sum(r["n_cigar"] > dc.REQ_MAX_CIGAR for r in want) / n
    cuts = sum(dc.band_cuts(len(fam.q[i]), len(fam.t[i]), fam.w[i]) for i in range(n)) / n
    zdropped = sum(r["zdropped"] for r in want) / n
    kinds = [sum(f == k for f in fam.f) / n for k in dc.KINDS]
    print(name, preset, "n=%d n_cigar>20: %.3f band cuts: %.3f zdropped: %.3f kinds: %s largest CIGAR: %d" %
          (n, long_cigar, cuts, zdropped, ["%.2f" % k for k in kinds], max(r["n_cigar"] for r in want)))
    if name in ("random_requests", "long_random_requests"):
        assert long_cigar <= 0.20
    if name == "boundary_table":                     # (related sequences: only a band narrower than the indel makes the path zigzag)
        assert long_cigar <= 0.01
    assert cuts >= 0.30
    assert zdropped >= 0.10
    assert min(kinds) >= 0.20


@pytest.mark.parametrize("preset", sorted(dc.PRESETS))
def test_request_families_fit_a_request(preset):
    for name in ("boundary_table", "random_requests"):
        fam = dc.family(name, preset)
        assert all(dc.fits_request(len(q), len(t)) for q, t in zip(fam.q, fam.t))
    sides = [(len(q), len(t)) for q, t in zip(dc.family("random_requests", preset).q, dc.family("random_requests", preset).t)]
    assert sum(q <= 192 and t <= 192 for q, t in sides) >= 3000 and sum(t > 192 for q, t in sides) >= 500


def test_ref_ksw_ll_hand_cases(oracle):
    """ksw_ll_i16 through the ctypes glue: local alignment score and the reference's end coordinates on cases worked by hand"""
    mat = oracle.simple_mat(2, 4, 1)
    assert oracle.ref_ksw_ll([0], [1], mat, 4, 2)[0] == 0
    assert oracle.ref_ksw_ll([0, 1, 2, 3], [3, 0, 1, 2, 3, 3], mat, 4, 2)[0] == 8
    q = [0, 1, 2, 3, 0, 1, 2, 3]                                   # a whole stripe of eight, the match ends on the last target base
    assert oracle.ref_ksw_ll(q, [3, 3] + q, mat, 4, 2) == (16, 7, 9)
    assert oracle.ref_ksw_ll([0, 1, 2, 3, 0, 1, 2, 3], [0, 1, 2, 3, 1, 0, 1, 2, 3], mat, 4, 2)[0] == 8 + 8 - 6   # one base of the target in a gap
