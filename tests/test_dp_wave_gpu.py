"""Every device implementation of ksw_extd2, and sw_ll, on requests of their own against ksw_extd2_sse / ksw_ll_i16 of the compiled
reference (src/3rdparty/minimap2/ksw2_extd2_sse.c, ksw2_ll_sse.c), field by field of ksw_extz_t and CIGAR by CIGAR, through
pmx_align_dp_probe: the register kernel ksw_extd2_reg<NC = 1, 2, 3> and the anti-diagonal kernel of the all-LDS unit as the DP service
launches them (SERVE, SERVE_ONE_CLASS), the rows kernel ksw_extd2_rows_t<SW = 4 .. 16>, ksw_extd2_t<true> on the dp_fast LDS copy and
ksw_extd2_t<false> on the layouts of the wave-per-read kernels (WAVE_LONG, WAVE_GENERAL), the wave branch of sw_ll (SW_LL) -- with the
sr, map-ont and map-hifi scoring, the four call shapes of mm_align1 (flag 0, the second pass of a gap fill, included), bands from none
to one that leaves no cell, and the sizes at which the dispatchers change kernels.  Integer DP: equality, no tolerance.

Measured on an MI355X, seconds per case (sr / map-ont / map-hifi): test_boundary_table 0.21 / 0.23 / 0.19, test_random_requests
0.48 / 0.54 / 0.40, test_long_boundary_table 0.68 / 1.17 / 1.11, test_long_random_requests 0.13 / 0.26 / 0.26, test_sw_ll 0.01.

The rows kernel's exact mode never runs with SW = 12 or 16 from ksw_extd2: its replay arrays, 8 * (qlen + tlen) + 8 bytes, share the
5,824-byte dp_fast area with the 2,048-byte traceback window and the query copy, so a target beyond 472 columns cannot have them
(test_long_boundary_table asserts exact mode for SW = 4 and 8, approximate mode for all four widths)."""
import numpy as np
import pytest

import dp_checks as dc

pytestmark = pytest.mark.gpu

REQ_READ_LEN = 300      # request paths: the layouts hold a query of 320 and, with the sr preset's max_gap, a target of 448 bases
LONG_READ_LEN = 1100    # wave paths


@pytest.fixture(scope="module", params=sorted(dc.PRESETS))
def preset(request, pmx, ctx):
    rng = np.random.default_rng(1)
    ref = bytes(rng.choice(list(b"ACGT"), 3000).astype(np.uint8))
    aligner = pmx.Aligner(ctx, ref, request.param)
    sc = aligner.scoring()
    assert {k: sc[k] for k in sc} == {k: dc.PRESETS[request.param][k] for k in sc}     # the families were drawn with this scoring
    return request.param, aligner


def _run(pmx, preset, name, path, max_read_len, **switches):
    mean_len, aligner = preset
    fam, want = dc.family(name, mean_len), dc.reference(name, mean_len)
    got, arena, caps = aligner.dp_probe(path, fam.q, fam.t, fam.w, fam.z, fam.eb, fam.f, max_read_len, **switches)
    served, paths = dc.compare(fam, want, got, arena, caps, small_class=path == "SERVE")
    print(name, mean_len, path, switches, "served %d of %d" % (served, len(fam)), sorted(hex(p) for p in paths))
    return served, paths, caps, len(fam)


def _request_paths(pmx, preset, name):
    P = pmx.api
    served, paths, caps, n = _run(pmx, preset, name, "SERVE", REQ_READ_LEN)
    want = {P.DP_PATH_REG | nc | tb for nc in (1, 2, 3) for tb in (0, P.DP_PATH_TB_LDS)}
    assert want <= paths, sorted(hex(p) for p in want - paths)
    assert all(p & P.DP_PATH_KIND == P.DP_PATH_REG or p & P.DP_PATH_ALL_LDS for p in paths)
    class2 = int(caps[0]["max_tlen"]) > 0      # (max_gap of map-hifi: the arrays of the one-class layout exceed the LDS of a CU; nothing of it can run)
    if class2:
        assert served >= 0.75 * n
    served1, paths1, _, _ = _run(pmx, preset, name, "SERVE_ONE_CLASS", REQ_READ_LEN)
    served2, paths2, _, _ = _run(pmx, preset, name, "SERVE_ONE_CLASS", REQ_READ_LEN, no_rows_dp=True)
    if class2:
        A = P.DP_PATH_ALL_LDS
        assert any(p & (A | P.DP_PATH_KIND) == A | P.DP_PATH_ROWS for p in paths1)
        assert {A | P.DP_PATH_DIAG, A | P.DP_PATH_DIAG | P.DP_PATH_TB_LDS} <= paths1
        assert paths2 == {A | P.DP_PATH_DIAG, A | P.DP_PATH_DIAG | P.DP_PATH_TB_LDS}
        assert served1 == served and served2 == served
    else:
        assert served1 == 0 and served2 == 0


def test_boundary_table(pmx, oracle, preset):
    _request_paths(pmx, preset, "boundary_table")


def test_random_requests(pmx, oracle, preset):
    _request_paths(pmx, preset, "random_requests")


def _wave_paths(pmx, preset, name):
    P = pmx.api
    rows = lambda sw, exact: P.DP_PATH_ROWS | sw | (P.DP_PATH_EXACT if exact else 0)
    fast, general = P.DP_PATH_DIAG | P.DP_PATH_FAST, P.DP_PATH_DIAG
    served, paths, _, n = _run(pmx, preset, name, "WAVE_LONG", LONG_READ_LEN)
    seen = {}
    for no_rows in (False, True):
        for no_fast in (False, True):
            if no_rows or no_fast:
                s, seen[no_rows, no_fast], _, _ = _run(pmx, preset, name, "WAVE_LONG", LONG_READ_LEN, no_rows_dp=no_rows, no_dp_fast=no_fast)
                assert 0 < s <= served      # (the rows kernel's row-major traceback fits the slab for some matrices the anti-diagonal one does not)
    s, pg, _, _ = _run(pmx, preset, name, "WAVE_GENERAL", LONG_READ_LEN)
    assert pg == {general} and s > 0
    assert all(p & P.DP_PATH_KIND != P.DP_PATH_ROWS for p in seen[True, False] | seen[True, True])
    assert seen[False, True] == {general} and seen[True, True] == {general}        # (the rows kernel runs on the dp_fast area)
    assert seen[True, False] == {fast, general}
    return served, paths, n, rows, fast, general


def test_long_boundary_table(pmx, oracle, preset):
    served, paths, n, rows, fast, general = _wave_paths(pmx, preset, "long_boundary_table")
    want = {rows(4, True), rows(8, True), fast, general} | {rows(sw, False) for sw in (4, 8, 12, 16)}
    assert want <= paths, sorted(hex(p) for p in want - paths)
    assert {sw for sw in (4, 8, 12, 16) if any(p & ~dc.EXACT_BIT == rows(sw, False) for p in paths)} == {4, 8, 12, 16}
    assert served >= 0.3 * n      # (the sr preset plans 422 KB of traceback: its wide matrices are over capacity)


def test_long_random_requests(pmx, oracle, preset):
    served, paths, n, rows, fast, general = _wave_paths(pmx, preset, "long_random_requests")
    assert {fast, general} <= paths and served >= 0.3 * n


def test_sw_ll(pmx, oracle, preset):
    mean_len, aligner = preset
    sc = aligner.scoring()
    mat = oracle.simple_mat(sc["a"], sc["b"], sc["sc_ambi"])
    shapes = dc.sw_ll_shapes(mean_len)
    _, _, caps = aligner.dp_probe("SW_LL", [], [], [], [], [], [], LONG_READ_LEN)
    over = (int(caps[0]["max_tlen"]) + 32) // 2      # four 16-bit columns of qlen8 + 8 entries in W.H (max_tlen + 32 words): this query is past it
    rng = np.random.default_rng(9)
    shapes.append(([int(x) for x in rng.integers(0, 4, over)], [int(x) for x in rng.integers(0, 4, 64)]))
    qs, ts = [s[0] for s in shapes], [s[1] for s in shapes]
    got, _, _ = aligner.dp_probe("SW_LL", qs, ts, -1, -1, -1, 0, LONG_READ_LEN)
    bad = []
    for i, (q, t) in enumerate(shapes[:-1]):
        want = oracle.ref_ksw_ll(q, t, mat, sc["q"], sc["e"])
        g = got[i]
        if not g["ok"] or (int(g["score"]), int(g["qe"]), int(g["te"])) != want:
            bad.append((len(q), len(t), i % 4, int(g["ok"]), (int(g["score"]), int(g["qe"]), int(g["te"])), want))
    assert not bad, (len(bad), bad[:5])
    assert int(got[-1]["ok"]) == 0 and int(got[-1]["served"]) == 0
