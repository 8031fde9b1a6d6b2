"""Every device form of the anchor sort and of chaining against the compiled reference, list by list, through pmx_align_chain_probe:
radix_sort_128x / radix_sort_64 (wave_rank_sort, the s0 skip, the pending stack), chain_dp (chain_fill_wave for n <= 64,
chain_fill_wide_wave beyond, the scalar packed fill in its mask and wide-window forms; the bit-mask, ballot and scalar backtracks)
and chain_rmq (the restated AVL trees) -- on the layouts of the long-read launch and of the general wave tier (WAVE_LONG,
WAVE_GENERAL: one list per wave) and on the interleaved arena of the thread-per-pair kernel (LANE: 64 different lists per wave
through the scalar forms).  The families and what each is for: tests/chain_checks.py; that each reaches its edge under the
reference's rules: tests/test_chain_families.py.  The reference is called live (radix_sort_128x, radix_sort_64, mg_lchain_dp,
mg_lchain_rmq of the compiled reference), with the short-read preset and map-ont.  Comparison is exact: n_u, every u[i], every
anchor's x and y in order.  Every list within the reported capacities is served; the lists of the named edges carry exactly
their status bit (chain_checks.compare).

Measured on an MI355X, seconds per case (sr / map-ont): test_chain_probe sort 0.05 / 0.05 on the wave paths and 0.01 / 0.01 on
LANE; chain_dp 0.09 / 0.10 (WAVE_LONG), 0.09 / 0.10 (WAVE_GENERAL), 0.08 / 0.07 (LANE); chain_rmq 0.13 / 0.45 (both wave paths),
0.06 / 0.11 (LANE); test_caps_without_lists under 0.01.  The families and the reference's answers are made once per preset and
shared by its cases: 2.3 s for the second preset in the module's set-up (the first also waits for the build check).
"""
import time

import numpy as np
import pytest

import chain_checks as cc

pytestmark = pytest.mark.gpu

PATHS = ("WAVE_LONG", "WAVE_GENERAL", "LANE")
GROUPS = {"sort": ("SORT128", "SORT64"), "chain_dp": ("CHAIN_DP",), "chain_rmq": ("CHAIN_RMQ",)}


@pytest.fixture(scope="module", params=sorted(cc.PRESETS))
def preset(request, pmx, ctx, oracle):
    rng = np.random.default_rng(1)
    ref = bytes(rng.choice(list(b"ACGT"), 3000).astype(np.uint8))
    aligner = pmx.Aligner(ctx, ref, cc.PRESETS[request.param])
    return request.param, aligner, cc.families(request.param)


def _probe(aligner, path, fam):
    a, off, ql = fam.flat()
    P = cc.params_record(fam.params)
    res, oa, ou, caps = aligner.chain_probe(path, fam.op, a, off, ql, P, fam.max_read_len, fam.n_segs)
    return (res, oa, ou, off), caps, P[0]


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("path", PATHS)
def test_chain_probe(preset, path, group):
    name, aligner, ent = preset
    t0 = time.time()
    served = lists = 0
    for key, (fam, P, ref, _) in ent.items():
        if fam.op not in GROUPS[group]:
            continue
        got, caps, Pg = _probe(aligner, path, fam)
        assert Pg.tobytes() == P.tobytes(), (key, Pg, P)       # the preset's defaults are the ones the reference was called with
        lane = path == "LANE"
        assert int(caps["max_anchor"]) == (96 if lane else 16160 if fam.n_segs == 1 else 32288) and int(caps["max_reg"]) == (5 if lane else 32), (key, caps)
        msg = cc.compare(fam, got, caps, ref, wave=not lane)
        assert msg is None, "%s %s: %s" % (name, path, msg)
        served += int(np.sum(got[0]["served"]))
        lists += len(fam.lists)
    print("chain probe %s %s %s: %d lists, %d served, %.2f s" % (name, path, group, lists, served, time.time() - t0))
    assert served >= (0.25 if lane else 0.95) * lists


def test_caps_without_lists(preset):
    """the capacities and the parameters in force come back for n = 0, as the DP probe reports its capacities"""
    name, aligner, ent = preset
    for path in PATHS:
        fam = cc.Family("none", "CHAIN_DP", [])
        got, caps, P = _probe(aligner, path, fam)
        assert int(caps["max_anchor"]) == (96 if path == "LANE" else 16160) and int(caps["max_qlen"]) == 2016
        assert P.tobytes() == cc.preset_params(cc.PRESETS[name], fam.params).tobytes()
