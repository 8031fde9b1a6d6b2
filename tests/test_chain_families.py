"""The sort / chaining families of tests/chain_checks.py on the CPU: for every family

  * the plain-Python restatement of mg_lchain_dp equals the compiled reference on every list, so its event counts can be trusted;
  * the family reaches the edge it is named for -- a predicate over those event counts and the reference's outputs, never over a
    device's answer: a family that misses its edge fails here, not silently on the GPU;
  * hs_chain_probe of both CPU builds of the align sources (PMX_W = 1: the scalar mask and wide-window fills, the scalar backtrack,
    the insertion sort, the RMQ trees) equals the reference.

Findings the predicates record:
  * strand change: the issue of this test expected max_ii to lie before st at the first reverse-strand anchor.  The reference compares
    a[i].x - a[max_ii].x as UNSIGNED (lchain.c:190), so across a strand change the difference is huge and max_ii is looked up again in the
    (empty) window: it is -1 there, never before st.  Where max_ii does lie before st is behind the max_chain_iter clamp, which moves
    st past anchors that are still within max_dist_x: the iter-clamp families assert that.
  * the sort's 64-entry pending stack: 70 first-level buckets of 65 elements overflow it; the device forms flag the list
    (PMX_ST_OVERFLOW) instead of sorting it (see test_stack_edge_is_flagged)."""
import numpy as np
import pytest

import chain_checks as cc

PRESETS = sorted(cc.PRESETS)


def setup(preset):
    return cc.families(preset, restate=True)


@pytest.mark.parametrize("preset", PRESETS)
def test_restatement_equals_reference(preset):
    n = 0
    for key, (fam, P, ref, py) in setup(preset).items():
        if py is None:
            continue
        for i, (r, g) in enumerate(zip(ref, py)):
            assert np.array_equal(r[2], g["u"]) and np.array_equal(r[0], g["x"]) and np.array_equal(r[1], g["y"]), (key, i, len(fam.lists[i][0]))
            n += 1
    assert n > 1500


def _ev(ent, name):
    fam, P, ref, py = ent[name + ":CHAIN_DP"]
    return fam, ref, [g["ev"] for g in py]


@pytest.mark.parametrize("preset", PRESETS)
def test_dp_families_reach_their_edges(preset):
    ent = setup(preset)
    for n_seg in (1, 2):
        fam, ref, ev = _ev(ent, "colinear_seg%d" % n_seg)
        # (one anchor scores its span, below every preset's min_chain_score; from two anchors on there is one chain of all of them)
        P = ent[fam.name + ":CHAIN_DP"][1]
        want = [int(len(x) >= int(P["min_cnt"]) and 15 * len(x) >= int(P["min_chain_score"])) for x, _ in fam.lists]
        assert [len(r[2]) for r in ref] == want and sum(want) >= len(want) - 2, fam.name
        assert [int(r[2][0]) & 0xffffffff for r, w in zip(ref, want) if w] == [len(x) for (x, _), w in zip(fam.lists, want) if w]
    for n in (3, 64, 65, 129):
        fam, ref, ev = _ev(ent, "colinear_min_cnt%d" % n)
        assert [len(r[2]) for r in ref] == [0, 1, 1], fam.name
    for W in (63, 64, 65, 128, 129):
        for suffix in ("", "_skip"):
            fam, ref, ev = _ev(ent, "window%d%s" % (W, suffix))
            for e in ev[:2]:
                assert e["max_window"] == W and e["windows"] == set(range(W + 1)), fam.name
            assert all(e["max_window"] <= W + 60 for e in ev)
            assert (ev[0]["breaks"] > 0) == (suffix == "_skip"), fam.name
    for it in (64, 65, 70):
        for suffix in ("", "_skip"):
            fam, ref, ev = _ev(ent, "iter_clamp%d%s" % (it, suffix))
            for e in ev:
                assert e["clamps"] > 0 and e["max_window"] == it, fam.name
            assert ev[3]["mii_before_st"] > 0 and ev[3]["rescues"] > 0, fam.name      # max_ii before st: only behind the clamp (module docstring)
    for skip in ("1", "2", "_preset"):
        fam, ref, ev = _ev(ent, "skip_break" + skip)
        assert sum(e["breaks_inside"] for e in ev) > 0 and sum(1 for e in ev if e["rescues"] > 0) > 0, fam.name
        assert all(e["rescues"] > 0 for e in ev[:4]) or skip == "_preset", fam.name     # the crafted lists (run of 5: only the small limits)
        assert ev[2]["rescues"] > 0 and ev[3]["rescues"] > 0, fam.name                 # run of 28: every limit
    fam, ref, ev = _ev(ent, "far_marks")
    for (x, _), e, r in zip(fam.lists, ev, ref):
        assert e["max_mark_dist"] == len(x) - 22 and max(len(x) for x, _ in fam.lists) - 22 >= 64, (fam.name, len(x), e["max_mark_dist"])
        assert e["breaks_inside"] > 0 and e["rescues"] == 0, fam.name
    # ... and the mark decides the answer: the last anchor chains to j1 (two anchors: the mark on j0 ended the scan before P)
    P = cc.preset_params(cc.PRESETS[preset], fam.params)
    for x, y in fam.lists:
        g = cc.py_lchain_dp(x, y, P)
        assert g["p"][-1] == len(x) - 2 and g["p"][len(x) - 2] == 20, fam.name
    fam, ref, ev = _ev(ent, "strand_change")
    for e in ev:
        assert e["strand_resets"] == 1 and e["mii_before_st"] == 0, fam.name
    assert {len(x) <= 64 for x, _ in fam.lists} == {True, False}
    for n_seg in (1, 2):
        for span in (15, 255):
            fam, ref, ev = _ev(ent, "score_edges_seg%d_span%d" % (n_seg, span))
            # T either joins the lead's chain, or starts its own with the follower, or nothing of it is kept
            outcomes = {tuple(int(v) for v in r[2]) for r in ref[:len(ref) // 2]}
            assert len(outcomes) >= 4, (fam.name, len(outcomes))
            assert {len(x) <= 64 for x, _ in fam.lists} == {True, False}
        fam, ref, ev = _ev(ent, "qlen_sum_seg%d" % n_seg)
        assert all(int(y[-1]) & 0xffffffff == 65535 for _, y in fam.lists) and all(len(r[2]) == 1 for r in ref)
    fam, ref, ev = _ev(ent, "bt_shared_trunk")
    assert all(e["hit_used"] >= 1 for e in ev) and all(len(r[2]) >= 2 for r in ref), fam.name
    fam, ref, ev = _ev(ent, "bt_max_drop")
    assert all(e["drop_cuts"] > 0 for e in ev[:6]) and all(e["drop_exact"] > 0 and e["drop_cuts"] == 0 for e in ev[6:]) and len(ev) == 10, fam.name
    assert [len(x) for x, _ in fam.lists[6:]] == [14, 84, 74, 134] and all(int(r[2][-1]) & 0xffffffff == len(x) - p for (x, _), r, p in zip(fam.lists[6:], ref[6:], (0, 70, 0, 0)))
    fam, ref, ev = _ev(ent, "bt_none")
    assert all(e["n_z"] == 0 for e in ev) and all(len(r[0]) == 0 for r in ref)
    fam, ref, ev = _ev(ent, "bt_used_run")
    assert [e["max_used_run"] for e in ev] == [20, 62, 63, 64, 65, 128, 129, 130] and all(len(r[2]) == 2 for r in ref), fam.name
    fam, ref, ev = _ev(ent, "bt_many_chains")
    assert [len(r[2]) for r in ref] == [19, 20, 21, 30, 127, 128, 129, 140]
    for name, key in (("bt_hit_used", "hit_used"), ("bt_rejected_marks", "rejected_marking"), ("bt_drop_cut", "drop_cuts"), ("bt_end_ties", "end_ties")):
        fam, ref, ev = _ev(ent, name)
        assert len(ev) >= 8 and all(e[key] > 0 for e in ev), (name, len(ev))
        assert {len(x) <= 64 for x, _ in fam.lists} == {True, False}, name
    for n_seg in (1, 2):
        fam, ref, ev = _ev(ent, "random_seg%d" % n_seg)
        assert len(fam.lists) == 300 and max(len(x) for x, _ in fam.lists) > 550 and min(len(x) for x, _ in fam.lists) < 10
        for key in ("breaks_inside", "hit_used", "end_ties", "strand_resets"):
            assert sum(e[key] for e in ev) > 0, (fam.name, key)
        assert max(e["max_window"] for e in ev) > 64


@pytest.mark.parametrize("preset", PRESETS)
def test_rmq_families_reach_their_edges(preset):
    ent = setup(preset)
    mean = cc.PRESETS[preset]

    def other(fam, **par):
        q = dict(fam.params)
        q.update(par)
        return cc.reference(fam, cc.preset_params(mean, q))

    def differs(a, b):
        return any(not (np.array_equal(r[0], s[0]) and np.array_equal(r[1], s[1]) and np.array_equal(r[2], s[2])) for r, s in zip(a, b))

    P0 = cc.preset_params(mean, {})
    fam, P, ref, _ = ent["rmq_sizes:CHAIN_RMQ"]
    assert [len(x) for x, _ in fam.lists] == [1, 2, 64, 65, 300, 2000] and all(len(r[2]) >= 1 for r in ref[2:])
    fam, P, ref, _ = ent["rmq_equal_x:CHAIN_RMQ"]
    assert all(len(np.unique(x)) < len(x) for x, _ in fam.lists)
    fam, P, ref, _ = ent["rmq_priority_ties:CHAIN_RMQ"]
    for x, y in fam.lists:     # anchors of equal x + y on the mirrored sub-chains (their f is equal by construction: identical chains)
        s = (x & np.uint64(0xffffffff)) + (y & np.uint64(0xffffffff))
        assert len(np.unique(s)) <= len(s) - 10
    # every override changes the reference's answer on some list of its family: the edge it stands for is live
    for cap in (8, 64):
        fam, P, ref, _ = ent["rmq_size_cap%d:CHAIN_RMQ" % cap]
        assert differs(ref, other(fam, rmq_size_cap=int(P0["rmq_size_cap"]))), fam.name
    fam, P, ref0, _ = ent["rmq_inner0:CHAIN_RMQ"]
    fam, P, ref1, _ = ent["rmq_inner%d:CHAIN_RMQ" % cc.rmq_inner_on(P0)]
    fam, P, ref2, _ = ent["rmq_inner%d:CHAIN_RMQ" % cc.rmq_inner_off(P0)]
    assert differs(ref0, ref1) and not differs(ref0, ref2)        # off, on, and off again
    assert "rmq_inner1000:CHAIN_RMQ" in ent and "rmq_inner%d:CHAIN_RMQ" % int(P0["max_gap"]) in ent
    fam, P, ref, _ = ent["rmq_skip1:CHAIN_RMQ"]
    assert differs(ref, other(fam, max_chain_skip=int(P0["max_chain_skip"]))), fam.name        # the inner loop's skip break fires
    fam, P, ref, _ = ent["rmq_beyond_max_dist:CHAIN_RMQ"]
    assert len(ref[0][2]) >= 2
    fam, P, ref, _ = ent["rmq_strand_change:CHAIN_RMQ"]
    assert all(len(r[2]) >= 2 for r in ref)
    fam, P, ref, _ = ent["rmq_random:CHAIN_RMQ"]
    assert len(fam.lists) == 200
    fam, P, ref, _ = ent["rmq_64k:CHAIN_RMQ"]
    assert len(fam.lists[0][0]) == 65534


@pytest.mark.parametrize("tpp", [False, True], ids=["wave_layout", "lane_layout"])
@pytest.mark.parametrize("preset", PRESETS)
def test_hostsim_equals_reference(preset, tpp):
    served = 0
    for key, (fam, P, ref, _) in setup(preset).items():
        got, caps, Pg = cc.run_hostsim(fam, cc.PRESETS[preset], tpp)
        assert Pg.tobytes() == P.tobytes(), key
        assert int(caps["max_anchor"]) == (96 if tpp else 16160 if fam.n_segs == 1 else 32288) and int(caps["max_reg"]) == (5 if tpp else 32), key
        msg = cc.compare(fam, got, caps, ref, wave=False)
        assert msg is None, msg
        served += int(np.sum(got[0]["served"]))
    assert served > (700 if tpp else 2000)


@pytest.mark.parametrize("preset", PRESETS[:1])
def test_stack_edge_is_flagged(preset):
    """what the parent does with more pending ranges than the sort's stack holds: PMX_ST_OVERFLOW, not a wrong order (64 buckets fit)"""
    for op in ("SORT128", "SORT64"):
        fam, P, ref, _ = setup(preset)["stack_edge:" + op]
        got, caps, _ = cc.run_hostsim(fam, cc.PRESETS[preset], False)
        assert [int(s) for s in got[0]["status"]] == [0, cc.ST_OVERFLOW], op


def test_compare_names_the_first_difference():
    """the compare function itself: a changed anchor, a changed u[], a clean status on a wrong order are all reported"""
    fam, P, ref, _ = setup("150")["colinear_seg1:CHAIN_DP"]
    got, caps, _ = cc.run_hostsim(fam, 150, False)
    assert cc.compare(fam, got, caps, ref, wave=False) is None
    res, ga, gu, off = got
    i = 5
    ga2 = ga.copy(); ga2[off[i] + 1, 1] ^= np.uint64(1)
    assert "colinear_seg1[5]" in cc.compare(fam, (res, ga2, gu, off), caps, ref, wave=False)
    gu2 = gu.copy(); gu2[off[i]] += np.uint64(1 << 32)
    assert "u[0]" in cc.compare(fam, (res, ga, gu2, off), caps, ref, wave=False)
    res2 = res.copy(); res2["status"][i] = cc.ST_OVERFLOW
    assert "status" in cc.compare(fam, (res2, ga, gu, off), caps, ref, wave=False)
    res3 = res.copy(); res3["served"][i] = 0
    assert "not served" in cc.compare(fam, (res3, ga, gu, off), caps, ref, wave=False)
