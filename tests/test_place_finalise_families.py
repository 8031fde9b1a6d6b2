"""The cases of tests/test_place_finalise_gpu.py against the oracle and the table model alone (no GPU): the table cases reach
every branch of the reservation, the clusters really share a home slot or wrap the table's end, the mask cases cut where they say
and inside a run of equal counts, the support cases sit on the threshold, the sums depend on their order, the root lists have
their lengths -- or the GPU comparison would pass on inputs that reach nothing."""
import os
import re

import numpy as np
import pytest

import finalise_checks as fc
import place_tree_checks as tc


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_mixing_helpers_restate_the_device_hash():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "panmap_amd", "csrc", "device", "pmx_math.h")).read()
    body = re.search(r"uint64_t mix64\(uint64_t x\) \{(.*?)return x;", src, re.S).group(1)
    assert "".join(body.split()) == "x^=x>>33;x*=0x%xULL;x^=x>>33;x*=0x%xULL;x^=x>>33;" % (fc._C1, fc._C2)
    rng = np.random.default_rng(1)
    vs = [0, 1, fc.M64, 1 << 63] + [int(v) for v in rng.integers(0, 2 ** 63, 200, dtype=np.int64)]
    for v in vs:
        assert fc.mix64(fc.unmix64(v)) == v and fc.unmix64(fc.mix64(v)) == v
    assert fc.mix64_array(np.array(vs, np.uint64)).tolist() == [fc.mix64(v) for v in vs]
    for cap in (1 << 7, 1 << 16, 1 << 20):       # a case chooses a key's home slot
        assert set((fc.mix64_array(fc.keys_homed((fc.HOME,), 50, 5)) & np.uint64(cap - 1)).tolist()) == {fc.HOME & (cap - 1)}
        assert set((fc.mix64_array(fc.keys_homed(fc.LAST4, 50, 6)) & np.uint64(cap - 1)).tolist()) == set(range(cap - 4, cap))


def test_generation_rules(oracle):
    assert len(set(fc.homopolymer_hashes())) == len(fc.homopolymer_keys()) == 2    # poly-A and poly-T share a canonical hash, as C and G
    assert [n for f in "ABCD" for n in fc.names(f)] + ["empty"] == list(fc.cases())
    for name, c in fc.cases().items():
        assert c.steps or name == "empty"
        for _, keys, counts in c.merges():
            assert keys.dtype == np.uint64 and counts.dtype == np.int64 and len(keys) == len(counts) <= 140000, name
            assert counts.min() >= 1 and counts.max() <= 2 ** 40 + 1000 and fc.EMPTY_KEY not in keys, name
        keys, counts = fc.final_histogram(c.steps)
        assert len(keys) <= 140000, name
        if c.family != "A":
            w = fc.want(name)
            assert np.all(np.isfinite(w["scores"])) and np.all(np.isfinite(w["metrics"]))
            hits = np.isin(fc.tree(c.tree).hash, w["kept_hash"]).sum()
            assert hits > 0 or w["state"].n_kept == 0, name                      # the index meets the kept seeds


@pytest.mark.parametrize("name", ["default", "sizes", "clusters"] + ["root_%d" % m for m in fc.ROOT_LENGTHS])
def test_indexes_are_consistent(name):
    t = fc.tree(name)
    tc.check_consistent(t)
    assert t.n_nodes == 3 and t.parent.tolist() == [0, 0, 1]
    assert np.any(t.parent_count != t.child_count)


# ------------------------------------------------------------------------------------------------ A
def test_table_cases_reach_every_branch():
    c = fc.cases()
    model = {n: fc.table_model(c[n].steps) for n in fc.names("A")}
    for n, m in model.items():
        print(n, m)
    assert [b for b, _ in model["A_growth"]] == fc.GROWTH_WANT and [cap for _, cap in model["A_growth"]] == fc.GROWTH_CAPS
    assert model["A_after_reset"][:5] == model["A_growth"]
    assert model["A_after_reset"][5:] == [("clear_and_keep", 1 << 19), ("shrink", 1 << 16), ("clear_and_keep", 1 << 16), ("grow_after_reset", 1 << 18)]
    seen = {b for m in model.values() for b, _ in m}
    assert seen == {"first_allocation", "clear_and_keep", "shrink", "first_rehash", "rehash_into_spares", "grow_after_reset", "fits"}
    # the growth merges: 40,000 and 40,000 new keys, two of 60,000 that half-overlap, one that adds no key and still grows the table
    g = c["A_growth"].merges()
    assert [len(m[1]) for m in g] == [40000, 40000, 60000, 60000, 45000]
    have = np.zeros(0, np.uint64)
    for (_, keys, _), old in zip(g, (0, 0, 30000, 30000, 45000)):
        assert np.isin(keys, have).sum() == old
        have = np.union1d(have, keys)
    assert len(have) == 140000
    # histogram() after every merge, and a score() between two merges: finalised, then merged into again
    kinds = [st[0] for st in c["A_growth"].steps]
    assert kinds == ["merge", "histogram", "merge", "histogram", "score", "merge", "histogram", "merge", "histogram", "merge", "histogram"]
    # after a reset the smaller tables hold keys that the larger one held too, with other counts: a stale slot would show
    r = c["A_after_reset"].merges()
    assert [len(m[1]) for m in r[5:]] == [80000, 100, 30000, 120000]
    for _, keys, _ in r[5:]:
        assert 0 < np.isin(keys, have).sum()
    assert np.isin(r[5][1], have).sum() < 80000 and np.isin(r[7][1], have).sum() < 30000
    # duplicates: 20,000 distinct keys, each one to five times in one merge, counts up to 2^40
    (_, keys, counts), = c["A_duplicates"].merges()
    u, times = np.unique(keys, return_counts=True)
    assert len(u) == 20000 and set(times.tolist()) == {1, 2, 3, 4, 5} and counts.max() == 2 ** 40
    assert np.any(keys[:-1] != keys[1:]) and np.any(np.diff(keys.astype(np.float64)) < 0)      # shuffled
    assert fc.unique_sum([(keys, counts)])[1].max() > 2 ** 41


def _cluster_runs(keys, cap):
    """the runs of occupied slots through the one-slot cluster's home and through the table's last slot"""
    occ = fc.fill_table(keys, cap)
    home = fc.HOME & (cap - 1)
    a, n, wraps = fc.run_through(occ, home)
    b, m, wraps_end = fc.run_through(occ, cap - 1)
    return (a, n, wraps), (b, m, wraps_end), occ


def test_table_clusters_share_a_home_slot_and_wrap_the_end():
    c = fc.cases()["A_clusters"]
    model = fc.table_model(c.steps)
    assert [cap for _, cap in model] == [1 << 17, 1 << 17]
    have = []
    for (_, keys, _), (_, cap) in zip(c.merges(), model):
        u, times = np.unique(keys, return_counts=True)
        assert np.all(times == 3) and len(u) == 15000 + fc.N_CLUSTER_A           # half of each cluster and of the random keys, three times
        have.append(u)
        (a, n, wraps), (b, m, wraps_end), occ = _cluster_runs(np.concatenate(have), cap)
        print("capacity %d: run at the home slot %d, run over the end %d (from slot %d)" % (cap, n, m, b))
        assert 200 <= n <= 1000 and not wraps
        assert 200 <= m <= 1000 and wraps_end and occ[cap - 1] and occ[0]
    mixed = fc.mix64_array(np.concatenate(have)) & np.uint64((1 << fc.CLUSTER_BITS) - 1)
    assert (mixed == np.uint64(fc.HOME)).sum() == fc.N_CLUSTER_A and np.isin(mixed, np.array(fc.LAST4, np.uint64)).sum() == fc.N_CLUSTER_A


# ------------------------------------------------------------------------------------------------ B
MASKED = [n for n in fc.names("B") if n.startswith(("B_mask_", "B_tie_run_"))]


@pytest.mark.parametrize("name", MASKED)
def test_mask_cuts_where_the_case_says(oracle, name):
    c = fc.cases()[name]
    e, w = c.expect, fc.want(name)
    keys, counts = w["hist_hash"], w["hist_count"]
    frac = c.params["seedMaskFraction"]
    assert frac == e["fraction"] and c.params["minReadSupport"] == 1
    left, alive, n_mask = fc.mask_model(keys, counts, frac)
    assert alive == e["alive"] and min(int(frac * alive), alive) == n_mask == e["n_mask"]
    assert (round(frac * alive) != int(frac * alive)) == e["round_differs"]
    assert np.array_equal(w["kept_hash"], left) and w["state"].n_unique_in == alive - n_mask == w["state"].n_kept
    other, _, _ = fc.mask_model(keys, counts, frac, descending_ties=True)
    if "tie_run" in e or "all_ties" in e:
        # the cut is strictly inside a run of equal counts: the other order of the run keeps other seeds
        live = np.sort(counts[~np.isin(keys, fc.homopolymer_keys())])[::-1]
        assert live[n_mask - 1] == live[n_mask]
        assert not np.array_equal(other, left)
        run = int((live == live[n_mask]).sum())
        assert run == e.get("tie_run", run) and 0 < int((live[:n_mask] == live[n_mask]).sum()) < run
        if "all_ties" in e:
            assert len(np.unique(counts)) == 3
    else:
        assert np.array_equal(other, left)               # all counts distinct: exactly the n_mask largest die
        assert len(np.unique(counts[~np.isin(keys, fc.homopolymer_keys())])) == alive


def test_mask_table_is_the_stated_one():
    assert [(a, f, n) for a, f, n, _ in fc.MASK_CUTS] == [(100, 0.29, 28), (100, 0.07, 7), (300, 0.01, 3), (9, 0.1, 0), (10, 0.999, 9), (10, 1.0, 10),
                                                          (10, 1.5, 10)]
    assert sum(d for _, _, _, d in fc.MASK_CUTS) == 3     # 28.99..., 0.9 and 9.99: a round-to-nearest masks one seed more
    assert int(0.01 * 70000) == 700


@pytest.mark.parametrize("name", [n for n in fc.names("B") if n.startswith("B_homopolymer")])
def test_homopolymer_seeds_lead_the_histogram_and_stay_dead(oracle, name):
    c = fc.cases()[name]
    w, hp = fc.want(name), fc.homopolymer_keys()
    keys, counts = w["hist_hash"], w["hist_count"]
    is_hp = np.isin(keys, hp)
    assert is_hp.sum() == len(hp)
    if not is_hp.all():
        assert counts[is_hp].min() > counts[~is_hp].max()                  # a mask sort that let them in would spend the mask on them
    st = w["state"]
    assert st.n_unique_in == c.expect["alive"] - c.expect["n_mask"] and not np.isin(w["kept_hash"], hp).any()
    assert st.total_freq == np.sort(counts[~is_hp])[:len(counts) - len(hp) - c.expect["n_mask"]].sum()
    if c.params["seedMaskFraction"] >= 1.0:
        assert st.n_kept == 0 and int(c.params["seedMaskFraction"] * c.expect["alive"]) >= c.expect["alive"]


@pytest.mark.parametrize("name", [n for n in fc.names("B") if n.startswith(("B_auto_", "B_support_"))])
def test_support_cases_sit_on_the_threshold(oracle, name):
    c = fc.cases()[name]
    st, counts = fc.want(name)["state"], fc.want(name)["hist_count"]
    print(name, st.est_coverage, st.min_support, st.n_kept)
    assert st.min_support == c.expect["support"] and st.n_kept == c.expect["n_kept"]
    if name.startswith("B_auto_"):
        assert c.params.get("minReadSupport", -1) == -1
        if "estimate" in c.expect:
            assert st.est_coverage == c.expect["estimate"]
    else:
        s = c.params["minReadSupport"]
        assert {s - 1, s, s + 1} & set(counts.tolist()) == {s - 1, s, s + 1} - {0}
    if name == "B_auto_2pow40":
        assert counts.min() >= 2 ** 40 and st.total_freq == int(counts.sum()) > 2 ** 49


def test_support_table_is_the_stated_one(oracle):
    assert [(n, e, s) for n, _, e, s, _ in fc.AUTO_SUPPORT] == [("all3", 3.0, 1), ("alt24", 3.0, 1), ("nine3_one4", 3.1, 2), ("all1", 0.0, 1),
                                                               ("nine1_one4", 4.0, 2)]
    a, b = fc.want("B_auto_flip_unmasked"), fc.want("B_auto_flip_masked")
    assert np.array_equal(a["hist_count"], b["hist_count"]) and (a["state"].min_support, b["state"].min_support) == (2, 1)
    assert np.sort(a["hist_count"])[-10:].tolist() == [100] * 10 and b["state"].est_coverage == 3.0


# ------------------------------------------------------------------------------------------------ C
def test_sum_sizes_reach_every_tail():
    n = np.array(fc.SUM_SIZES)
    assert {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 63 * 1024, 64 * 1024, 64 * 1024 + 1, 65 * 1024 + 9,
            128 * 1024 + 1} <= set(n.tolist())
    last = (n - 1) % fc.SUM_BLOCK + 1                       # values in the last block
    assert set(range(8)) <= set((last % 64 % 8).tolist())   # every tail of the 8-way add ...
    assert {0, 1, 63} <= set((last % 64).tolist())          # ... and of the 64-value chunk
    blocks = (n + fc.SUM_BLOCK - 1) // fc.SUM_BLOCK
    assert {1, 2, 7, 8, 9, 63, 64, 65, 129} <= set(blocks.tolist())


@pytest.mark.parametrize("n", fc.SUM_SIZES)
def test_sums_depend_on_their_order(oracle, n):
    w = fc.want("C_sum_%d" % n)
    st = w["state"]
    assert st.n_kept == n and w["hist_count"].max() < 2 ** 40 and (n < 64 or w["hist_count"].max() > 2 ** 30)
    (mag_f, den_f), (mag_b, den_b) = fc.plain_sums(w["kept_log"])
    front = (_bits(st.log_magnitude) != _bits(mag_f), _bits(st.log_cont_den) != _bits(den_f))
    back = (_bits(st.log_magnitude) != _bits(mag_b), _bits(st.log_cont_den) != _bits(den_b))
    print(n, front, back)
    if n > fc.SUM_BLOCK + 1:
        assert all(front)
    else:
        # up to one block the canonical order IS front to back; so it is at 1,025, whose second block holds one value:
        # (a1 + ... + a1024) + (0 + a1025).  There the back-to-front sum below is what tells the orders apart.
        assert not any(front)
    if n >= 8:
        assert all(back)


# ------------------------------------------------------------------------------------------------ D
def test_probe_table_sizes():
    assert [fc.probe_table_cap(n) for n in fc.SIZE_BOUNDARY] == [128, 1024, 2048] and 2 * 480 + 64 == 1024
    for n in fc.SIZE_BOUNDARY:
        assert fc.want("D_size_%d" % n)["state"].n_kept == n
    t = fc.tree("sizes")
    root = t.hash[:int(t.offsets[1])]
    assert fc.pool()[0] in root and np.isin(root, fc.pool()[:480]).sum() == 150 and len(root) == 300


def test_probe_clusters_and_misses(oracle):
    w = fc.want("D_clusters")
    kept = w["kept_hash"]
    cap = fc.probe_table_cap(len(kept))
    assert len(kept) == 3000 and cap == 8192
    (a, n, wraps), (b, m, wraps_end), occ = _cluster_runs(kept, cap)
    print("run at the home slot %d, run over the end %d (from slot %d)" % (n, m, b))
    assert 200 <= n <= 1000 and 200 <= m <= 1000 and wraps_end and not wraps and occ[0] and occ[cap - 1]
    t = fc.tree("clusters")
    root = t.hash[:int(t.offsets[1])]
    hit = np.isin(root, kept)
    mixed = fc.mix64_array(root) & np.uint64(cap - 1)
    home = fc.HOME & (cap - 1)
    assert (hit & (mixed == np.uint64(home))).sum() == 50 and (hit & (mixed >= np.uint64(cap - 4))).sum() == 50      # hits inside both clusters
    walked = np.array([fc.probes_of_miss(occ, k) for k in root[~hit]])
    m_home = mixed[~hit]
    assert walked.max() >= 200 and (walked >= 100).sum() >= 60
    assert walked[m_home == np.uint64(home)].min() >= n - (home - a) >= 200                  # from the cluster's first slot to the empty one
    mid = walked[m_home == np.uint64(home + fc.MID)]
    assert len(mid) == 30 and mid.min() >= 100                                             # homed in the middle of the cluster
    last = walked[m_home == np.uint64(cap - 1)]
    assert len(last) == 30 and last.min() >= 100                                           # homed on the last slot: the walk wraps


@pytest.mark.parametrize("m", fc.ROOT_LENGTHS)
def test_root_lists_have_their_lengths_and_hits(oracle, m):
    t = fc.tree("root_%d" % m)
    w = fc.want("D_root_%d" % m)
    assert int(t.offsets[1]) == m and w["state"].n_kept == fc.N_ROOT_HIST
    root, cc = t.hash[:m], t.child_count[:m]
    hit = np.isin(root, w["kept_hash"])
    assert hit.sum() == (m + 1) // 2 and cc.min() >= 0
    if m >= 1023:
        assert 0.05 <= np.mean(cc == 0) <= 0.15 and (hit & (cc == 0)).any() and np.any(hit[:-1] != hit[1:])
    terms = np.where(hit & (cc > 0), 1.0 / np.maximum(cc, 1), 0.0)
    assert _bits(np.cumsum(terms)[-1]) == _bits(w["wc_den"]) and w["wc_den"] > 0
    if m >= 1023:
        assert _bits(np.cumsum(terms[::-1])[-1]) != _bits(w["wc_den"])                       # the order of the additions shows
