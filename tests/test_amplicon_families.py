"""The amplicon read family's own conditions, against the restatement alone (tests/amplicon_checks.py): every setting the device
tests use changes something against the ungrouped run, a hash is masked in one group and kept in another, a group has
threshold 0 under the relative options, the 20 kb read is the only one on the sorted counting path -- and the worked example of
the rule, number by number.  No device, no product code."""
import numpy as np
import pytest

import amplicon_checks as amp
import mask_checks as mc


def _lists(off, h, v):
    return sorted((tuple(h[off[r]:off[r + 1]].tolist()), tuple(v[off[r]:off[r + 1]].tolist())) for r in range(len(off) - 1))


def test_the_family_is_dealt_as_described():
    D = amp.family()
    assert D.group_names == ["amp_1", "amp_2", "amp_3", "amp_empty"]
    merged, n_raw, where = amp.family_merged()
    assert n_raw == [40, 48, 3, 0, 6] and len(D.reads) == 97 and len(set(D.names)) == 97
    assert sorted(D.reads) == sorted(mc.family().reads)                                  # the same sample, dealt
    assert [len(m[3]) for m in merged] == [35, 48, 2, 0, 6] and len(mc.family_merged()[3]) == 86
    assert D.groups[D.names.index("single")] == 2                                        # (the later line of the read id counted)
    # five lists sit in two groups
    in_1, in_2 = _lists(*merged[0][:3]), _lists(*merged[1][:3])
    assert len(set(in_1) & set(in_2)) == 5
    # the 20 kb read is the only one above 1,024 entries
    sizes = np.concatenate([np.diff(m[0]) for m in merged])
    assert (sizes > 1024).sum() == 1 and np.diff(merged[4][0]).max() > 1024


@pytest.mark.parametrize("setting", amp.SETTINGS)
def test_every_setting_differs_from_the_ungrouped_run(setting):
    merged, n_raw, _ = amp.family_merged()
    got = amp.restate_groups(merged, n_raw, *setting)
    off, h, v, mult, _ = mc.family_merged()
    # the ungrouped run of the same parameters (a relative one does nothing there: the single group is the unlisted one)
    u_off, u_h, u_v, u_mult = mc.restate_masks(off, h, v, mult, setting[0], setting[1])[:4]
    assert (len(got["mult"]), len(got["lists"][1])) != (len(u_mult), len(u_h))
    assert len(got["mult"]) > 0


def test_the_numbers_of_the_family():
    merged, n_raw, _ = amp.family_merged()
    assert [i[3] for i in amp.restate_groups(merged, n_raw)["info"]] == [35, 48, 2, 0, 6]
    masked = amp.restate_groups(merged, n_raw, mask_reads=1)
    assert [i[3] for i in masked["info"]] == [28, 37, 1, 0, 1]
    off, h, v, mult, _ = mc.family_merged()
    assert len(mc.restate_masks(off, h, v, mult, 1, 0)[3]) == 71
    for kind in ("reads_rf", "seeds_rf"):
        rel = amp.restate_groups(merged, n_raw, **{kind: 0.05})
        assert [i[1] for i in rel["info"]] == [2, 2, 0, 0, 0]                            # a group with threshold 0, the unlisted one unmasked
    assert [i[3] for i in amp.restate_groups(merged, n_raw, reads_rf=0.05)["info"]] == [5, 2, 2, 0, 6]


def test_a_hash_is_masked_in_one_group_and_kept_in_another():
    merged, n_raw, _ = amp.family_merged()
    got = amp.restate_groups(merged, n_raw, mask_reads=1)
    by_hash = {}
    for g, x, c in got["triples"]:
        by_hash.setdefault(x, {})[g] = c
    split = [x for x, per in by_hash.items() if min(per.values()) <= 1 < max(per.values())]
    assert split
    assert all(got["counts"][x] == sum(by_hash[x].values()) for x in by_hash)


def test_truncation():
    """0.29 x 100 as a double is below 29: the threshold is 28"""
    assert amp.thresholds([100, 1], reads_rf=0.29) == (True, [28, 0]) and 0.29 * 100.0 < 29.0
    D = amp.truncation_set()
    merged, n_raw, _ = amp.merge_by_group(D.reads, D.groups, 1)
    got = amp.restate_groups(merged, n_raw, reads_rf=0.29)
    assert n_raw == [100, 1] and [i[1] for i in got["info"]] == [28, 0]
    assert sorted(got["mult"].tolist()) == [1, 29, 43] and got["reads_dropped"] == 1


def _group(lists):
    """[(hash list, multiplicity)] -> (offsets, hashes, orientations, multiplicities)"""
    off = np.concatenate([[0], np.cumsum([len(x) for x, _ in lists])]).astype(np.int64)
    h = np.array([y for x, _ in lists for y in x], np.uint64)
    return off, h, np.zeros(len(h), np.uint8), np.array([m for _, m in lists], np.int64)


def test_the_worked_example():
    h1, h2, h3, h4, h5 = 11, 12, 13, 14, 15
    A = _group([([h1, h2], 3), ([h2, h3], 2), ([h4], 5)])
    B = _group([([h1, h2], 1), ([h2], 3)])
    U = _group([([h5], 1)])
    n_raw = [10, 4, 1]
    assert amp.thresholds(n_raw, reads_rf=0.25) == (True, [2, 1, 0])                     # 2.5 -> 2, 1.0 -> 1, the unlisted group 0
    got = amp.restate_groups([A, B, U], n_raw, reads_rf=0.25)
    assert got["triples"] == [(0, h1, 3), (0, h2, 5), (0, h3, 2), (0, h4, 5), (1, h1, 1), (1, h2, 4), (2, h5, 1)]
    assert got["counts"][h1] == 4                                                        # (h1 occurs 4 times in the sample, and r3 goes)
    assert got["reads_dropped"] == 2 and got["seeds_removed"] == 0 and len(got["mult"]) == 4
    assert got["old_to_new"][0].tolist() == [0, -1, 1] and got["old_to_new"][1].tolist() == [-1, 2] and got["old_to_new"][2].tolist() == [3]
    assert got["amplicons"].tolist() == [0, 0, 1, 2] and got["mult"].tolist() == [3, 5, 3, 1]
    assert [i for i in got["info"]] == [(10, 2, 3, 2), (4, 1, 2, 1), (1, 0, 1, 1)]
    seeds = amp.restate_groups([A, B, U], n_raw, seeds_rf=0.25)
    assert seeds["seeds_removed"] == 2 and seeds["reads_dropped"] == 0 and len(seeds["mult"]) == 6
    off, h, _ = seeds["lists"]
    assert [h[off[r]:off[r + 1]].tolist() for r in range(6)] == [[h1, h2], [h2], [h4], [h2], [h2], [h5]]
    assert seeds["mult"].tolist() == [3, 2, 5, 1, 3, 1]                                  # r3 = [h2] x1 stays apart from r4 = [h2] x3
    with pytest.raises(AssertionError, match="Only one masking parameter"):
        amp.thresholds(n_raw, mask_reads=1, seeds_rf=0.25)
