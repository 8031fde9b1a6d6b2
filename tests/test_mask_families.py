"""The read family of the --mask-reads / --mask-seeds tests (tests/mask_checks.py) meets the conditions the device tests rely
on, judged by the restatement and oracle_meta.seedmers alone; and the restatement itself on a hand-worked example."""
import numpy as np

import mask_checks as mc
from oracle import oracle_meta as om


def _lists(off, h, rev):
    return [[(int(h[q]), int(rev[q])) for q in range(off[r], off[r + 1])] for r in range(len(off) - 1)]


def test_hand_worked_example():
    """four merged reads over the hashes 10, 20, 30, 40, 50:
         r0 = [10+, 20+, 10-]  x 1      (10 twice: counted once)
         r1 = [20+, 30-]       x 2
         r2 = [40+]            x 1
         r3 = [30+, 50+, 20-]  x 3
       counts: 10 -> 1 (r0), 20 -> 1 + 2 + 3 = 6, 30 -> 2 + 3 = 5, 40 -> 1 (r2), 50 -> 3 (r3)"""
    off = np.array([0, 3, 5, 6, 9], np.int64)
    h = np.array([10, 20, 10, 20, 30, 40, 30, 50, 20], np.uint64)
    rev = np.array([0, 0, 1, 0, 1, 0, 0, 0, 1], np.uint8)
    mult = np.array([1, 2, 1, 3], np.int64)
    # off: the lists come back as they are
    o, hh, vv, mm, to, nr, ns, counts = mc.restate_masks(off, h, rev, mult, 0, 0)
    assert counts == {10: 1, 20: 6, 30: 5, 40: 1, 50: 3}
    assert np.array_equal(o, off) and np.array_equal(hh, h) and np.array_equal(vv, rev) and np.array_equal(mm, mult)
    assert to.tolist() == [0, 1, 2, 3] and (nr, ns) == (0, 0)
    # mask_reads 1: r0 (10) and r2 (40) go as wholes
    o, hh, vv, mm, to, nr, ns, _ = mc.restate_masks(off, h, rev, mult, 1, 0)
    assert _lists(o, hh, vv) == [[(20, 0), (30, 1)], [(30, 0), (50, 0), (20, 1)]]
    assert mm.tolist() == [2, 3] and to.tolist() == [-1, 0, -1, 1] and (nr, ns) == (2, 0)
    # mask_reads 3: r3 goes too (50 has count 3 <= 3)
    o, hh, vv, mm, to, nr, ns, _ = mc.restate_masks(off, h, rev, mult, 3, 0)
    assert _lists(o, hh, vv) == [[(20, 0), (30, 1)]] and mm.tolist() == [2] and to.tolist() == [-1, 0, -1, -1] and (nr, ns) == (3, 0)
    # mask_seeds 1: both 10s leave r0 (two entries), r2 is left empty and goes; three entries removed
    o, hh, vv, mm, to, nr, ns, _ = mc.restate_masks(off, h, rev, mult, 0, 1)
    assert _lists(o, hh, vv) == [[(20, 0)], [(20, 0), (30, 1)], [(30, 0), (50, 0), (20, 1)]]
    assert mm.tolist() == [1, 2, 3] and to.tolist() == [0, 1, -1, 2] and (nr, ns) == (0, 3)
    # mask_seeds 5: only 20 stays; r0, r1 and r3 are [20] / [20] / [20-] and r0, r1 stay two reads; 10, 10, 30, 40, 30, 50 removed
    o, hh, vv, mm, to, nr, ns, _ = mc.restate_masks(off, h, rev, mult, 0, 5)
    assert _lists(o, hh, vv) == [[(20, 0)], [(20, 0)], [(20, 1)]] and mm.tolist() == [1, 2, 3] and to.tolist() == [0, 1, -1, 2] and (nr, ns) == (0, 6)
    # mask_seeds 6: nothing is left
    o, hh, vv, mm, to, nr, ns, _ = mc.restate_masks(off, h, rev, mult, 0, 6)
    assert o.tolist() == [0] and len(hh) == 0 and len(mm) == 0 and to.tolist() == [-1] * 4 and (nr, ns) == (0, 9)


def test_family_conditions():
    F = mc.family()
    off, h, rev, mult, raw_to_merged = mc.family_merged()
    n = len(mult)
    lists = _lists(off, h, rev)
    counts = mc.restate_masks(off, h, rev, mult, 0, 0)[7]
    sm = lambda r: om.seedmers(r, mc.K, mc.S, mc.L)
    # the members are what their names say
    assert len(sm(F.single)) == 1
    assert len(sm(F.long)) > 1024 and len(F.long) == 20000
    assert 64 < len(sm(F.window)) <= 1024
    assert mult.max() == 3 and (mult == 3).sum() >= len(F.triplicated) and (raw_to_merged >= 0).all()
    for r in F.tiles[20:28]:                                       # a reverse-complement copy: the same hashes, the other orientation, not the same list
        f, b = sm(r), sm(mc.revcomp(r))
        assert b == [(x, not v) for x, v in reversed(f)] and tuple(b) != tuple(f)
    tandem = sm(F.tandem)
    repeated = [x for x in {x for x, _ in tandem} if sum(1 for y, _ in tandem if y == x) >= 3]
    assert repeated
    carriers = lambda x: sum(int(mult[r]) for r in range(n) if any(y == x for y, _ in lists[r]))
    for x in repeated:                                             # counted once per carrier, with its multiplicity
        assert counts[x] == carriers(x) and counts[x] < sum(1 for y, _ in tandem if y == x) * 2
    assert any(counts[x] == 2 for x in repeated)                    # (only the tandem read, twice in the sample, and nothing else carries it)
    for w in F.isolated:                                           # k-min-mers that occur once
        assert sm(w) and all(counts[x] == 1 for x, _ in sm(w))
    # mask_reads 1: some reads go, some stay
    dropped = mc.restate_masks(off, h, rev, mult, 1, 0)[5]
    assert 0 < dropped < n
    # mask_seeds 1: a read loses some but not all entries, another loses all
    new_off, _, _, _, to, _, removed, _ = mc.restate_masks(off, h, rev, mult, 0, 1)
    new_len = np.diff(new_off)
    partly = [r for r in range(n) if to[r] >= 0 and new_len[to[r]] < len(lists[r])]
    assert partly and (to < 0).any() and removed > 0
    # counts of exactly 2 and of exactly 3: mask_seeds 2 removes the first and keeps the second
    twos, threes = {x for x, c in counts.items() if c == 2}, {x for x, c in counts.items() if c == 3}
    assert twos and threes
    left = set(mc.restate_masks(off, h, rev, mult, 0, 2)[1].tolist())
    assert not (twos & left) and threes <= left
    # every threshold of the device tests changes something, and none empties the sample
    for reads, seeds in mc.MASKS:
        o = mc.restate_masks(off, h, rev, mult, reads, seeds)
        assert 0 < len(o[3]) and (len(o[3]) < n or len(o[1]) < len(h)), (reads, seeds)
