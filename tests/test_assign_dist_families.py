"""The inputs of tests/test_meta_assign_dist_gpu.py reach what the collective --filter-and-assign has to get right (no GPU): the
conditions of assign_dist_checks.conditions, shown with the restatements of assign_checks and breadth_checks alone, for every
two-rank cut that test uses, and the row split of its three-rank case.  A cut that misses a condition is replaced, not excused."""
import os

import numpy as np
import pytest

import assign_checks as ac
import assign_dist_checks as adc
import breadth_checks as bc
import dist_meta_worker as dmw
from conftest import GOLDEN


def _check_two_rank_cut(R, shards, label):
    c = adc.conditions(R, shards)
    print(label, c)
    assert c["shared_lists"] > 0, (label, "no merged list occurs in both shards")
    assert c["only"][0] > 0 and c["only"][1] > 0 and c["both"] > 0, (label, c["only"], c["both"])
    assert c["assigned"][0] > 0 and c["assigned"][1] > 0, (label, "the row boundary is not inside the assigned reads", c["assigned"])
    assert sum(n for _, n in c["rows"]) == c["n_merged"] and c["rows"][1][0] == c["rows"][0][1]


def test_crafted_cut_meets_the_conditions():
    tree, reads = adc.crafted()
    assert len(tree.parent) % 64 != 0 and len(tree.parent) > 64
    R = adc.crafted_restated()
    _check_two_rank_cut(R, [adc.cut("rsv", len(reads), r, 2) for r in range(2)], "crafted halves")
    # the closed form the device computes and the literal walk agree on this tree too
    heads = ac.heads_np(tree.parent, tree.oriented["offsets"])
    total, observed, depth = bc.restate_breadth(tree.oriented, R, R.lists)
    obs2, dep2 = bc.closed_form(R)
    assert np.array_equal(observed, obs2[heads]) and np.array_equal(depth, dep2[heads]) and observed.sum() > 0


def test_the_cuts_restate_the_workers():
    for case in ("rsv", "shards", "empty"):
        for world in (2, 3):
            for rank in range(min(world, 2) if case != "rsv" else world):
                assert adc.cut(case, 1000, rank, world) == dmw.cut(case, 1000, rank, world)


def test_three_ranks_give_one_rank_no_rows():
    tree, _ = adc.crafted()
    two = adc.two_reads()
    R = ac.restate(tree.oriented, two, bc.DISCARD)
    assert len(R.lists) == 2 and (R.state == ac.ASSIGNED).all()
    assert [adc.rows(2, r, 3)[1] for r in range(3)] == [0, 1, 1]
    assert [adc.cut("rsv", 2, r, 3) for r in range(3)] == [(0, 0), (0, 1), (1, 2)]


_rsv = {}


def _rsv_restated(pmx):
    """the mixture restated once: both cuts are cuts of the same reads"""
    if not _rsv:
        _, reads, _, discard = dmw.sample(pmx, "rsv")
        arrays = pmx.Index.build(pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")), flank_mask=0, mode=0x100).arrays()
        _rsv["R"], _rsv["reads"] = ac.restate(arrays, reads, discard), reads
    return _rsv["R"], _rsv["reads"]


@pytest.mark.parametrize("case", ["rsv", "shards"])
def test_rsv_cuts_meet_the_conditions(pmx, case):
    R, reads = _rsv_restated(pmx)
    _check_two_rank_cut(R, [adc.cut(case, len(reads), r, 2) for r in range(2)], case)
