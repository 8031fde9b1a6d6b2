"""The input families of the taxonomy tests (tests/taxa_checks.py) have what the device tests rely on: under the LITERAL
restatement of the reference's rule every leg has reads over the taxon limit and reads that stay, the "absolute" leg has reads
whose fate hangs on the records (touched nodes) and not on the scores alone, and the closed form that the device uses for lo >=
1 (the union over all nodes with score >= lo) equals the literal rule.  Restatement and reference rules only: no product code
except the host-side index build of the rsv tree.  Counts are merged reads.

Measured (over, kept): default 77/48, 30/105, 86/37, 95/39 (star71, binary127, binary129, random300); two 9/148; ratio M=1
119/38, M=2 1/156; absolute over 13, 18, 31 and flips 27, 20, 12 (star71, binary127, random300); rsv with T=16: 550/124 at discard 0 (T=4: fewer over, T=64: 31 raw reads kept).
"""
import os

import numpy as np
import pytest

import assign_checks as ac
import taxa_checks as tc
from conftest import GOLDEN


@pytest.mark.parametrize("case", tc.LEGS["default"], ids=lambda c: c[0])
def test_default_leg(case):
    over, kept = tc.counts(tc.crafted_leg(*case)[2])
    assert over >= 30 and kept >= 30, (over, kept)


def test_two_leg():
    over, kept = tc.counts(tc.crafted_leg(*tc.LEGS["two"][0])[2])
    assert over >= 5 and kept >= 100, (over, kept)


def test_ratio_leg():
    one, two = (tc.counts(tc.crafted_leg(*case)[2]) for case in tc.LEGS["ratio"])
    assert one[0] >= 30 and one[1] >= 30 and two[0] >= 1, (one, two)


@pytest.mark.parametrize("case", tc.LEGS["absolute"], ids=lambda c: c[0])
def test_absolute_leg_hangs_on_the_records(case):
    literal, by_scores = tc.crafted_leg(*case)[2], tc.crafted_leg(*case, qualifying="all")[2]
    flips = len(set(literal.merged[literal.state != by_scores.state].tolist()))
    assert flips >= 10 and tc.counts(literal)[0] >= 10, (flips, tc.counts(literal))


@pytest.mark.parametrize("tree", list(tc.TREES))
def test_closed_form_equals_the_literal_rule_from_lo_1(tree):
    checked = 0
    for A, ratio in ((0, 0.0), (2, 0.0), (3, 0.0), (0, 0.25), (0, 0.99)):
        literal, by_scores = (tc.crafted_leg(tree, 0.0, A, ratio, 16, 1, qualifying=q)[2] for q in ("touched", "all"))
        for r in np.nonzero(literal.max > 0)[0].tolist():
            mx = int(literal.max[r])
            if mx - max(A, int(mx * ratio)) >= 1:
                assert literal.state[r] == by_scores.state[r] and literal.taxa[r] == by_scores.taxa[r], (tree, A, ratio, r)
                checked += 1
    assert checked >= 5 * 100


@pytest.mark.parametrize("case", tc.LEGS["small"], ids=lambda c: c[0])
def test_one_taxon_keeps_every_mapped_read(case):
    want = tc.crafted_leg(*case)[2]
    base = ac.crafted_restated(tc.TREES[case[0]])
    assert np.array_equal(want.state, base.state) and (want.state == ac.ASSIGNED).sum() >= 100


def test_rsv_family(pmx):
    """126 words a row: two 64-word steps.  T = 16 of (4, 16, 64) gives enough of both kinds."""
    arrays = pmx.Index.build(pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")), flank_mask=0, mode=0x100).arrays()
    assert 64 < (len(arrays["parent"]) + 63) // 64 <= 128
    over, kept = tc.counts(tc.rsv_leg(arrays))
    assert over >= 20 and kept >= 20, (over, kept)
