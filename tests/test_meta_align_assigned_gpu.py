"""align_assigned (panmap_amd/meta.py; alignAssignedReads, src/main.cpp:615-717) on rsv_4K with the rsv family: which heads it
aligns (against the restatement of the assignment, tests/assign_checks.py), in which order, and every head's records against
the compiled reference aligner run on that head's genome and reads."""
import os

import numpy as np
import pytest

import align_assigned_checks as aa
import align_checks
import assign_checks as ac
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rsv(pmx, ctx):
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    meta = pmx.Meta.build(ctx, pm)
    reads = ac.rsv_reads()
    meta.set_reads(reads)
    res = meta.assign(aa.DISCARD)
    arrays = meta.index_oriented.arrays()
    heads = ac.heads_np(arrays["parent"], arrays["offsets"])
    R = ac.rsv_restated(arrays, aa.DISCARD)
    by_node = aa.restated_by_node(R, heads)
    assigned = [reads[r] for r in range(len(reads)) if R.state[r] == ac.ASSIGNED]
    return pm, meta, reads, res, by_node, assigned


@pytest.fixture(scope="module")
def aligned(pmx, ctx, rsv):
    """the generator run to its end at K, without qualities: [(head, indices, genome, results)]"""
    pm, meta, reads, res, by_node, _ = rsv
    out = []
    for head, idx, genome, recs, cig in pmx.align_assigned(ctx, pm, meta.index, res, reads, min_num_align=aa.choose_threshold(by_node)):
        assert len(recs) == len(idx)
        out.append((head, idx, genome, pmx.records_to_results(recs, cig, False)))
    return out


def test_heads_and_reads_are_the_restatements(rsv, aligned):
    pm, _, _, _, by_node, _ = rsv
    K = aa.choose_threshold(by_node)
    want = [h for h in sorted(by_node) if len(by_node[h]) >= K]
    assert [h for h, _, _, _ in aligned] == want and 2 <= len(want) <= 12
    for head, idx, genome, _ in aligned:
        assert idx == by_node[head] and idx == sorted(idx)
        assert genome == pm.genome(head) and len(genome) > 10000


def test_records_equal_the_reference_aligner(oracle, rsv, aligned):
    assigned = rsv[5]
    for head, idx, genome, got in aligned:
        want = oracle.ref_align_reads_direct(genome, [assigned[i] for i in idx], False, 8)
        assert len(got) == len(want) == len(idx)
        assert all(x["flags"] & 3 == 0 for x in got), head
        bad = align_checks.compare_results(got, want)
        assert not bad, (head, bad[:10])
        assert sum(w["mapped"] for w in want) > len(want) // 2


def test_thresholds(pmx, ctx, rsv):
    pm, meta, reads, res, by_node, _ = rsv
    above = max(len(v) for v in by_node.values()) + 1
    assert list(pmx.align_assigned(ctx, pm, meta.index, res, reads, min_num_align=above)) == []
    for k in (0, -3):      # every head with a read qualifies: the first one only, thousands follow
        gen = pmx.align_assigned(ctx, pm, meta.index, res, reads, min_num_align=k)
        head, idx, _, recs, _ = next(gen)
        gen.close()
        assert head == min(by_node) and idx == by_node[head] and len(recs) == len(idx)


def test_a_second_call_and_qualities_change_nothing(pmx, ctx, rsv, aligned):
    pm, meta, reads, res, by_node, _ = rsv
    K = aa.choose_threshold(by_node)
    quals = [bytes(33 + (5 * i + j) % 41 for j in range(len(r))) for i, r in enumerate(reads)]
    for q in (None, quals):
        again = [(h, idx, g, pmx.records_to_results(recs, cig, False))
                 for h, idx, g, recs, cig in pmx.align_assigned(ctx, pm, meta.index, res, reads, quals=q, min_num_align=K)]
        assert again == aligned
