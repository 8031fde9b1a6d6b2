"""The inputs of the --align-reads tests are what they claim to be (tests/align_assigned_checks.py), checked without a device: the
rsv family at the chosen threshold K has a handful of qualifying heads that share reads and hold reverse-complemented and
mutated reads, the select family has every length its kernel steps at, and the two small text functions of the feature
(sanitize_node_id, format_reference_fasta) equal their literal restatements on hand-written cases."""
import os

import pytest

import align_assigned_checks as aa
import assign_checks as ac
from conftest import GOLDEN


@pytest.fixture(scope="module")
def rsv(pmx):
    arrays = pmx.Index.build(pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")), flank_mask=0, mode=0x100).arrays()
    heads = ac.heads_np(arrays["parent"], arrays["offsets"])
    R = ac.rsv_restated(arrays, aa.DISCARD)
    return R, aa.restated_by_node(R, heads)


def test_rsv_family_at_the_chosen_threshold(rsv):
    """all of rsv_reads() is used: at K (the third most populated head's count; 356 when this was written, three heads at or
    above it) the restatement stays inside the caps, so no prefix is needed"""
    R, by_node = rsv
    K = aa.choose_threshold(by_node)
    qualifying = [h for h in sorted(by_node) if len(by_node[h]) >= K]
    assert 2 <= len(qualifying) <= 12, (K, len(qualifying))
    assert any(len(v) < K for v in by_node.values())
    assert all(v == sorted(set(v)) for v in by_node.values())
    # a read in two qualifying heads
    seen = {}
    for h in qualifying:
        for i in by_node[h]:
            seen[i] = seen.get(i, 0) + 1
    assert max(seen.values()) >= 2
    # a qualifying head with a reverse-complemented read and a mutated read: by content -- a forward read is a window of one of
    # the two genomes, a reverse-complemented one has its reverse complement there, a mutated one neither (and is assigned)
    genomes = [ac._fasta(os.path.join(GOLDEN, f)).encode() for f in ("MZ515733.1.fa", "rsv_4K.panman.random.node_1330.fa")]
    reads = ac.rsv_reads()
    assigned = [r for r in range(len(reads)) if R.state[r] == ac.ASSIGNED]

    def kind(read):
        if any(read in g for g in genomes):
            return "forward"
        return "revcomp" if any(ac.revcomp(read) in g for g in genomes) else "mutated"
    assert any({"revcomp", "mutated"} <= {kind(reads[assigned[i]]) for i in by_node[h]} for h in qualifying)


def test_select_family_covers_every_length():
    reads, quals = aa.select_family()
    assert tuple(len(r) for r in reads) == (0, 1, 31, 32, 33, 63, 64, 65, 159, 160, 161, 2000, 20000)
    assert [len(q) for q in quals] == [len(r) for r in reads]
    lists = aa.select_index_lists()
    assert lists["empty"] == [] and len(lists["one"]) == 1 and lists["all"] == list(range(13)) and lists["reversed"] == lists["all"][::-1]
    assert len(lists["repeated"]) > len(set(lists["repeated"])) and lists["zero_length_alone"] == [0] and lists["last_alone"] == [12]
    assert len(lists["random_1000"]) == 1000 and set(lists["random_1000"]) == set(range(13))


def test_sanitize_and_fasta_on_hand_written_cases(pmx):
    for node_id, want in (("a/b\\c\td e", "a_b_c_d_e"), ("node_1", "node_1"), ("x\ny\rz\v\f", "x_y_z__"), ("", "")):
        assert aa.sanitize(node_id) == want and pmx.sanitize_node_id(node_id) == want
    pairs = [("n%d x" % n, "ACGTN"[n % 5] * n) for n in (0, 79, 80, 81, 160)]
    want = aa.reference_fasta(pairs)
    assert want == (">n0 x\n" ">n79 x\n" + "N" * 79 + "\n" ">n80 x\n" + "A" * 80 + "\n" ">n81 x\n" + "C" * 80 + "\nC\n"
                    ">n160 x\n" + "A" * 80 + "\n" + "A" * 80 + "\n")
    assert pmx.format_reference_fasta(pairs) == want
    assert pmx.format_reference_fasta([(i, g.encode()) for i, g in pairs]) == want
    assert pmx.format_reference_fasta([]) == ""
