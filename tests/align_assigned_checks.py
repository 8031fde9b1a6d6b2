"""--align-reads (a BAM per assigned node) and ReadSet.select: what their tests share.  No product code in here, and no test.

  * the select family: 13 reads whose lengths sit on either side of every step of the copy kernel (a 64-lane wave, pieces of up
    to 16 bytes, the 160-base limit of the read records) -- 0, 1, 31, 32, 33, 63, 64, 65, 159, 160, 161, 2,000 and 20,000 bases --
    with N, lower case and R among the bases, and a quality string per read;
  * the restatement's head -> FASTQ indices map, and the threshold K the rsv tests align at;
  * literal restatements of alignAssignedReads' `sanitize` and of its 80-column FASTA (src/main.cpp:649-654, 683-689)."""
import functools

import numpy as np

import assign_checks as ac

SELECT_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 159, 160, 161, 2000, 20000)
DISCARD = 0.6


@functools.lru_cache(maxsize=None)
def select_family():
    """(reads, quals): one read per length of SELECT_LENGTHS, in that order"""
    rng = np.random.default_rng(613)
    letters = np.frombuffer(b"ACGTACGTACGTACGTNacgtR", np.uint8)
    reads, quals = [], []
    for n in SELECT_LENGTHS:
        reads.append(letters[rng.integers(0, len(letters), n)].tobytes())
        quals.append((33 + rng.integers(0, 41, n)).astype(np.uint8).tobytes())
    for want in (b"N", b"a", b"R"):
        assert any(want in r for r in reads)
    return reads, quals


def select_index_lists():
    """name -> index list into the select family"""
    n = len(SELECT_LENGTHS)
    rng = np.random.default_rng(7)
    return {"empty": [], "one": [4], "all": list(range(n)), "reversed": list(range(n))[::-1], "repeated": [3, 8, 3, 3, 11, 8],
            "zero_length_alone": [0], "last_alone": [n - 1], "random_1000": rng.integers(0, n, 1000).tolist()}


def restated_by_node(R, heads):
    """{head: ascending FASTQ indices} of a restatement (assign_checks.restate): the assigned reads, numbered in input order, under
    the head of every node they are assigned to"""
    out, pos = {}, 0
    for r in range(len(R.state)):
        if R.state[r] != ac.ASSIGNED:
            continue
        for h in sorted({int(heads[v]) for v in R.nodes[r]}):
            out.setdefault(h, []).append(pos)
        pos += 1
    return out


def choose_threshold(by_node) -> int:
    """K = the read count of the third most populated head"""
    return sorted((len(v) for v in by_node.values()), reverse=True)[2]


def sanitize(s: str) -> str:
    out = list(s)
    for i, c in enumerate(out):
        if c == "/" or c == "\\" or c in " \t\n\v\f\r":      # isspace in the "C" locale
            out[i] = "_"
    return "".join(out)


def reference_fasta(pairs) -> str:
    text = ""
    for node_id, genome in pairs:
        text += ">" + node_id + "\n"
        i = 0
        while i < len(genome):
            text += genome[i:i + min(80, len(genome) - i)] + "\n"
            i += 80
    return text
