"""Read pairs whose mates overlap on the reference, for tests/test_chain_overlap_host.py and tests/test_chain_overlap_gpu.py:
150-base mates of fragments with inserts drawn uniformly from 150..290 (the mates share 10..150 bases) on node_7618 of the
golden SARS tree.  Where the mates overlap both carry the same minimizers, the sorted anchors alternate between the mates,
and the chain fill of the compact align tier (align/aln_compact.hpp) ends its predecessor loop early ("dominated tail").
Three cases: no errors; 0.5 % substitutions; one 1-3 base indel in every third read.  The reads are in the orientation
readFastqPaired hands over (mate 2 already on the forward strand)."""
import numpy as np

CASES = ("clean", "subs", "indel")
READ_LEN = 150
INSERT_LO, INSERT_HI = 150, 290


def overlap_pairs(genome: bytes, case: str, n_pairs: int):
    rng = np.random.default_rng({"clean": 1101, "subs": 1102, "indel": 1103}[case])
    g = np.frombuffer(genome, np.uint8)
    ins = rng.integers(INSERT_LO, INSERT_HI + 1, n_pairs)
    start = (rng.random(n_pairs) * (len(g) - ins + 1)).astype(np.int64)
    ar = np.arange(READ_LEN)
    reads = np.empty((2 * n_pairs, READ_LEN), np.uint8)
    reads[0::2] = g[start[:, None] + ar[None, :]]
    reads[1::2] = g[(start + ins - READ_LEN)[:, None] + ar[None, :]]
    bases = np.frombuffer(b"ACGT", np.uint8)
    if case == "subs":
        err = rng.random(reads.shape) < 0.005
        code = np.zeros(256, np.int64)
        for i, b in enumerate(b"ACGT"):
            code[b] = i
        reads[err] = bases[(code[reads[err]] + rng.integers(1, 4, int(err.sum()))) & 3]
    out = [bytes(r) for r in reads]
    if case == "indel":
        for i in range(0, len(out), 3):
            r = bytearray(out[i])
            p = int(rng.integers(10, READ_LEN - 10))
            ln = int(rng.integers(1, 4))
            if (i // 3) % 2:
                del r[p:p + ln]
            else:
                r[p:p] = bytes(rng.choice(bases, ln))
            out[i] = bytes(r)
    return out
