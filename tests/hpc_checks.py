"""Helpers of the homopolymer-compression (HPC) tests: the plain-Python restatement of seeding::hpcCompressWithMapping
(src/seeding.cpp:291-306), the small hand-made HPC index, and the read families that aim at the places where the device
kernels (csrc/hpc_kernels.hip: one wave per read, 64 bases per step) can go wrong.  Every family comes with the condition it
exists for, as a predicate over its reads (tests/test_hpc_families.py asserts them).  No tests here."""
import numpy as np

BASES = b"ACGT"


def hpc(seq: bytes):
    """(compressed, mapping): base 0 is kept, base i > 0 iff toupper(seq[i]) != toupper(seq[i-1]); kept characters are copied
    as they are; mapping[j] = index of the j-th kept base"""
    up = seq.upper()          # bytes.upper() changes a..z only, like toupper in the "C" locale
    mapping = [i for i in range(len(seq)) if i == 0 or up[i] != up[i - 1]]
    return bytes(seq[i] for i in mapping), mapping


def hpc_reads(reads, quals=None):
    """the reads as the place stage sees them with an HPC index (src/placement.cpp:1143-1165); with quals: (reads, quals), the
    quality of a run being that of its first base"""
    if quals is None:
        return [hpc(r)[0] for r in reads]
    out_r, out_q = [], []
    for r, q in zip(reads, quals):
        c, m = hpc(r)
        out_r.append(c)
        out_q.append(bytes(q[i] for i in m))
    return out_r, out_q


def hpc_index(oracle, genome, k, s, l, open_, t):
    """a three-node index over the real seeds of hpc(genome), marked HPC (the shape test_place_other_parameters uses)"""
    import panmap_amd as pmx
    hs, cn = oracle.histogram([hpc(genome)[0]], k, s, l, open_, t)
    keep = cn < 30000
    hs, cn = hs[keep], cn[keep]
    half = len(hs) // 2
    parent = np.array([0, 0, 1], np.uint32)
    offsets = np.array([0, len(hs), len(hs) + half, len(hs) + half + 10], np.uint64)
    hash_ = np.concatenate([hs, hs[:half], hs[half:half + 10]])
    pc = np.concatenate([np.zeros(len(hs)), cn[:half], cn[half:half + 10]]).astype(np.int16)
    cc = np.concatenate([cn, cn[:half] + 1, np.zeros(10)]).astype(np.int16)
    return pmx.Index.from_arrays(k, s, t, l, open_, parent, offsets, hash_, pc, cc, hpc=True)


# ------------------------------------------------------------------------------------------------ sequences
def runs_of(seq: bytes):
    """[(start, length)] of the maximal runs of one letter (case-insensitive)"""
    _, m = hpc(seq)
    return [(m[j], (m[j + 1] if j + 1 < len(m) else len(seq)) - m[j]) for j in range(len(m))]


def random_seq(rng, n, run_p=0.3):
    """n bases; with probability run_p a base repeats its predecessor (runs of geometric length, as in real genomes)"""
    out = bytearray()
    while len(out) < n:
        if out and rng.random() < run_p:
            out.append(out[-1])
        else:
            out.append(BASES[int(rng.integers(0, 4))])
    return bytes(out)


def run_free_seq(rng, n):
    out = bytearray()
    while len(out) < n:
        c = BASES[int(rng.integers(0, 4))]
        if not out or c != out[-1]:
            out.append(c)
    return bytes(out)


def with_run_at(rng, n, a, b):
    """n bases with ONE run covering exactly the bases a..b (inclusive), random elsewhere"""
    left = random_seq(rng, a)
    c = BASES[int(rng.integers(0, 4))]
    while left and left[-1] == c:
        c = BASES[int(rng.integers(0, 4))]
    right = random_seq(rng, n - b - 1)
    while right and right[0] == c:
        right = random_seq(rng, n - b - 1)
    return left + bytes([c]) * (b - a + 1) + right


def run_length_errors(rng, seq: bytes, p=0.3):
    """the dominant error of long noisy reads: with probability p a run is lengthened or shortened by 1 to 3 bases (never to
    nothing); no other error, so hpc() of the result equals hpc() of the input"""
    out = bytearray()
    for st, ln in runs_of(seq):
        if rng.random() < p:
            ln = max(1, ln + int(rng.integers(1, 4)) * (1 if rng.random() < 0.5 else -1))
        out += seq[st:st + 1] * ln
    return bytes(out)


# ------------------------------------------------------------------------------------------------ families
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 150)


def fam_lengths(rng):
    return [random_seq(rng, n) for n in EDGE_LENGTHS for _ in range(100)]


def cond_lengths(reads):
    """every length at which the last step of a read is empty, one base, full or one over: 0, 1, 2, 63, 64, 65, 127, 128, 129, 150"""
    return {len(r) for r in reads} == set(EDGE_LENGTHS)


def fam_step_runs(rng):
    return [with_run_at(rng, 150, 62, 66) for _ in range(150)] + [with_run_at(rng, 150, 126, 130) for _ in range(150)] + \
           [with_run_at(rng, 150, 63, 64) for _ in range(50)]


def cond_step_runs(reads):
    """runs that cover bases 62..66, 126..130 and exactly 63..64 of a read: the predecessor of lane 0 comes from the step before"""
    def has(r, a, b):
        return any(st == a and st + ln - 1 == b for st, ln in runs_of(r))
    return any(has(r, 62, 66) for r in reads) and any(has(r, 126, 130) for r in reads) and any(has(r, 63, 64) for r in reads)


def fam_long_runs(rng):
    out = []
    for _ in range(60):
        n_run = int(rng.integers(131, 400))
        lead = int(rng.integers(0, 70))
        out.append(with_run_at(rng, lead + n_run + int(rng.integers(1, 80)), lead, lead + n_run - 1))
    return out + [b"A" * 150, b"A" * 64, b"A" * 65, b"A" * 1000, b"T" * 129]


def cond_long_runs(reads):
    """a run longer than 130 bases (a whole 64-base step keeps nothing) and reads that are one run (all A)"""
    return any(max((ln for _, ln in runs_of(r)), default=0) > 130 and len(runs_of(r)) > 1 for r in reads) and b"A" * 150 in reads


def fam_boundaries(rng):
    reads = []
    last = None
    for _ in range(1000):
        n = 2 * int(rng.integers(0, 80)) + 1
        r = bytearray(random_seq(rng, n))
        if last is not None:
            r[0] = last
        last = r[-1]
        reads.append(bytes(r))
    return reads


def cond_boundaries(reads):
    """consecutive reads where read i ends with the base read i+1 starts with (a run must not reach across a read boundary);
    every length is odd, so the reads do not start on 16-byte boundaries of the concatenated buffer"""
    starts = np.cumsum([0] + [len(r) for r in reads])[:-1]
    return all(len(r) % 2 == 1 for r in reads) and all(a[-1] == b[0] for a, b in zip(reads, reads[1:])) and \
        np.count_nonzero(starts % 16) > len(reads) // 2


def fam_letters(rng):
    out = []
    for i in range(500):
        r = bytearray(random_seq(rng, int(rng.integers(20, 200))))
        if i % 3 == 0:
            r = bytearray(bytes(r).lower())
        if i % 3 == 1:   # mixed case inside runs
            for j in range(len(r)):
                if rng.random() < 0.5:
                    r[j] = bytes(r[j:j + 1]).lower()[0]
        if i % 4 == 0:
            p = int(rng.integers(0, len(r) - 10))
            r[p:p + int(rng.integers(1, 9))] = b"N" * 8
        if i % 5 == 0:
            p = int(rng.integers(0, len(r) - 10))
            r[p:p + 3] = b"RYK"
        out.append(bytes(r))
    return out + [b"aAaA", b"AaTt", b"NNNN", b"nNnN", b"RY", b"RRYYKK", b"ACGT@`[{", b"a`A@", b"zZ{["]


def cond_letters(reads):
    """lower case, mixed case inside a run (aAaA -> a), N runs (NNNN -> N), IUPAC letters (RY stays RY) and the bytes next to
    the letters in ASCII ('@' '`' '[' '{' are not upper-cased)"""
    return hpc(b"aAaA")[0] == b"a" and hpc(b"NNNN")[0] == b"N" and hpc(b"RY")[0] == b"RY" and hpc(b"a`A@")[0] == b"a`A@" and \
        all(x in reads for x in (b"aAaA", b"NNNN", b"RY", b"a`A@")) and any(r != r.upper() and r != r.lower() for r in reads)


def fam_long_read(rng):
    return [run_length_errors(rng, random_seq(rng, 20000))[:20000]]


def cond_long_read(reads):
    """one read of 20,000 bases with run-length errors: hundreds of steps of one wave"""
    return len(reads) == 1 and len(reads[0]) == 20000


FAMILIES = {
    "lengths": (fam_lengths, cond_lengths),
    "step_runs": (fam_step_runs, cond_step_runs),
    "long_runs": (fam_long_runs, cond_long_runs),
    "boundaries": (fam_boundaries, cond_boundaries),
    "letters": (fam_letters, cond_letters),
    "long_read": (fam_long_read, cond_long_read),
}


def family(name, seed=11):
    return FAMILIES[name][0](np.random.default_rng([seed, sorted(FAMILIES).index(name)]))


def all_families(seed=11):
    """the families one after the other (about 3,000 reads, the boundary family contiguous)"""
    out = []
    for name in FAMILIES:
        out += family(name, seed)
    return out


def random_quals(rng, reads):
    return [(rng.integers(2, 41, len(r)).astype(np.uint8) + 33).tobytes() for r in reads]
