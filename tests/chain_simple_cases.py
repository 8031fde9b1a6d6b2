"""Read pairs for tests/test_chain_simple_host.py and tests/test_chain_simple_gpu.py: the families at which the compact align
tier's register-only chain path (align/aln_compact_simple.hpp) can go wrong, on node_7618 of the golden SARS tree, and the host
build of that path beside the two forms it must agree with (tests/hostsim/chain_simple.cpp).  The reads are in the orientation
readFastqPaired hands over (mate 2 already reverse-complemented), so a fragment of the forward strand gives two forward reads."""
import ctypes as C
import os
import subprocess

import numpy as np

import align_checks as ac

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (read length, insert low, insert high, what else)
FAMILIES = {
    "clean": (150, 301, 500, ""),          # mates apart, error-free
    "subs": (150, 301, 500, "subs"),       # 0.5 % substitutions: steps longer than k inside a run
    "indel": (150, 301, 500, "indel"),     # a 1-3 base indel in every third read: those pairs must bail
    "strands": (150, 301, 500, "strands"), # every other fragment from the reverse strand: runs in reversed seed order
    "mixed": (150, 250, 350, ""),          # both classes in every wave
    "overlap": (150, 150, 290, ""),        # no simple pair
    "far": (150, 560, 900, ""),            # the junction at and beyond max_dist_x: two chains
    "len160": (160, 321, 500, ""),         # the longest runs the tier holds (the max_skip break)
    "len75": (75, 200, 200, ""),
    "sparse": (34, 69, 200, ""),           # mates with one or two seeds
    "ends": (150, 301, 500, "ends"),       # fragments at both ends of the reference
}
GPU_FAMILIES = ("clean", "indel", "mixed", "far")   # first, third, fifth and seventh


def _revcomp(a):
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGTN", b"TGCAN"):
        comp[x] = y
    return comp[a[:, ::-1]]


def family_pairs(genome: bytes, family: str, n_pairs: int):
    read_len, lo, hi, what = FAMILIES[family]
    rng = np.random.default_rng(2200 + sorted(FAMILIES).index(family))
    g = np.frombuffer(genome, np.uint8)
    ins = rng.integers(lo, hi + 1, n_pairs)
    start = (rng.random(n_pairs) * (len(g) - ins + 1)).astype(np.int64)
    if what == "ends":   # within 40 bases of the first / the last base
        off = rng.integers(0, 40, n_pairs)
        start = np.where(np.arange(n_pairs) % 2 == 0, off, len(g) - ins - off)
    ar = np.arange(read_len)
    left = g[start[:, None] + ar[None, :]]
    right = g[(start + ins - read_len)[:, None] + ar[None, :]]
    reads = np.empty((2 * n_pairs, read_len), np.uint8)
    reads[0::2] = left
    reads[1::2] = right
    if what == "strands":
        rv = np.arange(n_pairs) % 2 == 1
        reads[0::2][rv] = _revcomp(right[rv])
        reads[1::2][rv] = _revcomp(left[rv])
    bases = np.frombuffer(b"ACGT", np.uint8)
    code = np.zeros(256, np.int64)
    for i, b in enumerate(b"ACGT"):
        code[b] = i
    if what == "subs":
        err = rng.random(reads.shape) < 0.005
        reads[err] = bases[(code[reads[err]] + rng.integers(1, 4, int(err.sum()))) & 3]
    out = [bytes(r) for r in reads]
    if what == "indel":
        for i in range(0, len(out), 3):
            r = bytearray(out[i])
            p = int(rng.integers(10, read_len - 10))
            ln = int(rng.integers(1, 4))
            if (i // 3) % 2:
                del r[p:p + ln]
            else:
                r[p:p] = bytes(rng.choice(bases, ln))
            out[i] = bytes(r)
    return out


_LIB = []


def _lib(tmp_dir):
    if not _LIB:
        out = os.path.join(str(tmp_dir), "libchain_simple.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(HERE, "..", "panmap_amd", "csrc"), os.path.join(HERE, "hostsim", "chain_simple.cpp"), "-o", out], check=True)
        L = C.CDLL(out)
        L.hs_chain_simple.restype = C.c_int
        _LIB.append(L)
    return _LIB[0]


def host_chain_simple(tmp_dir, reference: bytes, reads, pos32=False, want_edits=False):
    """-> cls (int8 per pair: 0 seeding bailed, 1 not simple, 2 simple and finished, 3 simple and bailed) and, for the simple
    path, the first form and the second form: (results, done flags, edit counts per read; -1 where the form did not finish)"""
    L = _lib(tmp_dir)
    n = len(reads)
    arr = (C.c_char_p * n)(*reads)
    lens = (C.c_int * n)(*[len(r) for r in reads])
    cls = np.zeros(n // 2, np.int8)
    recs = [(ac.Rec * n)() for _ in range(3)]
    cig = [np.zeros(n, np.uint32) for _ in range(3)]
    edits = [np.zeros(n, np.int32) for _ in range(3)]
    done = [np.zeros(n // 2, np.int8) for _ in range(3)]
    rc = L.hs_chain_simple(C.c_char_p(reference), C.c_int64(len(reference)), C.c_int(n), arr, lens, C.c_int(0), C.c_int(int(pos32)), C.c_int(int(want_edits)),
                           C.c_void_p(cls.ctypes.data), (C.c_void_p * 3)(*[C.addressof(r) for r in recs]),
                           (C.c_void_p * 3)(*[c.ctypes.data for c in cig]), (C.c_void_p * 3)(*[e.ctypes.data for e in edits]),
                           (C.c_void_p * 3)(*[d.ctypes.data for d in done]))
    assert rc == 0, rc
    done[0] = (cls == 2).astype(np.int8)
    return cls, [(ac.records_to_results(recs[f], cig[f], n, True), done[f], edits[f]) for f in range(3)]
