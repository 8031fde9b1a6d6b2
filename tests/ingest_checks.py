"""The read-ingest path -- k_read_word_counts, k_pack_reads, k_pack_reads_fixed, pack_record, k_collapse_reads and the two forms
of k_seed_histogram_ks -- checked on the packed form itself (tests/test_ingest_gpu.py on the GPU, tests/test_ingest_families.py
for the reference and the read sets themselves).  pack_reference restates the packing RULES in numpy, not the kernels; the
read sets are built by name with fixed seeds over one 3,000-base random genome, and each aims at one edge of the kernels:
every byte shift of the fixed-length kernel's 16-byte loads, every word count and tail, the far gallop of the read search, the
1,024-read collapse block, the 64-read tile, the 4,096-read locality order.  Nothing here touches a GPU at import."""
import functools

import numpy as np

GENOME_LEN = 3000
FIXED_LENGTHS = (1, 19, 31, 32, 33, 64, 95, 96, 128, 150, 151, 160, 161, 200)   # (128: the one word count, four, the others leave out)
FIXED_SMALL, FIXED_LARGE = 67, 4200         # 4,200: the locality order is on (>= 4,096) and the collapse runs five blocks
FIXED_FEW = (19, 33, 150, 161)              # the fixed lengths of the generic-kernel legs
WRAP_OFFSETS = (1, 2, 7, 8, 13, 15)         # byte offsets (mod 16) of a wrapped set's first read; an uploaded set starts at 0
WRAP_PAD = 16                               # spare bytes in front of the first read, on top of the offset, and behind the last
SLICE_R0 = 3                                # the slice form starts at this read
COUNT_EDGES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
PLANTED = (150, 160, 161)
REC_MAX = 160                               # reads of up to 160 bases have a 64-byte record

# the seeding parameters of the histogram sweep: (k, s, l, open, t); the first two run the specialised kernel
SPECIALISED = ((19, 8, 3, False, 0), (19, 8, 1, False, 0))
GENERIC = ((15, 8, 1, False, 0), (21, 10, 4, False, 2), (19, 8, 2, True, 3))
TRIMS = ((0, 0), (10, 25), (0, 200))        # (0, 200) leaves no valid k-mer in any read of up to 200 bases
MIN_Q = 20


# ------------------------------------------------------------------------------------------------ the rules
def _tables():
    code, amb = np.zeros(256, np.uint8), np.ones(256, np.uint8)
    for c in range(256):
        u = c & 0xDF
        if u in b"ACGT":
            code[c], amb[c] = b"ACGT".index(u), 0
        elif u == ord("U"):
            code[c] = 3
    return code, amb


CODE, AMB = _tables()


def pack_reference(reads):
    """(words uint64[n_words], amb uint32[n_words], woff int64[n+1], records uint8[n, 64] | None) of a list of reads: base j of
    a word at bits 2j+1:2j of `words` and bit j of `amb`; a byte c with c & 0xDF in A C G T has code 0..3 and ambiguity 0, U / u
    ambiguity 1 and code 3, every other byte ambiguity 1 and code 0; nothing past a read's end; every read starts on a word.
    Records (no read longer than 160 bases): words at bytes 0..39, ambiguity words at 40..59, the length at 60, unused slots 0"""
    n = len(reads)
    lens = np.fromiter((len(r) for r in reads), np.int64, n)
    nw = (lens + 31) // 32
    woff = np.zeros(n + 1, np.int64)
    np.cumsum(nw, out=woff[1:])
    n_words = int(woff[-1])
    cat = np.frombuffer(b"".join(reads), np.uint8)
    boff = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=boff[1:])
    pos = np.repeat(woff[:-1] * 32 - boff[:-1], lens) + np.arange(len(cat), dtype=np.int64)   # a base's place among the words' 32 x n_words
    code, am = np.zeros(n_words * 32, np.uint64), np.zeros(n_words * 32, np.uint32)
    code[pos] = CODE[cat]
    am[pos] = AMB[cat]
    words = (code.reshape(-1, 32) << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)     # (disjoint bits: the sum is the OR)
    amb = (am.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    records = None
    if n > 0 and int(lens.max()) <= REC_MAX:
        records = np.zeros((n, 64), np.uint8)
        read_of = np.repeat(np.arange(n), nw)
        slot = np.arange(n_words) - woff[read_of]
        records.view(np.uint64)[read_of, slot] = words
        records.view(np.uint32)[read_of, 10 + slot] = amb
        records.view(np.uint32)[:, 15] = lens
    return words, amb, woff, records


def unpack(words, amb, woff, lens):
    """the reads of a packed form, as the packing keeps them: A C G T, `U` for code 3 under an ambiguity bit, `N` for code 0
    under one; an ambiguity bit over code 1 or 2, or anything but zeros past a read's end, is an error"""
    out = []
    for r, n in enumerate(lens):
        n = int(n)
        w, a = words[woff[r]:woff[r + 1]], amb[woff[r]:woff[r + 1]]
        assert len(w) == (n + 31) // 32
        code = ((w[:, None] >> (2 * np.arange(32, dtype=np.uint64))) & np.uint64(3)).astype(np.uint8).reshape(-1)
        am = ((a[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(np.uint8).reshape(-1)
        assert not code[n:].any() and not am[n:].any(), "bits past the read's end"
        code, am = code[:n], am[:n]
        assert not np.any(am.astype(bool) & ((code == 1) | (code == 2))), "an ambiguous base with code 1 or 2"
        ch = np.frombuffer(b"ACGT", np.uint8)[code].copy()
        ch[am.astype(bool) & (code == 0)] = ord("N")
        ch[am.astype(bool) & (code == 3)] = ord("U")
        out.append(ch.tobytes())
    return out


def kept_form(read):
    """what unpack gives back for a read: the rules once more, byte by byte"""
    out = bytearray()
    for c in read:
        u = c & 0xDF
        out.append(u if u in b"ACGT" else ord("U") if u == ord("U") else ord("N"))
    return bytes(out)


# ------------------------------------------------------------------------------------------------ read sets
@functools.lru_cache(maxsize=None)
def genome():
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(101).integers(0, 4, GENOME_LEN)].tobytes()


def _windows(rng, lens):
    g, out = genome(), []
    for n in lens:
        s = int(rng.integers(0, GENOME_LEN - int(n) + 1))
        out.append(g[s:s + int(n)])
    return out


def fixed(L, n):
    """n reads of L bases, windows of the genome (n = 4,200 over 3,000 starts: many reads are copies of another)"""
    return "fixed_%d_%d" % (L, n), _windows(np.random.default_rng(1000 + L), [L] * n)


def ragged_all_lengths(lo, hi, n):
    """lengths cycling lo..hi in shuffled order; every seventh read carries an N, every eleventh is lower case"""
    rng = np.random.default_rng(2000 + hi)
    lens = lo + np.arange(n) % (hi - lo + 1)
    lens = lens[rng.permutation(n)]
    reads = _windows(rng, lens)
    for i in range(n):
        if i % 7 == 0 and len(reads[i]):
            r = bytearray(reads[i])
            r[int(rng.integers(0, len(r)))] = ord("N")
            reads[i] = bytes(r)
        if i % 11 == 0:
            reads[i] = reads[i].lower()
    return "ragged_%d_%d_%d" % (lo, hi, n), reads


def _random_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def skewed():
    """words per read as far from uniform as they get: the proportional guess of k_pack_reads lands thousands of reads away
    from the read that holds the word, in both directions, next to runs of reads without a word"""
    rng = np.random.default_rng(3000)
    reads = [b"", _random_bases(rng, 20000)]
    reads += _windows(rng, rng.integers(0, 4, 3000))
    reads += [_random_bases(rng, 9000)]
    reads += [b""] * 500
    reads += _windows(rng, [40])
    # (with the reads above alone the guess is never more than 700 reads off: a longer run and a longer read behind them)
    reads += [b""] * 5000
    reads += [_random_bases(rng, 30000)]
    reads += [b""]
    return "skewed", reads


ALPHABET_POS = (0, 18, 31, 32, 63, 64, 131, 149)


def alphabet():
    rng = np.random.default_rng(4000)
    every = bytes(range(256))
    r = bytearray(_windows(rng, [150])[0])
    for i, p in enumerate(ALPHABET_POS):
        r[p] = b"NnUuR"[i % 5]
    r = bytes(r)
    return "alphabet", [every, r, every.lower(), r.lower()]


def planted_positions(L):
    return (0, 18, 19, 31, 32, L - 20, L - 19, L - 1)


def planted_n(L):
    rng = np.random.default_rng(5000 + L)
    base = _windows(rng, [L])[0]
    reads = []
    for p in planted_positions(L):
        r = bytearray(base)
        r[p] = ord("N")
        reads.append(bytes(r))
    return "planted_n_%d" % L, reads


def _distinct_reads(n, L=150):
    """n different reads of L bases: the genome's windows in turn, and from the second round on with base 75 rotated"""
    g, m = genome(), GENOME_LEN - L + 1
    reads = []
    for i in range(n):
        r = bytearray(g[i % m:i % m + L])
        r[75] = b"ACGT"[(b"ACGT".index(r[75]) + i // m) % 4]
        reads.append(bytes(r))
    assert len(set(reads)) == n
    return reads


def copies(n, distinct):
    if distinct:
        return "distinct_%d" % n, _distinct_reads(n)
    return "identical_%d" % n, [genome()[1200:1350]] * n


def copies_mixed():
    """700 copies each of three reads, dealt in turn: every 1,024-read block of the collapse holds copies of all three"""
    three = [genome()[s:s + 150] for s in (100, 900, 2100)]
    return "mixed_3x700", [three[i % 3] for i in range(2100)]


def _registry():
    reg = {}
    for L in FIXED_LENGTHS:
        for n in (FIXED_SMALL, FIXED_LARGE):
            reg["fixed_%d_%d" % (L, n)] = functools.partial(fixed, L, n)
    reg["ragged_0_160_4200"] = functools.partial(ragged_all_lengths, 0, 160, 4200)
    reg["ragged_0_200_4200"] = functools.partial(ragged_all_lengths, 0, 200, 4200)
    reg["skewed"] = skewed
    reg["alphabet"] = alphabet
    for L in PLANTED:
        reg["planted_n_%d" % L] = functools.partial(planted_n, L)
    for n in COUNT_EDGES:
        reg["identical_%d" % n] = functools.partial(copies, n, False)
        reg["distinct_%d" % n] = functools.partial(copies, n, True)
    reg["mixed_3x700"] = copies_mixed
    return reg


REGISTRY = _registry()
RAGGED = ("ragged_0_160_4200", "ragged_0_200_4200")
# the read sets of the histogram sweep: all of them for the specialised kernel, a few for the generic one
SWEEP_FULL = (["fixed_%d_%d" % (L, n) for L in FIXED_LENGTHS for n in (FIXED_SMALL, FIXED_LARGE)] + list(RAGGED) +
              ["planted_n_%d" % L for L in PLANTED] + ["alphabet"])
SWEEP_FEW = ["fixed_%d_%d" % (L, n) for L in FIXED_FEW for n in (FIXED_SMALL, FIXED_LARGE)] + list(RAGGED)


@functools.lru_cache(maxsize=None)
def read_set(name):
    got, reads = REGISTRY[name]()
    assert got == name
    return reads


@functools.lru_cache(maxsize=None)
def packed(name, r0=0):
    """pack_reference of the reads [r0, n) of a named set, computed once"""
    return pack_reference(read_set(name)[r0:])


def qualities(name):
    """Phred+33 strings for a named set: half the reads clean, every read with a low stretch (as test_place_min_seed_quality)"""
    rng = np.random.default_rng(6000)
    out = []
    for r in read_set(name):
        q = rng.integers(2, 41, len(r)).astype(np.uint8) + 33
        if rng.random() < 0.5:
            q[:] = 73
        lo = int(rng.integers(0, max(1, len(r) - 30)))
        q[lo:lo + int(rng.integers(5, 40))] = 35
        out.append(q.tobytes())
    return out


_want = {}


def want_histogram(oracle, name, params, trim=(0, 0), dedup=False, min_q=0):
    """oracle.histogram of a named set, computed once per (set, parameters, trims, dedup, quality threshold)"""
    key = (name, params, trim, dedup, min_q)
    if key not in _want:
        k, s, l, open_syncmer, t = params
        _want[key] = oracle.histogram(read_set(name), k, s, l, open_syncmer, t, trim[0], trim[1], dedup,
                                      qualities(name) if min_q else None, min_q)
    return _want[key]


# ------------------------------------------------------------------------------------------------ what the sets reach
def fixed_shifts(L, n, offset):
    """per word of a fixed-length set whose first read starts `offset` bytes behind a 16-byte boundary:
    (sh = address & 15, bytes needed, 16-byte blocks loaded = n_q of k_pack_reads_fixed)"""
    nw = (L + 31) // 32
    r, j = np.divmod(np.arange(n * nw), nw)
    nb = np.minimum(L - 32 * j, 32)
    sh = (offset + r * L + 32 * j) & 15
    return sh, nb, (sh + nb + 15) >> 4


def proportional_guess_error(woff):
    """per word w of a packed set: (the read that holds it, the read k_pack_reads guesses first = w * n / n_words, clamped)"""
    n, n_words = len(woff) - 1, int(woff[-1])
    w = np.arange(n_words)
    true = np.searchsorted(woff, w, side="right") - 1
    guess = np.clip((w.astype(np.float64) * float(n) / float(n_words)).astype(np.int64), 0, n - 1)
    return true, guess


def range_bounds(name):
    """pack_range bounds that cover a named set: for `skewed`, cuts inside both runs of reads without a word and right
    behind the long reads; for the others, an empty range, a range of one read and uneven thirds"""
    n = len(read_set(name))
    if name == "skewed":
        return [0, 1, 2, 700, 700, 3002, 3003, 3200, 3499, 3503, 3504, 6000, n - 2, n - 1, n]
    return [0, 1, n // 3, n // 3, (2 * n) // 3 + 1, n] if n >= 3 else [0, n]
