"""--meta --mask-reads / --mask-seeds: the restatement the tests compare the device path with, and the read family.
No product code in here: the rule is the reference's loops (ThreadsManager::initializeQueryData, src/mgsr.cpp:2049-2139) on
merged seedmer lists, the family's seedmers come from oracle_meta.seedmers.

The rule, on the reads after equal seedmer lists were merged into one read with a multiplicity:
  * count[h] = sum of the multiplicities of the merged reads that carry h -- once per read (the loop is over uniqueSeedmers),
    whatever the orientation;
  * mask_reads T > 0: a merged read is dropped when any entry of its list has count <= T (numMaskReads counts them);
  * else mask_seeds T > 0: every entry with count <= T is removed, the order of the rest is kept (numMaskSeeds counts the
    entries), a read left empty is dropped, and reads that became equal stay two reads.

Family (rsv_4K's two FASTA genomes): tiles of MZ515733.1 whose neighbours share k-min-mers, isolated windows of node_1330,
triplicated reads, reverse-complement copies, a tandem read (one hash several times in its list), a 2,000-base window (more
than 64 seedmers), a 20 kb concatenation (more than 1,024), a read with exactly one seedmer, reads with two substitutions."""
import functools
import os

import numpy as np

from conftest import GOLDEN
from oracle import oracle_meta as om

K, S, L = 19, 8, 3
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s.translate(_RC)[::-1]


def restate_masks(off, hash, rev, mult, mask_reads, mask_seeds):
    """merged lists (offsets, hashes, orientations, multiplicities) -> (new offsets, new hashes, new orientations, new
    multiplicities, old read -> new read with -1 = dropped, reads dropped by mask_reads, entries removed by mask_seeds,
    {hash: count})"""
    assert not (mask_reads > 0 and mask_seeds > 0), "Only one masking parameter can be set at a time"
    n = len(off) - 1
    lists = [[(int(hash[q]), int(rev[q])) for q in range(off[r], off[r + 1])] for r in range(n)]
    counts = {}
    for r in range(n):
        for h in {h for h, _ in lists[r]}:                       # uniqueSeedmers: once per read
            counts[h] = counts.get(h, 0) + int(mult[r])
    kept, num_mask_reads, num_mask_seeds = [], 0, 0
    if mask_reads > 0:
        for r in range(n):
            if any(counts[h] <= mask_reads for h, _ in lists[r]):
                num_mask_reads += 1
            else:
                kept.append((r, lists[r]))
    elif mask_seeds > 0:
        for r in range(n):
            left = [(h, v) for h, v in lists[r] if counts[h] > mask_seeds]
            num_mask_seeds += len(lists[r]) - len(left)
            if left:
                kept.append((r, left))
    else:
        kept = list(enumerate(lists))
    old_to_new = np.full(n, -1, np.int64)
    new_off, new_hash, new_rev, new_mult = [0], [], [], []
    for i, (r, x) in enumerate(kept):
        old_to_new[r] = i
        new_hash += [h for h, _ in x]
        new_rev += [v for _, v in x]
        new_off.append(len(new_hash))
        new_mult.append(int(mult[r]))
    return (np.array(new_off, np.int64), np.array(new_hash, np.uint64), np.array(new_rev, np.uint8), np.array(new_mult, np.int64), old_to_new,
            num_mask_reads, num_mask_seeds, counts)


def merge_lists(reads):
    """what pmx_meta_set_reads makes of raw reads, restated from the strings: the distinct non-empty seedmer lists in the order
    of (hash list, orientation list) with their multiplicities -> (offsets, hashes, orientations, multiplicities, raw -> merged)"""
    lists = [tuple(om.seedmers(r, K, S, L)) for r in reads]
    distinct = sorted({x for x in lists if x}, key=lambda x: (tuple(h for h, _ in x), tuple(int(v) for _, v in x)))
    index = {x: i for i, x in enumerate(distinct)}
    mult = np.zeros(len(distinct), np.int64)
    for x in lists:
        if x:
            mult[index[x]] += 1
    off = np.concatenate([[0], np.cumsum([len(x) for x in distinct])]).astype(np.int64)
    h = np.array([hh for x in distinct for hh, _ in x], np.uint64)
    v = np.array([int(vv) for x in distinct for _, vv in x], np.uint8)
    return off, h, v, mult, np.array([index[x] if x else -1 for x in lists], np.int64)


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def genomes():
    return _fasta(os.path.join(GOLDEN, "MZ515733.1.fa")).encode(), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa")).encode()


def _prefix_with(seq, want):
    """the shortest prefix of seq with `want` seedmers (a base more adds at most one)"""
    lo, hi = K, len(seq)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(om.seedmers(seq[:mid], K, S, L)) < want:
            lo = mid + 1
        else:
            hi = mid
    return seq[:lo]


class Family:
    """reads: the raw reads in a shuffled order; the named members are the reads themselves"""


@functools.lru_cache(maxsize=None)
def family():
    rng = np.random.default_rng(2049)
    a, b = genomes()
    F = Family()
    F.tiles = [a[i:i + 150] for i in range(0, 3000, 50)]                 # neighbours overlap by 100 bases
    # isolated windows of b: past the part of b the 20 kb read holds, none of their k-min-mers in a (every other read is made of
    # a), in the head of b or in each other -- found by search, the two genomes are close
    taken = {h for h, _ in om.seedmers(a, K, S, L)} | {h for h, _ in om.seedmers(b[:20000 - len(a)], K, S, L)}
    F.isolated = []
    for i in range(20000 - len(a) + 150, len(b) - 150, 150):
        hs = {h for h, _ in om.seedmers(b[i:i + 150], K, S, L)}
        if hs and not (hs & taken) and len(F.isolated) < 4:
            F.isolated.append(b[i:i + 150])
            taken |= hs
    F.triplicated = F.tiles[5:10]
    F.revcomp = [revcomp(r) for r in F.tiles[20:28]]
    unit = a[3300:3380]
    F.tandem = unit * 5
    F.window = a[7000:9000]
    F.long = a + b[:20000 - len(a)]
    F.single = _prefix_with(a[6000:6300], 1)
    F.mutated = []
    for r in F.tiles[30:40]:
        q = bytearray(r)
        for p in rng.choice(len(q), 2, replace=False):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4]
        F.mutated.append(bytes(q))
    reads = (F.tiles + F.isolated + F.triplicated * 2 + F.revcomp + [F.tandem] * 2 + [F.window, F.long, F.single] + F.mutated)
    F.reads = [reads[i] for i in rng.permutation(len(reads))]
    return F


@functools.lru_cache(maxsize=None)
def family_merged():
    return merge_lists(family().reads)


MASKS = ((1, 0), (2, 0), (0, 1), (0, 2), (0, 3))                        # (mask_reads, mask_seeds) of the exact comparisons
