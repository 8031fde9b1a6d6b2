"""Checker of the bias pass, kept apart from the library: a numpy restatement of the five histograms `bcftools mpileup`
feeds to its rank tests (bcf_call_glfgen, bcftools/bam2bcf.c:488-527, with get_position, :144-193), over the same reads
and reconciled qualities as the pileup tables of tests/geno_checks.py.  Which reads are in the pileup, the reconciliation of
overlapping mates and the late neighbour are not restated here: geno_checks.pileup_tables runs, and the Read objects it
builds (qualities as the reconciliation left them, late_idx / late_q) are taken from it.  Shares no code with panmap_amd.

Layout of one site's row (include/panmap_amd.h, PMX_PLB_*): pos [2][100], scl [2][100], mq [2][60], bq [2][60] by ref/alt,
mqs [2][60] by strand -- 760 counters."""
import numpy as np

import geno_checks as gc
from geno_checks import M, EQ, X, I, S, D, N

POS, SCL, MQ, BQ, MQS, CELLS = 0, 200, 400, 520, 640, 760
BLOCKS = dict(pos=(POS, 100), scl=(SCL, 100), mq=(MQ, 60), bq=(BQ, 60), mqs=(MQS, 60))
KEYS = ("VDB", "SGB", "RPBZ", "MQBZ", "MQSBZ", "BQBZ", "SCBZ", "MQ0F")


def _tables_and_reads(*args, **kw):
    """geno_checks.pileup_tables and the reads it admitted, as it left them"""
    reads, plain = {}, gc.Read

    class Kept(plain):
        def __init__(self, r, *a):
            super().__init__(r, *a)
            reads[r] = self

    gc.Read = Kept
    try:
        hist, aux, info = gc.pileup_tables(*args, **kw)
    finally:
        gc.Read = plain
    return hist, aux, info, reads


def position_of(i, length, c5, c3):
    """get_position (bam2bcf.c:144-193) + the scalings of :493-498 for the query bases i (an index array)
    -> (epos, sc_len, mask of the bases whose clip the reference leaves unset)"""
    i = np.asarray(i, np.int64)
    epos = ((i + 1 - c5).astype(np.float64) / (length - c5 - c3 + 1) * 99).astype(np.int64)
    left = i + 1 - c5 if c5 else np.full(i.shape, -1, np.int64)
    right = length - c3 - i if c3 else np.full(i.shape, -1, np.int64)
    take_left = (left >= 0) & ((right < 0) | (left < right))
    unset = (left >= 0) & ~take_left                            # both ends clipped, the right clip at least as near
    take_right = (left < 0) & (right >= 0)
    clip = np.where(take_left, c5, np.where(take_right, c3, 0))
    dist = np.where(take_left, left, np.where(take_right, right, 0))
    sc_len = np.minimum((15.0 * clip / (dist + 1)).astype(np.int64), 99)
    return epos, sc_len, unset


def bias_tables(recs, cig, concat, offsets, reference: bytes, paired, revcomp_mate2, rank, quals=None, names=None, max_depth=250, min_baseq=1,
                max_baseq=60, delta_baseq=30, cap_mapq=60):
    """-> hist, aux, info of geno_checks.pileup_tables, bias uint32 [ref_len, 760], bases that took the unset-clip branch"""
    ref_len = len(reference)
    hist, aux, info, reads = _tables_and_reads(recs, cig, concat, offsets, ref_len, paired, revcomp_mate2, rank, quals=quals, names=names,
                                               max_depth=max_depth, min_baseq=min_baseq, max_baseq=max_baseq, delta_baseq=delta_baseq,
                                               cap_mapq=cap_mapq)
    ref4 = np.full(256, 4, np.int64)
    for k, c in enumerate(b"ACGT"):
        ref4[c] = ref4[c + 32] = k
    ref4 = ref4[np.frombuffer(reference, np.uint8)]
    bias = np.zeros(ref_len * CELLS, np.uint32)
    n_unset = 0
    for rd in reads.values():
        mapq = min(rd.mapq if rd.mapq < 255 else 20, cap_mapq, 59)
        c5 = rd.cigar[0][1] if rd.cigar[0][0] == S else 0
        c3 = rd.cigar[-1][1] if len(rd.cigar) > 1 and rd.cigar[-1][0] == S else 0
        x, y = rd.rs, 0
        for op, ln in rd.cigar:
            if op in (M, EQ, X):
                n = max(min(ln, ref_len - x, rd.len - y), 0)
                i = np.arange(y, y + n)
                q = rd.q[i].copy()
                has_l = i > 0
                q[has_l] = np.minimum(q[has_l], rd.q[i[has_l] - 1] + delta_baseq)
                has_r = i + 1 < rd.len
                right = rd.q[np.minimum(i + 1, rd.len - 1)].copy()
                right[i == rd.late_idx] = rd.late_q
                q[has_r] = np.minimum(q[has_r], right[has_r] + delta_baseq)
                keep = q >= min_baseq
                i, p = i[keep], np.arange(x, x + n)[keep]
                bq = np.minimum(np.minimum(q[keep], max_baseq), 59)
                base = gc._B4[rd.code[i]]
                alt = np.where((ref4[p] < 4) & (base == ref4[p]), 0, 1)
                epos, sc_len, unset = position_of(i, rd.len, c5, c3)
                n_unset += int(unset.sum())
                for cell in (POS + alt * 100 + epos, SCL + alt * 100 + sc_len, MQ + alt * 60 + mapq, BQ + alt * 60 + bq, MQS + rd.strand * 60 + mapq):
                    bias[p * CELLS + cell] += 1                         # within one M run every p is distinct
                x += ln; y += ln
            elif op in (I, S):
                y += ln
            elif op in (D, N):
                x += ln
    return hist, aux, info, bias.reshape(ref_len, CELLS), n_unset


def golden_tests(line: str):
    """a `call` line -> (0-based position, {key: text} of the eight keys it carries), None when it has no alternative"""
    f = line.split("\t")
    if f[4] == ".":
        return None
    kv = dict(x.split("=", 1) for x in f[7].split(";") if "=" in x)
    return int(f[1]) - 1, {k: kv[k] for k in KEYS if k in kv}
