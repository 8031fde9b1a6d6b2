"""Checker of the genotype stage, kept apart from the library: a numpy restatement of the pileup rules of
`bcftools mpileup -B` (bcftools/mpileup.c:196-299, 1363-1384; htslib-1.20/sam.c:5750-6151; bcftools/bam2bcf.c:248-573) over
fetched alignment records, and a plain restatement of the htslib error model (htslib-1.20/errmod.c:51-208) and of
bcf_call_combine (bam2bcf.c:955-1115) with loops and math.lgamma.  Shares no table and no code with panmap_amd.

The BAM order of the records is an input (`rank`: place of every read in the BAM, 0xffffffff = not written): the reference
sorts with an unstable sort on the position alone, so the order of equal positions is a property of the file.
"""
import functools
import heapq
import math

import numpy as np

NONE = 0xffffffff
HAS_ALN = 4
M, I, D, N, S, H, P, EQ, X = range(9)


def name_keeps_first(qname: bytes) -> bool:
    """tweak_overlap_quality (sam.c:5853): Wang hash of the X31 string hash of the read name, lowest bit"""
    h = 0
    if qname:
        h = qname[0] if qname[0] < 128 else qname[0] - 256
        for c in qname[1:]:
            h = (h * 31 + (c if c < 128 else c - 256)) & 0xffffffff
        h &= 0xffffffff
    k = h
    k = (k + (~(k << 15) & 0xffffffff)) & 0xffffffff
    k ^= k >> 10
    k = (k + (k << 3)) & 0xffffffff
    k ^= k >> 6
    k = (k + (~(k << 11) & 0xffffffff)) & 0xffffffff
    k ^= k >> 16
    return bool(k & 1)


_CODE = np.full(256, 15, np.uint8)
for _c, _v in zip(b"ACGT", (1, 2, 4, 8)):
    _CODE[_c] = _v
    _CODE[_c + 32] = _v
# what the BAM holds for a letter (build_bam_from_result, src/conversion.cpp:288-388; htslib's seq_nt16_table): a read placed as
# given keeps every code of "=ACMGRSVTWYHKDBN", either case; a read placed on the other strand has A C G T of either case
# complemented and N for every other letter.  A mate 2 the pipeline reverse-complements first (seeding::reverseComplement,
# src/seeding.cpp:271-284) has only its upper-case A C G T complemented by that step.  ('=' in a read is not modelled.)
_NT16 = np.full(256, 15, np.uint8)
for _v, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _NT16[_c] = _v
    if _c != ord("="):
        _NT16[_c + 32] = _v
_NT16_OTHER_STRAND = np.full(256, 15, np.uint8)
for _c, _v in zip(b"ACGT", (8, 4, 2, 1)):
    _NT16_OTHER_STRAND[_c] = _NT16_OTHER_STRAND[_c + 32] = _v
_RC_UPPER = np.arange(256, dtype=np.uint8)
_RC_UPPER[list(b"ACGT")] = list(b"TGCA")
_B4 = np.full(16, 4, np.int64)
_B4[[1, 2, 4, 8]] = [0, 1, 2, 3]


class Read:
    """one record as the BAM shows it (build_bam_from_result, src/conversion.cpp:288-388)"""

    def __init__(self, r, rec, cig, concat, offsets, quals, paired, revcomp_mate2):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        self.r, self.len = r, hi - lo
        self.rs, self.re, self.rev, self.mapq = int(rec["rs"]), int(rec["re"]), int(rec["rev"]), int(rec["mapq"])
        qs, qe = int(rec["qs"]), int(rec["qe"])
        c5 = self.len - qe if self.rev else qs
        c3 = qs if self.rev else self.len - qe
        ops = [(int(x) & 0xf, int(x) >> 4) for x in cig[int(rec["cigar_off"]):int(rec["cigar_off"]) + int(rec["n_cigar"])]]
        self.cigar = ([(S, c5)] if c5 > 0 else []) + ops + ([(S, c3)] if c3 > 0 else [])
        m2 = bool(revcomp_mate2 and (r & 1))
        flip = m2 != bool(self.rev)
        given = _RC_UPPER[concat[lo:hi][::-1]] if m2 else concat[lo:hi]
        code = _NT16_OTHER_STRAND[given[::-1]] if self.rev else _NT16[given]
        q = np.full(self.len, ord("I"), np.int64) if quals is None else quals[lo:hi].astype(np.int64)
        q[q == 0] = ord("I")
        q = np.maximum(q - 33, 0)
        if flip:
            q = q[::-1]
        self.code, self.q = code.copy(), q.copy()
        self.strand = (0 if self.rev else 1) if (paired and (r & 1)) else (1 if self.rev else 0)
        self.late_idx, self.late_q = -1, 0


class _Walk:
    """cigar_iref2iseq_set / _next (sam.c:5750-5816)"""

    def __init__(self, read, iref):
        self.c, self.ci, self.icig, self.iseq, self.iref = read.cigar, 0, 0, 0, iref
        self.ret = self._set()

    def _set(self):
        pos = self.iref
        if pos < 0:
            return -1
        self.icig = self.iseq = self.iref = 0
        while self.ci < len(self.c):
            op, n = self.c[self.ci]
            if op == S:
                self.ci += 1; self.iseq += n; self.icig = 0
            elif op in (H, P):
                self.ci += 1; self.icig = 0
            elif op in (M, EQ, X):
                pos -= n
                if pos < 0:
                    self.icig = n + pos; self.iseq += self.icig; self.iref += self.icig
                    return 0
                self.ci += 1; self.iseq += n; self.icig = 0; self.iref += n
            elif op == I:
                self.ci += 1; self.iseq += n; self.icig = 0
            elif op in (D, N):
                pos -= n
                if pos < 0:
                    pos = 0
                self.ci += 1; self.icig = 0; self.iref += n
            else:
                return -2
        self.iseq = -1
        return -1

    def next(self):
        while self.ci < len(self.c):
            op, n = self.c[self.ci]
            if op in (M, EQ, X):
                if self.icig >= n - 1:
                    self.icig = -1; self.ci += 1
                    continue
                self.iseq += 1; self.icig += 1; self.iref += 1
                self.ret = 0
                return 0
            if op in (D, N):
                self.ci += 1; self.iref += n; self.icig = -1
            elif op in (I, S):
                self.ci += 1; self.iseq += n; self.icig = -1
            elif op in (H, P):
                self.ci += 1; self.icig = -1
            else:
                self.ret = -2
                return -2
        self.iseq = -1; self.iref = -1; self.ret = -1
        return -1

    def prev_is_del(self):
        return self.ci > 0 and self.c[self.ci - 1][0] == D


def reconcile(a: Read, b: Read, a_keeps: bool, seen=None):
    """tweak_overlap_quality (sam.c:5824-5963): a came first in the BAM.  `seen`: a dict that counts the branches taken
    (for the preconditions of the crafted fixtures)"""
    def note(what):
        if seen is not None:
            seen[what] = seen.get(what, 0) + 1
    amul, bmul = (1, 0) if a_keeps else (0, 1)
    iref = b.rs
    wa = _Walk(a, iref - a.rs)
    if wa.ret < 0:
        return
    wb = _Walk(b, iref - b.rs)
    if wb.ret < 0:
        return
    while True:
        while wa.ret >= 0 and wa.iref >= 0 and wa.iref < iref - a.rs:
            wa.next()
        if wa.ret < 0:
            break
        while wb.ret >= 0 and wb.iref >= 0 and wb.iref < iref - b.rs:
            wb.next()
        if wb.ret < 0:
            break
        iref = max(iref, wa.iref + a.rs, wb.iref + b.rs) + 1
        if wa.iref + a.rs != wb.iref + b.rs:
            if wa.iref + a.rs < wb.iref + b.rs and wb.prev_is_del():
                note("deletion in b")
                while True:
                    if wa.iseq >= a.len:
                        return
                    a.q[wa.iseq] = a.q[wa.iseq] * 4 // 5 if amul else 0
                    if wa.next() < 0:
                        return
                    if not wa.iref + a.rs < wb.iref + b.rs:
                        break
            elif wa.prev_is_del():
                note("deletion in a")
                while True:
                    if wb.iseq >= b.len:
                        return
                    b.q[wb.iseq] = b.q[wb.iseq] * 4 // 5 if bmul else 0
                    if wb.next() < 0:
                        return
                    if not wb.iref + b.rs < wa.iref + a.rs:
                        break
            else:
                note("unequal positions skipped")
                continue
        if wa.iseq >= a.len or wb.iseq >= b.len:
            return
        qa, qb = int(a.q[wa.iseq]), int(b.q[wb.iseq])
        if a.code[wa.iseq] == b.code[wb.iseq]:
            note("agree, a keeps" if a_keeps else "agree, b keeps")
            s = min(qa + qb, 200)
            a.q[wa.iseq], b.q[wb.iseq] = amul * s, bmul * s
        elif qa > qb:
            note("differ, a better")
            a.q[wa.iseq], b.q[wb.iseq] = qa * 4 // 5, 0
        elif qa < qb:
            note("differ, b better")
            b.q[wb.iseq], a.q[wa.iseq] = qb * 4 // 5, 0
        else:
            note("differ, equal quality")
            a.q[wa.iseq], b.q[wb.iseq] = amul * (qa * 4 // 5), bmul * (qb * 4 // 5)


def features(recs, cig, concat, offsets, paired):
    """which rules the records exercise (for the tests' own precondition)"""
    f = dict(soft_clip=0, insertion=0, deletion=0, n_base=0, improper=0)
    for r, rec in enumerate(recs):
        if not rec["mapped"] or not rec["flags"] & HAS_ALN:
            continue
        ln = int(offsets[r + 1] - offsets[r])
        if rec["qs"] > 0 or rec["qe"] < ln:
            f["soft_clip"] += 1
        ops = [int(x) & 0xf for x in cig[int(rec["cigar_off"]):int(rec["cigar_off"]) + int(rec["n_cigar"])]]
        f["insertion"] += I in ops
        f["deletion"] += D in ops
        f["n_base"] += bool((_CODE[concat[int(offsets[r]):int(offsets[r + 1])]] == 15).any())
        f["improper"] += bool(paired and not rec["proper_frag"])
    return f


def pileup_tables(recs, cig, concat, offsets, ref_len, paired, revcomp_mate2, rank, quals=None, names=None, max_depth=250, min_baseq=1,
                  max_baseq=60, delta_baseq=30, cap_mapq=60):
    """-> hist uint32 [ref_len, 64, 2, 5], aux uint32 [ref_len, 4], info dict (admitted mask, refused by the cap, reconciled pairs)"""
    concat = np.frombuffer(concat, np.uint8) if isinstance(concat, (bytes, bytearray)) else np.asarray(concat, np.uint8)
    if quals is not None:
        quals = np.frombuffer(quals, np.uint8) if isinstance(quals, (bytes, bytearray)) else np.asarray(quals, np.uint8)
    n = len(recs)
    rank = np.asarray(rank, np.uint32)
    order = [int(r) for r in np.argsort(rank, kind="stable") if rank[r] != NONE]
    # mplp_func's filters, then the depth cap of bam_plp_push in BAM order
    admitted, refused = np.zeros(n, bool), 0
    live, last_start = [], -1
    adm_order, adm_start = [], []
    for r in order:
        rec = recs[r]
        if not rec["mapped"] or not rec["flags"] & HAS_ALN:
            continue
        if paired and not rec["proper_frag"]:
            continue                                            # MPLP_NO_ORPHAN (mpileup.c:294)
        rs, re = int(rec["rs"]), int(rec["re"])
        if rs >= ref_len:
            continue                                            # mpileup.c:239-243
        if max_depth > 0 and rs == last_start:                  # sam.c:6104: the pileup stands at this start already
            while live and live[0] < rs:                        # (bam_plp64_next freed the reads with end <= rs - 1)
                heapq.heappop(live)
            if len(live) + 1 > max_depth:                       # + the list's tail node
                refused += 1
                continue
        last_start = rs
        admitted[r] = True
        heapq.heappush(live, re)
        adm_order.append(r)
        adm_start.append(rs)
    adm_start = np.asarray(adm_start, np.int64)
    reads = {r: Read(r, recs[r], cig, concat, offsets, quals, paired, revcomp_mate2) for r in adm_order}
    n_reconciled, late_reads, branches = 0, [], {}
    if paired:
        for u in range(0, n - 1, 2):
            if not (admitted[u] and admitted[u + 1]):
                continue                                        # overlap_push: both mates pushed (and proper: they are)
            ra, rb = (u, u + 1) if rank[u] < rank[u + 1] else (u + 1, u)
            a, b = reads[ra], reads[rb]
            qname = bytes(names[ra]) if names is not None else b"r%d" % ra
            if len(qname) >= 2 and qname[-2:] in (b"/1", b"/2"):
                qname = qname[:-2]
            # the last base of a in front of b's start and its right neighbour, before the reconciliation
            x, y, p_last, q_last = a.rs, 0, -1, -1
            for op, ln in a.cigar:
                if x >= b.rs:
                    break
                if op in (M, EQ, X):
                    cover = min(ln, b.rs - x)
                    p_last, q_last = x + cover - 1, y + cover - 1
                    x += ln; y += ln
                elif op in (I, S):
                    y += ln
                elif op in (D, N):
                    x += ln
            neighbour = int(a.q[q_last + 1]) if q_last >= 0 and q_last + 1 < a.len else None
            reconcile(a, b, name_keeps_first(qname), branches)
            n_reconciled += 1
            if neighbour is not None:
                # the position is piled up when the first admitted read that starts behind it is pushed (sam.c:6034); the
                # neighbour is reconciled by then only if that read is b
                j = int(np.searchsorted(adm_start, p_last + 1, "left"))
                first = adm_order[j] if j < len(adm_order) else -1
                if first != rb:
                    a.late_idx, a.late_q = q_last, neighbour
                    late_reads.append(ra)
    hist = np.zeros((ref_len, 64, 2, 5), np.uint32)
    aux = np.zeros((ref_len, 4), np.uint32)
    for r in adm_order:
        rd = reads[r]
        mapq = rd.mapq if rd.mapq < 255 else 20
        mq0 = mapq == 0
        mapq = min(mapq, cap_mapq)
        x, y = rd.rs, 0
        for op, ln in rd.cigar:
            if op in (M, EQ, X):
                ln_eff = min(ln, ref_len - x, rd.len - y)
                idx = np.arange(y, y + ln_eff)
                pos = np.arange(x, x + ln_eff)
                q = rd.q[idx].copy()
                has_l = idx > 0
                q[has_l] = np.minimum(q[has_l], rd.q[idx[has_l] - 1] + delta_baseq)
                has_r = idx + 1 < rd.len
                right = rd.q[np.minimum(idx + 1, rd.len - 1)].copy()
                if rd.late_idx >= 0:
                    right[idx == rd.late_idx] = rd.late_q
                q[has_r] = np.minimum(q[has_r], right[has_r] + delta_baseq)
                aux[pos, 0] += 1
                keep = q >= min_baseq
                q = np.maximum(np.minimum(np.minimum(np.minimum(q, max_baseq), mapq), 63), 4)
                hist[pos[keep], q[keep], rd.strand, _B4[rd.code[idx[keep]]]] += 1
                aux[pos[keep], 1] += mapq
                if mq0:
                    aux[pos[keep], 2] += 1
                x += ln; y += ln
            elif op in (I, S):
                y += ln
            elif op == D:
                aux[x:min(x + ln, ref_len), 3] += 1
                x += ln
            elif op == N:
                x += ln
    return hist, aux, dict(admitted=admitted, refused_by_cap=refused, reconciled_pairs=n_reconciled, late_neighbours=len(late_reads), late_reads=late_reads,
                           branches=branches)


# ------------------------------------------------------------------------------------------------ error model
def _lbinom(n, k):
    return 0.0 if k <= 0 or k > n else math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


@functools.lru_cache(maxsize=None)
def _beta_row(q, n):
    """cal_coef (errmod.c:86-99) for one (quality, depth); the row is read, never written"""
    e = 10.0 ** (-q / 10.0)
    le, le1 = math.log(e), math.log(1.0 - e)
    row = [0.0] * (n + 1)
    row[n] = math.inf
    sum1 = _lbinom(n, n) + n * le
    for k in range(n - 1, -1, -1):
        s = sum1 + math.log1p(math.exp(_lbinom(n, k) + k * le + (n - k) * le1 - sum1))
        row[k] = -10.0 / math.log(10.0) * (sum1 - s)
        sum1 = s
    return row


def errmod_cal(hist):
    """errmod_cal (errmod.c:143-208), m = 5, over the bases of one hist[pos]; float32 where the reference holds floats.
    More than 255 bases: every (quality, strand, base) class keeps floor(count * 255 / n), the rest goes to the largest
    remainders, higher class code first (the library's stated rule; the reference draws at random)."""
    hist = np.asarray(hist).reshape(64, 2, 5)
    classes = [[q << 5 | s << 4 | b, int(hist[q, s, b])] for q in range(64) for s in range(2) for b in range(5) if hist[q, s, b]]
    n_all = sum(c for _, c in classes)
    out = np.zeros((5, 5), np.float32)
    if n_all == 0:
        return out
    n = min(n_all, 255)
    if n_all > 255:
        rem = sorted(range(len(classes)), key=lambda i: (-(classes[i][1] * 255 % n_all), -i))
        for cl in classes:
            cl[1] = cl[1] * 255 // n_all
        for i in rem[:255 - sum(c for _, c in classes)]:
            classes[i][1] += 1
    fsum, bsum, c, w = [0.0] * 5, [0.0] * 5, [0] * 5, [0] * 32
    rows = {}
    for code, cnt in reversed(classes):
        qual = min(max(code >> 5, 4), 63)
        beta = rows.setdefault(qual, _beta_row(qual, n))
        bs, base = code & 0x1f, code & 0xf
        for _ in range(cnt):
            f = 1.0 if w[bs] == 0 else (1.0 - 0.17) ** w[bs] * (1.0 - 0.03) + 0.03
            fsum[base] += f
            bsum[base] += f * beta[c[base]]
            c[base] += 1
            w[bs] += 1
    f32 = np.float32
    for j in range(5):
        t1, t2 = f32(0), 0
        for k in range(5):
            if k != j:
                t1 = f32(float(t1) + bsum[k]); t2 += c[k]
        if t2:
            out[j, j] = t1
        for k in range(j + 1, 5):
            cjk = c[j] + c[k]
            t1, t2 = f32(0), 0
            for i in range(5):
                if i != j and i != k:
                    t1 = f32(float(t1) + bsum[i]); t2 += c[i]
            lhet = _lbinom(cjk, c[k]) - math.log(2.0) * cjk
            out[j, k] = out[k, j] = f32(-4.343 * lhet + float(t1)) if t2 else f32(-4.343 * lhet)
        for k in range(5):
            if out[j, k] < 0:
                out[j, k] = 0
    return out


def site(hist, ref_base: bytes):
    """bcf_call_combine (bam2bcf.c:955-1046) for one sample -> alleles (reference first, then by falling quality sum), the
    homozygotes' PL as mpileup scales them, AD, DP4"""
    hist = np.asarray(hist).reshape(64, 2, 5).astype(np.int64)
    p = errmod_cal(hist)
    ref4 = b"ACGT".find(ref_base.upper()[:1])
    ref4 = 4 if ref4 < 0 else ref4
    qs = [int((hist[:, :, b].sum(axis=1) * np.arange(64)).sum()) for b in range(4)]
    f32 = np.float32
    tot = f32(0)
    for v in qs:
        tot = f32(tot + f32(v))
    qsum = [f32(0)] * 4
    if tot != 0:
        qsum = [f32(f32(v) / tot) for v in qs]
    order = [0, 1, 2, 3]
    for i in range(1, 4):
        j = i
        while j > 0 and qsum[order[j]] < qsum[order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    al, i = [ref4], 3
    while i >= 0:
        if order[i] != ref4:
            if qsum[order[i]] == 0:
                break
            al.append(order[i])
        i -= 1
    n_seen = len(al)
    if ((ref4 < 4 and len(al) < 4) or (ref4 == 4 and len(al) < 5)) and i >= 0:
        al.append(order[i])                                    # the unseen allele takes part in the minimum
    mn = min(p[al[y], al[x]] for x in range(len(al)) for y in range(x + 1))
    pl = [min(int(float(f32(p[a, a] - mn)) + .499), 255) for a in al[:n_seen]]
    ad = [int(hist[:, :, a].sum()) for a in al[:n_seen]]
    dp4 = [0, 0, 0, 0]
    for b in range(5):
        for s in range(2):
            dp4[(0 if (ref4 < 4 and b == ref4) else 2) + s] += int(hist[:, s, b].sum())
    return dict(alleles=al[:n_seen], pl=pl, ad=ad, dp4=dp4)


# ------------------------------------------------------------------------------------------------ glue for the tests
REC_DTYPE = np.dtype([("rs", "<i4"), ("re", "<i4"), ("qs", "<i4"), ("qe", "<i4"), ("mapq", "u1"), ("rev", "u1"), ("proper_frag", "u1"),
                      ("mapped", "u1"), ("n_cigar", "<u2"), ("flags", "<u2"), ("cigar_off", "<u4"), ("score", "<i4")])


def results_to_records(results, paired):
    """align_pair_result_t-shaped dicts (oracle.ref_align_reads_direct) -> 32-byte records + CIGAR arena"""
    n = len(results) * (2 if paired else 1)
    recs, cig = np.zeros(n, REC_DTYPE), []
    for k, res in enumerate(results):
        for m, key in enumerate(("r1", "r2") if paired else ("r1",)):
            a, r = res[key], (2 * k + m if paired else k)
            if not res["mapped"] or a["pos"] == 2147483647:
                continue
            recs[r] = (a["rs"], a["re"], a["qs"], a["qe"], a["mapq"], a["rev"], a["proper_frag"], 1, len(a["cigar"]), HAS_ALN, len(cig), 0)
            cig.extend(a["cigar"])
        if paired and res["mapped"]:
            recs[2 * k]["mapped"] = recs[2 * k + 1]["mapped"] = 1
    return recs, np.asarray(cig if cig else [0], np.uint32)


def rank_from_bam(bam_records, names, paired):
    """place of every read in a parsed BAM (test_bam.parse_bam): records are told apart by name and the READ2 flag"""
    where = {}
    for k, rec in enumerate(bam_records):
        where[(rec["name"], bool(rec["flag"] & 0x80))] = k
    rank = np.full(len(names), NONE, np.uint32)
    for r, nm in enumerate(names):
        nm = nm.decode() if isinstance(nm, bytes) else nm
        if len(nm) >= 2 and nm[-2:] in ("/1", "/2"):
            nm = nm[:-2]
        k = where.get((nm, bool(paired and (r & 1))))
        if k is not None:
            rank[r] = k
    return rank
