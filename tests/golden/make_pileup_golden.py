#!/usr/bin/env python3
"""Generates the recorded results of the genotype stage: what the REFERENCE's own `bcftools mpileup -B` and
`bcftools call --ploidy 1 -m -A` (oracle/_ref/ref_bcftools, built by oracle/Makefile from the reference tree) say about

  * the README demo reads as the compiled reference aligner places them      -> pileup_demo_golden.json.gz
  * crafted read sets on a 300 bp reference (12.5 windows of the device pileup) -> pileup_crafted_golden.json.gz
    whose inputs are committed as data too                                      -> pileup_crafted_inputs.json.gz

Per mpileup record that is not an INDEL: POS, REF, ALT, DP, I16[0..3], I16[8], I16[10], QS, MQ0F, PL, AD; per `call` record
that is not an INDEL: the line.  Every set asserts that it exercises what it is for, and that no position holds more than
255 counted bases (beyond that the reference samples at random).  CPU only.

    python3 tests/golden/make_pileup_golden.py            # all three files
    python3 tests/golden/make_pileup_golden.py crafted    # the crafted sets only
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import geno_checks as gc          # noqa: E402
import pileup_golden as pg        # noqa: E402

REF_BCFTOOLS = os.path.join(ROOT, "oracle", "_ref", "ref_bcftools")
OPS = "MIDNSHP=X"
MAPQS = (0, 1, 13, 20, 37, 60, 255)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def parse_cigar(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((OPS.index(ch), int(n)))
            n = ""
    return out


# ------------------------------------------------------------------------------------------------ building a set
class SetBuilder:
    """collects reads given in BAM terms (start, CIGAR with its soft clips, bases and qualities in reference orientation)
    and states them as the library takes them: records + CIGAR arena, reads and qualities as given to the aligner"""

    def __init__(self, ref: bytes, paired: bool, seed: int):
        self.ref, self.paired = ref, paired
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.err = 0.0                                           # substitutions in the bases this builder makes up
        self.recs, self.cig, self.reads, self.quals, self.names = [], [], [], [], []

    def bases(self, rs, ops, template=None, err=0.0, n_rate=0.0):
        """the read's bases in reference orientation: M = X copy the template (X: another base), I S are random"""
        t = template or self.ref
        out, x = bytearray(), rs
        for op, n in ops:
            if op in (gc.M, gc.EQ, gc.X):
                for k in range(n):
                    c = t[x + k] if x + k < len(t) else ord("A")
                    if op == gc.X or (op == gc.M and err and self.rng.random() < err):
                        c = b"ACGT"[(b"ACGT".find(bytes([c]).upper()) + 1 + int(self.rng.integers(3))) % 4]
                    out.append(c)
                x += n
            elif op in (gc.I, gc.S):
                out += bytes(b"ACGT"[int(i)] for i in self.rng.integers(0, 4, n))
            elif op in (gc.D, gc.N):
                x += n
        for k in range(len(out)):
            if n_rate and self.rng.random() < n_rate:
                out[k] = ord("N")
        return bytes(out)

    def quality(self, n, lo=25, hi=41):
        return bytes(int(q) + 33 for q in self.rng.integers(lo, hi + 1, n))

    def _one(self, rs, cigar, seq, qual, mapq, rev, proper, mapped=1):
        ops = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
        c5 = ops[0][1] if ops and ops[0][0] == gc.S else 0
        c3 = ops[-1][1] if len(ops) > 1 and ops[-1][0] == gc.S else 0
        inner = ops[(1 if c5 else 0):(len(ops) - 1 if c3 else len(ops))]
        if seq is None:
            seq = self.bases(rs, ops, err=self.err)
        if qual is None:
            qual = self.quality(len(seq))
        qlen = sum(n for op, n in ops if op in (gc.M, gc.EQ, gc.X, gc.I, gc.S))
        assert len(seq) == qlen == len(qual), (cigar, len(seq), qlen, len(qual))
        re = rs + sum(n for op, n in inner if op in (gc.M, gc.EQ, gc.X, gc.D, gc.N))
        assert 0 <= rs < re <= len(self.ref), (rs, re, cigar)
        qs, qe = (c3, qlen - c5) if rev else (c5, qlen - c3)
        # as given to the aligner: a read placed on the other strand is the reverse complement of what the BAM shows
        given, gq = (seq.translate(_COMP)[::-1], qual[::-1]) if rev else (seq, qual)
        self.recs.append([rs, re, qs, qe, mapq, int(rev), int(proper), mapped, len(inner), gc.HAS_ALN, len(self.cig), 0])
        self.cig.extend(n << 4 | op for op, n in inner)
        self.reads.append(given)
        self.quals.append(gq)

    def pair(self, name, a, b, mapq=60, proper=1, rev=0, name2=None):
        """a, b: (start, cigar[, bases[, qualities]]) of mate 1 and mate 2"""
        for m, spec in enumerate((a, b)):
            spec = tuple(spec) + (None,) * (4 - len(spec))
            mq = mapq[m] if isinstance(mapq, tuple) else mapq
            self._one(spec[0], spec[1], spec[2], spec[3], mq, rev, proper)
            self.names.append(name if m == 0 or name2 is None else name2)

    def unmapped_pair(self, name, length=50):
        for _ in range(2):
            self.recs.append([0] * 12)
            self.reads.append(self.bases(0, [(gc.S, length)]))
            self.quals.append(self.quality(length))
            self.names.append(name)

    def single(self, name, rs, cigar, seq=None, qual=None, mapq=60, rev=0):
        self._one(rs, cigar, seq, qual, mapq, rev, 0)
        self.names.append(name)

    def inputs(self):
        return dict(ref=self.ref.decode(), paired=int(self.paired), recs=self.recs, cig=[int(x) for x in self.cig] or [0],
                    reads=[x.decode("latin-1") for x in self.reads], quals=[x.hex() for x in self.quals],
                    names=[x.decode("latin-1") for x in self.names])


def reference_300(seed=300):
    rng = np.random.Generator(np.random.PCG64(seed))
    return bytes(b"ACGT"[int(i)] for i in rng.integers(0, 4, 300))


def random_cigar(rng, length):
    """M / I / D runs with soft clips now and then, `length` query bases"""
    ops, left = [], length
    c5 = int(rng.integers(1, 9)) if rng.random() < 0.25 else 0
    c3 = int(rng.integers(1, 9)) if rng.random() < 0.25 else 0
    left -= c5 + c3
    if c5:
        ops.append((gc.S, c5))
    while left > 0:
        m = int(min(left, rng.integers(5, 60)))
        ops.append((gc.M, m))
        left -= m
        if left > 6 and rng.random() < 0.5:
            if rng.random() < 0.5:
                i = int(rng.integers(1, 5))
                ops.append((gc.I, i))
                left -= i
            else:
                ops.append((gc.D, int(rng.integers(1, 8))))
    if ops[-1][0] != gc.M:
        ops.pop()
        if not ops or ops[-1][0] != gc.M:
            ops.append((gc.M, 3))
    if c3:
        ops.append((gc.S, c3))
    return ops


def ref_span(ops):
    return sum(n for op, n in ops if op in (gc.M, gc.EQ, gc.X, gc.D, gc.N))


def random_pairs(ref, n_pairs, seed, planted=None):
    """seeded pairs: M / I / D CIGARs, soft clips, 2 % N, overlapping mates (mate 2 starts between rs1 - 3 and re1 + 10),
    5 % improper, qualities 0..93 for half the reads and 25..41 for the other half, mapQ from MAPQS, a few pairs placed on
    the other strand and a few unmapped.  planted: {position: (fraction, alt, second alt)} substitutions of the sample"""
    sb = SetBuilder(ref, True, seed)
    rng = sb.rng
    k = 0
    while k < n_pairs:
        l1, l2 = int(rng.integers(30, 121)), int(rng.integers(30, 121))
        o1, o2 = random_cigar(rng, l1), random_cigar(rng, l2)
        rs1 = int(rng.integers(0, len(ref) - 20))
        re1 = rs1 + ref_span(o1)
        rs2 = int(rng.integers(rs1 - 3, re1 + 11))
        if rs2 < 0 or re1 > len(ref) or rs2 + ref_span(o2) > len(ref):
            continue
        if rng.random() < 0.02:
            sb.unmapped_pair(b"p%d" % k)
            k += 1
            continue
        template = bytearray(ref)
        for p, (frac, alt, alt2) in (planted or {}).items():
            u = rng.random()
            if u < frac:
                template[p] = alt
            elif u < frac + 0.1:
                template[p] = alt2
        specs = []
        for rs, ops in ((rs1, o1), (rs2, o2)):
            seq = sb.bases(rs, ops, bytes(template), err=0.01, n_rate=0.02)
            qual = sb.quality(len(seq), 0, 93) if rng.random() < 0.5 else sb.quality(len(seq), 25, 41)
            specs.append((rs, ops, seq, qual))
        sb.pair(b"p%d" % k, specs[0], specs[1], mapq=(MAPQS[int(rng.integers(len(MAPQS)))], MAPQS[int(rng.integers(len(MAPQS)))]),
                proper=0 if rng.random() < 0.05 else 1, rev=1 if rng.random() < 0.1 else 0)
        k += 1
    return sb


def planted_variants(ref):
    fracs = (0.35, 0.5, 0.6, 0.8, 1.0)
    out = {}
    for j, p in enumerate(range(3, len(ref), 7)):
        r = b"ACGT".find(ref[p:p + 1])
        out[p] = (fracs[j % 5], b"ACGT"[(r + 1 + j % 3) % 4], b"ACGT"[(r + 2 + j % 3) % 4 if (r + 2 + j % 3) % 4 != r else (r + 3) % 4])
    return out


def single_reads(ref, seed=150):
    sb = SetBuilder(ref, False, seed)
    rng = sb.rng
    k = 0
    while k < 150:
        ops = random_cigar(rng, int(rng.integers(30, 201)))
        rs = int(rng.integers(0, len(ref) - 20))
        if rs + ref_span(ops) > len(ref):
            continue
        seq = sb.bases(rs, ops, err=0.02, n_rate=0.02)
        sb.single(b"s%d" % k, rs, ops, seq, sb.quality(len(seq), 0, 93) if k % 2 else sb.quality(len(seq)), mapq=MAPQS[int(rng.integers(len(MAPQS)))],
                  rev=int(rng.random() < 0.5))
        k += 1
    return sb


def cap_pairs(ref):
    """40 pairs starting at one position and 20 at the next: -d 8 refuses reads, the default depth none"""
    sb = SetBuilder(ref, True, 8)
    for k in range(60):
        d = 0 if k < 40 else 1
        a, b = (100 + d, "50M"), (120 + d, "50M")
        seq = [sb.bases(s, parse_cigar(c), err=0.03) for s, c in (a, b)]
        sb.pair(b"c%d" % k, a + (seq[0],), b + (seq[1],))
    return sb


def edge_pairs(ref):
    """hand-written pairs, one property each (windows of the device pileup end at multiples of 24)"""
    sb = SetBuilder(ref, True, 24)
    sb.err = 0.1   # one base in ten differs from the reference: a quality shows in QS and PL only where a site has two alleles
    q = lambda n, v: bytes([v]) * n                              # noqa: E731
    P = sb.pair
    P(b"start0", (0, "40M"), (20, "40M"))
    P(b"end_at_ref_len", (232, "40M"), (260, "40M"))
    P(b"cross_23_24", (10, "30M"), (22, "30M"))
    P(b"one_base_each_side", (23, "2M"), (47, "2M"))
    P(b"ins_at_window_end", (30, "18M3I20M"), (40, "8M2I30M"))
    P(b"del_over_window_end", (60, "10M5D30M"), (93, "30M"))
    P(b"del_covers_windows", (101, "15M60D20M"), (171, "30M"))
    P(b"del_in_first_mate", (180, "20M6D20M"), (191, "40M"))
    P(b"del_in_second_mate", (185, "40M"), (196, "10M6D25M"))
    P(b"del_in_both", (201, "20M4D20M"), (211, "10M4D30M"))
    P(b"del_in_both_shifted", (203, "20M5D20M"), (213, "12M5D30M"))
    P(b"mate2_starts_first", (175, "30M"), (160, "30M"))
    P(b"mate2_starts_first_del", (100, "30M"), (90, "12M4D20M"))
    P(b"same_start", (130, "35M"), (130, "30M"))
    P(b"same_start_b_longer", (133, "20M"), (133, "45M"))
    # the last base of a in front of b looks at a neighbour that b's arrival changes: b alone at its start, b behind another
    # read with that start, b behind a deletion of a with and without a read starting under the deletion
    # (a's base in front of b is good, its neighbour poor: the neighbour's quality + 30 caps it before the reconciliation only)
    lq = lambda n, i: q(i, 33 + 40) + q(1, 33 + 2) + q(n - i - 1, 33 + 40)   # noqa: E731
    b38 = lambda n: q(n, 33 + 38)                                # noqa: E731

    def mm(rs, cigar, i):   # that base differs from the reference, so its quality shows in QS and PL of the site
        seq = bytearray(sb.bases(rs, parse_cigar(cigar), err=sb.err))
        seq[i] = b"ACGT"[(b"ACGT".find(bytes([seq[i]])) + 2) % 4]
        return bytes(seq)
    P(b"late_alone", (236, "30M", mm(236, "30M", 12), lq(30, 13)), (249, "30M", None, b38(30)))
    P(b"late_alone_too", (150, "30M", mm(150, "30M", 14), lq(30, 15)), (165, "30M", None, b38(30)))
    P(b"late_third_too", (153, "30M", mm(153, "30M", 14), lq(30, 15)), (168, "30M", None, b38(30)))
    P(b"late_third_too_same_start", (168, "20M"), (190, "20M"))
    P(b"late_third_same_start", (253, "20M"), (280, "20M"))
    P(b"late_third", (238, "30M", mm(238, "30M", 14), lq(30, 15)), (253, "30M", None, b38(30)))
    P(b"late_del_alone", (2, "10M3D20M", mm(2, "10M3D20M", 9), lq(30, 10)), (15, "25M", None, b38(25)))
    P(b"late_del_third", (50, "10M3D20M", mm(50, "10M3D20M", 9), lq(30, 10)), (63, "25M", None, b38(25)))
    P(b"late_del_third_inside", (61, "20M"), (95, "20M"))
    P(b"b_after_last_base", (110, "20M"), (130, "20M"))
    P(b"b_after_last_base_clip", (112, "20M6S"), (132, "20M"))
    P(b"b_one_later_clip", (114, "20M6S"), (135, "20M"))
    P(b"b_in_soft_clip", (20, "25M10S"), (48, "30M"))
    P(b"b_in_soft_clip_5prime", (70, "6S25M"), (72, "8S30M"))
    P(b"ops_eq_x_n", (100, "10=1X10=5N10M"), (112, "20M"))
    P(b"ops_n_in_second", (140, "40M"), (150, "10M7N20M"))
    P(b"ops_pad", (160, "12M2P13M"), (170, "20M"))
    P(b"qual_zero_bytes", (30, "30M", None, q(30, 0)), (45, "30M", None, q(30, 0)))
    P(b"qual_zero_tail", (32, "30M", None, sb.quality(12) + q(18, 0)), (47, "30M"))
    P(b"qual_bang", (34, "30M", None, q(30, ord("!"))), (49, "30M", None, q(15, ord("!")) + q(15, ord("5"))))
    P(b"qual_tilde", (36, "30M", None, q(30, ord("~"))), (51, "30M", None, q(30, ord("~"))))
    P(b"qual_steps", (38, "30M", None, bytes([33 + (3 * i) % 94 for i in range(30)])), (53, "30M", None, bytes([33 + (7 * i) % 94 for i in range(30)])))
    P(b"mapq_0", (215, "30M"), (230, "30M"), mapq=0)
    P(b"mapq_0_and_60", (217, "30M"), (232, "30M"), mapq=(0, 60))
    P(b"mapq_59", (219, "30M"), (234, "30M"), mapq=59)
    P(b"mapq_60", (221, "30M"), (236, "30M"), mapq=60)
    P(b"mapq_255", (223, "30M"), (238, "30M"), mapq=255)
    P(b"mapq_255_and_13", (225, "30M"), (240, "30M"), mapq=(255, 13))
    P(b"all_n", (80, "30M", b"N" * 30), (95, "30M"))
    P(b"all_n_both", (82, "30M", b"N" * 30), (97, "30M", b"N" * 30))
    P(b"lower_case", (84, "30M", ref[84:114].lower()), (99, "30M", ref[99:129].lower()))
    # bases that differ between the mates at equal, higher and lower quality
    a, b = bytearray(ref[260:290]), bytearray(ref[270:300])
    for i in (12, 14, 16):
        a[i] = b"ACGT"[(b"ACGT".find(bytes([a[i]])) + 1) % 4]
    qa, qb = bytearray(q(30, 33 + 30)), bytearray(q(30, 33 + 30))
    qa[14], qb[6] = 33 + 40, 33 + 40
    P(b"mates_differ", (260, "30M", bytes(a), bytes(qa)), (270, "30M", bytes(b), bytes(qb)))
    P(b"other_strand", (120, "30M"), (135, "4S30M"), rev=1)
    # ambiguity codes: the BAM keeps them apart (R is not N) for a read placed as given, and holds N for one placed on the
    # other strand; the mates are compared by those codes
    for name, rev in ((b"iupac", 0), (b"iupac_other_strand", 1)):
        a, b = bytearray(ref[186:216]), bytearray(ref[196:226])
        a[14:19], b[4:9] = b"RRYMn", b"NRK" + ref[203:204] + b"N"
        a[22:24], b[12:14] = b"SW", b"SN"
        P(name, (186, "30M", bytes(a)), (196, "30M", bytes(b)), rev=rev)
    P(b"slash/1", (5, "30M"), (18, "30M"), name2=b"slash/2")
    P(b"improper_overlap", (240, "30M"), (250, "30M"), proper=0)
    # names whose hash lets the first / the second mate keep the agreeing bases
    for k in range(6):
        P(b"keeper%d" % k, (124 + 20 * k, "40M"), (140 + 20 * k, "40M"))
    sb.unmapped_pair(b"unmapped")
    return sb


# ------------------------------------------------------------------------------------------------ running the reference
def run_reference(pmx, ds, chrom, workdir, flags=()):
    """BAM + FASTA -> (rank of every read in the BAM, mpileup columns, number of INDEL records, call lines)"""
    bam, fa = os.path.join(workdir, "x.bam"), os.path.join(workdir, "x.fa")
    pmx.write_bam(bam, chrom, len(ds["ref"]), ds["reads"], ds["quals"], ds["names"], ds["results"] if "results" in ds else pg.to_results(ds), ds["paired"])
    import test_bam as tb
    rank = gc.rank_from_bam(tb.parse_bam(bam)[2], ds["names"], ds["paired"])
    with open(fa, "wb") as fh:
        fh.write(b">" + chrom.encode() + b"\n" + ds["ref"] + b"\n")
    mp, vcf = os.path.join(workdir, "x.mpileup.vcf"), os.path.join(workdir, "x.call.vcf")
    subprocess.run([REF_BCFTOOLS, "mpileup", "-Ov", "-B", "-f", fa] + list(flags) + ["-o", mp, bam], check=True, stderr=subprocess.DEVNULL)
    subprocess.run([REF_BCFTOOLS, "call", "--ploidy", "1", "-m", "-A", "-O", "v", "-o", vcf, mp], check=True, stderr=subprocess.DEVNULL)
    cols = {c: [] for c in pg.COLUMNS}
    n_indel = 0
    for line in open(mp):
        if line.startswith("#"):
            continue
        f = line.rstrip("\n").split("\t")
        info = f[7].split(";")
        if "INDEL" in info:
            n_indel += 1
            continue
        kv = dict(x.split("=", 1) for x in info if "=" in x)
        i16 = [float(x) for x in kv["I16"].split(",")]
        assert all(v == int(v) for v in i16[:4] + [i16[8], i16[10]])
        assert f[8].split(":")[:2] == ["PL", "AD"], f[8]
        sample = f[9].split(":")
        for c, v in zip(pg.COLUMNS, (int(f[1]), f[3], f[4], int(kv["DP"]), [int(i16[j]) for j in (0, 1, 2, 3, 8, 10)], kv["QS"], kv["MQ0F"],
                                     sample[0], sample[1])):
            cols[c].append(v)
    call = []
    n_call_indel = 0
    for line in open(vcf):
        if line.startswith("#"):
            continue
        line = line.rstrip("\n")
        if "INDEL" in line.split("\t")[7].split(";"):
            n_call_indel += 1
            continue
        call.append(line)
    return rank, dict(mpileup=cols, n_indel=n_indel, call=call, n_call_indel=n_call_indel, flags=list(flags))


def checker_tables(ds, rank, **params):
    concat = b"".join(ds["reads"])
    off = np.zeros(len(ds["reads"]) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in ds["reads"]])
    return gc.pileup_tables(ds["recs"], ds["cig"], concat, off, len(ds["ref"]), ds["paired"], False, rank, quals=b"".join(ds["quals"]),
                            names=ds["names"], **params)


def multi_allelic(leg):
    return sum(1 for line in leg["call"] if "," in line.split("\t")[4] and not line.split("\t")[9].startswith("0"))


LEGS = (  # name, input set, mpileup flags, the library's parameters
    ("random", "random", (), {}),
    ("variants40", "variants40", (), {}),
    ("variants250", "variants250", (), {}),
    ("single", "single", (), {}),
    ("edges", "edges", (), {}),
    ("edges_reversed", "edges", (), {}),
    ("cap", "cap", (), {}),
    ("cap_d8", "cap", ("-d", "8"), dict(max_depth=8)),
    ("random_Q13", "random", ("-Q", "13"), dict(min_baseq=13)),
    ("random_maxBQ40", "random", ("--max-BQ", "40"), dict(max_baseq=40)),
    ("random_deltaBQ5", "random", ("--delta-BQ", "5"), dict(delta_baseq=5)),
)


def build_crafted(pmx):
    """-> (the bytes of pileup_crafted_inputs.json.gz, of pileup_crafted_golden.json.gz, a summary per leg)"""
    ref = reference_300()
    sets = dict(random=random_pairs(ref, 220, 220), variants40=random_pairs(ref, 40, 40, planted_variants(ref)),
                variants250=random_pairs(ref, 250, 250, planted_variants(ref)), single=single_reads(ref), edges=edge_pairs(ref), cap=cap_pairs(ref))
    inputs = {k: sb.inputs() for k, sb in sets.items()}
    inputs_bytes = pg.dump(inputs)
    legs, summary = {}, {}
    same_start_late = set()
    for leg_name, set_name, flags, params in LEGS:
        ds = pg.input_set(set_name, inputs)
        if leg_name == "edges_reversed":
            ds = pg.reorder(ds, range(len(ds["reads"]) // 2 - 1, -1, -1))
        with tempfile.TemporaryDirectory() as wd:
            rank, leg = run_reference(pmx, ds, pg.CHROM, wd, flags)
        leg["set"], leg["params"] = set_name, params
        hist, aux, info = checker_tables(ds, rank, **params)
        concat = np.frombuffer(b"".join(ds["reads"]), np.uint8)
        off = np.zeros(len(ds["reads"]) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in ds["reads"]])
        feats = gc.features(ds["recs"], ds["cig"], concat, off, ds["paired"])
        deepest = int(hist.sum(axis=(1, 2, 3)).max())
        assert deepest <= 255, (leg_name, deepest)               # beyond 255 bases the reference samples at random
        summary[leg_name] = dict(records=len(leg["mpileup"]["pos"]), indel=leg["n_indel"], call=len(leg["call"]), deepest=deepest,
                                 refused=info["refused_by_cap"], reconciled=info["reconciled_pairs"], late=info["late_neighbours"],
                                 branches=info["branches"], features=feats, multi_allelic=multi_allelic(leg))
        # every set exercises what it is for
        if set_name in ("random", "variants40", "variants250"):
            assert all(v > 0 for v in feats.values()), (leg_name, feats)
            assert info["reconciled_pairs"] > 0 and info["late_neighbours"] > 0
        if set_name == "single":
            assert feats["soft_clip"] and feats["insertion"] and feats["deletion"] and feats["n_base"] and info["reconciled_pairs"] == 0
        if leg_name == "cap":
            assert info["refused_by_cap"] == 0
        if leg_name == "cap_d8":
            assert info["refused_by_cap"] >= 1
        if set_name == "edges":
            want = ("deletion in a", "deletion in b", "unequal positions skipped", "agree, a keeps", "agree, b keeps", "differ, a better",
                    "differ, b better", "differ, equal quality")
            assert all(info["branches"].get(b, 0) > 0 for b in want), (leg_name, info["branches"])
            late = {ds["names"][r] for r in info["late_reads"]}
            assert b"late_del_third" in late, (leg_name, late)
            same_start_late |= late & {b"late_third", b"late_third_too"}
            assert not late & {b"late_alone", b"late_alone_too", b"late_del_alone"}, (leg_name, late)
        legs[leg_name] = leg
    # which of several reads with one start comes first is the choice of the writer's sort: a read with b's start stands
    # in front of b in one of the two input orders of the edges set at least
    assert same_start_late, "no pair of the edges set sees a read with its second mate's start in front of that mate"
    assert summary["variants40"]["multi_allelic"] + summary["variants250"]["multi_allelic"] >= 20, summary
    return inputs_bytes, pg.dump(legs), summary


def build_demo(pmx):
    from oracle import oracle as orc
    g = b"".join(l.strip() for l in open(os.path.join(HERE, "isolate.ref.fa"), "rb") if not l.startswith(b">"))
    seqs, quals, names = pmx.read_fastq_paired(os.path.join(HERE, "isolate_R1.fastq.gz"), os.path.join(HERE, "isolate_R2.fastq.gz"))
    results = orc.ref_align_reads_direct(g, seqs, True, 8)
    ds = dict(ref=g, paired=True, reads=seqs, quals=quals, names=names, results=results)
    with tempfile.TemporaryDirectory() as wd:
        rank, leg = run_reference(pmx, ds, "node_7618", wd)
    ds["recs"], ds["cig"] = gc.results_to_records(results, True)
    hist, aux, info = checker_tables(ds, rank)
    deepest = int(hist.sum(axis=(1, 2, 3)).max())
    assert deepest <= 255, deepest
    leg["set"], leg["params"] = "demo", {}
    # the QS decimals of the demo are not needed to six digits for the file to stay under the size limit: kept as printed
    return pg.dump(leg), dict(records=len(leg["mpileup"]["pos"]), indel=leg["n_indel"], call=len(leg["call"]), deepest=deepest,
                              refused=info["refused_by_cap"], reconciled=info["reconciled_pairs"], late=info["late_neighbours"])


def main():
    import panmap_amd as pmx
    what = sys.argv[1:] or ["crafted", "demo"]
    if "crafted" in what:
        inputs_bytes, golden_bytes, summary = build_crafted(pmx)
        for path, data in ((pg.INPUTS, inputs_bytes), (pg.CRAFTED, golden_bytes)):
            with open(path, "wb") as fh:
                fh.write(data)
            print(path, len(data), "bytes")
        for k, v in summary.items():
            print(k, v)
    if "demo" in what:
        data, summary = build_demo(pmx)
        with open(pg.DEMO, "wb") as fh:
            fh.write(data)
        print(pg.DEMO, len(data), "bytes", summary)


if __name__ == "__main__":
    main()
