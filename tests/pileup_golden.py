"""Readers of the genotype stage's recorded results (tests/golden/pileup_*.json.gz, written by
tests/golden/make_pileup_golden.py from the reference's own `bcftools mpileup` and `bcftools call`), and the helper that
states, from the pileup tables (hist, aux) and the reference sequence, what an mpileup record states.  Plain module: no
fixtures, no pytest."""
import gzip
import json
import math
import os

import numpy as np

import geno_checks as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUTS = os.path.join(GOLDEN, "pileup_crafted_inputs.json.gz")
CRAFTED = os.path.join(GOLDEN, "pileup_crafted_golden.json.gz")
DEMO = os.path.join(GOLDEN, "pileup_demo_golden.json.gz")
CHROM = "ref300"

# the columns kept of a non-INDEL mpileup record; I16 in the order [0], [1], [2], [3], [8], [10]
COLUMNS = ("pos", "ref", "alt", "dp", "i16", "qs", "mq0f", "pl", "ad")
# the INFO keys the library writes, in its order (the rank tests of `call` are not restated)
INFO_KEYS = ("DP", "AC", "AN", "DP4", "MQ")

_cache = {}


def _load(path):
    if path not in _cache:
        with gzip.open(path, "rb") as fh:
            _cache[path] = json.loads(fh.read().decode())
    return _cache[path]


def dump(obj) -> bytes:
    """the committed bytes of a fixture: compact JSON, gzip without a time stamp"""
    import io
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0, compresslevel=9) as fh:
        fh.write(json.dumps(obj, separators=(",", ":"), sort_keys=True).encode())
    return buf.getvalue()


def crafted_legs():
    return _load(CRAFTED)


def demo_leg():
    return _load(DEMO)


def input_set(name, inputs=None):
    """one crafted input set as the library takes it: records, CIGAR arena, reads as given to the aligner (mate 2
    reverse-complemented, qualities reversed), qualities, names, reference; inputs: the sets, when not the committed ones"""
    s = (inputs if inputs is not None else _load(INPUTS))[name]
    recs = np.zeros(len(s["recs"]), gc.REC_DTYPE)
    for i, row in enumerate(s["recs"]):
        recs[i] = tuple(row)
    reads = [x.encode("latin-1") for x in s["reads"]]
    quals = [bytes.fromhex(x) for x in s["quals"]]
    names = [x.encode("latin-1") for x in s["names"]]
    return dict(name=name, ref=s["ref"].encode(), paired=bool(s["paired"]), recs=recs, cig=np.asarray(s["cig"], np.uint32), reads=reads,
                quals=quals, names=names)


def reorder(ds, order):
    """the same set with its pairs (reads, when single-end) in another order; the CIGAR arena stays"""
    unit = 2 if ds["paired"] else 1
    idx = [unit * k + m for k in order for m in range(unit)]
    return dict(ds, recs=ds["recs"][idx].copy(), reads=[ds["reads"][i] for i in idx], quals=[ds["quals"][i] for i in idx],
                names=[ds["names"][i] for i in idx])


def to_results(ds):
    """align_pair_result_t-shaped dicts for pmx.write_bam"""
    def one(r):
        if not r["mapped"] or not r["flags"] & gc.HAS_ALN:
            return dict(pos=2147483647, rs=0, re=0, qs=0, qe=0, mapq=0, rev=0, proper_frag=0, cigar=[])
        return dict(pos=int(r["rs"]) + 1, rs=int(r["rs"]), re=int(r["re"]), qs=int(r["qs"]), qe=int(r["qe"]), mapq=int(r["mapq"]), rev=int(r["rev"]),
                    proper_frag=int(r["proper_frag"]), cigar=[int(x) for x in ds["cig"][int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]])
    recs = ds["recs"]
    if ds["paired"]:
        return [dict(mapped=int(recs[2 * k]["mapped"]), r1=one(recs[2 * k]), r2=one(recs[2 * k + 1])) for k in range(len(recs) // 2)]
    return [dict(mapped=int(r["mapped"]), r1=one(r), r2=None) for r in recs]


def bam_order(pmx, ds, bam_path):
    """writes the BAM of the set and returns every read's place in it"""
    import test_bam as tb
    pmx.write_bam(bam_path, CHROM, len(ds["ref"]), ds["reads"], ds["quals"], ds["names"], to_results(ds), ds["paired"])
    return gc.rank_from_bam(tb.parse_bam(bam_path)[2], ds["names"], ds["paired"])


_demo = []


def demo_checker_tables(pmx, oracle, workdir):
    """the checker's tables of the README demo reads as the compiled reference aligner places them, in the order of the BAM
    written from those results -> (genome, hist, aux, info); one aligner run serves every test that asks"""
    if not _demo:
        g = b"".join(l.strip() for l in open(os.path.join(GOLDEN, "isolate.ref.fa"), "rb") if not l.startswith(b">"))
        seqs, quals, names = pmx.read_fastq_paired(os.path.join(GOLDEN, "isolate_R1.fastq.gz"), os.path.join(GOLDEN, "isolate_R2.fastq.gz"))
        want = oracle.ref_align_reads_direct(g, seqs, True, 8)
        import test_bam as tb
        bam = os.path.join(workdir, "isolate.bam")
        pmx.write_bam(bam, "node_7618", len(g), seqs, quals, names, want, True)
        rank = gc.rank_from_bam(tb.parse_bam(bam)[2], names, True)
        recs, cig = gc.results_to_records(want, True)
        concat, off = pmx.concat_reads(seqs)
        hist, aux, info = gc.pileup_tables(recs, cig, concat, off, len(g), True, False, rank, quals=b"".join(quals), names=names)
        for a in (hist, aux):
            a.setflags(write=False)
        _demo.append((g, hist, aux, info))
    return _demo[0]


# ------------------------------------------------------------------------------------------------ what a record states
def kputd(d: float) -> str:
    """htslib's kputd (htslib-1.20/kstring.c:38-140), the printer of every VCF float: six significant digits by rint of the
    scaled value, trailing zeros dropped; outside [0.0001, 999999] printf's %g"""
    d = float(d)
    if d == 0:
        return "-0" if math.copysign(1.0, d) < 0 else "0"
    sign, d = ("-", -d) if d < 0 else ("", d)
    if not (0.0001 <= d <= 999999):
        return sign + "%g" % d
    for bound, decimals in ((0.001, 9), (0.01, 8), (0.1, 7), (1, 6), (10, 5), (100, 4), (1000, 3), (10000, 2), (100000, 1), (None, 0)):
        if bound is None or d < bound:
            break
    i = int(np.rint(d * 10 ** decimals))                        # rint: to nearest, ties to even
    s = "%d" % i
    if decimals:
        s = s.rjust(decimals + 1, "0")
        s = (s[:-decimals] + "." + s[-decimals:]).rstrip("0").rstrip(".")
    return sign + s


_LETTER = "ACGTN"


def record_of(hist_p, aux_p, ref_base: bytes, site):
    """the compared columns of the mpileup record of one position, from its counters and its site quantities
    (pmx.site_call for the library, geno_checks.site for the checker): bam2bcf.c:955-1046 for the allele list and PL,
    :1263-1371 for what is printed"""
    h = np.asarray(hist_p).reshape(64, 2, 5).astype(np.int64)
    al = list(site["alleles"])
    ref4 = al[0]
    unseen = len(al) < (4 if ref4 < 4 else 5)                  # the '<*>' allele closes the list while a base is unseen
    # QS: per sample, the sums of the capped qualities of A C G T over their total, float arithmetic (bam2bcf.c:966-972)
    f32 = np.float32
    qs = [int((h[:, :, b].sum(axis=1) * np.arange(64)).sum()) for b in range(4)]
    tot = f32(0)
    for v in qs:
        tot = f32(tot + f32(v))
    qsum = [f32(f32(v) / tot) if tot != 0 else f32(0) for v in qs] + [f32(0)]
    dp = int(aux_p[0])
    return dict(ref=_LETTER[ref4] if ref4 < 4 else "N",
                alt=",".join([_LETTER[a] for a in al[1:]] + (["<*>"] if unseen else [])),
                dp=dp, dp4=[int(x) for x in site["dp4"]], mq_sum=int(aux_p[1]),
                qs=",".join([kputd(qsum[a]) for a in al] + (["0"] if unseen else [])),
                mq0f=kputd(f32(int(aux_p[2])) / f32(dp)) if dp else "0",
                pl_hom=[int(x) for x in site["pl"]], ad=[int(x) for x in site["ad"]])


def fixture_row(leg, k):
    """row k of a leg's mpileup columns in the shape of record_of"""
    m = leg["mpileup"]
    i16 = m["i16"][k]
    pl = [int(x) for x in m["pl"][k].split(",")]
    n_al = 1 + len(m["alt"][k].split(","))
    n_seen = n_al - (1 if m["alt"][k].endswith("<*>") else 0)
    assert len(pl) == n_al * (n_al + 1) // 2
    return dict(ref=m["ref"][k].upper(), alt=m["alt"][k], dp=m["dp"][k], dp4=i16[:4], mq_sum=i16[4] + i16[5], qs=m["qs"][k], mq0f=m["mq0f"][k],
                pl_hom=[pl[i * (i + 3) // 2] for i in range(n_seen)], ad=[int(x) for x in m["ad"][k].split(",")][:n_seen])


def compare_with_mpileup(leg, hist, aux, reference: bytes, site_fn):
    """every position of the tables against the leg's records -> list of differences (empty: equal everywhere)"""
    pos = leg["mpileup"]["pos"]
    row_of = {p: k for k, p in enumerate(pos)}
    assert len(row_of) == len(pos)
    bad = []
    for p in range(len(reference)):
        k = row_of.get(p + 1)
        if k is None:
            if aux[p, 0] != 0:
                bad.append((p + 1, "no record, raw depth %d" % aux[p, 0]))
            continue
        want = fixture_row(leg, k)
        got = record_of(hist[p], aux[p], reference[p:p + 1], site_fn(hist[p], reference[p:p + 1]))
        if got != want:
            bad.append((p + 1, {c: (got[c], want[c]) for c in want if got[c] != want[c]}))
    return bad


def project_info(line: str) -> str:
    """a VCF line with its INFO cut down to the keys the library writes, in the library's order"""
    f = line.split("\t")
    kv = dict(x.split("=", 1) for x in f[7].split(";") if "=" in x)
    f[7] = ";".join("%s=%s" % (k, kv[k]) for k in INFO_KEYS if k in kv)
    return "\t".join(f)


def expected_records(pmx, leg, phred, min_depth=1, min_qual=30.0):
    """the reference's `call` lines of a leg through the library's restatement of the reference's filter"""
    out = []
    for line in leg["call"]:
        kept = pmx.filter_line(line, phred, min_depth, min_qual)
        if kept:
            out.append(project_info(kept))
    return out


# three substitution spectra (phred, from -> to): flat, transitions cheap, and one under which every change to A is dear
def spectra():
    flat = np.full((4, 4), 40.0)
    np.fill_diagonal(flat, 0.0)
    ti = np.full((4, 4), 45.0)
    for a, b in ((0, 2), (2, 0), (1, 3), (3, 1)):
        ti[a, b] = 30.0
    np.fill_diagonal(ti, 0.01)
    skew = np.full((4, 4), 20.0)
    skew[:, 0] = 60.0
    np.fill_diagonal(skew, 0.5)
    return dict(flat=flat, transitions=ti, skew=skew)
