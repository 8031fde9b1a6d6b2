"""mpileup's bias annotations (VDB, SGB, RPBZ, MQBZ, MQSBZ, BQBZ, SCBZ, MQ0F), host side: the library's site_tests on the
numpy checker's tables (tests/bias_checks.py) against the `bcftools call` lines of the committed fixtures -- the same keys
present, the same text, no tolerance -- on every crafted leg and, where the compiled reference aligner is built, on the
README demo.  Then the statistics' edge branches on hand-made rows, the formatter on htslib's known answers, and what
Genotyper.annotate writes."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import bias_checks as bc
import geno_checks as gc
import pileup_golden as pg
from test_pileup_reference import leg_set

LEGS = sorted(pg.crafted_legs())
_tables = {}


def checker_bias(pmx, leg_name, tmp_path_factory):
    """the checker's hist, aux and bias tables of one crafted leg, with its flags, in the order of the BAM the library writes
    (computed once)"""
    if leg_name not in _tables:
        leg, ds = leg_set(leg_name)
        rank = pg.bam_order(pmx, ds, str(tmp_path_factory.mktemp("bias") / "x.bam"))
        concat, off = pmx.concat_reads(ds["reads"])
        hist, aux, info, bias, n_unset = bc.bias_tables(ds["recs"], ds["cig"], concat, off, ds["ref"], ds["paired"], False, rank,
                                                        quals=b"".join(ds["quals"]), names=ds["names"], **leg["params"])
        for a in (hist, aux, bias):
            a.setflags(write=False)
        _tables[leg_name] = (hist, aux, bias, n_unset, rank)
    return _tables[leg_name]


def compare_with_call(pmx, leg, hist, aux, bias, reference):
    """site_tests at every `call` line with an alternative -> (lines compared, differences)"""
    n, bad = 0, []
    for line in leg["call"]:
        g = bc.golden_tests(line)
        if g is None:
            continue
        p, want = g
        got = pmx.site_tests(hist[p], aux[p], bias[p], reference[p:p + 1])
        n += 1
        if got != want:
            bad.append((p + 1, {k: (got.get(k), want.get(k)) for k in bc.KEYS if got.get(k) != want.get(k)}))
    return n, bad


@pytest.mark.parametrize("leg_name", LEGS)
def test_site_tests_equal_the_call_lines(pmx, leg_name, tmp_path_factory):
    leg, ds = leg_set(leg_name)
    hist, aux, bias, n_unset, _ = checker_bias(pmx, leg_name, tmp_path_factory)
    n, bad = compare_with_call(pmx, leg, hist, aux, bias, ds["ref"])
    print(leg_name, n, "lines with an alternative,", n_unset, "bases whose clip stays unset")
    assert n > 0
    assert not bad, "%d of %d lines differ, first %s" % (len(bad), n, bad[:5])
    # every histogram counts exactly the bases of hist
    depth = hist.reshape(len(ds["ref"]), -1).sum(axis=1)
    for name, (at, bins) in bc.BLOCKS.items():
        assert np.array_equal(bias[:, at:at + 2 * bins].sum(axis=1), depth), name


def test_demo_site_tests_equal_the_call_lines(pmx, oracle, tmp_path):
    """the demo reads as the compiled reference aligner places them: all 8,449 lines with an alternative"""
    if not os.path.isdir(os.path.join(ROOT, "oracle", "_ref")):
        pytest.skip("oracle/_ref (compiled reference aligner) is absent")
    import test_bam as tb
    g = b"".join(l.strip() for l in open(os.path.join(GOLDEN, "isolate.ref.fa"), "rb") if not l.startswith(b">"))
    seqs, quals, names = pmx.read_fastq_paired(os.path.join(GOLDEN, "isolate_R1.fastq.gz"), os.path.join(GOLDEN, "isolate_R2.fastq.gz"))
    want = oracle.ref_align_reads_direct(g, seqs, True, 8)
    bam = str(tmp_path / "isolate.bam")
    pmx.write_bam(bam, "node_7618", len(g), seqs, quals, names, want, True)
    rank = gc.rank_from_bam(tb.parse_bam(bam)[2], names, True)
    recs, cig = gc.results_to_records(want, True)
    concat, off = pmx.concat_reads(seqs)
    hist, aux, _, bias, _ = bc.bias_tables(recs, cig, concat, off, g, True, False, rank, quals=b"".join(quals), names=names)
    n, bad = compare_with_call(pmx, pg.demo_leg(), hist, aux, bias, g)
    assert n == 8449
    assert not bad, "%d of %d lines differ, first %s" % (len(bad), n, bad[:5])
    # the written record's line is the published example's
    p = 24152 - 1
    gold = [l for l in open(os.path.join(GOLDEN, "isolate.vcf")).read().splitlines() if not l.startswith("#")][0].split("\t")[7]
    kv = dict(x.split("=", 1) for x in gold.split(";"))
    assert pmx.site_tests(hist[p], aux[p], bias[p], g[p:p + 1]) == {k: kv[k] for k in bc.KEYS}


def test_fixtures_reach_every_branch(pmx, tmp_path_factory):
    """a fixture set that never shows a key absent, or never reaches the unset clip, would pass while testing nothing"""
    present = dict.fromkeys(bc.KEYS, 0)
    absent = dict.fromkeys(bc.KEYS, 0)
    n_lines = scbz_nonzero = 0
    for leg in pg.crafted_legs().values():
        for line in leg["call"]:
            g = bc.golden_tests(line)
            if g is None:
                continue
            n_lines += 1
            for k in bc.KEYS:
                (present if k in g[1] else absent)[k] += 1
            scbz_nonzero += g[1].get("SCBZ", "0") not in ("0", "-0")
    print(n_lines, "lines", present, absent, scbz_nonzero, "with SCBZ != 0")
    assert n_lines == 1356 and sum(bc.golden_tests(l) is not None for l in pg.demo_leg()["call"]) == 8449
    assert all(v >= 900 for v in present.values()), present
    assert present["SGB"] == present["MQ0F"] == n_lines
    assert all(absent[k] >= 10 for k in bc.KEYS if k not in ("SGB", "MQ0F")), absent
    assert scbz_nonzero >= 1000
    for leg_name in ("random", "variants250", "single"):
        n_unset = checker_bias(pmx, leg_name, tmp_path_factory)[3]
        assert n_unset >= 500, (leg_name, n_unset)


def _rows(ref=(), alt=()):
    """hist, aux and bias rows of a site with reference A: ref / alt = lists of (epos, scl, mq, bq, strand)"""
    hist, aux, bias = np.zeros((64, 2, 5), np.uint32), np.zeros(4, np.uint32), np.zeros(bc.CELLS, np.uint32)
    for is_alt, bases in enumerate((ref, alt)):
        for epos, scl, mq, bq, strand in bases:
            hist[max(min(bq, mq), 4), strand, 1 if is_alt else 0] += 1
            aux[0] += 1
            aux[1] += mq
            aux[2] += mq == 0
            for at, v in ((bc.POS, epos), (bc.SCL, scl)):
                bias[at + is_alt * 100 + v] += 1
            for at, v in ((bc.MQ, mq), (bc.BQ, bq)):
                bias[at + is_alt * 60 + v] += 1
            bias[bc.MQS + strand * 60 + mq] += 1
    return hist, aux, bias


def test_hand_made_rows(pmx):
    ref = [(10 + 7 * k, 0, 59, 30 + k, k & 1) for k in range(6)]
    # no alt base: VDB, SGB and the four ref/alt scores are absent; MQSBZ compares strands, not alleles, and both are here
    got = pmx.site_tests(*_rows(ref=ref), b"A")
    assert set(got) == {"MQSBZ", "MQ0F"} and got["MQ0F"] == "0", got
    # all bases on one strand as well: nothing but MQ0F
    got = pmx.site_tests(*_rows(ref=[(e, s, m, b, 0) for e, s, m, b, _ in ref]), b"A")
    assert got == {"MQ0F": "0"}, got
    # one alt base: VDB needs two (calc_vdb: dp < 2), the rest is there.  SGB for one sample with nr alt bases:
    # logsumexp2(log 1, log .5 + nr log 2 - nr) + log .5 - nr + nr  ->  nr = 1: log(1 + exp(-1)) - log 2
    got = pmx.site_tests(*_rows(ref=ref, alt=[(50, 0, 59, 35, 0)]), b"A")
    assert set(got) == set(bc.KEYS) - {"VDB"}, got
    assert got["SGB"] == pg.kputd(np.float32(np.log1p(np.exp(-1.0)) + np.log(0.5))), got
    # two alt bases, the exact branch: positions 20 and 61 -> mean 40.5, mean distance 20.5 -> ipos 20;
    # (200 - 2 * 21 - 1) * 21 / 99 in integers = 33, / 50 = 0.66
    got = pmx.site_tests(*_rows(ref=ref, alt=[(20, 0, 59, 35, 0), (61, 0, 59, 35, 1)]), b"A")
    assert got["VDB"] == "0.66", got
    # both alt bases at one position: ipos 0 -> 197 / 99 = 1 -> 0.02
    got = pmx.site_tests(*_rows(ref=ref, alt=[(33, 0, 59, 35, 0), (33, 0, 59, 35, 1)]), b"A")
    assert got["VDB"] == "0.02", got
    # every base in one bin of every histogram: the tie correction takes the whole variance (var2 <= 0) -> 0
    same = [(40, 0, 59, 35, 0)] * 3
    got = pmx.site_tests(*_rows(ref=same, alt=[(40, 0, 59, 35, 1)] * 2), b"A")
    assert [got[k] for k in ("RPBZ", "MQBZ", "BQBZ", "SCBZ")] == ["0"] * 4, got
    # a Z score by hand: ref mapping qualities {20, 20}, alt {59}.  calc_mwu_biasZ: l = pairs with ref < alt = 2, e = 0
    # -> U = 2, m = 1; ties t = (2^3 - 2) + 0 = 6; var2 = 2 / 12 * (4 - 6 / 6) = 0.5 -> Z = 1 / sqrt(.5)
    got = pmx.site_tests(*_rows(ref=[(10, 0, 20, 30, 0), (30, 0, 20, 30, 1)], alt=[(50, 0, 59, 30, 0)]), b"A")
    assert got["MQBZ"] == pg.kputd(np.float32(1 / np.sqrt(0.5))), got
    # MQ0F = MQ-0 bases over the raw depth, as a float: one of three
    got = pmx.site_tests(*_rows(ref=[(10, 0, 0, 30, 0), (30, 0, 20, 30, 1)], alt=[(50, 0, 59, 30, 0)]), b"A")
    assert got["MQ0F"] == "0.333333", got
    # a reference letter that is no A C G T: every base is alt, so the ref/alt tests have nothing to compare
    got = pmx.site_tests(*_rows(alt=ref), b"N")
    assert set(got) == {"VDB", "SGB", "MQSBZ", "MQ0F"}, got


def test_formatter_prints_like_htslib(pmx):
    """the cases of test_pileup_reference.test_kputd_prints_like_htslib, and the checker's printer on a sweep"""
    f32 = np.float32
    for value, text in ((0.0, "0"), (1.0, "1"), (0.5, "0.5"), (f32(1) / f32(3), "0.333333"), (f32(2) / f32(3), "0.666667"), (f32(53) / f32(114), "0.464912"),
                        (f32(1) / f32(96), "0.0104167"), (0.05, "0.05"), (f32(0.05), "0.05"), (0.00999999999, "0.01"), (0.000123456, "0.000123456"),
                        (123.001, "123.001"), (123.0, "123"), (999999.0, "999999"), (0.00001, "1e-05"), (3.52045e-09, "3.52045e-09"), (-0.453602, "-0.453602"),
                        (-0.0, "-0"), (f32(1.01195e-37), "1.01195e-37"), (9.9999996, "10"), (99999.95, "100000"), (1234567.0, "1.23457e+06")):
        assert pmx.format_float(value) == text, (value, pmx.format_float(value), text)
    rng = np.random.Generator(np.random.PCG64(11))
    for v in np.concatenate([rng.normal(0, 3, 2000), 10.0 ** rng.uniform(-6, 7, 2000)]).astype(np.float32):
        assert pmx.format_float(v) == pg.kputd(v), v


def test_annotate_rewrites_info_and_header(pmx, tmp_path):
    """a two-record genotyper: annotate puts the tests between DP and AC in the golden lines' order, leaves the other
    columns, and the header gains the eight lines of the published example; without annotate nothing changes"""
    ref = b"CCGTACGTAC"
    hist, aux = np.zeros((len(ref), 64, 2, 5), np.uint32), np.zeros((len(ref), 4), np.uint32)
    bias = np.zeros((len(ref), bc.CELLS), np.uint32)
    for p in range(len(ref)):
        hist[p, 40, 0, b"ACGT".index(ref[p:p + 1])] = 10
        aux[p] = (10, 600, 0, 0)
    for p, alt in ((4, 3), (7, 0)):
        hist[p] = 0
        hist[p, 35, 0, alt], hist[p, 30, 1, alt] = 5, 4
        aux[p] = (9, 9 * 60, 0, 0)
        for k in range(9):
            for at, v in ((bc.POS + 100, 10 + 9 * k), (bc.SCL + 100, 0), (bc.MQ + 60, 59), (bc.BQ + 60, 35 if k < 5 else 30), (bc.MQS + (k >= 5) * 60, 59)):
                bias[p, at + v] += 1
    plain = pmx.Genotyper(hist, aux, ref, "chr", None)
    before = plain.records()
    assert [int(x) for x in plain.positions()] == [4, 7] and all(";VDB=" not in r for r in before)
    plain.write_vcf(str(tmp_path / "plain.vcf"), "s.bam")
    gt = pmx.Genotyper(hist, aux, ref, "chr", None)
    with pytest.raises(pmx.PmxError):
        gt.annotate([5], bias[[5]])                             # no record there
    assert gt.records() == before
    gt.annotate(gt.positions(), bias[gt.positions()])
    after = gt.records()
    for b, a, p in zip(before, after, (4, 7)):
        fb, fa = b.split("\t"), a.split("\t")
        assert fb[:7] == fa[:7] and fb[8:] == fa[8:]
        tests = pmx.site_tests(hist[p], aux[p], bias[p], ref[p:p + 1])
        assert set(tests) == {"VDB", "SGB", "MQSBZ", "MQ0F"}
        kb = fb[7].split(";")
        assert fa[7] == ";".join(kb[:1] + ["%s=%s" % (k, tests[k]) for k in bc.KEYS if k in tests] + kb[1:])
        assert [x.split("=")[0] for x in fa[7].split(";")] == ["DP", "VDB", "SGB", "MQSBZ", "MQ0F", "AC", "AN", "DP4", "MQ"]
    with pytest.raises(pmx.PmxError):
        gt.annotate(gt.positions(), bias[gt.positions()])       # twice
    gt.write_vcf(str(tmp_path / "ann.vcf"), "s.bam")
    ann = open(tmp_path / "ann.vcf").read().splitlines()
    old = open(tmp_path / "plain.vcf").read().splitlines()
    example = [l for l in open(os.path.join(GOLDEN, "isolate.vcf")).read().splitlines()
               if l.startswith("##INFO=<ID=") and l.split("=<ID=")[1].split(",")[0] in bc.KEYS]
    assert len(example) == 8 and [l for l in ann if l not in old and l.startswith("##")] == example
    assert [l for l in ann if l.startswith("##") and l not in example] == [l for l in old if l.startswith("##")]
    assert [l for l in old if not l.startswith("#")] == before and [l for l in ann if not l.startswith("#")] == after
