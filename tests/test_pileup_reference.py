"""The genotype stage against the reference's own programs, host side: the recorded results of `bcftools mpileup -B` and
`bcftools call --ploidy 1 -m -A` (tests/golden/pileup_*.json.gz, written by tests/golden/make_pileup_golden.py) pin

  * the numpy restatement of tests/geno_checks.py -- every compared column of every mpileup record, on crafted read sets
    and on the README demo as the compiled reference aligner places it;
  * the library's site quantities (pmx.site_call) on the same tables;
  * the records pmx.Genotyper writes, byte for byte (INFO cut down to the keys written), against the `call` lines passed
    through the reference's filter: the two variant sets hold calls (113 records over three spectra) and the demo three;
    on the other legs both sides hold no record.  No fixture holds a site where the filter's allele is not the first
    alternative or differs from `call`'s genotype; that case is a hand-made table here
    (test_second_alternative_called_reaches_record_and_consensus).

Everything is an integer and compared exactly; QS and MQ0F are floats the reference prints with htslib's kputd, and are
compared as that printer prints them (pileup_golden.kputd).  Not compared, because the tables cannot give them: I16[4..7]
(base-quality sums taken before the mapQ cap) and the tail-distance terms."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import geno_checks as gc
import pileup_golden as pg

REF_BCFTOOLS = os.path.join(ROOT, "oracle", "_ref", "ref_bcftools")
LEGS = sorted(pg.crafted_legs())
# INDEL records of mpileup per leg (skipped by their INDEL flag alone; the generator recorded the count)
N_INDEL = dict(random=1, variants40=0, variants250=0, single=7, edges=2, edges_reversed=2, cap=0, cap_d8=0, random_Q13=1, random_maxBQ40=1,
               random_deltaBQ5=1)
_tables = {}


def leg_set(leg_name):
    leg = pg.crafted_legs()[leg_name]
    ds = pg.input_set(leg["set"])
    if leg_name == "edges_reversed":
        ds = pg.reorder(ds, range(len(ds["reads"]) // 2 - 1, -1, -1))
    return leg, ds


def checker_tables(pmx, leg_name, tmp_path_factory):
    """the checker's tables of one leg, in the order of the BAM the library writes from the set (computed once)"""
    if leg_name not in _tables:
        leg, ds = leg_set(leg_name)
        rank = pg.bam_order(pmx, ds, str(tmp_path_factory.mktemp("plp") / "x.bam"))
        concat, off = pmx.concat_reads(ds["reads"])
        hist, aux, info = gc.pileup_tables(ds["recs"], ds["cig"], concat, off, len(ds["ref"]), ds["paired"], False, rank, quals=b"".join(ds["quals"]),
                                           names=ds["names"], **leg["params"])
        info["features"] = gc.features(ds["recs"], ds["cig"], np.frombuffer(concat, np.uint8), off, ds["paired"])
        for a in (hist, aux):
            a.setflags(write=False)
        _tables[leg_name] = (hist, aux, info, rank)
    return _tables[leg_name]


def check_preconditions(leg_name, leg, hist, info):
    """a set that does not exercise what it is for would pass while testing nothing"""
    assert hist.sum(axis=(1, 2, 3)).max() <= 255                # beyond 255 bases the reference samples at random
    assert leg["n_indel"] == N_INDEL[leg_name]
    f, br = info["features"], info["branches"]
    if leg["set"] in ("random", "variants40", "variants250"):
        assert all(v > 0 for v in f.values()), f
        assert info["reconciled_pairs"] > 0 and info["late_neighbours"] > 0
        assert all(br.get(b, 0) > 0 for b in ("agree, a keeps", "agree, b keeps", "differ, a better", "differ, b better", "deletion in a", "deletion in b"))
    if leg["set"] == "single":
        assert f["soft_clip"] and f["insertion"] and f["deletion"] and f["n_base"] and info["reconciled_pairs"] == 0
    if leg["set"] == "edges":
        assert all(br.get(b, 0) > 0 for b in ("deletion in a", "deletion in b", "unequal positions skipped", "agree, a keeps", "agree, b keeps",
                                              "differ, a better", "differ, b better", "differ, equal quality")), br
        assert info["late_neighbours"] > 0
    if leg_name == "cap":
        assert info["refused_by_cap"] == 0
    if leg_name == "cap_d8":
        assert info["refused_by_cap"] >= 1


def test_kputd_prints_like_htslib():
    """known answers worked out from kstring.c:38-140: six significant digits, rint, trailing zeros dropped"""
    f32 = np.float32
    for value, text in ((0.0, "0"), (1.0, "1"), (0.5, "0.5"), (f32(1) / f32(3), "0.333333"), (f32(2) / f32(3), "0.666667"), (f32(53) / f32(114), "0.464912"),
                        (f32(1) / f32(96), "0.0104167"), (0.05, "0.05"), (f32(0.05), "0.05"), (0.00999999999, "0.01"), (0.000123456, "0.000123456"),
                        (123.001, "123.001"), (123.0, "123"), (999999.0, "999999"), (0.00001, "1e-05"), (3.52045e-09, "3.52045e-09"), (-0.453602, "-0.453602")):
        assert pg.kputd(value) == text, (value, pg.kputd(value), text)


@pytest.mark.parametrize("leg_name", LEGS)
def test_checker_and_site_call_equal_mpileup(pmx, leg_name, tmp_path_factory):
    leg, ds = leg_set(leg_name)
    hist, aux, info, _ = checker_tables(pmx, leg_name, tmp_path_factory)
    print(leg_name, {k: v for k, v in info.items() if k not in ("admitted", "late_reads")}, len(leg["mpileup"]["pos"]), "records")
    check_preconditions(leg_name, leg, hist, info)
    bad = pg.compare_with_mpileup(leg, hist, aux, ds["ref"], gc.site)
    assert not bad, "checker: %d positions differ, first %s" % (len(bad), bad[:5])
    bad = pg.compare_with_mpileup(leg, hist, aux, ds["ref"], pmx.site_call)
    assert not bad, "library site_call: %d positions differ, first %s" % (len(bad), bad[:5])


@pytest.mark.parametrize("leg_name", LEGS)
def test_genotyper_writes_the_filtered_call_records(pmx, leg_name, tmp_path_factory):
    leg, ds = leg_set(leg_name)
    hist, aux, _, _ = checker_tables(pmx, leg_name, tmp_path_factory)
    n = 0
    for name, phred in pg.spectra().items():
        want = pg.expected_records(pmx, leg, phred)
        got = pmx.Genotyper(hist, aux, ds["ref"], pg.CHROM, phred).records()
        assert [l.split("\t")[1] for l in got] == [l.split("\t")[1] for l in want], name
        assert got == want, (name, [(g, w) for g, w in zip(got, want) if g != w][:3])
        n += len(want)
    print(leg_name, n, "records over three spectra")
    # only the variant sets hold calls; on every other leg the check is that the library writes no record either
    assert (n > 0) == leg["set"].startswith("variants")


def test_variant_sets_call_multi_allelic_sites(pmx):
    """at least 20 distinct called sites that list more than one alternative, across the two variant sets"""
    sites = set()
    for leg_name in ("variants40", "variants250"):
        for phred in pg.spectra().values():
            sites |= {(leg_name, l.split("\t")[1]) for l in pg.expected_records(pmx, pg.crafted_legs()[leg_name], phred) if "," in l.split("\t")[4]}
    print(len(sites), "multi-allelic called sites")
    assert len(sites) >= 20


def test_second_alternative_called_reaches_record_and_consensus(pmx, tmp_path):
    """A site where the spectrum makes the SECOND alternative the call: REF A, three T of quality 35 on one strand, four G
    of quality 24 on the other, transitions cheap.  The record lists both alternatives with GT 2, INFO as the raw line
    had it, and the consensus takes G: `bcftools consensus` without -s on a file with one sample applies the allele that
    sample's GT names (consensus.c:231-259, 606-622), not the first alternative."""
    ref = b"CCGTACGTAC"
    hist, aux = np.zeros((len(ref), 64, 2, 5), np.uint32), np.zeros((len(ref), 4), np.uint32)
    for p in range(len(ref)):
        hist[p, 40, 0, b"ACGT".index(ref[p:p + 1])] = 10
        aux[p] = (10, 600, 0, 0)
    hist[4] = 0
    hist[4, 35, 0, 3], hist[4, 24, 1, 2] = 3, 4
    aux[4] = (7, 7 * 60, 0, 0)
    phred = pg.spectra()["transitions"]
    site = gc.site(hist[4], b"A")
    assert site["alleles"] == [0, 3, 2] and site["ad"] == [0, 3, 4]
    gls = [site["pl"][k] + phred[0][a] for k, a in enumerate(site["alleles"])]
    assert min(range(3), key=lambda k: gls[k]) == 2 and min(range(3), key=lambda k: site["pl"][k]) == 1   # the spectrum overrides the likelihoods
    qual = gls[0] - gls[2]
    assert qual >= 30
    gt = pmx.Genotyper(hist, aux, ref, "chr", phred)
    recs = gt.records()
    assert recs == ["chr\t5\t.\tA\tT,G\t%.4f\t.\tDP=7;AC=1,0;AN=1;DP4=0,0,3,4;MQ=60\tGT:PL:AD\t2:%s:0,3,4" % (qual, ",".join(map(str, site["pl"])))]
    gt.write_vcf(str(tmp_path / "s.vcf"), "s.bam")
    fa = tmp_path / "chr.fa"
    fa.write_bytes(b">chr\n" + ref + b"\n")
    pmx.write_consensus(str(tmp_path / "s.vcf"), str(fa), str(tmp_path / "s.consensus.fa"), "s_consensus ref=chr")
    assert open(tmp_path / "s.consensus.fa").read() == ">s_consensus ref=chr\nCCGTGCGTAC\n"
    # a genotype that names the reference changes nothing; a file without a sample column gets its first alternative
    head = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    (tmp_path / "gt0.vcf").write_text(head + "\tFORMAT\ts\nchr\t5\t.\tA\tT,G\t40\t.\tDP=7\tGT:PL:AD\t0:0,55,69:0,3,4\n")
    pmx.write_consensus(str(tmp_path / "gt0.vcf"), str(fa), str(tmp_path / "gt0.fa"), "x")
    assert open(tmp_path / "gt0.fa").read() == ">x\n" + ref.decode() + "\n"
    (tmp_path / "sites.vcf").write_text(head + "\nchr\t5\t.\tA\tT,G\t40\t.\tDP=7\n")
    pmx.write_consensus(str(tmp_path / "sites.vcf"), str(fa), str(tmp_path / "sites.fa"), "x")
    assert open(tmp_path / "sites.fa").read() == ">x\nCCGTTCGTAC\n"


def test_demo_checker_equals_mpileup_and_call(pmx, oracle, tmp_path):
    """the demo reads through the compiled reference aligner: the checker's tables at all 29,514 records, and the library's
    records against the `call` fixture"""
    if not os.path.isdir(os.path.join(ROOT, "oracle", "_ref")):
        pytest.skip("oracle/_ref (compiled reference aligner) is absent")
    g, hist, aux, info = pg.demo_checker_tables(pmx, oracle, str(tmp_path))
    leg = pg.demo_leg()
    assert len(leg["mpileup"]["pos"]) == 29514 and leg["n_indel"] == 8 and int((aux[:, 0] == 0).sum()) >= len(g) - 29514
    assert hist.sum(axis=(1, 2, 3)).max() <= 255
    assert info["refused_by_cap"] > 0 and info["reconciled_pairs"] > 0 and info["late_neighbours"] > 0
    bad = pg.compare_with_mpileup(leg, hist, aux, g, gc.site)
    assert not bad, "checker: %d positions differ, first %s" % (len(bad), bad[:5])
    counts, branches, length = pmx.spectrum_counts(pmx.Panman(os.path.join(GOLDEN, "sars_20000_twilight_dipper.panman")))
    for phred in [pmx.spectrum_phred(counts, branches, length)] + list(pg.spectra().values()):
        assert pmx.Genotyper(hist, aux, g, "node_7618", phred).records() == pg.expected_records(pmx, leg, phred)


def test_generator_reproduces_the_committed_crafted_fixtures(pmx):
    if not os.path.exists(REF_BCFTOOLS):
        pytest.skip("oracle/_ref/ref_bcftools (the reference's mpileup / call) is absent")
    spec = importlib.util.spec_from_file_location("make_pileup_golden", os.path.join(GOLDEN, "make_pileup_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inputs_bytes, golden_bytes, _ = gen.build_crafted(pmx)
    assert inputs_bytes == open(pg.INPUTS, "rb").read()
    assert golden_bytes == open(pg.CRAFTED, "rb").read()
