"""Genotype + consensus stages, host side (pmx_genotype_*): the substitution spectrum, the reference's filter
(src/genotyping.cpp:167-279, src/conversion.cpp:163-178), the htslib error model against a restatement kept in
tests/geno_checks.py, the writers against the reference's golden VCF / FASTA of the README demo, and the checker itself
pinned to the golden line through the compiled reference aligner."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import geno_checks as gc

GOLDEN_LINE = [l for l in open(os.path.join(GOLDEN, "isolate.vcf")).read().splitlines() if not l.startswith("#")]


def _outward(lo, hi):
    return math.floor(lo * 1e4) / 1e4, math.ceil(hi * 1e4) / 1e4


def qual_interval(pmx, sars):
    """[Q(Lmax), Q(Lmin)] rounded outward to four decimals, Q(L) = 255 + s[C][C] - 69 - s[C][T] for the spectrum of genome
    length L, Lmin / Lmax the shortest / longest leaf genome of the tree: the whole tolerance on QUAL"""
    counts, branches, length = pmx.spectrum_counts(sars)
    parents = [sars.parent(i) for i in range(sars.num_nodes)]
    has_child = set(parents)
    lens = [len(sars.genome(i)) for i in range(sars.num_nodes) if i not in has_child]

    def q(L):
        s = pmx.spectrum_phred(counts, branches, L)
        return 255 + s[1][1] - 69 - s[1][3]
    lo, hi = _outward(q(max(lens)), q(min(lens)))
    return lo, hi, q(length), (counts, branches, length)


def test_spectrum_brackets_the_golden_qual(pmx, sars):
    assert len(GOLDEN_LINE) == 1 and GOLDEN_LINE[0].split("\t")[5] == "148.9584"
    lo, hi, q_lib, (counts, branches, length) = qual_interval(pmx, sars)
    print("QUAL interval [%.4f, %.4f], library %.4f (L = %d, %d branches, %d substitutions)" % (lo, hi, q_lib, length, branches, counts.sum()))
    assert branches == sars.num_nodes - 1 and np.all(np.diag(counts) == 0) and counts.sum() > 0
    assert lo <= 148.9584 <= hi
    assert lo <= float("%.4f" % q_lib) <= hi
    # the genome length that gives the golden QUAL to the digit (DESIGN.md records it)
    s = pmx.spectrum_phred(counts, branches, 29840)
    assert "%.4f" % (255 + s[1][1] - 69 - s[1][3]) == "148.9584"
    # a tree without substitutions has no spectrum (loadSubstMatrixFromIndex returns an empty matrix)
    assert pmx.spectrum_phred(np.zeros((4, 4), np.int64), 10, 1000) is None


def _line(ref="C", alt="T", gt="1", pl="255,69", ad="5,53", info="DP=75;AC=1;AN=1;DP4=3,2,38,15;MQ=57", qual="20.5"):
    return "\t".join(["node_7618", "24152", ".", ref, alt, qual, ".", info, "GT:PL:AD", "%s:%s:%s" % (gt, pl, ad)])


def test_filter_and_gate(pmx, sars):
    counts, branches, length = pmx.spectrum_counts(sars)
    s = pmx.spectrum_phred(counts, branches, length)
    # the golden line with the golden PLs: a record with GT 1 and QUAL = 255 + s[C][C] - 69 - s[C][T]
    raw = GOLDEN_LINE[0].split("\t")
    raw[5], raw[9] = "3.2", "0:255,69:5,53"
    out = pmx.filter_line("\t".join(raw), s).split("\t")
    assert out[9] == "1:255,69:5,53" and out[:5] == raw[:5] and out[6:9] == raw[6:9]
    assert out[5] == "%.4f" % (255 + s[1][1] - 69 - s[1][3])
    assert pmx.filter_line(_line(), s).split("\t")[9] == "1:255,69:5,53"
    assert pmx.filter_line(_line(ad="30,28"), s) == ""                      # ALT below a strict majority
    assert pmx.filter_line(_line(ad="29,29"), s) == ""
    assert pmx.filter_line(_line(ad="1,3"), s, min_depth=5) == ""           # total AD below --min-depth
    assert pmx.filter_line(_line(ad="1,3"), s, min_depth=4) != ""
    q = 255 + s[1][1] - 69 - s[1][3]
    assert pmx.filter_line(_line(), s, min_qual=q + 0.01) == ""             # QUAL below --min-qual
    assert pmx.filter_line(_line(), s, min_qual=q - 0.01) != ""
    assert pmx.filter_line(_line(pl="0,90"), s) == ""                       # the reference allele wins
    assert pmx.filter_line(_line(alt="."), s) == ""
    # a '*' ALT keeps its likelihood: with PL 255,0 it wins by exactly 255 + s[C][C]
    star = pmx.filter_line(_line(alt="*", pl="255,0", ad="5,53"), s).split("\t")
    assert star[5] == "%.4f" % (255 + s[1][1]) and star[9].startswith("1:")
    # three alleles: the likelihoods are taken as they stand when there is one per allele
    multi = pmx.filter_line(_line(alt="T,A", pl="255,69,255", ad="5,53,1"), s).split("\t")
    assert multi[9] == "1:255,69,255:5,53,1"
    # a non-ACGT REF (and an INFO that does not start with DP) takes the early return: kept as it is unless GT is 0
    assert pmx.filter_line(_line(ref="N"), s) == _line(ref="N")
    assert pmx.filter_line(_line(ref="N", gt="0"), s) == ""
    assert pmx.filter_line(_line(info="INDEL;DP=75"), s) == _line(info="INDEL;DP=75")
    assert pmx.filter_line("#CHROM\tPOS", s) == "#CHROM\tPOS"
    with pytest.raises(pmx.PmxError):
        pmx.filter_line(_line() + "\textra", s)
    # without a spectrum (src/conversion.cpp:163-178): header lines pass, records need ALT, a non-zero GT, QUAL and the gate
    assert pmx.filter_line("##fileformat=VCFv4.2", None) == "##fileformat=VCFv4.2"
    assert pmx.filter_line(_line(qual="148.9"), None) == _line(qual="148.9")
    assert pmx.filter_line(_line(qual="."), None) == _line(qual=".")
    assert pmx.filter_line(_line(qual="20.5"), None) == ""
    assert pmx.filter_line(_line(qual="148.9", gt="0"), None) == ""
    assert pmx.filter_line(_line(qual="148.9", alt="."), None) == ""
    assert pmx.filter_line(_line(qual="148.9", ad="30,28"), None) == ""
    assert pmx.filter_line(_line(qual="148.9", ad="1,3"), None, min_depth=5) == ""


def _hist(entries):
    h = np.zeros((64, 2, 5), np.uint32)
    for q, strand, base, n in entries:
        h[q, strand, base] += n
    return h


ERRMOD_CASES = {
    "single base": (b"C", [(40, 0, 3, 1)]),
    "one allele only": (b"C", [(37, 0, 1, 11), (25, 1, 1, 9)]),
    "reference only, low quality": (b"A", [(4, 0, 0, 3)]),
    "5 / 53 over both strands": (b"C", [(40, 0, 1, 3), (38, 1, 1, 2), (40, 0, 3, 30), (33, 0, 3, 8), (40, 1, 3, 10), (20, 1, 3, 5)]),
    "three alleles and an N": (b"G", [(40, 0, 2, 20), (40, 1, 0, 12), (30, 0, 3, 2), (12, 1, 4, 1)]),
    "more than 255 of one base and strand": (b"T", [(40, 0, 3, 300), (35, 1, 3, 40), (40, 0, 0, 280), (22, 1, 1, 7)]),
    "exactly 255": (b"A", [(40, 0, 0, 200), (40, 1, 2, 55)]),
    "N reference": (b"N", [(40, 0, 0, 6), (40, 1, 2, 3)]),
}


@pytest.mark.parametrize("case", sorted(ERRMOD_CASES))
def test_error_model_against_the_restatement(pmx, case):
    ref, entries = ERRMOD_CASES[case]
    h = _hist(entries)
    got, want = pmx.site_call(h, ref), gc.site(h, ref)
    print(case, got, want)
    assert got["alleles"] == want["alleles"] and got["ad"] == want["ad"] and got["dp4"] == want["dp4"]
    assert got["pl"] == want["pl"]
    assert got["n_bases"] == int(h.sum())


def test_writers_reproduce_the_golden_consensus(pmx, tmp_path):
    out = tmp_path / "isolate.consensus.fa"
    pmx.write_consensus(os.path.join(GOLDEN, "isolate.vcf"), os.path.join(GOLDEN, "isolate.ref.fa"), str(out), "isolate_consensus ref=node_7618")
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "isolate.consensus.fa"), "rb").read()
    # a record whose REF is not the reference base is an error, not a silent edit
    bad = tmp_path / "bad.vcf"
    bad.write_text("#CHROM\tPOS\tID\tREF\tALT\nnode_7618\t24152\t.\tG\tT\t1\t.\tDP=1\tGT:PL:AD\t1:255,0:0,9\n")
    with pytest.raises(pmx.PmxError):
        pmx.write_consensus(str(bad), os.path.join(GOLDEN, "isolate.ref.fa"), str(tmp_path / "x.fa"), "x")
    # tables -> records -> VCF: one hand-made site through the whole host path
    ref = b"ACGTACGTAC"
    hist, aux = np.zeros((len(ref), 64, 2, 5), np.uint32), np.zeros((len(ref), 4), np.uint32)
    for p in range(len(ref)):
        hist[p, 40, 0, b"ACGT".index(ref[p:p + 1])] = 20
        aux[p] = (20, 20 * 60, 0, 0)
    hist[4, 40, 0, 0], hist[4, 40, 0, 2], hist[4, 40, 1, 2] = 2, 30, 25      # A -> G at position 5
    aux[4] = (60, 57 * 60, 0, 3)
    phred = np.full((4, 4), 40.0)
    np.fill_diagonal(phred, 0.0)
    gt = pmx.Genotyper(hist, aux, ref, "chr", phred, min_depth=1, min_qual=30.0)
    recs = gt.records()
    assert len(recs) == 1
    f = recs[0].split("\t")
    want = gc.site(hist[4], b"A")
    assert f[:5] == ["chr", "5", ".", "A", "G"] and f[7] == "DP=60;AC=1;AN=1;DP4=2,0,30,25;MQ=60"
    assert f[9] == "1:%d,%d:2,55" % (want["pl"][0], want["pl"][1]) and f[5] == "%.4f" % (want["pl"][0] + 0.0 - want["pl"][1] - 40.0)
    gt.write_vcf(str(tmp_path / "s.vcf"), "s.bam")
    lines = open(tmp_path / "s.vcf").read().splitlines()
    assert lines[0] == "##fileformat=VCFv4.2" and lines[1] == "##contig=<ID=chr,length=10>" and lines[-1] == recs[0]
    assert lines[-2] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts.bam"
    for key in ("DP", "AC", "AN", "DP4", "MQ"):
        assert any(l.startswith("##INFO=<ID=%s," % key) for l in lines)
    pmx.write_consensus(str(tmp_path / "s.vcf"), _fasta(tmp_path, "chr", ref), str(tmp_path / "s.consensus.fa"), "s_consensus ref=chr")
    assert open(tmp_path / "s.consensus.fa").read() == ">s_consensus ref=chr\nACGTGCGTAC\n"


def _fasta(tmp_path, name, seq):
    p = tmp_path / (name + ".fa")
    p.write_bytes(b">" + name.encode() + b"\n" + seq + b"\n")
    return str(p)


def test_checker_reproduces_the_golden_line_from_the_reference_aligner(pmx, oracle, tmp_path):
    """The numpy pileup of tests/geno_checks.py on the compiled reference aligner's records of the demo reads, in the order
    of the BAM written from them: DP, AD, DP4, MQ and PL of the golden line at position 24152."""
    if not os.path.isdir(os.path.join(ROOT, "oracle", "_ref")):
        pytest.skip("oracle/_ref (compiled reference aligner) is absent")
    import pileup_golden as pg
    g, hist, aux, info = pg.demo_checker_tables(pmx, oracle, str(tmp_path))
    p = 24152 - 1
    site = gc.site(hist[p], g[p:p + 1])
    mq = int(np.float32(aux[p, 1]) / np.float32(hist[p].sum()))
    print("DP", aux[p, 0], site, "MQ", mq, "refused by the cap", info["refused_by_cap"], "reconciled pairs", info["reconciled_pairs"])
    assert aux[p, 0] == 75 and site["ad"] == [5, 53] and site["dp4"] == [3, 2, 38, 15] and mq == 57
    assert site["alleles"] == [1, 3] and site["pl"] == [255, 69]
    assert info["refused_by_cap"] > 0 and info["reconciled_pairs"] > 0
    # and the library's host path on those tables writes the golden record and the golden consensus
    counts, branches, length = pmx.spectrum_counts(pmx.Panman(os.path.join(GOLDEN, "sars_20000_twilight_dipper.panman")))
    gt = pmx.Genotyper(hist, aux, g, "node_7618", pmx.spectrum_phred(counts, branches, length))
    recs_out = gt.records()
    assert len(recs_out) == 1
    f, gold = recs_out[0].split("\t"), GOLDEN_LINE[0].split("\t")
    assert f[:5] == gold[:5] and f[8:] == gold[8:]
    gold_info = dict(kv.split("=") for kv in gold[7].split(";"))
    assert all(gold_info[k] == v for k, v in (kv.split("=") for kv in f[7].split(";")))
