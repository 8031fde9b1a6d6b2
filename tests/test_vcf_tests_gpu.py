"""mpileup's bias annotations on the GPU: the tables of the device's bias pass (k_pileup_bias, Pileup.bias) against the numpy
restatement of tests/bias_checks.py word for word on every crafted leg, the forms a site list can take, the README demo
through the aligner against all 8,449 `bcftools call` lines with an alternative, and `panmap --annotate-vcf` against the
reference's published VCF."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import bias_checks as bc
from cli_checks import DEMO, run
import pileup_golden as pg
from test_genotype_gpu import _demo_files
from test_genotype_host import qual_interval
from test_pileup_reference import LEGS, leg_set
from test_vcf_tests_host import checker_bias, compare_with_call


def _run_leg(pmx, ctx, leg_name):
    leg, ds = leg_set(leg_name)
    concat, off = pmx.concat_reads(ds["reads"])
    pu = pmx.Pileup(ctx)
    pu.run_records(ds["recs"], ds["cig"], concat, off, len(ds["ref"]), ds["paired"], False, quals=b"".join(ds["quals"]), names=ds["names"],
                   params=pmx.PileupParams(**leg["params"]))
    return ds, pu


@pytest.mark.gpu
@pytest.mark.parametrize("leg_name", LEGS)
def test_device_bias_tables_equal_the_restatement(pmx, ctx, leg_name, tmp_path_factory):
    """300 positions each: window edges, both reference ends, clips, deletions over a site, N, mapQ 0 and 255, the depth cap"""
    ds, pu = _run_leg(pmx, ctx, leg_name)
    ref = ds["ref"]
    w_hist, w_aux, w_bias, _, want_rank = checker_bias(pmx, leg_name, tmp_path_factory)
    assert np.array_equal(pu.read_info()[1], want_rank)
    hist, aux = pu.tables()
    assert np.array_equal(hist, w_hist) and np.array_equal(aux, w_aux)   # the shared quality rule left the window kernel's tables alone
    bias = pu.bias(np.arange(len(ref)), ref)
    print(leg_name, "bias pass %.3f ms for %d sites, %d bases" % (ctx.kernel_ms("pileup_bias"), len(ref), int(hist.sum())))
    assert bias.shape == (len(ref), 760) and bias.dtype == np.uint32
    bad = np.nonzero((bias != w_bias).any(axis=1))[0]
    assert bad.size == 0, "bias differs at %d positions, first %s: cells %s" % (bad.size, bad[:10], np.nonzero(bias[bad[0]] != w_bias[bad[0]])[0][:10])
    depth = hist.reshape(len(ref), -1).sum(axis=1)
    assert depth.sum() > 0
    for name, (at, bins) in bc.BLOCKS.items():
        assert np.array_equal(bias[:, at:at + 2 * bins].sum(axis=1), depth), name
    dp4_alt = np.asarray([sum(pmx.site_call(hist[p], ref[p:p + 1])["dp4"][2:]) for p in range(len(ref))])
    for name in ("pos", "scl", "mq", "bq"):
        at, bins = bc.BLOCKS[name]
        assert np.array_equal(bias[:, at + bins:at + 2 * bins].sum(axis=1), dp4_alt), name
    pu.close()


@pytest.mark.gpu
def test_site_list_forms(pmx, ctx, tmp_path_factory):
    fresh = pmx.Pileup(ctx)
    with pytest.raises(pmx.PmxError, match="nothing has been run"):
        fresh.bias([0], b"A")
    fresh.close()
    ds, pu = _run_leg(pmx, ctx, "variants250")
    ref, n = ds["ref"], len(ds["ref"])
    full = checker_bias(pmx, "variants250", tmp_path_factory)[2]
    assert pu.bias([], b"").shape == (0, 760)
    for sites in ([0], [n - 1], list(range(0, n, 2)), list(range(1, n, 2)), [0, n - 1]):
        got = pu.bias(sites, bytes(ref[p] for p in sites))
        assert np.array_equal(got, full[sites]), sites[:4]
    # the reference letter is an input: against N every base is alt
    p = int(np.argmax(full[:, :100].sum(axis=1)))
    as_n = pu.bias([p], b"N")[0]
    assert as_n[:100].sum() == 0 and as_n[100:200].sum() == full[p, :200].sum() and np.array_equal(as_n[bc.MQS:], full[p, bc.MQS:])
    for sites, what in (([5, 3], "ascending"), ([3, 3], "ascending"), ([-1], "outside"), ([n], "outside"), ([0, n], "outside")):
        with pytest.raises(pmx.PmxError, match=what):
            pu.bias(sites, b"A" * len(sites))
    a, b = pu.bias(np.arange(n), ref), pu.bias(np.arange(n), ref)
    assert np.array_equal(a, b) and np.array_equal(a, full)
    hist, aux = pu.tables()                                     # the run's own tables are untouched by the pass
    w = checker_bias(pmx, "variants250", tmp_path_factory)
    assert np.array_equal(hist, w[0]) and np.array_equal(aux, w[1])
    pu.close()
    # a site nobody covers: one read over [100, 150) of a 300-base reference
    import geno_checks as gc
    recs = np.zeros(1, gc.REC_DTYPE)
    recs[0] = (100, 150, 0, 50, 60, 0, 0, 1, 1, gc.HAS_ALN, 0, 0)
    lone = pmx.Pileup(ctx)
    lone.run_records(recs, np.asarray([50 << 4], np.uint32), b"A" * 50, np.asarray([0, 50], np.int64), 300, False, False, quals=b"5" * 50, names=[b"r0"])
    got = lone.bias([10, 99, 100, 149, 150, 299], b"AAAAAA")
    assert [int(r.sum()) for r in got] == [0, 0, 5, 5, 0, 0]
    assert got[2][bc.POS + int(1 / 51 * 99)] == 1 and got[3][bc.POS + int(50 / 51 * 99)] == 1 and got[2][bc.BQ + 20] == 1 and got[2][bc.MQ + 59] == 1
    lone.close()


@pytest.mark.gpu
def test_demo_through_the_aligner_equals_the_call_lines(pmx, ctx):
    """the demo reads through the device aligner and pileup, the bias pass at the 8,449 sites with an alternative -- more
    sites than the launch has blocks -- and site_tests against the reference's `call` lines, text for text"""
    import test_genotype_gpu as tg
    genome = tg._genome()
    got = tg._pileup(pmx, ctx, genome, tg._isolate_set(pmx), 250)
    leg = pg.demo_leg()
    sites = np.asarray([bc.golden_tests(l)[0] for l in leg["call"] if bc.golden_tests(l) is not None])
    assert len(sites) == 8449 and np.all(np.diff(sites) > 0)
    rows = got["pu"].bias(sites, bytes(genome[p] for p in sites))
    print("bias pass: %.3f ms for %d sites; window kernel %.3f ms" % (ctx.kernel_ms("pileup_bias"), len(sites), got["ms"]))
    bias = np.zeros((len(genome), 760), np.uint32)
    bias[sites] = rows
    n, bad = compare_with_call(pmx, leg, got["hist"], got["aux"], bias, genome)
    assert n == 8449
    assert not bad, "%d of %d lines differ, first %s" % (len(bad), n, bad[:5])
    # the same rows from a list of one and from every position
    p = 24152 - 1
    assert np.array_equal(got["pu"].bias([p], genome[p:p + 1])[0], bias[p])
    every = got["pu"].bias(np.arange(len(genome)), genome)
    assert np.array_equal(every[sites], rows)


PARENT_HEADER = """##fileformat=VCFv4.2
##contig=<ID=node_7618,length=29709>
##INFO=<ID=DP,Number=1,Type=Integer,Description="Raw read depth">
##INFO=<ID=AC,Number=A,Type=Integer,Description="Allele count in genotypes for each ALT allele, in the same order as listed">
##INFO=<ID=AN,Number=1,Type=Integer,Description="Total number of alleles in called genotypes">
##INFO=<ID=DP4,Number=4,Type=Integer,Description="Number of high-quality ref-forward , ref-reverse, alt-forward and alt-reverse bases">
##INFO=<ID=MQ,Number=1,Type=Integer,Description="Average mapping quality">
##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
##FORMAT=<ID=PL,Number=G,Type=Integer,Description="List of Phred-scaled genotype likelihoods">
##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Allelic depths (high-quality bases)">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s.bam
"""


@pytest.mark.gpu
def test_demo_command_line_annotates_the_record(pmx, sars, tmp_path):
    _demo_files(tmp_path)
    r = run(DEMO + ["-o", "ann", "--annotate-vcf"], tmp_path, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(tmp_path / "ann.vcf").read().splitlines()
    golden = open(os.path.join(GOLDEN, "isolate.vcf")).read().splitlines()
    gold = [l for l in golden if not l.startswith("#")][0].split("\t")
    recs = [l.split("\t") for l in lines if not l.startswith("#")]
    assert len(recs) == 1
    f = recs[0]
    print(f)
    assert f[7] == gold[7]                                      # INFO, byte for byte
    assert f[:5] == gold[:5] and f[6] == gold[6] and f[8:] == gold[8:]
    lo, hi, _, _ = qual_interval(pmx, sars)
    assert lo <= float(f[5]) <= hi and len(f[5].split(".")[1]) == 4
    want = [l for l in golden if l.startswith("##INFO=<ID=") and l.split("=<ID=")[1].split(",")[0] in bc.KEYS]
    assert len(want) == 8 and [l for l in lines if l in want] == want
    # without the switch: the file as it was before the switch existed
    r = run(DEMO + ["-o", "plain"], tmp_path, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = open(tmp_path / "plain.vcf").read()
    assert plain.startswith(PARENT_HEADER % "plain") and plain.count("\n") == PARENT_HEADER.count("\n") + 1
    pf = plain.splitlines()[-1].split("\t")
    assert pf[:7] == f[:7] and pf[8:] == f[8:]
    assert pf[7] == ";".join(kv for kv in f[7].split(";") if kv.split("=")[0] not in bc.KEYS) == "DP=75;AC=1;AN=1;DP4=3,2,38,15;MQ=57"
    for ext in (".bam", ".placement.tsv", ".ref.fa"):
        assert open(tmp_path / ("plain" + ext), "rb").read() == open(tmp_path / ("ann" + ext), "rb").read(), ext
    assert open(tmp_path / "plain.consensus.fa").read() == open(tmp_path / "ann.consensus.fa").read().replace(">ann_", ">plain_")
    # the switch under --batch
    (tmp_path / "batch.txt").write_text("isolate_R1.fastq.gz isolate_R2.fastq.gz out/b\n")
    r = run([DEMO[0], "--batch", "batch.txt", "--annotate-vcf"], tmp_path, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "out" / "b.vcf").read() == open(tmp_path / "ann.vcf").read().replace("ann.bam", "out/b.bam")
