"""Genotype + consensus stages on the GPU: the README demo through the command line against the reference's golden VCF and
consensus FASTA, and the device pileup tables against the numpy restatement of tests/geno_checks.py -- every counter at
every position, on real pairs, synthetic pairs and single-end long reads, with and without the depth cap."""
import os
import shutil

import numpy as np
import pytest

from cli_checks import DEMO, run
from conftest import GOLDEN

import geno_checks as gc
from test_genotype_host import GOLDEN_LINE, qual_interval


def _demo_files(tmp_path):
    for f in DEMO:
        shutil.copy(os.path.join(GOLDEN, f), tmp_path / f)


def _genome():
    return b"".join(l.strip() for l in open(os.path.join(GOLDEN, "isolate.ref.fa"), "rb") if not l.startswith(b">"))


@pytest.mark.gpu
def test_demo_default_stop_writes_the_golden_call_and_consensus(pmx, sars, tmp_path):
    _demo_files(tmp_path)
    r = run(DEMO + ["-o", "isolate"], tmp_path, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "not part of this build" not in r.stderr
    assert open(tmp_path / "isolate.consensus.fa", "rb").read() == open(os.path.join(GOLDEN, "isolate.consensus.fa"), "rb").read()
    lines = open(tmp_path / "isolate.vcf").read().splitlines()
    assert lines[0] == "##fileformat=VCFv4.2" and "##contig=<ID=node_7618,length=29709>" in lines
    assert [l for l in lines if l.startswith("#CHROM")] == ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tisolate.bam"]
    recs = [l.split("\t") for l in lines if not l.startswith("#")]
    gold = GOLDEN_LINE[0].split("\t")
    print(recs)
    assert len(recs) == 1
    f = recs[0]
    assert f[:5] == gold[:5] == ["node_7618", "24152", ".", "C", "T"] and f[6] == gold[6] and f[8:] == gold[8:] == ["GT:PL:AD", "1:255,69:5,53"]
    gold_info = dict(kv.split("=") for kv in gold[7].split(";"))
    info = dict(kv.split("=") for kv in f[7].split(";"))
    assert set(info) == {"DP", "DP4", "MQ", "AC", "AN"} and all(gold_info[k] == v for k, v in info.items())   # every key written equals the golden's
    assert info["DP"] == "75" and info["DP4"] == "3,2,38,15" and info["MQ"] == "57"
    lo, hi, _, _ = qual_interval(pmx, sars)
    assert lo <= float(f[5]) <= hi and len(f[5].split(".")[1]) == 4
    # the earlier stages are untouched by the later ones
    r2 = run(DEMO + ["-o", "upto", "--stop", "align"], tmp_path, timeout=240)
    assert r2.returncode == 0 and not os.path.exists(tmp_path / "upto.vcf") and not os.path.exists(tmp_path / "upto.consensus.fa")
    for ext in (".placement.tsv", ".ref.fa", ".bam"):
        assert open(tmp_path / ("isolate" + ext), "rb").read() == open(tmp_path / ("upto" + ext), "rb").read(), ext
    # --stop genotype ends before the consensus; the gate's options reach the filter; --baq is refused
    r3 = run(DEMO + ["-o", "geno", "--stop", "genotype", "--min-qual", "200"], tmp_path, timeout=240)
    assert r3.returncode == 0 and not os.path.exists(tmp_path / "geno.consensus.fa")
    assert [l for l in open(tmp_path / "geno.vcf").read().splitlines() if not l.startswith("#")] == []
    r4 = run(DEMO + ["-o", "baq", "--baq"], tmp_path, timeout=240)
    assert r4.returncode == 1 and "--baq" in r4.stderr


def _isolate_set(pmx):
    n1, s1, q1 = pmx.read_fastx(os.path.join(GOLDEN, "isolate_R1.fastq.gz"))
    n2, s2, q2 = pmx.read_fastx(os.path.join(GOLDEN, "isolate_R2.fastq.gz"))
    n = len(s1)
    seqs, quals, names = [None] * (2 * n), [None] * (2 * n), [None] * (2 * n)
    seqs[0::2], seqs[1::2] = s1, s2
    quals[0::2], quals[1::2] = q1, q2
    names[0::2], names[1::2] = n1, n2
    return dict(name="isolate pairs", reads=seqs, quals=quals, names=names, paired=True)


def _synth_pairs(pmx, genome):
    concat, off = pmx.simulate_paired_reads_8d(genome, 20000)
    return dict(name="20,000 synthetic pairs", reads=[bytes(concat[off[i]:off[i + 1]]) for i in range(len(off) - 1)], quals=None, names=None, paired=True)


def _long_reads(pmx, genome):
    return dict(name="300 long reads", reads=pmx.simulate_long_reads(genome, 300, 6000), quals=None, names=None, paired=False)


def _pileup(pmx, ctx, genome, ds, max_depth, order=None):
    """align + device pileup of one data set; order: a permutation of the pairs / reads"""
    unit = 2 if ds["paired"] else 1
    idx = list(range(len(ds["reads"])))
    if order is not None:
        idx = [unit * k + m for k in order for m in range(unit)]
    reads = [ds["reads"][i] for i in idx]
    quals = None if ds["quals"] is None else [ds["quals"][i] for i in idx]
    names = None if ds["names"] is None else [ds["names"][i] for i in idx]
    rs = pmx.ReadSet(ctx, reads)
    if quals is not None:
        rs.set_qualities(quals)
    al = pmx.Aligner(ctx, genome, sum(len(x) for x in reads) // len(reads))
    al.align_readset(rs, ds["paired"], ds["paired"])
    pu = pmx.Pileup(ctx)
    pu.run(al, rs, len(genome), ds["paired"], ds["paired"], names=names, params=pmx.PileupParams(max_depth=max_depth))
    hist, aux = pu.tables()
    flags, rank = pu.read_info()
    recs, cig = al.fetch()
    ms = ctx.kernel_ms("pileup")
    out = dict(hist=hist, aux=aux, flags=flags, rank=rank, recs=recs.copy(), cig=cig.copy(), reads=reads, quals=quals, names=names, ms=ms,
               bytes=pu.bytes_moved(), pu=pu, al=al, rs=rs)
    return out


def _check_against_restatement(pmx, genome, ds, got, max_depth):
    concat, off = pmx.concat_reads(got["reads"])
    hist, aux, info = gc.pileup_tables(got["recs"], got["cig"], concat, off, len(genome), ds["paired"], ds["paired"], got["rank"],
                                       quals=None if got["quals"] is None else b"".join(got["quals"]), names=got["names"], max_depth=max_depth)
    print("%s, max_depth %d: %d reads in the pileup, %d refused by the cap, %d reconciled pairs, kernel %.3f ms, %d bytes" %
          (ds["name"], max_depth, int(info["admitted"].sum()), info["refused_by_cap"], info["reconciled_pairs"], got["ms"], got["bytes"]))
    assert np.array_equal((got["flags"] & 1).astype(bool), info["admitted"])
    assert int(((got["flags"] & 2) != 0).sum()) == 2 * info["reconciled_pairs"]
    assert np.array_equal(got["aux"], aux), "aux differs at positions %s" % np.nonzero((got["aux"] != aux).any(axis=1))[0][:10]
    bad = np.nonzero((got["hist"] != hist).reshape(len(genome), -1).any(axis=1))[0]
    assert bad.size == 0, "hist differs at %d positions, first %s" % (bad.size, bad[:10])
    assert hist.sum() > 0
    return info


@pytest.mark.gpu
def test_device_tables_equal_the_restatement(pmx, ctx, tmp_path):
    genome = _genome()
    seen = dict(soft_clip=0, insertion=0, deletion=0, n_base=0, improper=0, overlapping=0, refused=0)
    for ds in (_isolate_set(pmx), _synth_pairs(pmx, genome), _long_reads(pmx, genome)):
        for max_depth in (250, 0):
            got = _pileup(pmx, ctx, genome, ds, max_depth)
            if max_depth == 250:
                # the inputs exercise the rules; the rank the library reports is a BAM order (ascending starts, no gaps)
                concat, off = pmx.concat_reads(got["reads"])
                for k, v in gc.features(got["recs"], got["cig"], np.frombuffer(concat, np.uint8), off, ds["paired"]).items():
                    seen[k] += v
                written = got["rank"] != gc.NONE
                by_rank = np.argsort(got["rank"][written], kind="stable")
                assert np.array_equal(np.sort(got["rank"][written]), np.arange(written.sum()))
                starts = got["recs"]["rs"][written][by_rank]
                mapped = (got["recs"]["flags"][written][by_rank] & 4) != 0
                assert np.all(np.diff(starts[mapped]) >= 0)
            info = _check_against_restatement(pmx, genome, ds, got, max_depth)
            if max_depth == 250:
                seen["overlapping"] += info["reconciled_pairs"]
                seen["refused"] += info["refused_by_cap"]
            else:
                assert info["refused_by_cap"] == 0
            if ds["name"] == "isolate pairs" and max_depth == 250:
                # the order the library admits the reads in is the order of the BAM written from the same records
                import test_bam as tb
                seqs, quals, names = pmx.read_fastq_paired(os.path.join(GOLDEN, "isolate_R1.fastq.gz"), os.path.join(GOLDEN, "isolate_R2.fastq.gz"))
                bam = str(tmp_path / "iso.bam")
                pmx.write_bam(bam, "node_7618", len(genome), seqs, quals, names, pmx.records_to_results(got["recs"], got["cig"], True), True)
                assert np.array_equal(gc.rank_from_bam(tb.parse_bam(bam)[2], names, True), got["rank"])
                # and the golden line's numbers come out of the device tables
                p = 24152 - 1
                site = pmx.site_call(got["hist"][p], genome[p:p + 1])
                assert got["aux"][p, 0] == 75 and site["pl"] == [255, 69] and site["ad"] == [5, 53] and site["dp4"] == [3, 2, 38, 15]
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.gpu
def test_tables_repeat_and_do_not_depend_on_the_read_order(pmx, ctx):
    """Two runs give identical tables.  With max_depth 0 a run on the shuffled reads does too for single-end reads.  For
    pairs the RULES depend on the file order of reads that start at one position (which mate htslib calls the first, and
    whether the base in front of an overlap sees its neighbour reconciled: sam.c:5969-6003, 6034), and that order follows
    the input order through the writer's sort; so for shuffled pairs the counters are compared with the quality bin summed
    out, and raw depth / deletions exactly."""
    genome = _genome()
    rng = np.random.Generator(np.random.PCG64(5))
    for ds in (_long_reads(pmx, genome), _synth_pairs(pmx, genome)):
        a = _pileup(pmx, ctx, genome, ds, 250)
        b = _pileup(pmx, ctx, genome, ds, 250)
        assert np.array_equal(a["hist"], b["hist"]) and np.array_equal(a["aux"], b["aux"])
        n_units = len(ds["reads"]) // (2 if ds["paired"] else 1)
        c = _pileup(pmx, ctx, genome, dict(ds, names=[b"r%d" % (i // 2 if ds["paired"] else i) for i in range(len(ds["reads"]))]), 0)
        d = _pileup(pmx, ctx, genome, dict(ds, names=[b"r%d" % (i // 2 if ds["paired"] else i) for i in range(len(ds["reads"]))]), 0,
                    order=rng.permutation(n_units))
        assert c["hist"].sum() == d["hist"].sum() > 0
        if not ds["paired"]:
            assert np.array_equal(c["hist"], d["hist"]) and np.array_equal(c["aux"], d["aux"])
        else:
            assert np.array_equal(c["hist"].sum(axis=1), d["hist"].sum(axis=1))
            assert np.array_equal(c["aux"][:, [0, 3]], d["aux"][:, [0, 3]])


@pytest.mark.gpu
def test_two_ranks_and_batch_write_the_same_files(pmx, tmp_path):
    _demo_files(tmp_path)
    r1 = run(DEMO + ["-o", "one"], tmp_path, timeout=240)
    assert r1.returncode == 0, r1.stderr[-2000:]
    meet = tmp_path / "meet"
    meet.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=str(meet))
    r2 = run(DEMO + ["-o", "two", "--gpus", "2"], tmp_path, env=env, timeout=1200)
    assert r2.returncode == 0, r2.stderr[-2000:]
    one_vcf = open(tmp_path / "one.vcf").read()
    assert open(tmp_path / "two.vcf").read() == one_vcf.replace("one.bam", "two.bam")
    assert open(tmp_path / "one.consensus.fa").read().replace(">one_", ">two_") == open(tmp_path / "two.consensus.fa").read()
    assert len([l for l in one_vcf.splitlines() if not l.startswith("#")]) == 1
    (tmp_path / "batch.txt").write_text("isolate_R1.fastq.gz isolate_R2.fastq.gz out/paired\nisolate_R1.fastq.gz single_end\n")
    r3 = run([DEMO[0], "--batch", "batch.txt"], tmp_path, timeout=600)
    assert r3.returncode == 0, r3.stderr[-2000:]
    for prefix in ("out/paired", "single_end"):
        assert os.path.exists(tmp_path / (prefix + ".vcf")) and os.path.exists(tmp_path / (prefix + ".consensus.fa")), prefix
    assert open(tmp_path / "out" / "paired.vcf").read() == one_vcf.replace("one.bam", "out/paired.bam")
    assert open(tmp_path / "out" / "paired.consensus.fa").read().startswith(">paired_consensus ref=node_7618\n")
