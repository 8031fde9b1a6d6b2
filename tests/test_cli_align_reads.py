"""`panmap <panman> <reads> --meta --filter-and-assign --align-reads --min-num-align K` (panmap_amd/csrc/cli/panmap_main.cpp):
what it refuses, that the mode's three files stay what they are without the two options, and `<prefix>_mgsr_aligned/` --
reference.fa against the restated text, every BAM against pmx.write_bam of align_assigned's result for that head."""
import os
import re
import shutil

import pytest

import align_assigned_checks as aa
import assign_checks as ac
from cli_checks import run
from conftest import GOLDEN

FILES = (".mgsr.assignedReads.fastq", ".mgsr.assignedReads.out", ".mgsr.assignedReadsLCANode.out")
BASE = ["--meta", "--filter-and-assign", "--discard", "0.6"]


def _qual(i, n):
    return "".join(chr(33 + (7 * j + i) % 40) for j in range(n))


def _write(path, reads, names, fasta=False):
    with open(path, "w") as f:
        for i, (nm, r) in enumerate(zip(names, reads)):
            f.write(">%s\n%s\n" % (nm, r.decode()) if fasta else "@%s\n%s\n+\n%s\n" % (nm, r.decode(), _qual(i, len(r))))


def test_refusals(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    for opts, what in ((["--meta", "--align-reads"], "option --align-reads is not accepted without --filter-and-assign"),
                       (["--meta", "--min-num-align", "5"], "option --min-num-align is not accepted without --filter-and-assign"),
                       (["--align-reads", "--min-num-align=5"], "option --align-reads is not accepted without --filter-and-assign"),
                       (["--meta", "--filter-and-assign", "--min-num-align", "5"], "option --min-num-align is not accepted without --align-reads")):
        r = run(["rsv.panman", "r.fastq"] + opts, tmp_path, retry=True)
        assert r.returncode == 1 and what in r.stderr, (opts, r.stderr[-500:])
        assert "[index]" not in r.stderr and not os.path.exists(tmp_path / "r_mgsr_aligned")      # (before the PanMAN is opened)


@pytest.fixture(scope="module")
def library(pmx):
    """the library's side, once: (ids, genomes, FASTQ indices, results) per qualifying head at K, the names of the assigned
    reads, K and the number of heads below it"""
    ctx = pmx.Context(0)
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    meta = pmx.Meta.build(ctx, pm)
    reads = ac.rsv_reads()
    meta.set_reads(reads)
    res = meta.assign(aa.DISCARD)
    by_node = res.by_node()
    K = aa.choose_threshold(by_node)
    heads = [(meta.index.node_id(h), g, idx, pmx.records_to_results(recs, cig, False))
             for h, idx, g, recs, cig in pmx.align_assigned(ctx, pm, meta.index, res, reads, min_num_align=K)]
    assigned = [r for r in range(len(reads)) if res.fastq_index[r] >= 0]
    return heads, assigned, K, sum(1 for v in by_node.values() if len(v) < K), max(len(v) for v in by_node.values())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fastq", "fasta"])
def test_directory_equals_the_library(pmx, library, tmp_path, form):
    heads, assigned, K, below, _ = library
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    reads = ac.rsv_reads()
    names = ["read%d/x" % i for i in range(len(reads))]
    src = "reads.fa" if form == "fasta" else "reads.fastq"
    _write(tmp_path / src, reads, names, fasta=form == "fasta")
    plain = run(["rsv.panman", src] + BASE + ["-o", "plain"], tmp_path, retry=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert not os.path.exists(tmp_path / "plain_mgsr_aligned") and "Aligned reads" not in plain.stderr
    r = run(["rsv.panman", src] + BASE + ["--align-reads", "--min-num-align", str(K), "-o", "out"], tmp_path, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for sfx in FILES:
        assert open(tmp_path / ("out" + sfx), "rb").read() == open(tmp_path / ("plain" + sfx), "rb").read(), sfx
    d = tmp_path / "out_mgsr_aligned"
    assert 2 <= len(heads) <= 12
    want_names = {"reference.fa"} | {aa.sanitize(i) + e for i, _, _, _ in heads for e in (".bam", ".bam.bai")}
    assert set(os.listdir(d)) == want_names and len(want_names) == 1 + 2 * len(heads)
    assert open(d / "reference.fa").read() == aa.reference_fasta([(i, g.decode()) for i, g, _, _ in heads])
    assert "Aligned reads for %d nodes (%d below minNumAlign=%d)" % (len(heads), below, K) in r.stderr
    # every BAM, byte for byte (the writer's block layout is deterministic), and its index
    for node_id, genome, idx, results in heads:
        raw = [assigned[i] for i in idx]
        quals = [("I" * len(reads[x]) if form == "fasta" else _qual(x, len(reads[x]))).encode() for x in raw]
        want = tmp_path / "want.bam"
        pmx.write_bam(str(want), node_id, len(genome), [reads[x] for x in raw], quals, [names[x].encode() for x in raw], results, False)
        stem = aa.sanitize(node_id)
        assert open(d / (stem + ".bam"), "rb").read() == open(want, "rb").read(), node_id
        assert open(d / (stem + ".bam.bai"), "rb").read() == open(str(want) + ".bai", "rb").read(), node_id
        assert sum(x["mapped"] for x in results) > len(results) // 2


@pytest.mark.gpu
def test_a_threshold_above_every_count(library, tmp_path):
    _, _, _, _, most = library
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    reads = ac.rsv_reads()
    _write(tmp_path / "reads.fastq", reads, ["r%d" % i for i in range(len(reads))])
    r = run(["rsv.panman", "reads.fastq"] + BASE + ["--align-reads", "--min-num-align=%d" % (most + 1), "-o", "none"], tmp_path, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.listdir(tmp_path / "none_mgsr_aligned") == ["reference.fa"] and os.path.getsize(tmp_path / "none_mgsr_aligned" / "reference.fa") == 0
    m = re.search(r"Aligned reads for 0 nodes \((\d+) below minNumAlign=(\d+)\)", r.stderr)
    assert m and int(m.group(2)) == most + 1 and int(m.group(1)) > 1000
