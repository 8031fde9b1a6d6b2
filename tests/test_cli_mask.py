"""`panmap <panman> <reads> --meta --mask-reads N | --mask-seeds N` (panmap_amd/csrc/cli/panmap_main.cpp): what it refuses, its
abundance file against the library under the same mask, and --gpus 2 against --gpus 1."""
import os
import random
import shutil

import pytest

from cli_checks import run
from conftest import GOLDEN


def test_refusals(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    r = run(["rsv.panman", "r.fastq", "--meta", "--mask-reads", "1", "--mask-seeds", "1"], tmp_path, retry=True)
    assert r.returncode == 1 and "Only one masking parameter can be set at a time" in r.stderr
    for opt in (["--mask-reads", "-1"], ["--mask-seeds=-2"]):
        r = run(["rsv.panman", "r.fastq", "--meta"] + opt, tmp_path, retry=True)
        assert r.returncode == 1 and "negative" in r.stderr, opt
    for opt in (["--mask-reads", "1"], ["--mask-seeds", "1"]):
        r = run(["rsv.panman", "r.fastq"] + opt, tmp_path, retry=True)
        assert r.returncode == 1 and "not accepted without --meta" in r.stderr, opt
        r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign"] + opt, tmp_path, retry=True)
        assert r.returncode == 1 and "not accepted with --filter-and-assign" in r.stderr, opt
    for opt in (["--amplicon-depth", "depth.tsv"], ["--mask-reads-relative-frequency", "0.01"], ["--mask-seeds-relative-frequency", "0.01"]):
        r = run(["rsv.panman", "r.fastq", "--meta"] + opt, tmp_path, retry=True)
        assert r.returncode == 1 and "not accepted" in r.stderr and "amplicon groups, which this build does not make" in r.stderr, opt
    for name in os.listdir(tmp_path):
        assert not name.endswith(".abundance.out"), name


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def _tile(g, n, length=150):
    step = max(1, (len(g) - length) // n)
    return [g[i:i + length] for i in range(0, len(g) - length + 1, step)][:n]


def _reads():
    """the 70 / 30 mixture with every 25th read once more, two bases changed: k-min-mers that occur once; and five random
    reads, which hold nothing else"""
    a, b = _fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    reads = _tile(a, 700) + _tile(b, 300)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    planted = []
    for r in reads[::25]:
        q = list(r)
        for p in (40, 110):
            q[p] = flip.get(q[p], q[p])
        planted.append("".join(q))
    rnd = random.Random(2049)
    return reads + planted + ["".join(rnd.choice("ACGT") for _ in range(150)) for _ in range(5)]


def _write(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


@pytest.mark.gpu
def test_abundance_equals_the_library(pmx, tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    reads = _reads()
    _write(tmp_path / "reads.fastq", reads)
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    meta.set_reads([r.encode() for r in reads])
    n_unmasked = meta.n_reads
    meta.set_masks(seeds=1)
    meta.set_reads([r.encode() for r in reads])
    info = meta.mask_info()
    assert info["seeds_removed"] >= 40 and info["reads_left"] == meta.n_reads == n_unmasked - 5
    meta.score(top_oc=1000)
    want = pmx.format_abundance(meta.em(), meta.index.node_id)
    meta.close()
    r = run(["rsv.panman", "reads.fastq", "--meta", "--mask-seeds", "1", "-o", "out"], tmp_path, timeout=300, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "out.mgsr.abundance.out").read() == want and len(want.splitlines()) == 2
    line = [l for l in r.stderr.splitlines() if "Mask-seeds 1 turned on" in l]
    assert len(line) == 1 and ("turned on: %d seeds are removed during placement and EM... Total reads to process: %d"
                               % (info["seeds_removed"], info["reads_left"])) in line[0], r.stderr
    q = run(["rsv.panman", "reads.fastq", "--meta", "--mask-seeds", "1", "-o", "quiet", "--quiet"], tmp_path, timeout=300, retry=True)
    assert q.returncode == 0 and "Mask-seeds" not in q.stderr and open(tmp_path / "quiet.mgsr.abundance.out").read() == want


@pytest.mark.gpu
def test_gpus_two_equals_one(tmp_path):
    """`--gpus 2 --mask-reads 1` (two ranks on the one device): the abundance file and the reported numbers equal --gpus 1"""
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    _write(tmp_path / "reads.fastq", _reads())
    meet = tmp_path / "meet"
    meet.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=str(meet))
    r1 = run(["rsv.panman", "reads.fastq", "--meta", "--mask-reads", "1", "-o", "one"], tmp_path, timeout=300)
    r2 = run(["rsv.panman", "reads.fastq", "--meta", "--mask-reads", "1", "--gpus", "2", "-o", "two"], tmp_path, env=env, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-2000:])
    one = open(tmp_path / "one.mgsr.abundance.out", "rb").read()
    assert one and one == open(tmp_path / "two.mgsr.abundance.out", "rb").read()
    said = [l for l in r1.stderr.splitlines() if "Mask-reads 1 turned on" in l]
    assert len(said) == 1 and " 0 reads containing" not in said[0]
    assert [l for l in r2.stderr.splitlines() if "Mask-reads 1 turned on" in l] == said, (r1.stderr, r2.stderr)
