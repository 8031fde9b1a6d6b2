"""`panmap <panman> <reads> --meta --amplicon-depth FILE [--mask-reads-relative-frequency X | --mask-seeds-relative-frequency X |
--mask-reads N | --mask-seeds N]` (panmap_amd/csrc/cli/panmap_main.cpp): what it refuses, its abundance file and printed numbers
against the library under the same file and option, --gpus 2 against --gpus 1, and mates looked up by their own names."""
import os
import shutil

import numpy as np
import pytest

from cli_checks import run
from conftest import GOLDEN

RELATIVE = ("--mask-reads-relative-frequency", "--mask-seeds-relative-frequency")


def test_refusals(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    (tmp_path / "ok.tsv").write_text("a\tP1\n")
    (tmp_path / "bad.tsv").write_text("a\tP1\nb P1\n")
    base = ["rsv.panman", "r.fastq", "--meta"]
    for opt in RELATIVE:                                               # a relative option without --amplicon-depth
        r = run(base + [opt, "0.01"], tmp_path)
        assert r.returncode == 1 and "option %s is not accepted without --amplicon-depth" % opt in r.stderr, r.stderr
    r = run(base + ["--amplicon-depth", "absent.tsv"], tmp_path)       # a file that cannot be read, or is malformed
    assert r.returncode == 1 and "option --amplicon-depth is not accepted: cannot read absent.tsv" in r.stderr, r.stderr
    r = run(base + ["--amplicon-depth", "bad.tsv"], tmp_path)
    assert r.returncode == 1 and "option --amplicon-depth is not accepted" in r.stderr and "line 2" in r.stderr, r.stderr
    for opt in RELATIVE:                                               # negative values
        r = run(base + ["--amplicon-depth", "ok.tsv", opt, "-0.1"], tmp_path)
        assert r.returncode == 1 and opt in r.stderr and "negative" in r.stderr, r.stderr
    for two in ([RELATIVE[0], "0.1", RELATIVE[1], "0.1"], [RELATIVE[0], "0.1", "--mask-seeds", "1"], [RELATIVE[1], "0.1", "--mask-reads", "1"]):
        r = run(base + ["--amplicon-depth", "ok.tsv"] + two, tmp_path)
        assert r.returncode == 1 and "Only one masking parameter can be set at a time" in r.stderr, r.stderr
    for opt in (["--amplicon-depth", "ok.tsv"], [RELATIVE[0], "0.1"], [RELATIVE[1], "0.1"]):
        r = run(["rsv.panman", "r.fastq"] + opt, tmp_path)
        assert r.returncode == 1 and "option %s is not accepted without --meta" % opt[0] in r.stderr, r.stderr
        r = run(base + ["--filter-and-assign"] + opt, tmp_path)
        assert r.returncode == 1 and "option %s is not accepted with --filter-and-assign" % opt[0] in r.stderr, r.stderr
    for name in os.listdir(tmp_path):
        assert not name.endswith(".abundance.out"), name


def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def _tile(g, n, length=150):
    step = max(1, (len(g) - length) // n)
    return [g[i:i + length] for i in range(0, len(g) - length + 1, step)][:n]


def _sample():
    """the 70 / 30 rsv mixture, every 25th read once more with two bases changed -> (names, reads, the table's text, primer of
    every read or None): 50 consecutive reads a primer, every 7th read unlisted, the changed reads one more primer"""
    a, b = _fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    reads = _tile(a, 700) + _tile(b, 300)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    planted = []
    for r in reads[::25]:
        q = list(r)
        for p in (40, 110):
            q[p] = flip.get(q[p], q[p])
        planted.append("".join(q))
    primer = [None if i % 7 == 3 else "amp%02d" % (i // 50) for i in range(len(reads))] + ["amp_planted"] * len(planted)
    reads += planted
    names = ["r%d" % i for i in range(len(reads))]
    table = "".join("%s\t%s\n" % (n, p) for n, p in zip(names, primer) if p is not None)
    return names, reads, table, primer


def _write(path, names, reads, comment=""):
    with open(path, "w") as f:
        for n, r in zip(names, reads):
            f.write("@%s%s\n%s\n+\n%s\n" % (n, comment, r, "I" * len(r)))


def _library(pmx, tmp_path, names, reads, option, value):
    amplicons = pmx.load_amplicons(str(tmp_path / "depth.tsv"))
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    meta.set_amplicons(amplicons.groups_of(names), len(amplicons.names))
    if option in RELATIVE:
        meta.set_relative_masks(**{"reads" if option == RELATIVE[0] else "seeds": value})
    else:
        meta.set_masks(**{"reads" if option == "--mask-reads" else "seeds": value})
    meta.set_reads([r.encode() for r in reads])
    info = meta.mask_info()
    meta.score(top_oc=1000)
    want = pmx.format_abundance(meta.em(), meta.index.node_id)
    meta.close()
    return want, info, len(amplicons.names)


@pytest.mark.gpu
@pytest.mark.parametrize("option,value", [(RELATIVE[0], 0.05), (RELATIVE[1], 0.05), ("--mask-reads", 1)])
def test_abundance_equals_the_library(pmx, tmp_path, option, value):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    names, reads, table, primer = _sample()
    _write(tmp_path / "reads.fastq", names, reads, comment=" a comment after the name")
    (tmp_path / "depth.tsv").write_text(table)
    want, info, n_groups = _library(pmx, tmp_path, names, reads, option, value)
    assert info["reads_dropped"] + info["seeds_removed"] > 0 and info["reads_left"] > 0 and n_groups == 21
    r = run(["rsv.panman", "reads.fastq", "--meta", "--amplicon-depth", "depth.tsv", option, str(value), "-o", "out"], tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "out.mgsr.abundance.out").read() == want and len(want.splitlines()) >= 2
    kind = "Mask-reads" if "reads" in option else "Mask-seeds"
    line = [l for l in r.stderr.splitlines() if kind in l]
    tail = ("turned on: %d reads containing low coverage kminmers will be skipped during placement and EM... Total reads to process: %d"
            % (info["reads_dropped"], info["reads_left"]) if kind == "Mask-reads" else
            "turned on: %d seeds are removed during placement and EM... Total reads to process: %d" % (info["seeds_removed"], info["reads_left"]))
    assert len(line) == 1 and "%s %g %s" % (kind, value, tail) in line[0], r.stderr
    said = [l for l in r.stderr.splitlines() if "Amplicons:" in l]
    assert len(said) == 1 and "21 groups" in said[0] and "%d of %d reads not listed" % (sum(p is None for p in primer), len(reads)) in said[0]
    q = run(["rsv.panman", "reads.fastq", "--meta", "--amplicon-depth", "depth.tsv", option, str(value), "-o", "quiet", "--quiet"], tmp_path, timeout=300)
    assert q.returncode == 0 and "Mask-" not in q.stderr and "Amplicons" not in q.stderr and open(tmp_path / "quiet.mgsr.abundance.out").read() == want


@pytest.mark.gpu
def test_gpus_two_equals_one(tmp_path):
    """`--gpus 2` (two ranks on the one device) under a relative mask: the abundance file and the printed numbers equal --gpus 1"""
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    names, reads, table, _ = _sample()
    _write(tmp_path / "reads.fastq", names, reads)
    (tmp_path / "depth.tsv").write_text(table)
    meet = tmp_path / "meet"
    meet.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=str(meet))
    args = ["rsv.panman", "reads.fastq", "--meta", "--amplicon-depth", "depth.tsv", RELATIVE[0], "0.05"]
    r1 = run(args + ["-o", "one"], tmp_path, timeout=300)
    r2 = run(args + ["--gpus", "2", "-o", "two"], tmp_path, env=env, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-2000:])
    one = open(tmp_path / "one.mgsr.abundance.out", "rb").read()
    assert one and one == open(tmp_path / "two.mgsr.abundance.out", "rb").read()
    for word in ("Mask-reads 0.05 turned on", "Amplicons:"):
        said = [l for l in r1.stderr.splitlines() if word in l]
        assert len(said) == 1 and " 0 reads containing" not in said[0]
        assert [l for l in r2.stderr.splitlines() if word in l] == said, (r1.stderr, r2.stderr)


@pytest.mark.gpu
def test_mates_are_looked_up_by_their_own_names(pmx, tmp_path):
    """a paired run: the first file's reads and the second file's carry names of their own, and the table lists them apart"""
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    names, reads, table, primer = _sample()
    half = len(reads) // 2
    # R1 = the first half, R2 = the second half (as sequenced, one file after the other): the library sees R1 then R2
    _write(tmp_path / "r1.fastq", names[:half], reads[:half])
    _write(tmp_path / "r2.fastq", names[half:], reads[half:])
    (tmp_path / "depth.tsv").write_text(table)
    want, info, _ = _library(pmx, tmp_path, names, reads, RELATIVE[0], 0.05)
    r = run(["rsv.panman", "r1.fastq", "r2.fastq", "--meta", "--amplicon-depth", "depth.tsv", RELATIVE[0], "0.05", "-o", "pair"], tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "pair.mgsr.abundance.out").read() == want
    assert "turned on: %d reads" % info["reads_dropped"] in r.stderr and "%d of %d reads not listed" % (sum(p is None for p in primer), len(reads)) in r.stderr
