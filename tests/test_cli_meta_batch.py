"""`panmap <panman> --meta --batch FILE [--gpus N]` (panmap_amd/csrc/cli/panmap_main.cpp): the samples of a batch file against
ONE resident pmx_meta per process -- both indexes built and uploaded once --, alone and dealt to two ranks that share the
box's one device.  The yardstick: every sample run by itself (`--meta <reads> -o <prefix>`), whose files the batch must
reproduce byte for byte -- in particular the files of --filter-and-assign, which would differ if a tally or a list of one
sample survived into the next."""
import filecmp
import os
import re
import shutil

import pytest

from cli_checks import run
from conftest import GOLDEN

MIXES = ((700, 300), (300, 700), (1000, 0))
PREFIXES = ("s0", "sub/dir/s1", "s2")
ASSIGN_FILES = (".mgsr.assignedReads.fastq", ".mgsr.assignedReads.out", ".mgsr.assignedReadsLCANode.out", ".mgsr.breadths.out")
LINE = re.compile(r"^\[(\d+)/3\] (\S+) -> (.*) \(\d+ms\)$")


def _genome(path):
    return "".join(l.strip() for l in open(path) if not l.startswith(">")).upper()


@pytest.fixture(scope="module")
def mixes(tmp_path_factory):
    """a directory with the rsv tree, three mixtures tiled from two of its genomes (150-base reads at a fixed stride, as
    test_cli.py::test_meta_mixture_through_the_cli tiles them) and the batch file that names them by absolute path"""
    d = tmp_path_factory.mktemp("meta_batch")
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), d / "rsv_4K.panman")
    a, b = _genome(os.path.join(GOLDEN, "MZ515733.1.fa")), _genome(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    for k, (na, nb) in enumerate(MIXES):
        with open(d / ("mix%d.fastq" % k), "w") as out:
            def emit(g, n, pre):
                L = 150; step = max(1, (len(g) - L) // max(n, 1)); c = i = 0
                while c < n and i + L <= len(g):
                    out.write("@%s%d\n%s\n+\n%s\n" % (pre, c, g[i:i + L], "I" * L)); c += 1; i += step
            emit(a, na, "A"); emit(b, nb, "B")
    (d / "batch.txt").write_text("".join("%s %s\n" % (d / ("mix%d.fastq" % k), PREFIXES[k]) for k in range(3)))
    return d


def _solo(d, name, opts):
    """every sample by itself, under the prefix solo_k of a directory of its own"""
    out = d / name
    out.mkdir()
    for k in range(3):
        r = run([str(d / "rsv_4K.panman"), str(d / ("mix%d.fastq" % k)), "--meta", "-o", "solo_%d" % k] + opts, out, retry=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return out


def _batch(d, name, opts, gpus):
    out = d / name
    out.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1")
    r = run([str(d / "rsv_4K.panman"), "--meta", "--batch", str(d / "batch.txt")] + opts + (["--gpus", str(gpus)] if gpus > 1 else []), out, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.count("Batch mode: 3 samples") == 1 and r.stderr.count("Batch complete: 3 done, 0 failed") == 1, r.stderr[-2000:]
    assert r.stderr.count("[index]") == 1                              # built once, by the parent; the ranks above 0 are quiet
    reports = {}
    for line in r.stderr.splitlines():
        if re.match(r"^\[\d+/", line):
            m = LINE.match(line)
            assert m is not None and int(m.group(1)) not in reports, line
            reports[int(m.group(1))] = (m.group(2), m.group(3))
    assert sorted(reports) == [1, 2, 3] and [reports[i][0] for i in (1, 2, 3)] == list(PREFIXES), r.stderr[-2000:]
    if gpus == 1:                                                      # one process: the file's order
        assert [int(m.group(1)) for m in map(LINE.match, r.stderr.splitlines()) if m] == [1, 2, 3]
    return out, reports


def _same(solo, batch, suffixes):
    for k in range(3):
        for sfx in suffixes:
            a, b = open(solo / ("solo_%d%s" % (k, sfx)), "rb").read(), open(batch / (PREFIXES[k] + sfx), "rb").read()
            assert a == b, (k, sfx)


@pytest.mark.gpu
def test_abundances_alone_in_a_batch_and_over_two_ranks(pmx, mixes):
    solo = _solo(mixes, "em_solo", [])
    haps = [open(solo / ("solo_%d.mgsr.abundance.out" % k)).read().splitlines() for k in range(3)]
    print("haplotypes per sample:", [len(h) for h in haps])
    assert all(haps) and haps[0] != haps[1] and haps[1] != haps[2] and haps[0] != haps[2]   # (the samples differ: an equality below says something)
    for gpus in (1, 2):
        out, reports = _batch(mixes, "em_batch_%d" % gpus, [], gpus)
        _same(solo, out, (".mgsr.abundance.out",))
        assert [reports[i][1] for i in (1, 2, 3)] == ["%d haplotypes" % len(h) for h in haps]


@pytest.mark.gpu
def test_assigned_reads_alone_in_a_batch_and_over_two_ranks(pmx, mixes):
    opts = ["--filter-and-assign", "--breadth-ratio"]
    solo = _solo(mixes, "fa_solo", opts)
    n_assigned = [open(solo / ("solo_%d.mgsr.assignedReads.fastq" % k)).read().count("\n") // 4 for k in range(3)]
    sizes = [os.path.getsize(solo / ("solo_%d.mgsr.assignedReads.out" % k)) for k in range(3)]
    print("assigned reads per sample:", n_assigned, "bytes of assignedReads.out:", sizes)
    assert min(n_assigned) > 0 and min(sizes) > 0 and len(set(sizes)) == 3   # (three different answers)
    for k in range(3):
        assert open(solo / ("solo_%d.mgsr.breadths.out" % k)).read().count("\n") > 1              # (more than the header)
    for gpus in (1, 2):
        out, reports = _batch(mixes, "fa_batch_%d" % gpus, opts, gpus)
        _same(solo, out, ASSIGN_FILES)
        assert [reports[i][1] for i in (1, 2, 3)] == ["%d assigned reads" % n for n in n_assigned]


@pytest.mark.gpu
def test_align_reads_of_a_sample_of_the_batch(pmx, mixes):
    """--align-reads over two ranks: the directory of the second sample -- which follows another sample on its rank or runs
    beside one -- against the directory of that sample run by itself, file by file.  The threshold keeps the nodes that hold
    nearly all of the 700 reads of the sample's major genome: tens of BAMs, not the thousands of a low threshold"""
    opts = ["--filter-and-assign", "--align-reads", "--min-num-align", "690"]
    solo = mixes / "al_solo"
    solo.mkdir()
    r = run([str(mixes / "rsv_4K.panman"), str(mixes / "mix1.fastq"), "--meta", "-o", "solo_1"] + opts, solo, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, _ = _batch(mixes, "al_batch_2", opts, 2)
    want, got = solo / "solo_1_mgsr_aligned", out / (PREFIXES[1] + "_mgsr_aligned")
    names = sorted(os.listdir(want))
    print("files of the sample's directory:", len(names))
    assert "reference.fa" in names and len(names) >= 3 and sorted(os.listdir(got)) == names
    assert os.path.getsize(want / "reference.fa") > 0
    _, mismatch, errors = filecmp.cmpfiles(want, got, names, shallow=False)
    assert not mismatch and not errors
    for k in (0, 2):
        assert os.path.isdir(out / (PREFIXES[k] + "_mgsr_aligned"))


def test_a_missing_read_file(mixes, tmp_path):
    (tmp_path / "b.txt").write_text("nope.fastq\n")
    for opts in ([], ["--filter-and-assign", "--gpus", "2"]):
        r = run([str(mixes / "rsv_4K.panman"), "--meta", "--batch", "b.txt"] + opts, tmp_path, retry=True)
        assert r.returncode == 1 and "Batch line 1: reads file not found: nope.fastq" in r.stderr, r.stderr[-500:]
        assert "Batch mode" not in r.stderr
