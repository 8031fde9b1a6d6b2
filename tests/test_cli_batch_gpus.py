"""`panmap <panman> --batch FILE --gpus N` (panmap_amd/csrc/cli/panmap_main.cpp): the samples of the batch file dealt to N
processes that never meet, each sample whole on one GPU against that process's resident index.  The yardstick of every
equality is the same batch file under `--gpus 1`, one process and the file's order: every sample's files are byte-equal,
the report lines are the same set, the counts the same.  The ranks share the box's one device (PMX_DIST_SAME_DEVICE)."""
import gzip
import os
import re
import shutil
import time

import pytest

from cli_checks import run
from conftest import GOLDEN

PANMAN = "sars_20000_twilight_dipper.panman"
LINE = re.compile(r"^\[(\d+)/(\d+)\] (\S+) -> (.*) \(\d+ms\)$")


def _records(path):
    lines = gzip.open(path, "rt").read().split("\n")
    return ["\n".join(lines[i:i + 4]) + "\n" for i in range(0, len(lines) - 1, 4)]


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """a directory with the SARS tree, its index and five samples cut from the isolate's pairs: three paired ones of 2000, 1500
    and 1000 pairs, a single-end one, and a paired one whose mate file is one record short; -> (directory, batch lines)"""
    d = tmp_path_factory.mktemp("batch_gpus")
    shutil.copy(os.path.join(GOLDEN, PANMAN), d / PANMAN)
    r1, r2 = (_records(os.path.join(GOLDEN, "isolate_R%d.fastq.gz" % m)) for m in (1, 2))
    assert len(r1) == len(r2) >= 5500

    def cut(name, recs):
        with open(d / name, "w") as f:
            f.write("".join(recs))
        return str(d / name)
    lines = ["%s %s a\n" % (cut("a_R1.fastq", r1[:2000]), cut("a_R2.fastq", r2[:2000])),
             "%s %s deep/er/b\n" % (cut("b_R1.fastq", r1[2000:3500]), cut("b_R2.fastq", r2[2000:3500])),
             "%s %s short\n" % (cut("short_R1.fastq", r1[:500]), cut("short_R2.fastq", r2[:499])),
             "%s %s c\n" % (cut("c_R1.fastq", r1[3500:4500]), cut("c_R2.fastq", r2[3500:4500])),
             "%s single\n" % cut("single.fastq", r1[4500:5500])]
    assert run([PANMAN, "--stop", "index"], d, retry=True).returncode == 0
    return d, lines


def _batch(d, name, lines, gpus, stop, env=None):
    """the batch `lines` in a directory of its own; -> (the finished process, that directory)"""
    out = d / name
    out.mkdir()
    (out / "batch.txt").write_text("".join(lines))
    env = dict(os.environ if env is None else env, PMX_DIST_SAME_DEVICE="1")
    r = run([str(d / PANMAN), "--batch", "batch.txt", "--stop", stop, "--gpus", str(gpus)], out, env=env, timeout=600)
    return r, out


def _reports(stderr, n):
    """the report lines as {position: (prefix, what)}: every line that starts like one IS a whole one (no two ranks' lines
    interleaved), and every sample has exactly one"""
    got = {}
    for line in stderr.splitlines():
        if re.match(r"^\[\d+/", line) is None:
            continue                                              # (a stage's own `[index] ...` line, a message)
        m = LINE.match(line)
        assert m is not None and int(m.group(2)) == n and int(m.group(1)) not in got, line
        got[int(m.group(1))] = (m.group(3), m.group(4))
    assert sorted(got) == list(range(1, n + 1)), stderr[-2000:]
    return got


def _same_files(one, two, prefixes, exts):
    for p in prefixes:
        for ext in exts:
            a, b = open(one / (p + ext), "rb").read(), open(two / (p + ext), "rb").read()
            assert len(a) > 0 and a == b, (p, ext)


@pytest.mark.gpu
def test_two_ranks_write_what_one_process_writes(pmx, samples):
    d, lines = samples
    r1, one = _batch(d, "align_1", lines, 1, "align")
    r2, two = _batch(d, "align_2", lines, 2, "align")
    assert r1.returncode == 1 and r2.returncode == 1, (r1.stderr[-2000:], r2.stderr[-2000:])      # (the short sample)
    for r in (r1, r2):
        assert r.stderr.count("Batch mode: 5 samples") == 1 and r.stderr.count("Batch complete: 4 placed, 1 failed") == 1, r.stderr[-2000:]
    rep1, rep2 = _reports(r1.stderr, 5), _reports(r2.stderr, 5)
    print("report lines, --gpus 1:", rep1, "--gpus 2:", rep2)
    assert rep1 == rep2
    # the yardstick itself: the file's order, four samples placed on a node, the short one failed with the reference's message
    assert [int(m.group(1)) for m in map(LINE.match, r1.stderr.splitlines()) if m] == [1, 2, 3, 4, 5]
    assert [rep1[i][0] for i in range(1, 6)] == ["a", "deep/er/b", "short", "c", "single"]
    assert rep1[3][1].startswith("failed: File ") and "short_R2.fastq does not contain the same number of reads as" in rep1[3][1]
    good = ["a", "deep/er/b", "c", "single"]
    for i in (1, 2, 4, 5):
        assert rep1[i][1] in open(one / (rep1[i][0] + ".placement.tsv")).read().splitlines()[5].split("\t")[2].split(","), rep1[i]
    _same_files(one, two, good, (".placement.tsv", ".ref.fa", ".bam", ".bam.bai"))
    for out in (one, two):
        assert not os.path.exists(out / "short.placement.tsv")


@pytest.mark.gpu
def test_two_ranks_to_the_consensus(pmx, samples):
    d, lines = samples
    r1, one = _batch(d, "cons_1", [lines[3], lines[4]], 1, "consensus")
    r2, two = _batch(d, "cons_2", [lines[3], lines[4]], 2, "consensus")
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-2000:], r2.stderr[-2000:])
    assert "Batch complete: 2 placed, 0 failed" in r1.stderr and "Batch complete: 2 placed, 0 failed" in r2.stderr
    assert _reports(r1.stderr, 2) == _reports(r2.stderr, 2)
    _same_files(one, two, ["c", "single"], (".placement.tsv", ".ref.fa", ".bam", ".bam.bai", ".vcf", ".consensus.fa"))


@pytest.mark.gpu
def test_fewer_samples_than_gpus(pmx, samples):
    d, lines = samples
    r1, one = _batch(d, "few_1", [lines[3], lines[4]], 1, "place")
    r3, three = _batch(d, "few_3", [lines[3], lines[4]], 3, "place")
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr[-2000:], r3.stderr[-2000:])
    assert "Batch complete: 2 placed, 0 failed" in r3.stderr and _reports(r1.stderr, 2) == _reports(r3.stderr, 2)
    _same_files(one, three, ["c", "single"], (".placement.tsv",))


def test_a_device_nobody_has(samples):
    """every rank asks for a device ordinal the box does not have (without a GPU: for any device): the ranks exit non-zero
    before they take a sample, the parent ends the run with that code and says that nothing was reported"""
    d, lines = samples
    t0 = time.time()
    r, out = _batch(d, "no_device", lines, 2, "place", env=dict(os.environ, PMX_DEVICE="99"))
    assert r.returncode != 0 and time.time() - t0 < 60, (r.returncode, r.stderr[-500:])
    assert "opening the GPU" in r.stderr and "0 of 5 samples had been reported" in r.stderr, r.stderr[-1000:]
    assert "Batch mode: 5 samples" in r.stderr and "Batch complete" not in r.stderr and not any(LINE.match(l) for l in r.stderr.splitlines())
    assert not [f for f in os.listdir(out) if f != "batch.txt"]
