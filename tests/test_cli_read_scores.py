"""`panmap <panman> <reads> --meta --write-meta-read-scores-unfiltered | --write-meta-read-scores-filtered`
(panmap_amd/csrc/cli/panmap_main.cpp): what it refuses before anything is built; `<prefix>.read_scores_info.unfiltered.tsv` and
`.filtered.tsv` against the text restated (tests/read_best_checks.py) from the library's read_best, read_info and raw_to_merged
on the same reads; the three tallies; the abundance file untouched; a batch against every sample alone."""
import os
import re
import shutil

import pytest

import read_best_checks as rb
from cli_checks import run
from conftest import GOLDEN
from test_meta_dist_gpu import _mixture

UNFILTERED, FILTERED = "--write-meta-read-scores-unfiltered", "--write-meta-read-scores-filtered"
DISCARD = 0.5


def test_refusals(tmp_path):
    """decided before an index is built or a GPU opened"""
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    for opt in (UNFILTERED, FILTERED):
        r = run(["rsv.panman", "r.fastq", opt], tmp_path, retry=True)
        assert r.returncode == 1 and ("option %s is not accepted without --meta" % opt) in r.stderr, (opt, r.stderr[-300:])
        r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign", opt], tmp_path, retry=True)
        assert r.returncode == 1 and ("option %s is not accepted with --filter-and-assign" % opt) in r.stderr, (opt, r.stderr[-300:])
        r = run(["rsv.panman", "r.fastq", "--meta", "--gpus", "2", opt], tmp_path, retry=True)
        assert r.returncode == 1 and ("option %s is not accepted with one sample over --gpus 2" % opt) in r.stderr, (opt, r.stderr[-300:])
    r = run(["--help"], tmp_path, retry=True)
    assert all(w in r.stderr for w in (UNFILTERED, FILTERED, ".read_scores_info.unfiltered.tsv"))
    for name in os.listdir(tmp_path):
        assert not name.endswith(".tsv") and not name.endswith(".abundance.out") and not name.endswith(".idx"), name


def _fastq_reads(path):
    lines = open(path).read().splitlines()
    return [(lines[i][1:], lines[i + 1].encode()) for i in range(0, len(lines), 4)]


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    """the rsv mixture (every tiled read of it scores in full at its genome) and, appended, 60 of its reads with one, two or three
    substitutions, which break the seedmers around them: the reads --discard 0.5 has something to drop among"""
    d = tmp_path_factory.mktemp("read_scores")
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), d / "rsv_4K.panman")
    _mixture(d)
    tiled = [x for x in _fastq_reads(d / "mix.fastq") if x[0][0] in "AB"]
    with open(d / "mix.fastq", "a") as out:
        for j, (_, s) in enumerate(tiled[::len(tiled) // 60][:60]):
            q = bytearray(s)
            for p in ((75,), (50, 100), (40, 75, 110))[j % 3]:
                q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4] if q[p] in b"ACGT" else q[p]
            out.write("@X%d\n%s\n+\n%s\n" % (j, q.decode(), "I" * len(q)))
    return d, _fastq_reads(d / "mix.fastq")


def _restated(pmx, reads, discard):
    """(unfiltered text, filtered text, merged reads, max, n_seedmers, raw -> merged) from the library on these reads"""
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    meta.set_reads(reads)
    mx, nb = meta.read_best()
    ns, _ = meta.read_info()
    raw = meta.raw_to_merged()
    meta.close()
    return rb.scores_text(ns, mx, nb, raw, discard, False), rb.scores_text(ns, mx, nb, raw, discard, True), mx, ns, raw


@pytest.mark.gpu
def test_both_files_equal_the_restated_text(pmx, box):
    d, named = box
    unf, fil, mx, ns, raw = _restated(pmx, [s for _, s in named], DISCARD)
    plain = run(["rsv_4K.panman", "mix.fastq", "--meta", "--discard", str(DISCARD), "-o", "plain"], d, timeout=300, retry=True)
    both = run(["rsv_4K.panman", "mix.fastq", "--meta", "--discard", str(DISCARD), UNFILTERED, FILTERED, "-o", "both"], d, timeout=300, retry=True)
    only_u = run(["rsv_4K.panman", "mix.fastq", "--meta", "--discard", str(DISCARD), UNFILTERED, "-o", "onlyu"], d, timeout=300, retry=True)
    only_f = run(["rsv_4K.panman", "mix.fastq", "--meta", "--discard", str(DISCARD), FILTERED, "-o", "onlyf"], d, timeout=300, retry=True)
    for r in (plain, both, only_u, only_f):
        assert r.returncode == 0, r.stderr[-2000:]
    name = lambda p, kind: d / ("%s.read_scores_info.%s.tsv" % (p, kind))
    assert open(name("both", "unfiltered")).read() == unf == open(name("onlyu", "unfiltered")).read()
    assert open(name("both", "filtered")).read() == fil == open(name("onlyf", "filtered")).read()
    assert not os.path.exists(name("onlyu", "filtered")) and not os.path.exists(name("onlyf", "unfiltered"))
    assert not os.path.exists(name("plain", "filtered")) and not os.path.exists(name("plain", "unfiltered"))

    # the filtered file has the extra column and lacks exactly the reads below the threshold
    rows_u = [l.split("\t") for l in unf.splitlines()]
    rows_f = [l.split("\t") for l in fil.splitlines()]
    assert len(rows_u[0]) == 6 and len(rows_f[0]) == 7 and rows_f[0][5] == "OvermaximumTaxonNumber" and all(x[5] == "0" for x in rows_f[1:])
    below = {m for m in range(len(mx)) if 0 < mx[m] < int(float(ns[m]) * DISCARD)}
    in_u, in_f = {int(x[0]) for x in rows_u[1:]}, {int(x[0]) for x in rows_f[1:]}
    assert below and in_u - in_f == below and in_f <= in_u and in_u == {m for m in range(len(mx)) if mx[m] > 0}
    assert [x[:5] + x[6:] for x in rows_f[1:]] == [x for x in rows_u[1:] if int(x[0]) in in_f]

    # the poly-A and (AC)n reads are in neither file
    low = {i for i, (nm, _) in enumerate(named) if nm[0] in "LM"}
    listed = {int(i) for x in rows_u[1:] for i in x[5].split(",")}
    assert len(low) == 200 and not (low & listed) and all(raw[i] < 0 or mx[raw[i]] == 0 for i in low)

    # the tallies count merged reads
    tally = lambda r, what: [int(m.group(1)) for m in re.finditer(r"\[meta\] (\d+) reads %s" % what, r.stderr)]
    for r in (both, only_u, only_f):
        t = tally(r, "unmapped"), tally(r, "discarded due to low parsimony score"), tally(r, "mapped to nodes")
        assert all(len(x) == 1 for x in t), r.stderr[-1500:]
        assert t[0][0] + t[1][0] + t[2][0] == len(mx) and t[0][0] == int((mx == 0).sum()) and t[1][0] == len(below) > 0
    assert not tally(plain, "unmapped") and "read_scores_info" not in plain.stderr

    # the abundances are those of a run without the switches
    want = open(d / "plain.mgsr.abundance.out", "rb").read()
    assert want and all(open(d / (p + ".mgsr.abundance.out"), "rb").read() == want for p in ("both", "onlyu", "onlyf"))


@pytest.mark.gpu
def test_batch_equals_every_sample_alone(tmp_path, box):
    d, named = box
    halves = (named[:600], named[400:])
    for k, part in enumerate(halves):
        with open(tmp_path / ("mix%d.fastq" % k), "w") as f:
            for nm, s in part:
                f.write("@%s\n%s\n+\n%s\n" % (nm, s.decode(), "I" * len(s)))
    shutil.copy(d / "rsv_4K.panman", tmp_path / "rsv.panman")
    prefixes = ("s0", "sub/s1")
    (tmp_path / "batch.txt").write_text("".join("%s %s\n" % (tmp_path / ("mix%d.fastq" % k), prefixes[k]) for k in range(2)))
    opts = ["--meta", "--discard", str(DISCARD), UNFILTERED, FILTERED]
    for k in range(2):
        r = run(["rsv.panman", "mix%d.fastq" % k] + opts + ["-o", "solo%d" % k], tmp_path, timeout=300, retry=True)
        assert r.returncode == 0, r.stderr[-2000:]
    r = run(["rsv.panman", "--batch", "batch.txt"] + opts, tmp_path, timeout=300)
    assert r.returncode == 0 and "Batch complete: 2 done, 0 failed" in r.stderr, r.stderr[-2000:]
    for k in range(2):
        for sfx in (".read_scores_info.unfiltered.tsv", ".read_scores_info.filtered.tsv", ".mgsr.abundance.out"):
            a, b = open(tmp_path / ("solo%d%s" % (k, sfx)), "rb").read(), open(tmp_path / (prefixes[k] + sfx), "rb").read()
            assert a and a == b, (k, sfx)
    assert open(tmp_path / "solo0.read_scores_info.unfiltered.tsv", "rb").read() != open(tmp_path / "solo1.read_scores_info.unfiltered.tsv", "rb").read()
