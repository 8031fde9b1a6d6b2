"""`panmap <panman> <reads> --meta --filter-and-assign` (panmap_amd/csrc/cli/panmap_main.cpp): what it refuses, and its three
files against Meta.assign + format_assigned on the same reads -- from one FASTQ, from two mate files and from a FASTA."""
import os
import shutil

import numpy as np
import pytest

import assign_checks as ac
from cli_checks import run
from conftest import GOLDEN


def _write(path, reads, names, fasta=False):
    with open(path, "w") as f:
        for nm, r in zip(names, reads):
            q = "".join(chr(33 + (7 * i + len(nm)) % 40) for i in range(len(r)))
            f.write(">%s\n%s\n" % (nm, r.decode()) if fasta else "@%s\n%s\n+\n%s\n" % (nm, r.decode(), q))


def _fastq(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4) if lines[i][0] == "@" and lines[i + 2] == "+"]


def _groups(text):
    out = set()
    for line in text.splitlines():
        ids, taxon, count, idx = line.split("\t")
        idx = [int(x) for x in idx.split(",")]
        assert taxon == "." and int(count) == len(idx) and idx == sorted(set(idx))
        out.add((frozenset(ids.split(",")), frozenset(idx)))
    return out


def test_refusals(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    r = run(["rsv.panman", "r.fastq", "--filter-and-assign"], tmp_path, retry=True)
    assert r.returncode == 1 and "--meta" in r.stderr
    r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign", "--gpus", "2"], tmp_path, retry=True)
    assert r.returncode == 1 and "one GPU" in r.stderr
    r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign", "-l", "1"], tmp_path, retry=True)
    assert r.returncode == 1 and "l >= 2" in r.stderr
    for opt in (["--breadth-ratio", "0.5"], ["--jplace"], ["--taxonomic-metadata", "x.tsv"], ["--maximum-taxon-number", "3"],
                ["--ambiguous-score-threshold", "1"], ["--mask-read-ends", "3"]):
        r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign"] + opt, tmp_path, retry=True)
        assert r.returncode == 1 and "not accepted" in r.stderr, opt


def _reads():
    return ac.rsv_reads()[:240] + [b"ACACACACAC" * 15, b"AAT" * 50]                # two reads --dust 5 drops


@pytest.fixture(scope="module")
def library(pmx):
    """(Meta, its result on the test's reads with --dust 5 --discard 0.6): what every form of the input must reproduce"""
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    meta.set_dust(5.0)
    meta.set_reads(_reads())
    return meta, meta.assign(0.6)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fastq", "mates", "fasta"])
def test_files_equal_the_library(pmx, library, tmp_path, form):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    reads = _reads()
    meta, res = library
    names = ["read%d/x" % i for i in range(len(reads))]
    if form == "mates":                                                             # R1 then R2: the library's input order
        half = len(reads) // 2
        _write(tmp_path / "r1.fastq", reads[:half], names[:half])
        _write(tmp_path / "r2.fastq", reads[half:], names[half:])
        files = ["r1.fastq", "r2.fastq"]
    else:
        files = ["reads.fa" if form == "fasta" else "reads.fastq"]
        _write(tmp_path / files[0], reads, names, fasta=form == "fasta")
    r = run(["rsv.panman"] + files + ["--meta", "--filter-and-assign", "--discard", "0.6", "--dust", "5", "-o", "out"], tmp_path, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (res.merged[-2:] == -1).all() and (res.state == ac.DISCARDED).any() and (res.state == ac.ASSIGNED).sum() > 100
    want_out, want_lca = pmx.format_assigned(res, meta.index.node_id)
    assert open(tmp_path / "out.mgsr.assignedReads.out").read() == want_out
    assert open(tmp_path / "out.mgsr.assignedReadsLCANode.out").read() == want_lca
    assert _groups(want_out) and len(_groups(want_lca)) <= len(_groups(want_out))
    # the FASTQ: the assigned reads in input order, with their names and qualities (FASTA: I)
    records = _fastq(tmp_path / "out.mgsr.assignedReads.fastq")
    kept = np.nonzero(res.state == ac.ASSIGNED)[0]
    assert len(records) == len(kept)
    given = {} if form == "fasta" else {nm: q for f in files for nm, _, q in _fastq(tmp_path / f)}
    for pos, raw in enumerate(kept.tolist()):
        nm, seq, qual = records[pos]
        assert res.fastq_index[raw] == pos and nm == names[raw] and seq == reads[raw].decode()
        assert qual == ("I" * len(seq) if form == "fasta" else given[nm])
    # a line's indices point at reads that hold the line's node among their assigned nodes
    heads = res.heads
    id_of = {meta.index.node_id(v): v for v in range(len(heads))}
    for ids, idx in _groups(want_out):
        members = {id_of[i] for i in ids}
        assert len({int(heads[v]) for v in members}) == 1
        for pos in idx:
            assert members & set(res.nodes_of(int(kept[pos])).tolist())
