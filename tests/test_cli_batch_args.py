"""`panmap --batch FILE` with `--gpus N` and with `--meta` (panmap_amd/csrc/cli/panmap_main.cpp): what the command line refuses
before it builds an index or opens a device."""
import os
import shutil

import pytest

from cli_checks import run
from conftest import GOLDEN

READ = "@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"


@pytest.fixture()
def work(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text(READ)
    (tmp_path / "one.txt").write_text("r.fastq sample\n")
    (tmp_path / "none.txt").write_text("# reads1 [reads2] [prefix]\n\n   \n")
    return tmp_path


def _refused(r, *words):
    assert r.returncode == 1, (r.returncode, r.stderr[-500:])
    for w in words:
        assert w in r.stderr, (w, r.stderr[-500:])
    assert "Batch mode" not in r.stderr and "[index]" not in r.stderr       # nothing was built, no rank was started


@pytest.mark.parametrize("mode", [[], ["--meta"], ["--meta", "--filter-and-assign"]])
def test_more_than_sixteen_ranks(work, mode):
    _refused(run(["rsv.panman", "--batch", "one.txt", "--gpus", "17"] + mode, work, retry=True), "at most 16 ranks")


def test_meta_batch_with_an_amplicon_table(work):
    (work / "amp.tsv").write_text("a\tp1\n")
    _refused(run(["rsv.panman", "--meta", "--batch", "one.txt", "--amplicon-depth", "amp.tsv"], work, retry=True),
             "--amplicon-depth is not accepted with --batch")


def test_meta_batch_with_positional_reads(work):
    _refused(run(["rsv.panman", "r.fastq", "--meta", "--batch", "one.txt"], work, retry=True), "--batch takes the read files from the batch file")


@pytest.mark.parametrize("mode", [["--stop", "place"], ["--meta"], ["--gpus", "2"], ["--meta", "--gpus", "2"]])
def test_a_batch_file_without_a_sample(work, mode):
    _refused(run(["rsv.panman", "--batch", "none.txt"] + mode, work, retry=True), "No samples found in batch file")


def test_meta_alone_still_needs_reads(work):
    _refused(run(["rsv.panman", "--meta"], work, retry=True), "--meta needs reads")
