"""`panmap <panman> <reads> --meta --filter-and-assign --breadth-ratio` (panmap_amd/csrc/cli/panmap_main.cpp): the switch's
refusals, and `<prefix>.mgsr.breadths.out` against Meta.assign(breadth=True) + format_breadths on the same reads, with the
three other files byte-equal to a run without the switch."""
import os
import shutil

import pytest

import assign_checks as ac
import breadth_checks as bc
import test_cli_assign as tca
from cli_checks import run
from conftest import GOLDEN

FILES = ("assignedReads.fastq", "assignedReads.out", "assignedReadsLCANode.out")


def test_refusals(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    # a switch, as in the reference: a number after it is refused, not taken for a reads file
    for value in (["--breadth-ratio", "0.5"], ["--breadth-ratio", "2"], ["--breadth-ratio", "1e-3"], ["--breadth-ratio=0.5"]):
        r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign"] + value, tmp_path, retry=True)
        assert r.returncode == 1 and "option --breadth-ratio is not accepted with a value (" in r.stderr and "it is a switch, as in the reference" in r.stderr, value
    r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign", "--breadth-ratio", "0.5"], tmp_path, retry=True)
    assert "(0.5)" in r.stderr
    for args in (["--meta", "--breadth-ratio"], ["--breadth-ratio"]):
        r = run(["rsv.panman", "r.fastq"] + args, tmp_path, retry=True)
        assert r.returncode == 1 and "option --breadth-ratio is not accepted without --filter-and-assign" in r.stderr, args
    for opt in (["--jplace"], ["--mask-read-ends", "3"]):
        r = run(["rsv.panman", "r.fastq", "--meta", "--filter-and-assign", "--breadth-ratio"] + opt, tmp_path, retry=True)
        assert r.returncode == 1 and "not accepted" in r.stderr and "breadth ratios" not in r.stderr, opt
    r = run(["--help"], tmp_path, retry=True)
    assert r.returncode == 0 and "--breadth-ratio" in r.stderr and ".mgsr.breadths.out" in r.stderr


@pytest.mark.gpu
def test_the_file_equals_the_library_and_the_others_do_not_change(pmx, tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    reads = tca._reads()
    tca._write(tmp_path / "reads.fastq", reads, ["read%d/x" % i for i in range(len(reads))])
    meta = pmx.Meta.build(pmx.Context(0), pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")))
    meta.set_dust(5.0)
    meta.set_reads(reads)
    res = meta.assign(0.6, breadth=True)
    common = ["rsv.panman", "reads.fastq", "--meta", "--filter-and-assign", "--discard", "0.6", "--dust", "5"]
    r = run(common + ["--breadth-ratio", "-o", "with"], tmp_path, retry=True)      # (a switch: the option after it is parsed as usual)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(common + ["-o", "without"], tmp_path, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(tmp_path / "with.mgsr.breadths.out").read()
    assert text == pmx.format_breadths(res, meta.index.node_id)
    lines = text.splitlines()
    assert lines[0] == bc.HEADER and len(lines) == 1 + int((res.heads == range(len(res.heads))).sum())
    assert sum(int(x.split("\t")[2]) > 0 for x in lines[1:]) > 100 and (res.state == ac.ASSIGNED).sum() > 100
    assert not os.path.exists(tmp_path / "without.mgsr.breadths.out")
    for name in FILES:
        assert open(tmp_path / ("with.mgsr." + name), "rb").read() == open(tmp_path / ("without.mgsr." + name), "rb").read(), name
    meta.close()
