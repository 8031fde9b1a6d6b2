"""`panmap <panman> <reads> --meta --filter-and-assign ... --gpus N` for ONE sample (panmap_amd/csrc/cli/panmap_main.cpp): the
ranks shard the reads, each assigns its rows of the distinct reads, rank 0 gathers and writes.  Two ranks on the one device over
the host-directory transport, as tests/test_meta_dist_gpu.py runs `--meta --gpus 2`: the files of --gpus 2 are byte-equal to
those of --gpus 1 -- the FASTQ, the two node lists and the breadths with a taxonomy; the `_mgsr_aligned` directory
(reference.fa, every BAM and BAI) at the threshold tests/test_cli_align_reads.py chooses; the two read-score reports of the
abundance mode -- and --gpus 3 on a sample of two reads, where one rank has neither reads nor rows.  No run on more than one
physical GPU exists."""
import os
import shutil

import pytest

import align_assigned_checks as aa
import assign_checks as ac
import taxa_checks as tc
from cli_checks import run
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FILES = (".mgsr.assignedReads.fastq", ".mgsr.assignedReads.out", ".mgsr.assignedReadsLCANode.out")
BREADTHS = ".mgsr.breadths.out"


def _same(d, a, b, suffixes):
    for sfx in suffixes:
        one = open(d / (a + sfx), "rb").read()
        assert one and one == open(d / (b + sfx), "rb").read(), sfx


def _both(d, args, tag, gpus=2):
    """the same arguments under --gpus 1 (-o one<tag>) and --gpus N (-o two<tag>) -> (the two runs)"""
    meet = d / ("meet" + tag)
    meet.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=str(meet))
    r1 = run(args + ["-o", "one" + tag], d, timeout=300)
    r2 = run(args + ["--gpus", str(gpus), "-o", "two" + tag], d, env=env, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-2000:])
    return r1, r2


@pytest.fixture(scope="module")
def box(pmx, tmp_path_factory):
    d = tmp_path_factory.mktemp("assign_gpus")
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), d / "rsv.panman")
    reads = ac.rsv_reads()
    with open(d / "reads.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@read%d/x\n%s\n+\n%s\n" % (i, r.decode(), "".join(chr(33 + (7 * j + i) % 40) for j in range(len(r)))))
    with open(d / "two.fastq", "w") as f:                              # two reads with lists of their own
        for i in (0, len(reads) // 2):
            f.write("@read%d\n%s\n+\n%s\n" % (i, reads[i].decode(), "I" * len(reads[i])))
    oriented = pmx.Index.build(pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman")), flank_mask=0, mode=0x100)
    parent = oriented.arrays()["parent"]
    tc.write_metadata(d / "meta.tsv", [oriented.node_id(v) for v in range(len(parent))], tc.label(parent, tc.RSV_T))
    return d


def test_the_four_files_with_a_taxonomy_and_breadth(box):
    args = ["rsv.panman", "reads.fastq", "--meta", "--filter-and-assign", "--breadth-ratio", "--taxonomic-metadata", "meta.tsv",
            "--maximum-taxon-number", "2"]
    r1, r2 = _both(box, args, "t")
    _same(box, "onet", "twot", FILES + (BREADTHS,))
    lines = open(box / ("twot" + FILES[1])).read().splitlines()
    assert len(lines) > 3 and any(l.split("\t")[1] != "." for l in lines)                 # reads were assigned, taxa were named
    assert len(open(box / ("twot" + BREADTHS)).read().splitlines()) > 100
    tally = [[l.split(" (")[-1] for l in r.stderr.splitlines() if " assigned, " in l] for r in (r1, r2)]
    assert len(tally[0]) == 1 and tally[1] == tally[0] and "spanning more than 2 taxa" in tally[0][0]   # rank 0 reports the one-GPU run's tallies


def test_the_aligned_directory(box):
    base = ["rsv.panman", "reads.fastq", "--meta", "--filter-and-assign", "--discard", str(aa.DISCARD)]
    plain = run(base + ["-o", "plain"], box, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    counts = [int(l.split("\t")[2]) for l in open(box / ("plain" + FILES[1])).read().splitlines()]
    K = aa.choose_threshold({i: [0] * c for i, c in enumerate(counts)})                   # the third most populated head's count
    _both(box, base + ["--align-reads", "--min-num-align", str(K)], "a")
    _same(box, "onea", "twoa", FILES)
    names = sorted(os.listdir(box / "onea_mgsr_aligned"))
    assert names == sorted(os.listdir(box / "twoa_mgsr_aligned")) and "reference.fa" in names
    assert sum(n.endswith(".bam") for n in names) >= 2 and sum(n.endswith(".bam.bai") for n in names) == sum(n.endswith(".bam") for n in names)
    for n in names:
        one = open(box / "onea_mgsr_aligned" / n, "rb").read()
        assert one and one == open(box / "twoa_mgsr_aligned" / n, "rb").read(), n


def test_the_read_score_reports(box):
    args = ["rsv.panman", "reads.fastq", "--meta", "--discard", "0.5", "--write-meta-read-scores-unfiltered", "--write-meta-read-scores-filtered"]
    _both(box, args, "s")
    _same(box, "ones", "twos", (".read_scores_info.unfiltered.tsv", ".read_scores_info.filtered.tsv", ".mgsr.abundance.out"))
    assert len(open(box / "twos.read_scores_info.unfiltered.tsv").read().splitlines()) > 100


def test_three_ranks_on_two_reads(box):
    _both(box, ["rsv.panman", "two.fastq", "--meta", "--filter-and-assign", "--breadth-ratio"], "3", gpus=3)
    _same(box, "one3", "two3", FILES + (BREADTHS,))
    assert len(open(box / ("two3" + FILES[0])).read().splitlines()) == 8                  # both reads assigned
