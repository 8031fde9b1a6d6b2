"""The `panmap` command line and homopolymer-compressed (HPC) indexes: the index is authoritative (one that says hpc = 1 is
used as it is, with or without --hpc, and never rebuilt over), --hpc means "the index must be an HPC index", and this command
line does not build one.  CPU part: the argument and cache rules.  GPU part: `--stop place` against an HPC index."""
import os
import shutil

import numpy as np
import pytest

import hpc_checks as hc
from cli_checks import run
from conftest import GOLDEN


@pytest.fixture(scope="module")
def hpc_dir(pmx, tmp_path_factory):
    """a directory with the tree and an HPC index of it saved from Index.build(hpc=True) (reference defaults)"""
    d = tmp_path_factory.mktemp("hpc_cli")
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), d / "rsv.panman")
    pmx.Index.build(pmx.Panman(str(d / "rsv.panman")), hpc=True).save(str(d / "hpc.idx"))
    return d


def test_hpc_flag_needs_an_hpc_index(pmx, tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    r = run(["rsv.panman", "--hpc"], tmp_path)                          # nothing to load: it would have to build one
    assert r.returncode == 1 and "does not build one" in r.stderr, r.stderr
    assert "--hpc --stop index" in r.stderr and "PMX_INDEX_HPC" in r.stderr and "Index.build(hpc=True)" in r.stderr
    assert not (tmp_path / "rsv.panman.idx").exists()
    r = run(["rsv.panman", "--hpc", "--meta", "x.fq"], tmp_path)
    assert r.returncode == 1 and "--meta" in r.stderr
    # a usable index that is not homopolymer-compressed
    pmx.Index.build(pmx.Panman(str(tmp_path / "rsv.panman")), max_nodes=20).save(str(tmp_path / "plain.idx"))
    r = run(["rsv.panman", "-i", "plain.idx", "--hpc", "--stop", "index"], tmp_path)
    assert r.returncode == 1 and "plain.idx is not one" in r.stderr
    assert run(["rsv.panman", "-i", "plain.idx", "--stop", "index"], tmp_path).returncode == 0


def test_an_hpc_index_is_used_as_it_is_and_not_rebuilt_over(pmx, hpc_dir):
    idx = hpc_dir / "hpc.idx"
    before = idx.read_bytes()
    for extra in ([], ["--hpc"]):
        r = run(["rsv.panman", "-i", "hpc.idx", "--stop", "index"] + extra, hpc_dir)
        assert r.returncode == 0 and "(cached)" in r.stderr and "(built)" not in r.stderr, r.stderr
        assert pmx.Index.read_header(str(idx))["hpc"] is True and idx.read_bytes() == before
    # found in the cache (<panman>.idx) without --hpc on the command line
    shutil.copy(idx, hpc_dir / "rsv.panman.idx")
    r = run(["rsv.panman", "--stop", "index"], hpc_dir)
    assert r.returncode == 0 and "(cached)" in r.stderr
    assert pmx.Index.read_header(str(hpc_dir / "rsv.panman.idx"))["hpc"] is True
    # --meta does not take it
    (hpc_dir / "x.fq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    r = run(["rsv.panman", "x.fq", "-i", "hpc.idx", "--meta"], hpc_dir)
    assert r.returncode == 1 and "homopolymer-compressed" in r.stderr
    os.remove(hpc_dir / "rsv.panman.idx")


@pytest.mark.gpu
def test_place_stage_against_an_hpc_index(pmx, ctx, hpc_dir):
    """`panmap rsv.panman reads.fq -i hpc.idx --stop place`, with and without --hpc, writes the placement TSV place_lite
    writes for the same index and reads"""
    rsv = pmx.Panman(str(hpc_dir / "rsv.panman"))
    g = rsv.genome(rsv.find_node("MZ515733.1"))
    rng = np.random.default_rng(2)
    with open(hpc_dir / "reads.fq", "w") as f:
        for i in range(200):
            n = int(rng.integers(500, 3000))
            st = int(rng.integers(0, len(g) - n))
            r = hc.run_length_errors(rng, g[st:st + n]).decode()
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    index = pmx.Index.load(str(hpc_dir / "hpc.idx"))
    assert index.hpc
    placer = pmx.Placer(ctx, index)
    pmx.place_lite(ctx, placer, str(hpc_dir / "reads.fq"), "", str(hpc_dir / "want.placement.tsv"), pmx.TraversalParams(), index.node_id)
    want = (hpc_dir / "want.placement.tsv").read_text()
    assert "MZ515733.1" in want
    for prefix, extra in (("a", []), ("b", ["--hpc"])):
        r = run(["rsv.panman", "reads.fq", "-i", "hpc.idx", "--stop", "place", "-o", prefix] + extra, hpc_dir)
        assert r.returncode == 0, r.stderr
        assert (hpc_dir / (prefix + ".placement.tsv")).read_text() == want


@pytest.mark.gpu
def test_dedup_over_two_ranks_compares_the_compressed_reads(pmx, ctx, hpc_dir, tmp_path):
    """`--gpus 2 --dedup` with an HPC index: every rank compresses its shard explicitly, the dedup over the ranks hashes the
    compressed reads and the seeding call takes the same set.  Reads and their run-length twins sit on different ranks; a twin
    counts once, as in the one-rank run and in place_lite -- a dedup over the raw bytes would count it twice"""
    rsv = pmx.Panman(str(hpc_dir / "rsv.panman"))
    g = rsv.genome(rsv.find_node("MZ515733.1"))
    rng = np.random.default_rng(6)
    reads = []
    for _ in range(150):
        n = int(rng.integers(500, 2500))
        st = int(rng.integers(0, len(g) - n))
        reads.append(g[st:st + n])
    twins = [hc.run_length_errors(rng, r, 0.5) for r in reads]
    assert all(a != b and hc.hpc(a)[0] == hc.hpc(b)[0] for a, b in zip(reads, twins))
    allr = reads + twins + reads[:10]              # the first shard holds the originals, the second their twins and ten exact copies
    with open(hpc_dir / "twins.fq", "w") as f:
        for i, r in enumerate(allr):
            f.write("@t%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
    index = pmx.Index.load(str(hpc_dir / "hpc.idx"))
    want = {}
    for name, dd in (("dedup", True), ("plain", False)):
        placer = pmx.Placer(ctx, index)
        pmx.place_lite(ctx, placer, str(hpc_dir / "twins.fq"), "", str(tmp_path / (name + ".tsv")), pmx.TraversalParams(dedupReads=dd), index.node_id)
        want[name] = (tmp_path / (name + ".tsv")).read_text()
    assert want["dedup"] != want["plain"]
    # what a dedup over the raw bytes would give: the exact copies dropped, every twin still counted
    with open(tmp_path / "rawdedup.fq", "w") as f:
        for i, r in enumerate(reads + twins):
            f.write("@t%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
    pmx.place_lite(ctx, pmx.Placer(ctx, index), str(tmp_path / "rawdedup.fq"), "", str(tmp_path / "raw.tsv"), pmx.TraversalParams(), index.node_id)
    assert (tmp_path / "raw.tsv").read_text() != want["dedup"]
    meet = tmp_path / "meet"
    meet.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=str(meet))
    args = ["rsv.panman", "twins.fq", "-i", "hpc.idx", "--stop", "place", "--dedup"]
    r1 = run(args + ["-o", "d1"], hpc_dir)
    r2 = run(args + ["-o", "d2", "--gpus", "2"], hpc_dir, env=env, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-1500:])
    assert (hpc_dir / "d1.placement.tsv").read_text() == want["dedup"]
    assert (hpc_dir / "d2.placement.tsv").read_text() == want["dedup"]
