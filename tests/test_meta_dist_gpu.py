"""--meta over several GPUs (pmx_meta_attach_dist, panmap_amd/csrc/api_meta.hip; `panmap --meta --gpus N`) on a one-GPU box:
two ranks as two processes on the one device over the library's host-directory test transport, and a one-rank group on RCCL
itself.  The contract: N ranks give the same bits as one rank -- merged read lists and multiplicities, overlap coefficients,
candidates, each rank's score rows, column groups, proportions, log-likelihood, rounds and iterations."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from cli_checks import run
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EQUAL = ("lists_equal", "info_equal", "oc_equal", "candidates_equal", "scores_equal", "haplotypes_equal", "em_info_equal")


def _run_ranks(world, env_extra):
    procs = []
    for r in range(world):
        env = dict(os.environ, PMX_RANK=str(r), PMX_WORLD=str(world), **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join("tests", "dist_meta_worker.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    done = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=600)
            done.append((p.returncode, so, se))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    assert all(rc == 0 for rc, _, _ in done), [(rc, so[-500:], se[-1500:]) for rc, so, se in done]
    outs = [json.loads([l for l in so.splitlines() if l.startswith("RESULT ")][-1][7:]) for _, so, _ in done]
    return sorted(outs, key=lambda d: d["rank"])


def _check(outs):
    for d in outs:
        assert all(d[k] for k in EQUAL), {k: d[k] for k in EQUAL}
        assert d["n_reads"] == d["n_reads_one"] > 0 and d["n_haplotypes"] > 0 and d["em_info"]["iterations"] >= 2
    # every rank reports the whole sample's answer, and the ranks' score rows tile the merged reads
    assert len({json.dumps(d["top"]) for d in outs}) == 1
    at = 0
    for d in outs:
        assert d["row_range"][0] == at and d["scores_shape"][0] == d["row_range"][1]
        at += d["row_range"][1]
    assert at == outs[0]["n_reads"]


@pytest.mark.parametrize("case", ["rsv", "shards", "empty", "sars"])
def test_two_ranks_equal_one(tmp_path, case):
    """rsv: the 70 / 30 mixture in halves (fewer than 1,024 EM rows: rank 1 owns none); shards: cut 70 / 30; empty: rank 1
    holds no read; sars: 30,000 reads of five SARS-CoV-2 haplotypes with --dust 20 --discard 0.5 (both ranks own EM rows)"""
    outs = _run_ranks(2, {"PMX_DIST_HOST_DIR": str(tmp_path), "PMX_META_CASE": case})
    _check(outs)
    if case == "empty":
        assert outs[1]["shard"][0] == outs[1]["shard"][1]
    if case == "rsv":
        assert {k for k, _ in outs[0]["top"]} == {"MZ515733.1", "node_1330"}
    if case == "sars":
        assert outs[0]["n_reads"] > 2048 and outs[0]["n_haplotypes"] >= 5


@pytest.mark.parametrize("case", ["rsv", "sars"])
def test_one_rank_rccl_group_equals_no_dist(case):
    """a world-1 RCCL group attached: the real all-gathers run inside the EM loop (launches queued past convergence too) and
    the result equals the run without a dist bit for bit"""
    env = {"PMX_META_CASE": case, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    saved = os.environ.pop("PMX_DIST_HOST_DIR", None)
    try:
        outs = _run_ranks(1, env)
    finally:
        if saved is not None:
            os.environ["PMX_DIST_HOST_DIR"] = saved
    _check(outs)


def _mixture(tmp_path):
    def rd(p):
        return "".join(l.strip() for l in open(p) if not l.startswith(">")).upper()
    a, b = rd(os.path.join(GOLDEN, "MZ515733.1.fa")), rd(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    with open(tmp_path / "mix.fastq", "w") as out:
        def emit(g, n, pre):
            L = 150; step = max(1, (len(g) - L) // n); c = i = 0
            while c < n and i + L <= len(g):
                out.write("@%s%d\n%s\n+\n%s\n" % (pre, c, g[i:i + L], "I" * L)); c += 1; i += step
        emit(a, 700, "A"); emit(b, 300, "B")
        for i in range(100):
            out.write("@L%d\n%s\n+\n%s\n@M%d\n%s\n+\n%s\n" % (i, "A" * 150, "I" * 150, i, "AC" * 75, "I" * 150))


def test_meta_gpus_two_equals_one_through_the_cli(tmp_path):
    """`panmap rsv_4K.panman mix.fastq --meta --gpus 2` (two ranks on the one device): the abundance file is byte-equal to
    --gpus 1, and so is rank 0's summary line, with and without --dust 20 --discard 0.5"""
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv_4K.panman")
    _mixture(tmp_path)
    meet = tmp_path / "meet"
    meet.mkdir()
    env = dict(os.environ, PMX_DIST_SAME_DEVICE="1", PMX_DIST_HOST_DIR=str(meet))
    for extra in ([], ["--dust", "20", "--discard", "0.5"]):
        tag = "f" if extra else "p"
        r1 = run(["rsv_4K.panman", "mix.fastq", "--meta", "-o", "one" + tag] + extra, tmp_path, timeout=300)
        r2 = run(["rsv_4K.panman", "mix.fastq", "--meta", "--gpus", "2", "-o", "two" + tag] + extra, tmp_path, env=env, timeout=300)
        assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-2000:])
        one = open(tmp_path / ("one%s.mgsr.abundance.out" % tag), "rb").read()
        assert one and one == open(tmp_path / ("two%s.mgsr.abundance.out" % tag), "rb").read()
        summary = [l for l in r1.stderr.splitlines() if "distinct reads x" in l]
        assert len(summary) == 1 and [l for l in r2.stderr.splitlines() if "distinct reads x" in l] == summary, (r1.stderr, r2.stderr)
