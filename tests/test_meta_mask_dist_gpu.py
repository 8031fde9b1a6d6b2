"""--meta --mask-reads / --mask-seeds over several GPUs on a one-GPU box: two ranks as two processes on the one device over the
library's host-directory test transport (tests/dist_mask_worker.py, launched the way tests/test_meta_dist_gpu.py launches its
worker).  After the ranks' runs were merged every rank holds the whole sample's merged lists and masks them itself: N ranks
give the same bits as one rank -- occurrence counts, surviving lists and multiplicities, the reported numbers, overlap
coefficients, candidates, each rank's score rows, haplotypes, log-likelihood, rounds and iterations."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EQUAL = ("lists_equal", "info_equal", "counts_equal", "mask_info_equal", "oc_equal", "candidates_equal", "scores_equal", "haplotypes_equal",
         "em_info_equal")


def _run_ranks(world, env_extra):
    procs = []
    for r in range(world):
        env = dict(os.environ, PMX_RANK=str(r), PMX_WORLD=str(world), **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join("tests", "dist_mask_worker.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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


@pytest.mark.parametrize("case,mask_reads,mask_seeds", [("rsv", 0, 1), ("shards", 1, 0)])
def test_two_ranks_equal_one(tmp_path, case, mask_reads, mask_seeds):
    """rsv: the 70 / 30 mixture in halves, mask_seeds 1; shards: cut 70 / 30, mask_reads 1"""
    outs = _run_ranks(2, {"PMX_DIST_HOST_DIR": str(tmp_path), "PMX_META_CASE": case, "PMX_MASK_READS": str(mask_reads), "PMX_MASK_SEEDS": str(mask_seeds)})
    for d in outs:
        assert all(d[k] for k in EQUAL), {k: d[k] for k in EQUAL}
        assert d["n_reads"] == d["n_reads_one"] > 0 and d["n_haplotypes"] > 0 and d["em_info"]["iterations"] >= 2
        assert d["mask_info"]["reads_left"] == d["n_reads"]
        if mask_reads:                                             # the masks took something away
            assert 0 < d["mask_info"]["reads_dropped"] == d["n_reads_unmasked"] - d["n_reads"] and d["mask_info"]["seeds_removed"] == 0
        else:
            assert 0 < d["mask_info"]["seeds_removed"] == d["n_seedmers_unmasked"] - d["n_seedmers"] and d["mask_info"]["reads_dropped"] == 0
    # every rank reports the whole sample's answer, and the ranks' score rows tile the surviving reads
    assert len({json.dumps(d["top"]) for d in outs}) == 1
    at = 0
    for d in outs:
        assert d["row_range"][0] == at and d["scores_shape"][0] == d["row_range"][1]
        at += d["row_range"][1]
    assert at == outs[0]["n_reads"]
    assert {k for k, _ in outs[0]["top"]} == {"MZ515733.1", "node_1330"}
