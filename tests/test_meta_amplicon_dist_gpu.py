"""--meta --amplicon-depth with a mask over several GPUs on a one-GPU box: two ranks as two processes on the one device over the
library's host-directory test transport (tests/dist_amplicon_worker.py, launched the way tests/test_meta_mask_dist_gpu.py
launches its worker).  The runs the ranks exchange carry the amplicon of every merged read, the merge compares it first, the
raw reads of every amplicon are summed over the ranks: two ranks give the bits of one -- lists, amplicons, triples, per-group
numbers, overlap coefficients, candidates, each rank's score rows, haplotypes, log-likelihood, rounds and iterations.  One
amplicon lies entirely on rank 0, another is split across both.  And ranks that disagree on the groups all return an error."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EQUAL = ("lists_equal", "info_equal", "amplicons_equal", "triples_equal", "counts_equal", "amplicon_info_equal", "mask_info_equal", "oc_equal",
         "candidates_equal", "scores_equal", "haplotypes_equal", "em_info_equal")


def _run_ranks(world, env_extra):
    procs = []
    for r in range(world):
        env = dict(os.environ, PMX_RANK=str(r), PMX_WORLD=str(world), **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join("tests", "dist_amplicon_worker.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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


@pytest.mark.parametrize("setting", ["0,0,0.05,0", "0,1,0,0"])
def test_two_ranks_equal_one(tmp_path, setting):
    """reads-relative 0.05, and mask-seeds 1 with groups"""
    outs = _run_ranks(2, {"PMX_DIST_HOST_DIR": str(tmp_path), "PMX_AMP_SETTING": setting})
    relative = setting.startswith("0,0,0.05")
    for d in outs:
        assert all(d[k] for k in EQUAL), {k: d[k] for k in EQUAL}
        assert d["n_reads"] == d["n_reads_one"] > 0 and d["n_haplotypes"] > 0 and d["em_info"]["iterations"] >= 2
        # N_g summed over the ranks: amplicons 0..9 are rank 0's, amplicon 10 is split, the rest and the planted reads are rank 1's
        assert d["raw_reads"] == [sum(i % 7 != 3 for i in range(50 * g, 50 * g + 50)) for g in range(20)] + [40, 143]
        assert sum(d["merged_left"]) == d["n_reads"] == d["mask_info"]["reads_left"]
        if relative:
            assert d["threshold"] == [int(0.05 * float(n)) for n in d["raw_reads"][:-1]] + [0] and max(d["threshold"]) == 2
            assert 0 < d["mask_info"]["reads_dropped"] == sum(d["merged_before"]) - d["n_reads"] and d["merged_left"][-1] == d["merged_before"][-1]
        else:
            assert set(d["threshold"]) == {1} and d["mask_info"]["seeds_removed"] > 0
    assert len({json.dumps(d["top"]) for d in outs}) == 1
    at = 0
    for d in outs:
        assert d["row_range"][0] == at and d["scores_shape"][0] == d["row_range"][1]
        at += d["row_range"][1]
    assert at == outs[0]["n_reads"]


def test_ranks_that_disagree_on_the_groups_all_return_an_error(tmp_path):
    outs = _run_ranks(2, {"PMX_DIST_HOST_DIR": str(tmp_path), "PMX_AMP_SETTING": "0,0,0.05,0", "PMX_AMP_GROUPS_OFF": "1"})
    for d in outs:
        assert "disagree on the amplicon groups" in d["refused"], d
