"""--mask-read-ends and --em-leaves-only over several GPUs (pmx_meta_attach_dist) on a one-GPU box: two ranks as two processes
on the one device over the library's host-directory test transport, as tests/test_meta_dist_gpu.py runs them.  With n = 5 and
leaves-only the two ranks hold the same bits as one rank on the keys that test compares: every rank trims its own shard and no
exchange changes."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# the keys tests/test_meta_dist_gpu.py compares
EQUAL = ("lists_equal", "info_equal", "oc_equal", "candidates_equal", "scores_equal", "haplotypes_equal", "em_info_equal")


def _run_ranks(world, env_extra):
    procs = []
    for r in range(world):
        env = dict(os.environ, PMX_RANK=str(r), PMX_WORLD=str(world), **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join("tests", "dist_ends_worker.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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


@pytest.mark.parametrize("case", ["rsv", "shards"])
def test_two_ranks_equal_one_with_masked_ends_and_leaves_only(tmp_path, case):
    """rsv: the 70 / 30 mixture in halves; shards: cut 70 / 30"""
    outs = _run_ranks(2, {"PMX_DIST_HOST_DIR": str(tmp_path), "PMX_META_CASE": case, "PMX_ENDS": "5", "PMX_LEAVES": "1"})
    for d in outs:
        assert all(d[k] for k in EQUAL), {k: d[k] for k in EQUAL}
        assert d["trimmed_strings_equal"]
        assert d["n_reads"] == d["n_reads_one"] > 0 and d["n_haplotypes"] > 0 and d["em_info"]["iterations"] >= 2
        # the two settings took effect: fewer seedmers than untrimmed, and other candidates
        assert 0 < d["n_seedmers"] < d["n_seedmers_untrimmed"] and 0 < d["n_candidates"] != d["n_candidates_all_nodes"]
    assert len({json.dumps(d["top"]) for d in outs}) == 1
    at = 0
    for d in outs:
        assert d["row_range"][0] == at and d["scores_shape"][0] == d["row_range"][1]
        at += d["row_range"][1]
    assert at == outs[0]["n_reads"]
    assert outs[0]["n_sampled_candidates"] > 0
