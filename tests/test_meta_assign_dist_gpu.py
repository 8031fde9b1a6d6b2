"""--meta --filter-and-assign and the read-score pass over several GPUs on a one-GPU box: two or three ranks as processes on the
one device over the library's host-directory test transport (tests/dist_assign_worker.py, launched the way
tests/test_meta_mask_dist_gpu.py launches its worker).  pmx_meta_assign and pmx_meta_read_best are collective: every rank works on
its rows of the whole sample's merged reads, the breadth matrix is the OR of the ranks' (k_meta_breadth_or of
panmap_amd/csrc/meta_assign.hip), rank 0 gathers.  N ranks give the bits of one rank: each rank's rows equal the slices of the
one-rank run (state, max, LCA, node counts, CSR nodes, taxa), the rows tile the merged reads, the gathered result on rank 0 equals
the one-rank result, raw_to_merged equals the shard's slice of the one-rank map, and the breadth arrays are the one-rank arrays
on every rank.  tests/test_assign_dist_families.py shows what the inputs and their cuts reach.  No run on more than one
physical GPU exists."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
ERR_ARG = -1


def _run_ranks(world, host_dir, env_all, env_rank=None):
    """one process per rank, one communicate() each, the ranks killed on the way out; nothing is started again after a failure"""
    procs = []
    for r in range(world):
        env = dict(os.environ, PMX_RANK=str(r), PMX_WORLD=str(world), PMX_DIST_HOST_DIR=str(host_dir), **env_all)
        env.update((env_rank or {}).get(r, {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join("tests", "dist_assign_worker.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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


def _rows_tile(outs):
    at = 0
    for d in outs:
        assert d["row_range"][0] == at, [x["row_range"] for x in outs]
        at += d["row_range"][1]
    assert at == outs[0]["n_reads"] == outs[0]["n_reads_one"]


def _check_assign(outs):
    print([{k: d[k] for k in ("rank", "shard", "row_range", "n_assigned_mine", "n_over", "merge_ms")} for d in outs])
    _rows_tile(outs)
    for d in outs:
        assert d["rows_before"] == 0                                   # set_reads leaves no rows; the call set them itself
        assert d["rows_equal"] and d["rows_result_is_per_row"] and d["raw_to_merged_equal"] and d["breadth_equal"], d
        assert d["row_range_after_gather"] == d["row_range"]
        if d["rank"] == 0:
            assert d["gathered_equal"] and d["gathered_result_equal"] and d["gathered_breadth_equal"], d
        else:
            assert d["gathered_is_none"] and d["kept_rows"], d
    assert sum(d["n_assigned_mine"] for d in outs) == outs[0]["n_assigned"] > 0 and outs[0]["observed_total"] > 0


@pytest.mark.parametrize("slab", [None, 1, 7])
def test_crafted_tree_two_ranks_equal_one(tmp_path, slab):
    """109 nodes (two words a row, the last one partly filled); the slab of the breadth merge at its default, at one row (an
    edge after every row) and at seven rows (a last slab shorter than the rest)"""
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT="crafted", **({} if slab is None else {"PMX_ASSIGN_SLAB": str(slab)})))
    _check_assign(outs)
    assert outs[0]["n_nodes"] % 64 != 0 and all(d["n_assigned_mine"] > 0 and d["merge_ms"] > 0 for d in outs)


@pytest.mark.parametrize("case,slab", [("rsv", None), ("shards", 7)])
def test_rsv_two_ranks_equal_one(tmp_path, case, slab):
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT=case, **({} if slab is None else {"PMX_ASSIGN_SLAB": str(slab)})))
    _check_assign(outs)
    assert all(d["n_assigned_mine"] > 0 for d in outs)


@pytest.mark.parametrize("amb", [0, 2])
def test_rsv_with_a_taxonomy(tmp_path, amb):
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT="rsv", PMX_ASSIGN_TAXA="1", PMX_ASSIGN_AMB=str(amb)))
    _check_assign(outs)
    assert outs[0]["n_over"] > 0                                       # the filter took something away


def test_ranks_with_different_numbers_of_chunks(tmp_path):
    """chunks of one read on rank 0 alone: the ranks run different numbers of chunks, the collective still ends"""
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT="shards"), {0: {"PMX_META_ASSIGN_CHUNK": "1"}})
    _check_assign(outs)


def test_an_empty_shard_on_rank_one(tmp_path):
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT="empty"))
    _check_assign(outs)
    assert outs[1]["shard"][0] == outs[1]["shard"][1] and outs[1]["row_range"][1] > 0   # no reads of its own, rows all the same


def test_three_ranks_and_a_rank_without_rows(tmp_path):
    outs = _run_ranks(3, tmp_path, dict(PMX_ASSIGN_INPUT="two"))
    _check_assign(outs)
    assert [d["row_range"][1] for d in outs] == [0, 1, 1]


def test_ranks_that_disagree_all_get_err_arg(tmp_path):
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT="rsv", PMX_ASSIGN_MODE="disagree"))
    assert [d["rc"] for d in outs] == [ERR_ARG, ERR_ARG]


@pytest.mark.parametrize("mask_seeds", [0, 1])
def test_read_best_two_ranks_equal_one(tmp_path, mask_seeds):
    outs = _run_ranks(2, tmp_path, dict(PMX_ASSIGN_INPUT="rsv", PMX_ASSIGN_MODE="read_best", PMX_MASK_SEEDS=str(mask_seeds)))
    _rows_tile(outs)
    for d in outs:
        assert d["rows_equal"] and d["active_equal"] and d["raw_to_merged_equal"] and d["n_mapped"] > 0, d
        assert d["gathered_equal"] if d["rank"] == 0 else d["gathered_is_none"], d
