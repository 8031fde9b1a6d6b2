"""Worker of tests/test_meta_assign_dist_gpu.py: one rank of `--meta --filter-and-assign` (and of the read-score pass) over
several GPUs THROUGH THE C ABI.  Launched like tests/dist_meta_worker.py (PMX_RANK / PMX_WORLD, the host-directory transport)
and built from its pieces.  Every rank runs the collective calls on ITS shard, then the whole sample through a Meta without a
dist in the same process, and prints whether what it holds equals that run bit for bit.
  PMX_ASSIGN_INPUT  rsv | shards | empty (the mixture and the cuts of dist_meta_worker.py), crafted (the broom tree of
                    assign_dist_checks with breadth_checks.reads(), two halves), two (two reads of it: rows 0, 1, 1 over three ranks)
  PMX_ASSIGN_MODE   assign (with breadth) | read_best | disagree (rank 1 turns breadth off: every rank must get PMX_ERR_ARG)
  PMX_ASSIGN_TAXA   1: a taxonomy of six taxa, at most three a read;  PMX_ASSIGN_AMB: the ambiguity threshold
  PMX_MASK_SEEDS    read_best: --mask-seeds
  PMX_ASSIGN_SLAB   rows per slab of the breadth merge (Meta.set_breadth_slab; 0 = default)
The chunk switch (PMX_META_ASSIGN_CHUNK) comes through the environment, per rank."""
import json
import os
import sys

import numpy as np

from dist_meta_worker import join, sample

import assign_dist_checks as adc
import breadth_checks as bc

ERR_ARG = -1


def raw_assign(pmx, meta, n):
    """the getters of pmx_meta_assign as they are, for n rows"""
    lib = pmx._lib.lib
    state, mx, lca, cnt = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert lib.pmx_meta_assign_reads(meta._h, state.ctypes.data, mx.ctypes.data, lca.ctypes.data, cnt.ctypes.data, n) == 0
    off, nodes = np.zeros(n + 1, np.int64), np.zeros(max(int(lib.pmx_meta_assign_num_nodes(meta._h)), 1), np.uint32)
    assert lib.pmx_meta_assign_nodes(meta._h, off.ctypes.data, nodes.ctypes.data, len(nodes)) == 0
    out = dict(state=state, max=mx, lca=lca, count=cnt, off=off, nodes=nodes[:off[-1]])
    max_taxa = int(lib.pmx_meta_assign_max_taxa(meta._h))
    if max_taxa > 0:
        nt, tx = np.zeros(n, np.uint32), np.zeros((n, max_taxa), np.uint32)
        assert lib.pmx_meta_assign_taxa(meta._h, nt.ctypes.data, tx.ctypes.data, n) == 0
        out.update(ntax=nt, tax=tx)
    return out


def rows_equal(got, want, first, count):
    """rows [first, first + count) of the one-rank arrays against a rank's own"""
    ok = all(np.array_equal(got[k], want[k][first:first + count]) for k in got if k not in ("off", "nodes"))
    lo, hi = int(want["off"][first]), int(want["off"][first + count])
    return bool(ok and np.array_equal(got["off"], want["off"][first:first + count + 1] - lo) and np.array_equal(got["nodes"], want["nodes"][lo:hi]))


def results_equal(a, b):
    """two AssignResults, per raw read"""
    ok = all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("merged", "state", "max", "lca", "fastq_index"))
    return bool(ok and all(np.array_equal(a.nodes_of(r), b.nodes_of(r)) and np.array_equal(a.taxa_of(r), b.taxa_of(r)) for r in range(len(a.merged))))


def inputs(pmx, ctx, name):
    """-> (Meta with a dist to attach, the same indexes for the one-rank Meta, reads, discard, cut name)"""
    if name in ("crafted", "two"):
        tree, reads = adc.crafted()
        plain, oriented = tree.indexes(pmx)
        return pmx.Meta(ctx, plain, oriented), (adc.two_reads() if name == "two" else reads), bc.DISCARD, "rsv"
    pm, reads, _, discard = sample(pmx, name)
    return pmx.Meta.build(ctx, pm), reads, discard, name


def taxonomy(n_nodes):
    """six taxa in blocks of consecutive DFS indices (a subtree is a range of them: most span one or two taxa, the root's all
    six), every fourth node without a taxon"""
    v = np.arange(n_nodes)
    return np.where(v % 4 == 0, -1, v * 6 // n_nodes).astype(np.int32)


def main():
    rank, world = int(os.environ["PMX_RANK"]), int(os.environ["PMX_WORLD"])
    name, mode = os.environ.get("PMX_ASSIGN_INPUT", "rsv"), os.environ.get("PMX_ASSIGN_MODE", "assign")
    taxa, amb = os.environ.get("PMX_ASSIGN_TAXA", "0") == "1", int(os.environ.get("PMX_ASSIGN_AMB", "0"))
    mask_seeds = int(os.environ.get("PMX_MASK_SEEDS", "0"))
    import panmap_amd as pmx
    lib = pmx._lib.lib
    ctx = pmx.Context(0)
    dist = join(pmx, ctx, rank, world)
    dist.barrier()
    meta, reads, discard, cut_name = inputs(pmx, ctx, name)
    meta.attach_dist(dist)
    meta.set_breadth_slab(int(os.environ.get("PMX_ASSIGN_SLAB", "0")))
    lo, hi = adc.cut(cut_name, len(reads), rank, world)
    one = pmx.Meta(ctx, meta.index, meta.index_oriented)
    n_nodes = meta.index_oriented.info.n_nodes
    out = dict(rank=rank, input=name, mode=mode, shard=[lo, hi], n_nodes=n_nodes)
    for m in (meta, one):
        if taxa:
            m.set_taxonomy(taxonomy(n_nodes), max_taxa=3, n_taxa=6)
        m.set_masks(0, mask_seeds)
    meta.set_reads(reads[lo:hi])
    out.update(n_reads=meta.n_reads, rows_before=meta.row_range()[1])
    if mode == "disagree":
        # (straight through the C ABI: the Python mirror would raise on the code this case is about)
        lib.pmx_meta_set_breadth(meta._h, int(rank != 1))
        out.update(rc=int(lib.pmx_meta_assign(ctx._h, meta._h, float(discard))), err_arg=ERR_ARG)
    elif mode == "assign":
        one.set_reads(reads)
        want_res = one.assign(discard, ambiguous=amb, breadth=True)
        want = raw_assign(pmx, one, one.n_reads)
        mine = meta.assign(discard, ambiguous=amb, breadth=True)
        first, count = meta.row_range()
        got = raw_assign(pmx, meta, count)
        out.update(row_range=[first, count], n_reads_one=one.n_reads, rows_equal=rows_equal(got, want, first, count),
                   rows_result_is_per_row=bool(np.array_equal(mine.merged, np.arange(count)) and np.array_equal(mine.state, got["state"])),
                   raw_to_merged_equal=bool(np.array_equal(meta.raw_to_merged(), one.raw_to_merged()[lo:hi])),
                   breadth_equal=bool(all(np.array_equal(a, b) for a, b in zip(mine.breadth, want_res.breadth))),
                   merge_ms=ctx.kernel_ms("meta_breadth_merge"),
                   n_assigned=int((want["state"] == pmx.meta.ASSIGNED).sum()), n_over=int((want["state"] == pmx.meta.OVER_TAXA).sum()),
                   n_assigned_mine=int((got["state"] == pmx.meta.ASSIGNED).sum()), observed_total=int(want_res.breadth[1].sum()))
        whole = meta.assign(discard, ambiguous=amb, breadth=True, gather=True)
        out["row_range_after_gather"] = list(meta.row_range())
        if rank == 0:
            all_rows = raw_assign(pmx, meta, meta.n_reads)
            out.update(gathered_equal=bool(all(np.array_equal(all_rows[k], want[k]) for k in want) and set(all_rows) == set(want)),
                       gathered_result_equal=results_equal(whole, want_res),
                       gathered_breadth_equal=bool(all(np.array_equal(a, b) for a, b in zip(whole.breadth, want_res.breadth))))
        else:
            kept = raw_assign(pmx, meta, count)
            out.update(gathered_is_none=whole is None, kept_rows=rows_equal(kept, want, first, count))
    else:
        one.set_reads(reads)
        want = one.read_best()
        mine = meta.read_best()
        first, count = meta.row_range()
        out.update(row_range=[first, count], n_reads_one=one.n_reads, n_mapped=int((want[0] > 0).sum()),
                   rows_equal=bool(all(np.array_equal(g, w[first:first + count]) for g, w in zip(mine, want))),
                   active_equal=bool(np.array_equal(meta.active_nodes(), one.active_nodes())),
                   raw_to_merged_equal=bool(np.array_equal(meta.raw_to_merged(), one.raw_to_merged()[lo:hi])),
                   n_dropped=int((one.raw_to_merged() < 0).sum()))
        whole = meta.read_best(gather=True)
        if rank == 0:
            out["gathered_equal"] = bool(all(np.array_equal(g, w) for g, w in zip(whole, want)))
        else:
            out["gathered_is_none"] = whole is None
    one.close()
    meta.close()
    dist.barrier()
    print("RESULT " + json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
