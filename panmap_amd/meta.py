"""--meta: haplotype deconvolution of a mixed sample on the device (pmx_meta_*; src/main.cpp:1192-1313 runDeconvolution).
Host-side mirror of the reference's flow: reads -> Meta.set_reads -> Meta.score (candidates + parsimony scores) -> Meta.em
-> the `<prefix>.mgsr.abundance.out` text (node[,merged nodes...]<TAB>proportion with five decimals, by proportion)."""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import lib
from ._lib import check
from .api import Context, Index, Panman, concat_reads

ORIENTED = 0x100     # PMX_INDEX_ORIENTED
ORIENT_XOR = 0x9e3779b97f4a7c15
UNMAPPED, DISCARDED, ASSIGNED, OVER_TAXA = 0, 1, 2, 3    # PMX_META_*: the state of a read after Meta.assign


class AssignResult:
    """--meta --filter-and-assign, per RAW read of the last set_reads (input order): `state` (UNMAPPED / DISCARDED / ASSIGNED;
    a read dropped by --dust or without seedmers is UNMAPPED), `max` (its best score over all nodes), `lca` (the head of the
    LCA of its assigned nodes, -1 unless assigned), `merged` (its merged read, -1 = dropped).  `heads` folds identical
    nodes (Index.node_heads of the oriented index).  The assigned reads, in input order, are the records of
    `<prefix>.mgsr.assignedReads.fastq`: `fastq_index[read]` is a read's position there (-1 unless assigned).
    With a taxonomy (Meta.set_taxonomy) a read that spans too many taxa is OVER_TAXA: no nodes, no LCA, not in the FASTQ;
    `read_taxa` ((n_taxa, taxa[merged reads][max_taxa])) and `node_sets` (node -> S(node), None when over) feed taxa_of / node_taxa.
    `breadth`: None, or with Meta.assign(breadth=True) three int64 arrays per node (DFS index; a folded node carries its head's
    numbers): (total_ref_seeds, observed, depth) of pmx_meta_breadth -- format_breadths writes the file from them."""

    def __init__(self, merged, state, mx, lca, offsets, nodes, heads, read_taxa=None, node_sets=None, breadth=None):
        self.merged, self.heads, self._off, self._nodes = merged, heads, offsets, nodes
        self.breadth = breadth
        self._read_taxa, self._node_sets = read_taxa, node_sets
        has = merged >= 0
        at = np.where(has, merged, 0)
        self.state = np.where(has, state[at], UNMAPPED).astype(np.uint8) if len(state) else np.zeros(len(merged), np.uint8)
        self.max = np.where(has, mx[at], 0).astype(np.int64) if len(mx) else np.zeros(len(merged), np.int64)
        self.lca = np.full(len(merged), -1, np.int64)
        ok = self.state == ASSIGNED
        self.lca[ok] = heads[lca[at[ok]]]
        self.fastq_index = np.full(len(merged), -1, np.int64)
        self.fastq_index[ok] = np.arange(int(ok.sum()))

    def nodes_of(self, read: int) -> np.ndarray:
        """the assigned nodes of a raw read (all nodes whose score equals its maximum; DFS indices, ascending, not folded);
        empty unless the read is assigned"""
        r = int(self.merged[read])
        return self._nodes[self._off[r]:self._off[r + 1]] if r >= 0 else self._nodes[:0]

    def taxa_of(self, read: int) -> np.ndarray:
        """the taxa of a raw read (the union over its qualifying nodes' subtrees, ascending); empty unless the read is assigned
        and a taxonomy was set"""
        r = int(self.merged[read])
        if r < 0 or self._read_taxa is None:
            return np.zeros(0, np.uint32)
        return self._read_taxa[1][r, :self._read_taxa[0][r]]

    def node_taxa(self, v: int):
        """S(v): the taxa in the subtree of node v (identical nodes not folded), ascending; None when they exceed max_taxa;
        empty without a taxonomy"""
        return np.zeros(0, np.uint32) if self._node_sets is None else self._node_sets(int(v))

    def by_node(self):
        """{head: sorted FASTQ indices of the reads assigned to the head or to a node folded into it}"""
        out = {}
        for read in np.nonzero(self.state == ASSIGNED)[0]:
            for h in np.unique(self.heads[self.nodes_of(read)]).tolist():
                out.setdefault(h, []).append(int(self.fastq_index[read]))
        return out

    def by_lca(self):
        """{head of the LCA node: sorted FASTQ indices}"""
        out = {}
        for read in np.nonzero(self.state == ASSIGNED)[0]:
            out.setdefault(int(self.lca[read]), []).append(int(self.fastq_index[read]))
        return out


class Meta:
    def __init__(self, ctx: Context, index: Index, index_oriented: Index):
        self.ctx, self.index, self.index_oriented = ctx, index, index_oriented
        self._h = C.c_void_p()
        check(lib.pmx_meta_create(ctx._h, index._h, index_oriented._h, C.byref(self._h)), "pmx_meta_create")

    @classmethod
    def build(cls, ctx: Context, pm: Panman, k=19, s=8, t=0, l=3, open_syncmer=False, flank_mask=0):
        """both indexes of one tree (the MGSR index of the reference masks no flanks: flank_mask 0)"""
        idx = Index.build(pm, k=k, s=s, t=t, l=l, open_syncmer=open_syncmer, flank_mask=flank_mask)
        oidx = Index.build(pm, k=k, s=s, t=t, l=l, open_syncmer=open_syncmer, flank_mask=flank_mask, mode=ORIENTED)
        return cls(ctx, idx, oidx)

    def attach_dist(self, dist):
        """--gpus N: `dist` (a Dist on this Meta's context) makes set_reads / score / em collective -- every rank calls them in
        the same order, set_reads with its own shard of the reads -- and every rank ends with the whole sample's result.
        assign() and read_best() are collective too and work on this rank's rows of the merged reads (row_range()).
        Call before set_reads; keep `dist` alive as long as this Meta."""
        check(lib.pmx_meta_attach_dist(self._h, dist._h), "pmx_meta_attach_dist")
        self._dist = dist

    def row_range(self):
        """(first, count): the merged reads whose rows scores() returns (all of them without a dist); with a dist valid after
        score(), assign() or read_best()"""
        first, count = C.c_int64(0), C.c_int64(0)
        check(lib.pmx_meta_row_range(self._h, C.byref(first), C.byref(count)), "pmx_meta_row_range")
        return int(first.value), int(count.value)

    def set_reads(self, reads=None, concat=None, offsets=None):
        if reads is not None:
            cb, offsets = concat_reads(reads)
            concat = np.frombuffer(cb, np.uint8)
        concat = np.ascontiguousarray(concat, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        check(lib.pmx_meta_set_reads(self.ctx._h, self._h, concat.ctypes.data, offsets.ctypes.data, len(offsets) - 1), "pmx_meta_set_reads")

    def set_dust(self, threshold: float):
        """--dust: the next set_reads drops reads whose DUST score is non-zero and above `threshold` (100 = off)"""
        check(lib.pmx_meta_set_dust(self._h, float(threshold)), "pmx_meta_set_dust")

    def set_mask_read_ends(self, n: int):
        """--mask-read-ends: the next set_reads sees every read as read[n:len(read) - n] (empty when len(read) <= 2 * n) -- DUST,
        seedmer lists, overlap coefficients and all that follows; a read trimmed to nothing stays in the sample like any read
        without seedmers (raw_to_merged -1).  0 = off.  assign() refuses a read set made with n > 0.  --gpus N: the same n on every rank."""
        check(lib.pmx_meta_set_mask_read_ends(self._h, int(n)), "pmx_meta_set_mask_read_ends")

    def set_em_leaves_only(self, on: bool = True):
        """--em-leaves-only: score() without `candidates` chooses among the sampled genomes only -- nodes whose id does not begin
        with `node_`, or that Index.node_heads folds onto the same head as one -- and counts the top_oc ranks among those"""
        check(lib.pmx_meta_set_em_leaves_only(self._h, int(bool(on))), "pmx_meta_set_em_leaves_only")

    def set_masks(self, reads: int = 0, seeds: int = 0):
        """--mask-reads / --mask-seeds (src/mgsr.cpp:2049-2139) for the set_reads calls that follow; at most one above 0.  With
        count[h] = the summed multiplicities of the merged reads that carry hash h: `reads` = T drops every merged read with a
        seedmer of count <= T, `seeds` = T removes those seedmers from the lists (a read left empty goes).  Everything after
        set_reads is of the survivors; assign() refuses such a read set.  --gpus N: the same masks on every rank."""
        check(lib.pmx_meta_set_masks(self._h, int(reads), int(seeds)), "pmx_meta_set_masks")

    def mask_info(self):
        """of the last set_reads: merged reads dropped by mask-reads, seedmers removed by mask-seeds, merged reads left"""
        d, s, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib.pmx_meta_mask_info(self._h, C.byref(d), C.byref(s), C.byref(n)), "pmx_meta_mask_info")
        return dict(reads_dropped=int(d.value), seeds_removed=int(s.value), reads_left=int(n.value))

    def mask_counts(self):
        """(hash, count): the distinct hashes of the merged reads BEFORE masking, ascending, with their occurrence counts
        (a set_reads with a mask set must have run)"""
        n = int(lib.pmx_meta_mask_num_counts(self._h))
        h, c = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.int64)
        check(lib.pmx_meta_mask_counts(self._h, h.ctypes.data, c.ctypes.data, n), "pmx_meta_mask_counts")
        return h[:n], c[:n]

    def set_amplicons(self, groups=None, n_groups: int = 0):
        """--amplicon-depth (src/mgsr.cpp:1216-1342) for the set_reads calls that follow: `groups[r]` in [0, n_groups] is the
        amplicon of raw read r, the value n_groups meaning "not listed" (load_amplicons(...).groups_of makes it).  Reads are then
        merged within their amplicon only, ordered by (amplicon, hash list, orientation list), and a mask counts and thresholds
        per amplicon.  groups=None clears.  assign() refuses such a read set.  --gpus N: every rank passes its shard's groups."""
        if groups is None:
            check(lib.pmx_meta_set_amplicons(self._h, None, 0, 0), "pmx_meta_set_amplicons")
            return
        g = np.ascontiguousarray(groups, np.int32)
        check(lib.pmx_meta_set_amplicons(self._h, g.ctypes.data, len(g), int(n_groups)), "pmx_meta_set_amplicons")

    def set_relative_masks(self, reads: float = 0.0, seeds: float = 0.0):
        """--mask-reads-relative-frequency / --mask-seeds-relative-frequency (src/mgsr.cpp:2062-2075): as set_masks, with the
        threshold of a listed amplicon g being int(x * N_g), N_g its raw reads; the unlisted group stays unmasked.  At most one
        of the four masking parameters above 0; set_reads refuses a relative one without amplicons."""
        check(lib.pmx_meta_set_relative_masks(self._h, float(reads), float(seeds)), "pmx_meta_set_relative_masks")

    def read_amplicons(self) -> np.ndarray:
        """the amplicon of every merged read of the last set_reads (which ran with amplicons)"""
        out = np.zeros(self.n_reads, np.int32)
        check(lib.pmx_meta_read_amplicons(self._h, out.ctypes.data, len(out)), "pmx_meta_read_amplicons")
        return out

    def amplicon_info(self):
        """per amplicon of the last set_reads, the unlisted group last: raw reads N_g, the threshold applied (0 without a mask),
        merged reads before masking, merged reads left"""
        n = int(lib.pmx_meta_num_amplicon_groups(self._h))
        a = [np.zeros(max(n, 1), np.int64) for _ in range(4)]
        check(lib.pmx_meta_amplicon_info(self._h, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, n), "pmx_meta_amplicon_info")
        return dict(raw_reads=a[0][:n], threshold=a[1][:n], merged_before=a[2][:n], merged_left=a[3][:n])

    def amplicon_counts(self):
        """(group, hash, count) BEFORE masking, ascending by (group, hash) (a set_reads with amplicons and a mask must have run)"""
        n = int(lib.pmx_meta_amplicon_num_counts(self._h))
        g, h, c = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.int64)
        check(lib.pmx_meta_amplicon_counts(self._h, g.ctypes.data, h.ctypes.data, c.ctypes.data, n), "pmx_meta_amplicon_counts")
        return g[:n], h[:n], c[:n]

    def score(self, top_oc: int = 1000, candidates=None):
        if candidates is not None:
            c = np.ascontiguousarray(candidates, np.uint32)
            check(lib.pmx_meta_score(self.ctx._h, self._h, top_oc, c.ctypes.data, len(c)), "pmx_meta_score")
        else:
            check(lib.pmx_meta_score(self.ctx._h, self._h, top_oc, None, 0), "pmx_meta_score")

    def em(self, params: "_lib.MetaParams" = None):
        mp = params if params is not None else _lib.MetaParams()
        check(lib.pmx_meta_em(self.ctx._h, self._h, C.byref(mp)), "pmx_meta_em")
        return self.haplotypes()

    def set_taxonomy(self, node_taxon=None, max_taxa: int = 1, n_taxa=None):
        """--taxonomic-metadata / --maximum-taxon-number for the assign calls that follow: `node_taxon[v]` is the taxon of the
        node with DFS index v of the oriented index, -1 = none (load_taxonomy makes it); a read whose qualifying nodes span
        more than `max_taxa` taxa becomes OVER_TAXA.  max_taxa=0 clears the taxonomy."""
        if max_taxa == 0:
            check(lib.pmx_meta_set_taxonomy(self._h, None, 0, 0, 0), "pmx_meta_set_taxonomy")
            return
        t = np.ascontiguousarray(node_taxon, np.int32)
        n_taxa = int(t.max()) + 1 if n_taxa is None and len(t) else int(n_taxa or 0)
        check(lib.pmx_meta_set_taxonomy(self._h, t.ctypes.data, len(t), n_taxa, int(max_taxa)), "pmx_meta_set_taxonomy")

    def node_taxa(self, v: int):
        """S(v) of the taxonomy that is set (ascending ids), None when it exceeds max_taxa"""
        ids = np.zeros(16, np.uint32)
        n = int(lib.pmx_meta_node_taxa(self._h, int(v), ids.ctypes.data, len(ids)))
        if n < -1:
            raise ValueError("node_taxa: no taxonomy is set, or no such node")
        return None if n < 0 else ids[:n].copy()

    def set_breadth_slab(self, rows: int = 0):
        """with a dist: rows of the breadth hit matrix per exchange of its merge over the ranks (0 = what the slab buffer holds);
        the same value on every rank"""
        check(lib.pmx_meta_set_breadth_slab(self._h, int(rows)), "pmx_meta_set_breadth_slab")

    def _whole_raw_to_merged(self) -> np.ndarray:
        """with a dist, collective: the whole sample's raw -> merged map on every rank, assembled from the shards' slices.  The
        shards are contiguous in input order, rank by rank, so it is their concatenation; a zero-filled array with this rank's
        slice (+ 1) at its place, summed over the ranks, moves it."""
        d = self._dist
        mine = self.raw_to_merged()
        counts = np.zeros(d.world, np.int64)
        counts[d.rank] = len(mine)
        check(lib.pmx_dist_sum_i64(d._h, counts.ctypes.data, len(counts)), "pmx_dist_sum_i64")
        whole = np.zeros(max(int(counts.sum()), 1), np.int64)
        at = int(counts[:d.rank].sum())
        whole[at:at + len(mine)] = mine + 1
        check(lib.pmx_dist_sum_i64(d._h, whole.ctypes.data, len(whole)), "pmx_dist_sum_i64")
        return whole[:int(counts.sum())] - 1

    def assign(self, discard: float = 0.0, ambiguous: int = 0, ambiguous_ratio: float = 0.0, breadth: bool = False, gather: bool = False):
        """--filter-and-assign on the reads of the last set_reads: every read against every node (pmx_meta_assign).
        `ambiguous` / `ambiguous_ratio` (--ambiguous-score-threshold, -ratio) widen the nodes whose taxa count for a read from
        its best ones to those within max(ambiguous, int(max * ratio)) of its best score; they act through a taxonomy only.
        `breadth` (--breadth-ratio): also the per-node seed breadth of the assignment, in AssignResult.breadth.
        With an attached dist the call is collective and the result is of THIS RANK'S ROWS, one entry per merged read of
        row_range() instead of per raw read (`merged` is then 0 .. count - 1; the breadth is the whole sample's on every rank).
        `gather=True` (collective, to rank 0): rank 0 gets the whole sample's AssignResult, per raw read of the whole input and
        equal to what one rank makes of it -- the shards must be contiguous in input order, rank by rank -- the others None."""
        dist = getattr(self, "_dist", None)
        check(lib.pmx_meta_set_breadth(self._h, int(bool(breadth))), "pmx_meta_set_breadth")
        check(lib.pmx_meta_set_ambiguous(self._h, int(ambiguous), float(ambiguous_ratio)), "pmx_meta_set_ambiguous")
        check(lib.pmx_meta_assign(self.ctx._h, self._h, float(discard)), "pmx_meta_assign")
        n = self.n_reads if dist is None else self.row_range()[1]
        merged = None
        if gather:
            if dist is None:
                raise ValueError("assign(gather=True) needs an attached dist")
            merged = self._whole_raw_to_merged()
            check(lib.pmx_meta_assign_gather(self.ctx._h, self._h, 0), "pmx_meta_assign_gather")
            if dist.rank != 0:
                return None
            n = self.n_reads
        elif dist is not None:
            merged = np.arange(n, dtype=np.int64)
        state, mx = np.zeros(n, np.uint8), np.zeros(n, np.uint16)
        lca, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        check(lib.pmx_meta_assign_reads(self._h, state.ctypes.data, mx.ctypes.data, lca.ctypes.data, cnt.ctypes.data, n), "pmx_meta_assign_reads")
        off, nodes = np.zeros(n + 1, np.int64), np.zeros(max(int(lib.pmx_meta_assign_num_nodes(self._h)), 1), np.uint32)
        check(lib.pmx_meta_assign_nodes(self._h, off.ctypes.data, nodes.ctypes.data, len(nodes)), "pmx_meta_assign_nodes")
        assert np.array_equal(np.diff(off), cnt)
        read_taxa, node_sets = None, None
        max_taxa = int(lib.pmx_meta_assign_max_taxa(self._h))
        if max_taxa > 0:
            nt, tx = np.zeros(n, np.uint32), np.zeros((n, max_taxa), np.uint32)
            check(lib.pmx_meta_assign_taxa(self._h, nt.ctypes.data, tx.ctypes.data, n), "pmx_meta_assign_taxa")
            sets = [self.node_taxa(v) for v in range(self.index_oriented.info.n_nodes)]   # (copied: the result outlives a later set_taxonomy)
            read_taxa, node_sets = (nt, tx), sets.__getitem__
        numbers = None
        if breadth:
            n_nodes = self.index_oriented.info.n_nodes
            u = [np.zeros(n_nodes, np.uint64) for _ in range(3)]
            check(lib.pmx_meta_breadth(self._h, u[0].ctypes.data, u[1].ctypes.data, u[2].ctypes.data, n_nodes), "pmx_meta_breadth")
            numbers = tuple(x.astype(np.int64) for x in u)
        return AssignResult(self.raw_to_merged() if merged is None else merged, state, mx, lca, off, nodes[:off[-1]], self.index_oriented.node_heads(), read_taxa, node_sets, numbers)

    def read_best(self, gather: bool = False):
        """per merged read of the last set_reads: (max, n_best), its best score over ALL nodes and the number of active
        nodes (active_nodes) that reach it, 0 where max is 0 (pmx_meta_read_best; the numbers of the abundance mode's
        read-score reports).  Runs on masked reads too; needs no score().  With an attached dist: collective, and the arrays
        are of this rank's rows (row_range()); `gather=True` (collective, to rank 0): the whole sample's on rank 0, None elsewhere."""
        dist = getattr(self, "_dist", None)
        check(lib.pmx_meta_read_best(self.ctx._h, self._h), "pmx_meta_read_best")
        n = self.n_reads if dist is None else self.row_range()[1]
        if gather:
            if dist is None:
                raise ValueError("read_best(gather=True) needs an attached dist")
            check(lib.pmx_meta_read_best_gather(self.ctx._h, self._h, 0), "pmx_meta_read_best_gather")
            if dist.rank != 0:
                return None
            n = self.n_reads
        mx, nb = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
        check(lib.pmx_meta_read_best_get(self._h, mx.ctypes.data, nb.ctypes.data, n), "pmx_meta_read_best_get")
        return mx, nb

    def active_nodes(self) -> np.ndarray:
        """one flag per DFS index: the root and the nodes with a change whose hash the merged reads carry, as built by the
        last read_best()"""
        out = np.zeros(self.index_oriented.info.n_nodes, np.uint8)
        check(lib.pmx_meta_active_nodes(self._h, out.ctypes.data, len(out)), "pmx_meta_active_nodes")
        return out.astype(bool)

    def raw_to_merged(self) -> np.ndarray:
        """per read of the last set_reads (input order): its merged read, -1 when --dust dropped it, it has no seedmers or a mask
        dropped it.  With an attached dist: per read of this rank's shard, its merged read in the whole sample's numbering"""
        out = np.zeros(int(lib.pmx_meta_num_raw_reads(self._h)), np.int64)
        check(lib.pmx_meta_raw_to_merged(self._h, out.ctypes.data, len(out)), "pmx_meta_raw_to_merged")
        return out

    # ---- accessors
    @property
    def n_reads(self) -> int:
        return int(lib.pmx_meta_num_reads(self._h))

    def candidates(self) -> np.ndarray:
        out = np.zeros(int(lib.pmx_meta_num_candidates(self._h)), np.uint32)
        check(lib.pmx_meta_candidates(self._h, out.ctypes.data, len(out)), "pmx_meta_candidates")
        return out

    def overlap_coefficients(self) -> np.ndarray:
        out = np.zeros(self.index.info.n_nodes, np.float64)
        check(lib.pmx_meta_overlap_coefficients(self._h, out.ctypes.data, len(out)), "pmx_meta_overlap_coefficients")
        return out

    def read_info(self):
        n = self.n_reads
        ns, mult = np.zeros(n, np.int64), np.zeros(n, np.int64)
        check(lib.pmx_meta_read_info(self._h, ns.ctypes.data, mult.ctypes.data, n), "pmx_meta_read_info")
        return ns, mult

    def read_seedmers(self):
        n = self.n_reads
        ns, _ = self.read_info()
        tot = int(ns.sum())
        off, h, rev = np.zeros(n + 1, np.int64), np.zeros(max(tot, 1), np.uint64), np.zeros(max(tot, 1), np.uint8)
        check(lib.pmx_meta_read_seedmers(self._h, off.ctypes.data, h.ctypes.data, rev.ctypes.data, len(h)), "pmx_meta_read_seedmers")
        return off, h[:tot], rev[:tot]

    def scores(self) -> np.ndarray:
        """[rows][candidates] for the merged reads of row_range()"""
        n, c = self.row_range()[1], int(lib.pmx_meta_num_candidates(self._h))
        out = np.zeros((n, c), np.uint16)
        check(lib.pmx_meta_scores(self.ctx._h, self._h, out.ctypes.data, out.size), "pmx_meta_scores")
        return out

    def haplotypes(self):
        """[(node dfs index, proportion, [merged candidates])] by proportion, descending"""
        out = []
        for i in range(int(lib.pmx_meta_num_haplotypes(self._h))):
            node, prop, nm = C.c_uint32(0), C.c_double(0), C.c_int64(0)
            check(lib.pmx_meta_haplotype(self._h, i, C.byref(node), C.byref(prop), C.byref(nm), None, 0), "pmx_meta_haplotype")
            mem = np.zeros(max(nm.value, 1), np.uint32)
            check(lib.pmx_meta_haplotype(self._h, i, None, None, None, mem.ctypes.data, len(mem)), "pmx_meta_haplotype")
            out.append((int(node.value), float(prop.value), [int(x) for x in mem[:nm.value]]))
        return out

    def em_info(self):
        r, it, llh = C.c_int32(0), C.c_int32(0), C.c_double(0)
        check(lib.pmx_meta_em_info(self._h, C.byref(r), C.byref(it), C.byref(llh)), "pmx_meta_em_info")
        return dict(rounds=int(r.value), iterations=int(it.value), log_likelihood=float(llh.value))

    def close(self):
        if self._h:
            lib.pmx_meta_free(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_dust(seq: bytes, window: int = 64) -> float:
    """mgsr::getDust (src/mgsr.cpp:1505-1568) by the library (pmx_read_dust, host)"""
    return float(lib.pmx_read_dust(seq, len(seq), window))


def format_abundance(haplotypes, node_id) -> str:
    """`<prefix>.mgsr.abundance.out` (src/main.cpp:1288-1306): id[,merged ids]<TAB>proportion, %.5f, by proportion"""
    lines = []
    for node, prop, members in haplotypes:
        lines.append(",".join([node_id(node)] + [node_id(x) for x in members]) + "\t%.5f" % prop)
    return "\n".join(lines) + ("\n" if lines else "")


def load_taxonomy(path: str, rank: str, node_ids):
    """--taxonomic-metadata / --taxonomic-rank (pmx_taxonomy_load; loadTaxonomicMetadata, src/mgsr.cpp:198-256): (taxon names
    in order of first appearance, int32 array with the taxon of every identifier of `node_ids`, -1 = none).  With node_ids
    = [index.node_id(v) for v in range(n_nodes)] the array is Meta.set_taxonomy's node_taxon."""
    h = C.c_void_p()
    check(lib.pmx_taxonomy_load(os.fsencode(path), rank.encode(), C.byref(h)), "pmx_taxonomy_load")
    try:
        names = [lib.pmx_taxonomy_taxon_name(h, i).decode() for i in range(int(lib.pmx_taxonomy_num_taxa(h)))]
        taxon = np.array([lib.pmx_taxonomy_lookup(h, x.encode()) for x in node_ids], np.int32).reshape(-1)
    finally:
        lib.pmx_taxonomy_free(h)
    return names, taxon


class Amplicons:
    """the table of --amplicon-depth (load_amplicons): `names` = the primer ids by first appearance (the groups)"""

    def __init__(self, path: str):
        self._h = C.c_void_p()
        check(lib.pmx_amplicons_load(os.fsencode(path), C.byref(self._h)), "pmx_amplicons_load")
        self.names = [lib.pmx_amplicons_group_name(self._h, g).decode() for g in range(int(lib.pmx_amplicons_num_groups(self._h)))]

    def lookup(self, read_name) -> int:
        """the group of a read name (the FASTQ header up to the first white space), -1 when the file does not list it"""
        return int(lib.pmx_amplicons_lookup(self._h, read_name.encode() if isinstance(read_name, str) else read_name))

    def groups_of(self, names) -> np.ndarray:
        """Meta.set_amplicons' `groups` for reads with these names: an unlisted read gets len(self.names)"""
        g = np.array([self.lookup(x) for x in names], np.int32).reshape(-1)
        return np.where(g < 0, len(self.names), g).astype(np.int32)

    def __del__(self):
        try:
            if self._h:
                lib.pmx_amplicons_free(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def load_amplicons(path: str) -> Amplicons:
    """--amplicon-depth (pmx_amplicons_load; extractReadSequences, src/mgsr.cpp:1216-1342): `read id <TAB> primer id` lines"""
    return Amplicons(path)


def format_assigned(result: AssignResult, node_id, heads=None, taxon_names=None):
    """(`<prefix>.mgsr.assignedReads.out`, `<prefix>.mgsr.assignedReadsLCANode.out`) (writeAssignedReadsOut,
    src/main.cpp:522-558): one line per head node that has reads, `head[,folded nodes]<TAB>taxa<TAB>count<TAB>i,j,k` -- the
    indices are positions in the assigned-reads FASTQ, ascending.  The taxon column is `.` without `taxon_names`; with them
    (a result of a Meta with a taxonomy) the names of the head's S(head) by ascending taxon index joined with `,` (the
    reference iterates a hash set), `.` when the set is empty or over max_taxa.  Canonical order (the
    reference's comes from hash-map iteration): lines by ascending DFS index of the head, ids on a line the head, then the
    nodes folded into it by ascending DFS index."""
    heads = np.asarray(result.heads if heads is None else heads)
    members = {}
    for v in np.nonzero(heads != np.arange(len(heads)))[0].tolist():
        members.setdefault(int(heads[v]), []).append(v)

    def text(groups):
        lines = []
        for h in sorted(groups):
            ids = ",".join(node_id(x) for x in [h] + members.get(h, []))
            taxa = result.node_taxa(h) if taxon_names is not None else None
            col = ",".join(taxon_names[t] for t in taxa) if taxa is not None and len(taxa) else "."
            lines.append("%s\t%s\t%d\t%s" % (ids, col, len(groups[h]), ",".join(str(i) for i in sorted(groups[h]))))
        return "\n".join(lines) + ("\n" if lines else "")
    return text(result.by_node()), text(result.by_lca())


def sanitize_node_id(node_id: str) -> str:
    """the file stem of a node's BAM (alignAssignedReads' sanitize, src/main.cpp:615-717): `/`, `\\` and every character that
    isspace() knows in the "C" locale become `_`"""
    return "".join("_" if ch in "/\\ \t\n\v\f\r" else ch for ch in node_id)


def format_reference_fasta(pairs) -> str:
    """`<prefix>_mgsr_aligned/reference.fa` from (id, genome) pairs in node order: `>id`, then the genome in lines of at most 80
    bases (an empty genome: the header alone)"""
    out = []
    for node_id, genome in pairs:
        g = genome.decode() if isinstance(genome, (bytes, bytearray)) else genome
        out.append(">%s\n" % node_id)
        out.extend(g[i:i + 80] + "\n" for i in range(0, len(g), 80))
    return "".join(out)


def align_assigned(ctx: Context, pm: Panman, index: Index, result: AssignResult, reads, quals=None, min_num_align: int = 10):
    """--align-reads (alignAssignedReads, src/main.cpp:615-717): a generator over the head nodes of result.by_node() that have at
    least `min_num_align` reads (negative: 0), by ascending DFS index; it yields (head, fastq_indices, genome, records, cigars)
    with the node's reads -- ascending FASTQ index, every read single-end, a mate 2 as sequenced -- aligned to the node's own
    ungapped genome.  `reads` (and `quals`) are the raw reads given to Meta.set_reads; the assigned ones are uploaded once,
    each node's reads are one ReadSet.select of that set, and one Aligner is re-targeted node by node.  mean_read_len is the
    mean over the node's reads: the reference's aligner call sees only those.  `index`: the tree's index (its nodes are the
    PanMAN's, in DFS order)."""
    from .api import Aligner, ReadSet
    if index.info.n_nodes != pm.num_nodes or len(result.heads) != pm.num_nodes:
        raise ValueError("align_assigned: the index, the result and the PanMAN are not of one tree")
    by_node = result.by_node()
    k = max(int(min_num_align), 0)
    todo = [h for h in sorted(by_node) if len(by_node[h]) >= k]
    if not todo:
        return
    order = np.nonzero(result.fastq_index >= 0)[0]           # input order == ascending FASTQ index
    assigned = [bytes(reads[i]) for i in order.tolist()]
    lens = np.fromiter((len(r) for r in assigned), np.int64, len(assigned))
    rs = ReadSet(ctx, assigned, pack=False)
    if quals is not None:
        rs.set_qualities([bytes(quals[i]) for i in order.tolist()])
    aligner, sel = None, None
    try:
        for h in todo:
            idx = np.asarray(sorted(by_node[h]), np.int64)
            genome = pm.genome(h)
            mean_len = int(lens[idx].sum() // max(len(idx), 1))
            sel = rs.select(idx, out=sel)
            if aligner is None:
                aligner = Aligner(ctx, genome, mean_len)
            else:
                aligner.set_reference(genome, mean_len)
            aligner.align_readset(sel, paired=False)
            recs, cig = aligner.fetch()
            yield h, idx.tolist(), genome, recs.copy(), cig.copy()
    finally:
        if aligner is not None:
            aligner.close()
        if sel is not None:
            sel.close()
        rs.close()


BREADTHS_HEADER = ("NodeId\tTotalRefSeeds\tObservedBreadthCount\tObservedBreadthRatio\tTotalDepth\tMeanDepth\tExpectedBreadthRatio\t"
                   "ObservedToExpectedBreadthRatio")


def format_breadths(result: AssignResult, node_id, heads=None) -> str:
    """`<prefix>.mgsr.breadths.out` (src/main.cpp:957-1015; calculateBreadthRatio, src/mgsr.cpp:6518-6584) from a result of
    Meta.assign(breadth=True): the header, then one line per HEAD node, with or without reads, by ascending DFS index (the
    reference's pre-order of the collapsed tree): `head[,folded nodes]`, TotalRefSeeds, ObservedBreadthCount, its ratio to
    TotalRefSeeds, TotalDepth, MeanDepth = depth / TotalRefSeeds, ExpectedBreadthRatio = 1 - exp(-MeanDepth), observed over
    expected; a ratio whose denominator is 0 is 0; doubles as %g.  The header alone when no read is assigned."""
    if result.breadth is None:
        raise ValueError("format_breadths: the result was made without breadth=True")
    heads = np.asarray(result.heads if heads is None else heads)
    lines = [BREADTHS_HEADER]
    if (result.state == ASSIGNED).any():
        members = {}
        for v in np.nonzero(heads != np.arange(len(heads)))[0].tolist():
            members.setdefault(int(heads[v]), []).append(v)
        total, observed, depth = result.breadth
        for h in np.nonzero(heads == np.arange(len(heads)))[0].tolist():
            t, o, d = int(total[h]), int(observed[h]), int(depth[h])
            ratio = o / t if t > 0 else 0.0
            mean = d / t if t > 0 else 0.0
            expected = 1.0 - math.exp(-mean) if mean > 0 else 0.0
            lines.append("%s\t%d\t%d\t%g\t%d\t%g\t%g\t%g" % (",".join(node_id(x) for x in [h] + members.get(h, [])), t, o, ratio, d, mean, expected,
                                                              ratio / expected if expected > 0 else 0.0))
    return "\n".join(lines) + "\n"
