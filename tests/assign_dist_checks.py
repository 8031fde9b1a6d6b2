"""--meta --filter-and-assign over several ranks: the inputs of tests/test_meta_assign_dist_gpu.py and the conditions they must
meet, shown with the restatements of assign_checks and breadth_checks alone (tests/test_assign_dist_families.py).  No product
code in here.

Inputs:
  * rsv: the 70 / 30 mixture of dist_meta_worker.sample (700 + 300 tiled reads of rsv_4K), cut `rsv` (two halves) and `shards`
    (70 / 30), discard 0;
  * crafted: the `broom` shape of place_tree_checks (109 nodes: two words a row, the second one partly filled) carrying the
    seedmers of breadth_checks.reads() the way assign_checks places them (gained and lost at random nodes in either
    orientation), cut in two halves, discard breadth_checks.DISCARD;
  * two: two reads of the crafted set with distinct lists, over three ranks: the merged reads' rows are 0, 1, 1.
A rank's SHARD is a contiguous piece of the raw reads (`cut`); its ROWS are a contiguous piece of the whole sample's merged
reads (`rows`), the rule of pmx_meta_score.  The two have nothing to do with one another.

conditions(R, shards): what a cut must give for the collective to be tested at all --
  shared_lists    merged lists that occur in more than one shard (the multiplicities add across ranks);
  only / both     (seedmer, node) hits of the breadth matrix that come from one rank's rows alone, per rank, and from more than
                  one rank's (the union over ranks is an OR, not a sum);
  assigned        assigned merged reads per rank's rows (the row boundary falls strictly inside the assigned reads when two
                  neighbouring ranks both have some)."""
import functools

import numpy as np

import assign_checks as ac
import breadth_checks as bc
import place_tree_checks as ptc

CRAFTED_SHAPE = "broom"


def cut(case, n, rank, world):
    """the shard of `rank`: the cuts of dist_meta_worker.cut, restated"""
    if case == "shards":
        c = n * 7 // 10
        return (0, c) if rank == 0 else (c, n)
    if case == "empty":
        return (0, n) if rank == 0 else (n, n)
    return n * rank // world, n * (rank + 1) // world


def rows(n_merged, rank, world):
    """(first, count): the merged reads whose rows `rank` owns"""
    first = n_merged * rank // world
    return first, n_merged * (rank + 1) // world - first


@functools.lru_cache(maxsize=None)
def crafted():
    """(CraftedTree on the broom shape, its reads)"""
    reads, seqs, random_reads = ac.crafted_reads()
    rng = np.random.default_rng(109)
    in_seqs = {h for q in seqs for h, _ in ac.om.seedmers(q, ac.K, ac.S, ac.L)}
    extra = sorted({h for r in reads if r not in random_reads for h, _ in ac.om.seedmers(r, ac.K, ac.S, ac.L)} - in_seqs)
    parent = np.asarray(ptc.shape_parent(CRAFTED_SHAPE)[0], np.uint32)
    return ac._make_tree(CRAFTED_SHAPE, parent, seqs, extra, rng), bc.reads()


@functools.lru_cache(maxsize=None)
def crafted_restated():
    tree, reads = crafted()
    return ac.restate(tree.oriented, reads, bc.DISCARD)


@functools.lru_cache(maxsize=None)
def two_reads():
    """two reads of the crafted set that are assigned and have distinct seedmer lists, in input order"""
    R = crafted_restated()
    _, reads = crafted()
    first = int(np.nonzero(R.state == ac.ASSIGNED)[0][0])
    second = int(np.nonzero((R.state == ac.ASSIGNED) & (R.merged != R.merged[first]))[0][0])
    return [reads[first], reads[second]]


def hit_matrix(R, first, count):
    """[distinct seedmers][nodes] bool: the (seedmer, node) pairs the assigned merged reads of rows [first, first + count) hit --
    the seedmer is one of the read's, the node one of its assigned nodes, and the node's genome holds it in either orientation"""
    P = R.presence.any(axis=2)
    H = np.zeros(P.shape, bool)
    raw_of = {}
    for r in np.nonzero(R.merged >= 0)[0].tolist():
        raw_of.setdefault(int(R.merged[r]), r)
    for m in range(first, first + count):
        r = raw_of[m]
        if R.state[r] != ac.ASSIGNED:
            continue
        u = np.unique(np.searchsorted(R.uniq, np.array([h for h, _ in R.lists[m]], np.uint64)))
        nodes = np.asarray(R.nodes[r], np.int64)
        H[np.ix_(u, nodes)] |= P[np.ix_(u, nodes)]
    return H


def conditions(R, shards):
    """R: assign_checks.restate of the WHOLE sample; shards: [(lo, hi)] per rank"""
    world = len(shards)
    n_merged = len(R.lists)
    in_shard = [set(R.merged[lo:hi].tolist()) - {-1} for lo, hi in shards]
    seen, shared = set(), set()
    for s in in_shard:
        shared |= s & seen
        seen |= s
    assigned_merged = set(R.merged[R.state == ac.ASSIGNED].tolist())
    own = [rows(n_merged, r, world) for r in range(world)]
    H = [hit_matrix(R, f, c) for f, c in own]
    covered = np.sum(H, axis=0)
    return dict(n_merged=n_merged, rows=own, shared_lists=len(shared),
                only=[int((H[r] & (covered == 1)).sum()) for r in range(world)], both=int((covered > 1).sum()),
                assigned=[sum(1 for m in range(f, f + c) if m in assigned_merged) for f, c in own])
