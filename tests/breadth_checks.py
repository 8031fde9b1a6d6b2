"""--meta --filter-and-assign --breadth-ratio: the restatement the tests compare the device path with, the text of
`<prefix>.mgsr.breadths.out`, the read family and a hand-written tree.  No product code in here.

Restatement (reference: mgsrPlacer::calculateBreadthRatio, src/mgsr.cpp:6518-6584; the file, src/main.cpp:957-1015), LITERAL: one
walk over the tree with `refSeedsCount`, a dict hash -> countFwd + countRev that a node's changes are applied to on the way in
(erased at 0) and reverted on the way out; at every node the loops over `assignedReadsByNode[node]` (merged reads, keyed by
HEAD) and over the read's distinct hashes, `seedHitCounts[hash] += dup`, `totalDepth += dup` (the inner loop as one set
intersection: rsv has 1.4 M (node, read) pairs).  The index is oriented: a hash is the
pair {key, key ^ XOR}, named here by the smaller of the two.  A node folded into its head has no changes and no entry of its
own; it gets its head's numbers afterwards.  The assignment comes from assign_checks.restate (or taxa_checks.restate_taxa on top
of it): the reference derives it a second time from the assigned FASTQ, to the same end.

closed_form is the matrix statement of the same thing (numpy), what the device computes; test_breadth_families holds the two
against each other."""
import functools
import math

import numpy as np

import assign_checks as ac
from oracle import oracle_meta as om

XOR = ac.XOR
HEADER = ("NodeId\tTotalRefSeeds\tObservedBreadthCount\tObservedBreadthRatio\tTotalDepth\tMeanDepth\tExpectedBreadthRatio\t"
          "ObservedToExpectedBreadthRatio")
DISCARD = 0.5                                                        # of the crafted family, as in assign_checks.crafted_restated
FLUSH = 3                                                            # the lowered PMX_META_BREADTH_FLUSH of the tests


def canon(key):
    key = int(key)
    return min(key, key ^ XOR)


# ------------------------------------------------------------------------------------------------ read family
@functools.lru_cache(maxsize=None)
def reads():
    """assign_checks.crafted_reads() plus two tandem reads (a read that repeats hashes: 92 and 85 seedmers, 49 and 36 distinct)
    and a second copy of the first of them (a merged read of multiplicity 2 that repeats hashes)"""
    base, seqs, _ = ac.crafted_reads()
    tandem = [seqs[0][100:250] * 2, seqs[2][40:160] * 2 + seqs[2][40:100]]
    return list(base) + tandem + [tandem[0]]


@functools.lru_cache(maxsize=None)
def crafted_restated(tree_index):
    return ac.restate(ac.crafted_trees()[tree_index].oriented, reads(), DISCARD)


# ------------------------------------------------------------------------------------------------ restatement
def multiplicities(merged):
    dup = {}
    for m in np.asarray(merged).tolist():
        if m >= 0:
            dup[m] = dup.get(m, 0) + 1
    return dup


def assigned_reads_by_node(want, heads):
    """{head: [merged reads assigned to it or to a node folded into it]}; want: per RAW read merged / state / nodes"""
    out, seen = {}, set()
    for r in range(len(want.state)):
        m = int(want.merged[r])
        if want.state[r] != ac.ASSIGNED or m in seen:
            continue
        seen.add(m)
        for h in sorted({int(heads[v]) for v in want.nodes[r]}):
            out.setdefault(h, []).append(m)
    return out


def restate_breadth(arrays, want, lists):
    """(total_ref_seeds, observed, depth): int64 per node.  arrays: the ORIENTED index; want: the assignment per raw read
    (assign_checks.Restated or taxa_checks.RestatedTaxa); lists: the merged reads' seedmer lists (Restated.lists)"""
    parent, off = np.asarray(arrays["parent"], np.int64), np.asarray(arrays["offsets"], np.int64)
    keys = np.asarray(arrays["hash"], np.uint64)
    keys = np.minimum(keys, keys ^ np.uint64(XOR)).tolist()          # canon() of every key
    pc, cc = arrays["parent_count"].tolist(), arrays["child_count"].tolist()
    n = len(parent)
    heads = ac.heads_np(parent, arrays["offsets"])
    by_node, dup = assigned_reads_by_node(want, heads), multiplicities(want.merged)
    unique = {m: frozenset(canon(h) for h, _ in lists[m]) for m in {m for ms in by_node.values() for m in ms}}
    children = [[] for _ in range(n)]
    for v in range(1, n):
        children[parent[v]].append(v)
    ref = {}                                                         # refSeedsCount

    def apply(v, frm, to):
        for q in range(off[v], off[v + 1]):
            x = ref.get(keys[q], 0) + to[q] - frm[q]
            assert x >= 0
            if x == 0:
                ref.pop(keys[q], None)
            else:
                ref[keys[q]] = x

    total, observed, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = [(0, False)]
    while stack:
        v, leaving = stack.pop()
        if leaving:
            apply(v, cc, pc)
            continue
        apply(v, pc, cc)
        hits, d = set(), 0                                           # the keys of seedHitCounts (its values are never read), totalDepth
        for m in by_node.get(v, ()):
            found = unique[m] & ref.keys()                           # the read's distinct hashes that are in refSeedsCount
            hits |= found
            d += dup[m] * len(found)
        total[v], observed[v], depth[v] = len(ref), len(hits), d
        stack.append((v, True))
        for c in reversed(children[v]):
            stack.append((c, False))
    assert not ref
    return total[heads], observed[heads], depth[heads]


def closed_form(R):
    """(observed, depth) from matrices, R an assign_checks.Restated: P[s][v] = present in either orientation, mask[r][v] = the
    best columns of an assigned merged read, carry[r][s] = read r has hash s"""
    P = R.presence.any(axis=2)
    n_merged = len(R.lists)
    mask = np.zeros((n_merged, P.shape[1]), bool)
    for r in np.nonzero(R.state == ac.ASSIGNED)[0].tolist():
        mask[int(R.merged[r]), R.nodes[r]] = True
    carry = np.zeros((n_merged, len(R.uniq)), bool)
    for m, x in enumerate(R.lists):
        carry[m, np.searchsorted(R.uniq, np.array([h for h, _ in x], np.uint64))] = True
    dup = multiplicities(R.merged)
    mult = np.array([dup[m] for m in range(n_merged)], np.int64)
    observed = (((carry.T.astype(np.int64) @ mask.astype(np.int64)) > 0) & P).sum(axis=0)
    depth = ((carry.astype(np.int64) @ P.astype(np.int64)) * mask * mult[:, None]).sum(axis=0)
    return observed, depth


def restate_text(numbers, heads, node_id, any_assigned):
    """the file: the header, then (when a read is assigned) one line per head in pre-order"""
    lines = [HEADER]
    total, observed, depth = numbers
    folded = {}
    for v in range(len(heads)):
        if heads[v] != v:
            folded.setdefault(int(heads[v]), []).append(v)
    for h in range(len(heads) if any_assigned else 0):
        if heads[h] != h:
            continue
        ids = ",".join(node_id(v) for v in [h] + folded.get(h, []))
        t, o, d = int(total[h]), int(observed[h]), int(depth[h])
        ratio = float(o) / float(t) if t > 0 else 0.0
        mean = float(d) / float(t) if t > 0 else 0.0
        expected = 1.0 - math.exp(-mean) if mean > 0 else 0.0
        o2e = ratio / expected if expected > 0 else 0.0
        lines.append("%s\t%d\t%d\t%g\t%d\t%g\t%g\t%g" % (ids, t, o, ratio, d, mean, expected, o2e))
    return "\n".join(lines) + "\n"


def check_numbers(got, want, heads, label=""):
    """AssignResult.breadth against restate_breadth, bit for bit at every node; folded nodes equal their heads"""
    assert got is not None, label
    for name, g, w in zip(("total_ref_seeds", "observed", "depth"), got, want):
        g = np.asarray(g)
        assert g.dtype == np.int64 and np.array_equal(g, w), (label, name, np.nonzero(g != w)[0][:5], g[g != w][:5], w[g != w][:5])
        assert np.array_equal(g, g[heads]), (label, name)


# ------------------------------------------------------------------------------------------------ a hand-written tree
@functools.lru_cache(maxsize=None)
def three_nodes():
    """(CraftedTree, reads, (total, observed, depth)): a root with two children, numbers worked out by hand.

    X = the window [0, 150) of the family's first sequence, Z = that of its second one; all their seedmers are distinct
    hashes (asserted).  A = the first 10 seedmers of X, nz = the seedmers of Z.
      node 0 (root)  gains A the way X holds it, count 1.
      node 1         loses all of A: its genome holds nothing.
      node 2         loses the first 2 of A; gains every seedmer of Z in the orientation Z does NOT have, count 2.
    Reads: X twice (one merged read, multiplicity 2), revcomp(X) (the same hashes, the orientations flipped: another merged
    read), Z.  Scores: X and revcomp(X) 10 at the root, 0 at node 1, 8 at node 2 -> both assigned to the root alone; Z 0, 0, nz
    -> assigned to node 2 (through the other orientation).  At discard 0:
      node 0: TotalRefSeeds 10, observed 10 (A, by both reads: counted once), depth 2 * 10 + 1 * 10 = 30
      node 1: 0, 0, 0 -> all four ratios 0
      node 2: TotalRefSeeds 8 + nz, observed nz, depth nz (Z alone; X is not assigned here although 8 of its hashes are present)"""
    seqs = ac.crafted_reads()[1]
    X, Z = seqs[0][:150], seqs[1][:150]
    sx, sz = om.seedmers(X, ac.K, ac.S, ac.L), om.seedmers(Z, ac.K, ac.S, ac.L)
    assert len({h for h, _ in sx} | {h for h, _ in sz}) == len(sx) + len(sz) and len(sx) > 12
    A, nz = sx[:10], len(sz)
    key = lambda h, o: int(h) ^ XOR if o else int(h)
    o_rows = [[(key(h, int(rv)), 0, 1) for h, rv in A],
              [(key(h, int(rv)), 1, 0) for h, rv in A],
              [(key(h, int(rv)), 1, 0) for h, rv in A[:2]] + [(key(h, 1 - int(rv)), 0, 2) for h, rv in sz]]
    p_rows = [[(int(h), 0, 1) for h, _ in A], [(int(h), 1, 0) for h, _ in A], [(int(h), 1, 0) for h, _ in A[:2]] + [(int(h), 0, 2) for h, _ in sz]]
    parent = np.array([0, 0, 0], np.uint32)

    def arrays(rows):
        off = np.zeros(4, np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows])
        flat = [e for r in rows for e in sorted(r)]
        return dict(parent=parent, offsets=off, hash=np.array([e[0] for e in flat], np.uint64),
                    parent_count=np.array([e[1] for e in flat], np.int16), child_count=np.array([e[2] for e in flat], np.int16))
    numbers = (np.array([10, 0, 8 + nz], np.int64), np.array([10, 0, nz], np.int64), np.array([30, 0, nz], np.int64))
    return ac.CraftedTree("three", parent, arrays(o_rows), arrays(p_rows)), [X, Z, ac.revcomp(X), X], numbers
