"""The taxonomy filter of --meta --filter-and-assign: the labelling of the test trees, subtree taxon sets, a metadata file
with every feature of the parser, and the LITERAL restatement of the reference's rule on top of assign_checks.restate.  No
product code in here.

The rule (fillTaxonIndices, src/mgsr.cpp:156-196; checkTaxonIndicesBatch, :6463-6496; scoreReadsBatchHelper, :7488-7552):
  * S(v) = the taxa of the nodes in the subtree of v, in the tree as indexed (identical nodes not folded);
  * a read has a RECORD at node v when one of its seedmers changes presence there, 0 <-> positive, in either orientation
    (at the root: is present): touched = presence XOR the parent's presence;
  * an assigned read (max != 0 after the discard step) with amb = max(A, int(max * ratio)), lo = max(0, max - amb) collects S(v)
    over the touched nodes with score >= lo; it is over, and loses its nodes and its LCA, when the union holds more than M taxa.
`qualifying="all"` is the rule without the records (the union over ALL nodes with score >= lo): equal for lo >= 1, and what the
"absolute" leg must differ from."""
import numpy as np

import assign_checks as ac

OVER_TAXA = 3
TREES = {t: i for i, t in enumerate(("one", "path3", "star71", "binary127", "binary129", "random300"))}

# leg -> [(tree, discard, A, ratio, T, M)]
LEGS = {
    "default": [(t, 0.5, 0, 0.0, 16, 1) for t in ("star71", "binary127", "binary129", "random300")],
    "two": [("binary129", 0.0, 0, 0.0, 16, 2)],
    "ratio": [("star71", 0.0, 0, 0.25, 16, 1), ("star71", 0.0, 0, 0.25, 16, 2)],
    "absolute": [(t, 0.0, 20, 0.0, 16, 8) for t in ("star71", "binary127", "random300")],
    "small": [(t, 0.5, 0, 0.0, 16, 1) for t in ("one", "path3")],
}


def label(parent, T):
    """the taxon of every node, -1 = none: a leaf v with v % 7 != 3 and an internal node with v % 11 == 5 get (v * T) // n"""
    n = len(parent)
    internal = np.zeros(n, bool)
    internal[np.asarray(parent[1:], np.int64)] = True
    v = np.arange(n)
    own = np.where(internal, v % 11 == 5, v % 7 != 3)
    return np.where(own, (v * T) // n, -1).astype(np.int32)


def subtree_sets(parent, node_taxon):
    """S(v) as a list of sets"""
    n = len(parent)
    S = [set() if node_taxon[v] < 0 else {int(node_taxon[v])} for v in range(n)]
    for v in range(n - 1, 0, -1):                                    # pre-order: children come after their parents
        S[int(parent[v])] |= S[v]
    return S


def write_metadata(path, ids, node_taxon, rank="Family"):
    """a table with the rank in the third column, a decoy column before and after it, a `.` row, an unknown identifier (with a
    taxon of its own) and a repeated identifier whose later row counts.  Taxon t is named `tax<t>`.  Returns the names in
    order of first appearance, as the parser must number them."""
    rows = [("no_such_node", "x", "elsewhere", "y")]
    labelled = [v for v in range(len(ids)) if node_taxon[v] >= 0]
    bare = [v for v in range(len(ids)) if node_taxon[v] < 0]
    if labelled:
        rows.append((ids[labelled[-1]], "x", "overwritten", "y"))    # the node's own row comes later
    for v in labelled:
        rows.append((ids[v], "tax%d" % ((node_taxon[v] + 1) % 7), "tax%d" % node_taxon[v], "decoy%d" % v))
    if bare:
        rows.append((ids[bare[0]], "x", ".", "y"))
    names = []
    for r in rows:
        if r[2] != "." and r[2] not in names:
            names.append(r[2])
    with open(path, "w") as f:
        f.write("sample\tGenus \t%s\tOrder\n" % rank)
        for i, r in enumerate(rows):
            f.write(("\t" if i % 2 else "  ").join(r) + "\n")
            if i == 1:
                f.write("\n")                                        # an empty line is skipped
    return names


class RestatedTaxa:
    """per RAW read: state (assign_checks' with OVER_TAXA), max, nodes, lca (as assign_checks.Restated; over reads have no
    nodes and lca -1), taxa (sorted list; empty unless assigned); merged"""


def restate_taxa(R, parent, node_taxon, M, A=0, ratio=0.0, qualifying="touched"):
    parent = np.asarray(parent, np.int64)
    S = subtree_sets(parent, node_taxon)
    P = R.presence                                                   # [uniq][node][orientation]
    changed = P ^ P[:, parent, :]
    changed[:, 0, :] = P[:, 0, :]
    touch = changed.any(axis=2)                                      # [uniq][node]
    out = RestatedTaxa()
    out.merged, out.max = R.merged, R.max
    out.state, out.lca = R.state.copy(), R.lca.copy()
    out.nodes, out.taxa = list(R.nodes), [[] for _ in R.nodes]
    per_merged = {}
    for r in np.nonzero(R.state == ac.ASSIGNED)[0].tolist():
        m = int(R.merged[r])
        if m not in per_merged:
            row, mx = R.scores[m], int(R.max[r])
            lo = max(0, mx - max(A, int(mx * ratio)))
            ok = row >= lo
            if qualifying == "touched":
                u = np.searchsorted(R.uniq, np.array([h for h, _ in R.lists[m]], np.uint64))
                ok &= touch[u].any(axis=0)
            U = set()
            for v in np.nonzero(ok)[0].tolist():
                U |= S[v]
            per_merged[m] = sorted(U)
        if len(per_merged[m]) > M:
            out.state[r], out.lca[r], out.nodes[r] = OVER_TAXA, -1, np.zeros(0, np.int64)
        else:
            out.taxa[r] = per_merged[m]
    return out


def with_discard(R, discard, parent):
    """assign_checks.restate's result at another discard ratio, from the scores it already holds"""
    out = ac.Restated()
    out.lists, out.uniq, out.presence, out.scores, out.merged, out.n, out.max = R.lists, R.uniq, R.presence, R.scores, R.merged, R.n, R.max
    out.state, out.lca, out.nodes = np.zeros_like(R.state), np.full_like(R.lca, -1), [np.zeros(0, np.int64)] * len(R.nodes)
    per_merged = {}
    for r in np.nonzero(R.merged >= 0)[0].tolist():
        m, mx = int(R.merged[r]), int(R.max[r])
        if m not in per_merged:
            st = ac.UNMAPPED if mx == 0 else ac.DISCARDED if mx < int(float(len(R.lists[m])) * discard) else ac.ASSIGNED
            nodes = np.nonzero(R.scores[m] == mx)[0] if st == ac.ASSIGNED else np.zeros(0, np.int64)
            per_merged[m] = (st, nodes, ac.lca_of_set(parent, nodes) if st == ac.ASSIGNED else -1)
        out.state[r], out.nodes[r], out.lca[r] = per_merged[m]
    return out


_restated = {}


def crafted_leg(tree, discard, A, ratio, T, M, qualifying="touched"):
    """(tree object, node_taxon, the restatement) of one case of LEGS"""
    key = (tree, discard, A, ratio, T, M, qualifying)
    t = ac.crafted_trees()[TREES[tree]]
    taxon = label(t.parent, T)
    if key not in _restated:
        base = ("base", tree, discard)
        if base not in _restated:
            R = ac.crafted_restated(TREES[tree])                     # (discard 0.5: the one the other test files share)
            _restated[base] = R if discard == 0.5 else with_discard(R, discard, t.parent)
        _restated[key] = restate_taxa(_restated[base], t.parent, taxon, M, A, ratio, qualifying)
    return t, taxon, _restated[key]


RSV_T, RSV_DISCARD = 16, 0.0


def rsv_leg(arrays):
    """the rsv family (assign_checks.rsv_reads) with the labelling at T = RSV_T, M = 1, no ambiguity option"""
    if "rsv" not in _restated:
        _restated["rsv"] = restate_taxa(ac.rsv_restated(arrays, RSV_DISCARD), arrays["parent"], label(arrays["parent"], RSV_T), 1)
    return _restated["rsv"]


def counts(want):
    """(over reads, kept reads) among the merged reads"""
    return tuple(len(set(want.merged[want.state == st].tolist())) for st in (OVER_TAXA, ac.ASSIGNED))


def check_taxa_result(res, want, heads, label=""):
    """a Meta.assign result with a taxonomy against the literal restatement, read by read"""
    assert np.array_equal(res.merged, want.merged), label
    assert np.array_equal(res.state, want.state), (label, np.nonzero(res.state != want.state)[0][:5])
    mapped = want.merged >= 0
    assert np.array_equal(res.max[mapped], want.max[mapped]), (label, np.nonzero(res.max != want.max)[0][:5])
    for r in range(len(want.state)):
        assert np.array_equal(res.nodes_of(r), want.nodes[r]), (label, r)
        assert res.lca[r] == (heads[want.lca[r]] if want.lca[r] >= 0 else -1), (label, r)
        assert res.taxa_of(r).tolist() == want.taxa[r], (label, r, res.taxa_of(r), want.taxa[r])
