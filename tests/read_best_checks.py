"""The read-score reports of --meta (--write-meta-read-scores-unfiltered / -filtered; Meta.read_best, pmx_meta_read_best): the
restatement the tests compare the device path and the command line with, and the edge family.  No product code in here: it
sits on assign_checks.restate / presence, the node side comes from the ORIENTED index arrays alone.

Restatement (reference: scoreReads, src/mgsr.cpp:7325-7420; collapseIdenticalScoringNodes, :794-847; writeMetaReadScores and
the discard loop, src/main.cpp:446-466, 1225-1243):
  * active(v): v is the root, or one of v's change rows has a hash -- as it stands or in the other orientation -- among the
    distinct seedmer hashes of the merged reads;
  * max(r) = max over ALL nodes of score(r, v), score as in assign_checks;
  * n_best(r) = the number of ACTIVE nodes with score(r, v) == max(r), 0 when max(r) == 0.
An inactive node scores as its nearest active ancestor, whose DFS index is lower: the maximum over the active nodes is the
maximum over all, and the FIRST column of a tie set is always active.  Inactive columns can sit right after it, inside the set
and at its last column.

Edge family (EDGE_CASES, edge_tree): paths and stars of N = 1, 63, 64, 65, 127, 128, 129, 8,191, 8,192 and 8,193 nodes through
assign_checks.tree_from_plan; 8,192 columns are the 64 word pairs of one lane round of k_meta_read_best, one column more gives
a second round.  Four 150-base reads with disjoint seedmers cut from two random 400-base sequences, a copy, a reverse
complement and a random read:
  * `one`: a single best node -- the root of a path (column 0), leaf 1 of a star;
  * `spots`: best at exactly the columns 63, 64, 127, 128, 8,190 .. 8,192 (and on a path N - 1) that exist: one tie set over
    two words (63 | 64), two lanes (127 | 128) and two lane rounds (8,191 | 8,192); on a path 64, 128 and 8,191 carry no
    change and are inactive (the last column of a run of the set, and inside it), on a star every one of them is active;
  * `wide`: best from column 1 (path) / at the root and every leaf that does not lose a seedmer (star): more than 64 active
    best nodes from N = 127 on, with the quiet nodes -- 2 and 3 right after its first column, every fifth inside, on a star
    N - 1 at its last column -- inactive among them;
  * `marks`: its seedmers are toggled one at a time at every node that is not quiet, which is what makes those nodes active.
The plane count of the kernels follows the longest read of a set, and these reads have some 40 seedmers: 7 planes.  On the two
trees of 8,193 nodes (LONG_CASES) the set is also run with a 1,400-base read appended, which holds the seedmers of the four
reads among its 128 and more: the same tie sets through the 16-plane form, its 64 lanes and its second lane round."""
import functools

import numpy as np

import assign_checks as ac
from oracle import oracle_meta as om

EDGE_NS = (1, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193)
SPOTS = (63, 64, 127, 128, 8190, 8191, 8192)
HEADER = "ReadIndex\tNumDuplicates\tTotalScore\tMaxScore\tNumMaxScoreNodes\t%sRawReadsIndices\n"


# ------------------------------------------------------------------------------------------------ restatement
def active_flags(arrays, uniq):
    """one flag per node of the oriented index `arrays`: the root, or a change whose hash is in `uniq` in either orientation"""
    off = np.asarray(arrays["offsets"], np.int64)
    keys = np.asarray(arrays["hash"], np.uint64)
    n = len(arrays["parent"])
    node = np.repeat(np.arange(n), np.diff(off))
    hit = np.isin(keys, uniq) | np.isin(keys ^ np.uint64(ac.XOR), uniq)
    active = np.zeros(n, bool)
    active[0] = True
    active[node[hit]] = True
    return active


class Best:
    """active: per node; per MERGED read: max, n_best, n_all (the nodes, active or not, that reach the maximum; 0 when it is 0),
    n (its seedmers); scores[m]: merged read m over all nodes; merged: per raw read, -1 = dropped"""


def best_of_scores(arrays, uniq, scores, n, merged):
    B = Best()
    B.active, B.scores, B.n, B.merged = active_flags(arrays, uniq), scores, np.asarray(n, np.int64), np.asarray(merged, np.int64)
    B.max = scores.max(axis=1) if len(scores) else np.zeros(0, np.int64)
    at_max = (scores == B.max[:, None]) & (B.max[:, None] > 0)
    B.n_all = at_max.sum(axis=1)
    B.n_best = (at_max & B.active[None, :]).sum(axis=1)
    return B


def restate_best(arrays, reads, dust=100.0):
    """raw reads -> Best, through assign_checks.restate (merged reads in its order, which is the library's)"""
    R = ac.restate(arrays, reads, 0.0, dust)
    return best_of_scores(arrays, R.uniq, R.scores, [len(x) for x in R.lists], R.merged)


def best_of_lists(arrays, off, h, rev, merged):
    """merged seedmer lists as they are (after a mask: mask_checks.restate_masks) -> Best"""
    h = np.asarray(h, np.uint64)
    uniq = np.unique(h)
    P = ac.presence(arrays, uniq)
    scores = np.zeros((len(off) - 1, len(arrays["parent"])), np.int64)
    for i in range(len(off) - 1):
        u = np.searchsorted(uniq, h[off[i]:off[i + 1]])
        rv = np.asarray(rev[off[i]:off[i + 1]], np.int64)
        scores[i] = np.maximum(P[u, :, rv].sum(axis=0), P[u, :, 1 - rv].sum(axis=0))
    return best_of_scores(arrays, uniq, scores, np.diff(off), merged)


def scores_text(n_seedmers, mx, n_best, raw_to_merged, discard, filtered):
    """the text of <prefix>.read_scores_info.unfiltered.tsv / .filtered.tsv (writeMetaReadScores): a line per merged read with a
    non-zero maximum, the filtered file without the reads below int(seedmers * discard) and with a column that is always 0"""
    copies = {}
    for raw, m in enumerate(raw_to_merged):
        if m >= 0:
            copies.setdefault(int(m), []).append(raw)
    out = [HEADER % ("OvermaximumTaxonNumber\t" if filtered else "")]
    for m in range(len(mx)):
        if mx[m] == 0 or (filtered and int(mx[m]) < int(float(n_seedmers[m]) * discard)):
            continue
        c = copies.get(m, [])
        cols = [m, len(c), int(n_seedmers[m]), int(mx[m]), int(n_best[m])] + ([0] if filtered else []) + [",".join(str(x) for x in c)]
        out.append("\t".join(str(x) for x in cols) + "\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------------ edge family
class EdgeReads:
    """reads: the raw reads; one / spots / wide / marks / random: the reads of the module docstring; long: the read that,
    appended to `reads`, makes the longest read of the set one of 128 seedmers and more"""


@functools.lru_cache(maxsize=None)
def edge_reads():
    rng = np.random.default_rng(7325)
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    a, b = rnd(400), rnd(400)
    E = EdgeReads()
    E.one, E.spots, E.wide, E.marks, E.random = a[:150], a[200:350], b[:150], b[200:350], rnd(150)
    E.reads = [E.one, E.spots, E.wide, E.marks, E.random, E.wide, ac.revcomp(E.spots)]
    E.long = a + b + rnd(600)                                    # holds the seedmers of the four reads among its own
    assert len(om.seedmers(E.long, ac.K, ac.S, ac.L)) >= 128
    sets = [{h for h, _ in om.seedmers(r, ac.K, ac.S, ac.L)} for r in E.reads[:5]]
    assert all(sets) and all(not (sets[i] & sets[j]) for i in range(5) for j in range(i))
    return E


def _quiet(n, shape):
    q = {2, 3, 64, 128, 8191} | set(range(5, n, 5))
    if shape == "star":
        q = (q - set(SPOTS)) | {n - 1}
    return q


def _edge_plan(n, shape):
    E = edge_reads()
    keys = lambda r: [(h, int(rev)) for h, rev in om.seedmers(r, ac.K, ac.S, ac.L)]
    plan = {}

    def toggle(v, key):
        assert key not in plan.setdefault(v, {})
        plan[v][key] = "toggle"

    one, spots, wide, marks = keys(E.one), keys(E.spots), keys(E.wide), keys(E.marks)
    want = {v for v in SPOTS if v < n} | ({n - 1} if shape == "path" or n == 1 else set())
    for key in spots[1:]:
        toggle(0, key)
    if shape == "path":
        for key in one:
            toggle(0, key)
        if n > 1:
            toggle(1, one[0])
            for key in wide:
                toggle(1, key)
        for v in range(n):                                       # spots[0] is present exactly on the columns of `want`
            if (v in want) != (v > 0 and v - 1 in want):
                toggle(v, spots[0])
    else:
        for key in one:
            toggle(min(1, n - 1), key)
        for key in wide:
            toggle(0, key)
        for v in sorted(want):
            toggle(v, spots[0])
        for v in range(1, n, 7):
            toggle(v, wide[v % len(wide)])
    quiet = _quiet(n, shape)
    for v in range(1, n):
        if v not in quiet:
            toggle(v, marks[v % len(marks)])
    return plan


# a path and a star of every N of EDGE_NS (N = 1: the one node once)
EDGE_CASES = tuple((n, shape) for n in EDGE_NS for shape in (("path", "star") if n > 1 else ("path",)))


@functools.lru_cache(maxsize=None)
def edge_tree(n, shape):
    parent = np.array([0] + ([v - 1 for v in range(1, n)] if shape == "path" else [0] * (n - 1)), np.uint32)
    return ac.tree_from_plan("%s%d" % (shape, n), parent, _edge_plan(n, shape), np.random.default_rng(794 + n))


@functools.lru_cache(maxsize=None)
def edge_restated(n, shape):
    return restate_best(edge_tree(n, shape).oriented, edge_reads().reads)


LONG_CASES = ((8193, "path"), (8193, "star"))


@functools.lru_cache(maxsize=None)
def edge_restated_long(n, shape):
    """the same tree with the 1,400-base read in the set: every read of it then goes through the 16-plane kernels"""
    E = edge_reads()
    return restate_best(edge_tree(n, shape).oriented, E.reads + [E.long])


@functools.lru_cache(maxsize=None)
def crafted_best(i):
    return restate_best(ac.crafted_trees()[i].oriented, ac.crafted_reads()[0])


def check_best(meta, want, label=""):
    """Meta.read_best() / active_nodes() / raw_to_merged() against a Best"""
    mx, nb = meta.read_best()
    assert np.array_equal(meta.raw_to_merged(), want.merged), label
    assert np.array_equal(meta.active_nodes(), want.active), (label, np.nonzero(meta.active_nodes() != want.active)[0][:5])
    assert mx.dtype == np.uint16 and nb.dtype == np.uint32 and len(mx) == len(want.max) == len(nb), label
    assert np.array_equal(mx, want.max), (label, np.nonzero(mx != want.max)[0][:5])
    assert np.array_equal(nb, want.n_best), (label, np.nonzero(nb != want.n_best)[0][:5], nb[nb != want.n_best][:5], want.n_best[nb != want.n_best][:5])
