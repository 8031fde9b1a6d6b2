"""--meta --filter-and-assign: the restatement the tests compare the device path with, and the two input families.
No product code in here: seedmers come from oracle_meta.seedmers, the node side from the ORIENTED index arrays alone.

Restatement (reference: scoreReadsBatch / assignReadsBatch, src/mgsr.cpp:7477-7575, 6415-6516; src/main.cpp:856-863):
  * presence[distinct read seedmer][node][orientation], by one pass over the nodes in DFS pre-order: a node starts from its
    parent's column and applies its own count changes (child count > 0 = present);
  * score(read, node) = max(#seedmers present in the read's orientation, #present in the other one); max over all nodes;
    max == 0 -> unmapped, max < int(discard * n) -> discarded, else assigned to ALL nodes with score == max;
  * LCA by walking parents; heads: a non-root node without changes folds into its nearest ancestor that has some.
Merged reads: distinct seedmer lists in the order of (hash list, orientation list); reads without seedmers or dropped by
DUST map to -1.

Families:
  * crafted: trees in DFS pre-order given as index arrays (one node, path of 3, star of 1 + 70, binary of 127 and of 129 nodes,
    random tree of 300), one read set for all of them (windows of four random 400-base sequences, their reverse complements,
    copies, windows with two substitutions, half-random reads, random reads, a read shorter than k, a 1,200-base read and
    its prefixes with 127 and 128 seedmers); every seedmer is gained and lost at randomly chosen nodes in either or both
    orientations, half of the nodes carry no change at all;
  * rsv: rsv_4K.panman whole, 600 reads tiled over two of its genomes, every third reverse-complemented, 100 with two
    substitutions, 20 copies, 60 random reads."""
import functools
import os

import numpy as np

from conftest import GOLDEN
from oracle import oracle_meta as om

K, S, L = 19, 8, 3
XOR = om.ORIENT_XOR
UNMAPPED, DISCARDED, ASSIGNED = 0, 1, 2
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s.translate(_RC)[::-1]


# ------------------------------------------------------------------------------------------------ tree arithmetic
def heads_np(parent, offsets):
    n = len(parent)
    head = np.arange(n)
    for v in range(1, n):
        if offsets[v] == offsets[v + 1]:
            head[v] = head[parent[v]]
    return head


def lca_np(parent, a, b):
    anc = set()
    v = int(a)
    while True:
        anc.add(v)
        if v == 0:
            break
        v = int(parent[v])
    v = int(b)
    while v not in anc:
        v = int(parent[v])
    return v


def lca_of_set(parent, nodes):
    out = int(nodes[0])
    for v in nodes[1:]:
        out = lca_np(parent, out, int(v))
    return out


# ------------------------------------------------------------------------------------------------ restatement
def presence(arrays, uniq):
    """[len(uniq)][n_nodes][2] bool: read seedmer `uniq[u]` present at node v in the forward (0) / reverse (1) orientation"""
    parent, off, cc = arrays["parent"], arrays["offsets"], arrays["child_count"]
    keys = np.asarray(arrays["hash"], np.uint64)
    n = len(parent)
    P = np.zeros((len(uniq), n, 2), bool)
    if len(uniq) == 0:
        return P
    uid = np.full(len(keys), -1, np.int64)
    ori = np.zeros(len(keys), np.int64)
    for o, kk in ((0, keys), (1, keys ^ np.uint64(XOR))):
        pos = np.minimum(np.searchsorted(uniq, kk), len(uniq) - 1)
        hit = (uniq[pos] == kk) & (uid < 0)
        uid[hit], ori[hit] = pos[hit], o
    for v in range(n):
        if v > 0:
            P[:, v, :] = P[:, parent[v], :]
        a, b = int(off[v]), int(off[v + 1])
        sel = uid[a:b] >= 0
        if sel.any():
            P[uid[a:b][sel], v, ori[a:b][sel]] = cc[a:b][sel] > 0
    return P


class Restated:
    """per RAW read: merged (-1 = dropped), n, max, state, nodes (list of arrays; empty unless assigned), lca (-1 unless
    assigned); `scores[m]` is merged read m's score row over all nodes, `lists` the merged reads' seedmer lists"""


def restate(arrays, reads, discard, dust=100.0, k=K, s=S, l=L):
    lists = []
    for r in reads:
        d = om.get_dust(r) if dust < 100.0 else 0.0
        lists.append(() if (d != 0 and d > dust) else tuple(om.seedmers(r, k, s, l)))
    distinct = sorted({x for x in lists if x}, key=lambda x: (tuple(h for h, _ in x), tuple(int(v) for _, v in x)))
    index = {x: i for i, x in enumerate(distinct)}
    uniq = np.array(sorted({h for x in distinct for h, _ in x}), np.uint64)
    P = presence(arrays, uniq)
    parent = arrays["parent"]
    R = Restated()
    R.lists, R.uniq, R.presence = distinct, uniq, P
    R.scores = np.zeros((len(distinct), len(parent)), np.int64)
    for i, x in enumerate(distinct):
        u = np.searchsorted(uniq, np.array([h for h, _ in x], np.uint64))
        rv = np.array([int(v) for _, v in x])
        R.scores[i] = np.maximum(P[u, :, rv].sum(axis=0), P[u, :, 1 - rv].sum(axis=0))
    n_raw = len(reads)
    R.merged = np.array([index[x] if x else -1 for x in lists], np.int64)
    R.n = np.array([len(x) for x in lists], np.int64)
    R.max = np.zeros(n_raw, np.int64)
    R.state = np.zeros(n_raw, np.int64)
    R.lca = np.full(n_raw, -1, np.int64)
    R.nodes = [np.zeros(0, np.int64)] * n_raw
    per_merged = {}
    for r in range(n_raw):
        m = int(R.merged[r])
        if m < 0:
            continue
        if m not in per_merged:
            row = R.scores[m]
            mx = int(row.max())
            st = UNMAPPED if mx == 0 else DISCARDED if mx < int(float(len(distinct[m])) * discard) else ASSIGNED
            nodes = np.nonzero(row == mx)[0] if st == ASSIGNED else np.zeros(0, np.int64)
            per_merged[m] = (mx, st, nodes, lca_of_set(parent, nodes) if st == ASSIGNED else -1)
        R.max[r], R.state[r], R.nodes[r], R.lca[r] = per_merged[m]
    return R


# ------------------------------------------------------------------------------------------------ crafted family
def _preorder(children):
    """children lists of a tree rooted at 0 (any numbering) -> the parent array in DFS pre-order numbering"""
    parent, stack = [], [(0, 0)]                                 # (node, new index of its parent)
    while stack:
        old, par = stack.pop()
        new = len(parent)
        parent.append(par)
        for c in reversed(children[old]):
            stack.append((c, new))
    return np.array(parent, np.uint32)


def _tree_shapes(rng):
    def heap(n):
        return [[c for c in (2 * v + 1, 2 * v + 2) if c < n] for v in range(n)]
    ch300 = [[] for _ in range(300)]
    for v in range(1, 300):
        ch300[int(rng.integers(max(0, v - 40), v))].append(v)
    return [("one", [[]]), ("path3", [[1], [2], []]), ("star71", [list(range(1, 71))] + [[]] * 70), ("binary127", heap(127)),
            ("binary129", heap(129)), ("random300", ch300)]


@functools.lru_cache(maxsize=None)
def crafted_reads():
    """(reads, the four sequences, the random reads among them): the one read set of the crafted family"""
    rng = np.random.default_rng(20240)
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    seqs = [rnd(400) for _ in range(4)]
    windows = [q[i:i + 150] for q in seqs for i in range(0, 251, 25)]
    reads = list(windows) + [revcomp(w) for w in windows]
    for w in windows:
        q = bytearray(w)
        for p in rng.integers(0, 150, 2):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4]
        reads.append(bytes(q))
    reads += windows[:10] + [revcomp(w) for w in windows[3:8]]                       # copies
    reads += [w[:75 + 5 * (i % 6)] + rnd(75 - 5 * (i % 6)) for i, w in enumerate(windows[::2])]   # half-random reads
    long_read = seqs[0] + seqs[1] + seqs[2]
    reads.append(long_read)                                                            # 1,200 bases: 16 planes
    for want in (127, 128):                                                            # ... and the plane threshold itself
        lo, hi = 150, 1200
        while lo < hi:
            mid = (lo + hi) // 2
            if len(om.seedmers(long_read[:mid], K, S, L)) < want:
                lo = mid + 1
            else:
                hi = mid
        if len(om.seedmers(long_read[:lo], K, S, L)) == want:
            reads.append(long_read[:lo])
    reads.append(seqs[1][:K - 1])                                                      # shorter than k
    random_reads = [rnd(150) for _ in range(len(reads) // 9 + 1)]                      # 10 % random reads: they match nothing
    reads += random_reads
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], seqs, frozenset(random_reads)


class CraftedTree:
    def __init__(self, name, parent, oriented, plain):
        self.name, self.parent, self.oriented, self.plain = name, parent, oriented, plain

    def indexes(self, pmx):
        """(plain index, oriented index) through Index.from_arrays"""
        a, o = self.plain, self.oriented
        return (pmx.Index.from_arrays(K, S, 0, L, False, self.parent, a["offsets"], a["hash"], a["parent_count"], a["child_count"]),
                pmx.Index.from_arrays(K, S, 0, L, False, self.parent, o["offsets"], o["hash"], o["parent_count"], o["child_count"], oriented=True))


def _make_tree(name, parent, seqs, extra_hashes, rng):
    n = len(parent)
    end = np.arange(n)
    for v in range(n - 1, 0, -1):
        end[parent[v]] = max(end[parent[v]], end[v])
    active = np.array([0] + [v for v in range(1, n) if rng.random() < 0.5], np.int64)   # the others carry no change
    pick = lambda: int(active[rng.integers(len(active))])
    plan = {}                                                                            # node -> {(hash, orientation): kind}

    def toggle(v, key):
        d = plan.setdefault(v, {})
        if d.get(key) == "toggle":
            del d[key]
        else:
            d[key] = "toggle"

    seen = set()
    for j, q in enumerate(seqs):
        # one or two origins in disjoint subtrees: the sequence's seedmers are gained there
        a = pick()
        origins = [a]
        others = [int(v) for v in active if not (a <= v <= end[a]) and not (v <= a <= end[v])]
        if others and j != 1:
            origins.append(others[int(rng.integers(len(others)))])
        for h, rev in om.seedmers(q, K, S, L):
            if h in seen:
                continue
            seen.add(h)
            o = int(rev)
            if j < 3 or rng.random() < 0.5:                      # (the last sequence is held by halves only: discarded reads)
                for v in origins:
                    toggle(v, (h, o))
            if rng.random() < 0.15:
                toggle(pick(), (h, 1 - o))                       # the other orientation somewhere
            if rng.random() < 0.12:
                toggle(pick(), (h, o))                           # lost below an origin, or gained on its own elsewhere
            if rng.random() < 0.05:
                toggle(pick(), (h, o))
            if rng.random() < 0.1:
                plan.setdefault(pick(), {}).setdefault((h, o), "bump")
    for h in extra_hashes:                                       # seedmers only junctions and mutated reads have
        if h not in seen and rng.random() < 0.3:
            toggle(pick(), (h, int(rng.integers(2))))
    return tree_from_plan(name, parent, plan, rng)


def tree_from_plan(name, parent, plan, rng):
    """plan: node -> {(hash, orientation): "toggle" | "bump"}; a toggle makes an absent seedmer present with a count of 1 to 3
    and a present one absent, a bump adds one to a present one's count.  One DFS turns the plan into count changes: the
    oriented index and the plain one (counts of both orientations added)"""
    n = len(parent)
    children = [[] for _ in range(n)]
    for v in range(1, n):
        children[int(parent[v])].append(v)
    state = {}
    o_rows, p_rows = [[] for _ in range(n)], [[] for _ in range(n)]

    def visit(v):
        undo = []
        by_hash = {}
        for (h, o), kind in sorted(plan.get(v, {}).items()):
            before = state.get((h, o), 0)
            if kind == "bump" and before == 0:
                continue
            after = before + 1 if kind == "bump" else (0 if before else int(rng.integers(1, 4)))
            by_hash.setdefault(h, []).append((o, before, after))
        for h, changes in by_hash.items():
            total_before = state.get((h, 0), 0) + state.get((h, 1), 0)
            for o, before, after in changes:
                o_rows[v].append((h ^ XOR if o else h, before, after))
                undo.append(((h, o), before))
                state[(h, o)] = after
            total_after = state.get((h, 0), 0) + state.get((h, 1), 0)
            if total_before != total_after:
                p_rows[v].append((h, total_before, total_after))
        return undo

    stack = [(0, None)]
    while stack:                                                 # (iterative: the star and the random tree are deep enough either way)
        v, undo = stack.pop()
        if undo is not None:
            for key, before in reversed(undo):
                state[key] = before
            continue
        stack.append((v, visit(v)))
        for c in reversed(children[v]):
            stack.append((c, None))

    def arrays(rows):
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows])
        flat = [e for r in rows for e in sorted(r)]
        return dict(parent=parent, offsets=off, hash=np.array([e[0] for e in flat], np.uint64),
                    parent_count=np.array([e[1] for e in flat], np.int16), child_count=np.array([e[2] for e in flat], np.int16))
    return CraftedTree(name, parent, arrays(o_rows), arrays(p_rows))


@functools.lru_cache(maxsize=None)
def crafted_trees():
    reads, seqs, random_reads = crafted_reads()
    rng = np.random.default_rng(77)
    in_seqs = {h for q in seqs for h, _ in om.seedmers(q, K, S, L)}
    extra = sorted({h for r in reads if r not in random_reads for h, _ in om.seedmers(r, K, S, L)} - in_seqs)
    return [_make_tree(name, _preorder(ch), seqs, extra, rng) for name, ch in _tree_shapes(rng)]


@functools.lru_cache(maxsize=None)
def crafted_restated(tree_index, discard=0.5, dust=100.0):
    return restate(crafted_trees()[tree_index].oriented, crafted_reads()[0], discard, dust)


# ------------------------------------------------------------------------------------------------ rsv family
def _fasta(path):
    return "".join(x.strip() for x in open(path) if not x.startswith(">")).upper()


def _tile(g, n, length=150):
    step = max(1, (len(g) - length) // n)
    return [g[i:i + length].encode() for i in range(0, len(g) - length + 1, step)][:n]


@functools.lru_cache(maxsize=None)
def rsv_reads():
    rng = np.random.default_rng(1330)
    a, b = _fasta(os.path.join(GOLDEN, "MZ515733.1.fa")), _fasta(os.path.join(GOLDEN, "rsv_4K.panman.random.node_1330.fa"))
    reads = _tile(a, 360) + _tile(b, 240)
    reads = [revcomp(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    mutated = []
    for r in reads[::6]:
        q = bytearray(r)
        for p in rng.integers(0, len(q), 2):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4] if q[p] in b"ACGT" else q[p]
        mutated.append(bytes(q))
    reads = reads + mutated + reads[5:25] + [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)) for _ in range(60)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


RSV_DISCARDS = (0.0, 0.6, 1.0)
_rsv_cache = {}


def rsv_restated(arrays, discard, dust=100.0):
    """the restatement on the rsv family; `arrays`: Index.arrays() of the oriented index of rsv_4K.panman (flank mask 0)"""
    key = (discard, dust)
    if key not in _rsv_cache:
        _rsv_cache[key] = restate(arrays, rsv_reads(), discard, dust)
    return _rsv_cache[key]


# ------------------------------------------------------------------------------------------------ comparison
def flat(lists):
    """seedmer lists -> (offsets, hashes, orientations)"""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, np.array([h for x in lists for h, _ in x], np.uint64), np.array([int(v) for x in lists for _, v in x], np.uint8)


def check_against_oracle(arrays, R, nodes):
    """the restatement's presence and scores at `nodes` against oracle_meta's tree-walking ones"""
    off, h, rev = flat(R.lists)
    read_hashes = set(h.tolist())
    for node in nodes:
        counts = om.node_seed_counts(arrays, int(node), read_hashes)
        for u, key in enumerate(R.uniq.tolist()):
            c = counts.get(key, [0, 0])
            assert (c[0] > 0, c[1] > 0) == tuple(R.presence[u, node]), (node, key)
        assert np.array_equal(om.read_scores_np(counts, off, h, rev), R.scores[:, node]), node


def check_result(res, want, parent, heads, label=""):
    """a Meta.assign result against the restatement, read by read"""
    assert np.array_equal(res.merged, want.merged), label
    assert np.array_equal(res.state, want.state), (label, np.nonzero(res.state != want.state)[0][:5])
    mapped = want.merged >= 0
    assert np.array_equal(res.max[mapped], want.max[mapped]), (label, np.nonzero(res.max != want.max)[0][:5])
    for r in range(len(want.state)):
        assert np.array_equal(res.nodes_of(r), want.nodes[r]), (label, r)
        assert res.lca[r] == (heads[want.lca[r]] if want.lca[r] >= 0 else -1), (label, r)
