"""Crafted trees for the place stage's node scoring and their comparison with the oracle (tests/test_place_trees_gpu.py on the
GPU, tests/test_place_tree_families.py for the trees themselves).  A shape is a seed index built by hand -- parent array in DFS
pre-order, consistent change lists -- whose form aims at one edge of the scoring kernels: chains of every short length, flags
published in batches of eight, zero-change nodes inside chains, every tail of the unrolled add loop, more chains than waves.
The read side is a histogram handed to Placer.merge (no seeding).  The oracle's answer is computed once per (shape, histogram,
parameters) and shared by every test of a session.  Nothing here touches a GPU at import."""
import functools

import numpy as np

K, S, L = 19, 8, 3                     # index parameters of every shape (only k matters to scoring: the homopolymer hashes)
CYCLE = (0, 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300)   # changes per node, by node id
POOL = 6007                            # change hashes (a prime: start + stride * j mod POOL never repeats inside a node)
N_KEYS = 4000
N_TIE_HITS = 3
FORMS = {                              # name -> (environment switches, Placer.score_info()["form"])
    "default": ((), "chains"),
    "tree_kernel": (("PMX_PLACE_TREE_KERNEL",), "tree"),
    "level_graph": (("PMX_PLACE_LEVEL_KERNELS",), "levels_graph"),
    "level_plain": (("PMX_PLACE_LEVEL_KERNELS", "PMX_PLACE_NO_GRAPH"), "levels"),
    "starved": (("PMX_PLACE_TEST_STARVED",), "chains"),
}
PUBLISHERS = (1, 7, 8, 9, 15, 16, 17)  # publishing nodes on a spine: around one and two batches of PMX_CHAIN_FLUSH = 8
SHAPES = (["single_empty", "single_300", "path", "star", "caterpillar"] + ["spine_%d_%s" % (p, v) for p in PUBLISHERS for v in ("end", "tail")] +
          ["broom", "binary", "random"])


# ------------------------------------------------------------------------------------------------ read side
@functools.lru_cache(maxsize=None)
def histogram(name="A"):
    """(keys ascending, counts): distinct 64-bit keys, counts 1, 2, 3, ... and random ones up to 2^40 (as
    test_log1p_device_restatement_is_exact).  A and B share no count pattern; C has another size (the term buffers and the
    probe table move); `low` keeps every count under 100 (for a minReadSupport no seed reaches); `empty` has no seed.
    T is the histogram for ties: only N_TIE_HITS of its keys are change hashes at all, so a node's scores take few distinct
    values and whole families of nodes share the best one (A's scores are all distinct: its ties are one node long)."""
    if name == "empty":
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    n = {"A": N_KEYS, "B": N_KEYS, "C": 9000, "low": N_KEYS, "T": N_KEYS}[name]
    rng = np.random.default_rng({"A": 11, "B": 12, "C": 13, "low": 14, "T": 15}[name])
    keys = _keys()[:n] if n <= N_KEYS else np.concatenate([_keys(), _other_hashes(20000)[-(n - N_KEYS):]])
    if name == "B":
        keys = np.concatenate([keys[:n // 2], _other_hashes(20000)[10000:10000 + n - n // 2]])    # half of A's keys, half new ones
    if name == "T":
        keys = np.concatenate([pool()[:N_TIE_HITS], _other_hashes(30000)[20000:20000 + n - N_TIE_HITS]])
    if name == "low":
        counts = rng.integers(1, 100, n)
    else:
        counts = np.concatenate([np.arange(1, n // 2 + 1), rng.integers(1, 2 ** 40, n - n // 2)])
        counts = counts[rng.permutation(n)]
        if name == "T":
            counts[:N_TIE_HITS] = np.maximum(counts[:N_TIE_HITS], 2)      # (kept whatever minReadSupport resolves to)
    order = np.argsort(keys)
    assert len(np.unique(keys)) == n
    return keys[order].astype(np.uint64), counts[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def _all_hashes():
    v = np.unique(np.random.default_rng(7).integers(1, 2 ** 63, 40000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1))
    v = v[np.random.default_rng(8).permutation(len(v))]
    assert len(v) > N_KEYS + 30000
    return v


def _keys():
    return _all_hashes()[:N_KEYS]


def _other_hashes(n):
    return _all_hashes()[N_KEYS:N_KEYS + n]


@functools.lru_cache(maxsize=None)
def pool():
    """the hashes the change lists draw from: half are keys of histogram A, half are in no histogram's first half"""
    half = POOL // 2
    p = np.concatenate([_keys()[:half], _other_hashes(POOL - half)])
    return p[np.random.default_rng(9).permutation(POOL)]


# ------------------------------------------------------------------------------------------------ tree forms
def _preorder(parent):
    """relabel a tree given by any parent array with parent[i] < i so that ids are in DFS pre-order (children keep their order)"""
    n = len(parent)
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[parent[i]].append(i)
    new_id, out, stack = np.zeros(n, np.int64), [], [0]
    while stack:
        v = stack.pop()
        new_id[v] = len(out)
        out.append(v)
        stack.extend(reversed(kids[v]))
    par = np.zeros(n, np.uint32)
    for v in range(1, n):
        par[new_id[v]] = new_id[parent[v]]
    return par


def _spine(n_pub, tail):
    """a spine whose first n_pub nodes each carry a leaf beside the spine child (so they publish a flag), followed by `tail`
    plain nodes.  The spine child comes first among the children and the spine's last node is made heavy (see tree()), so the
    whole spine is ONE chain: with tail == 1 its last publishing node is the chain's second-to-last node"""
    ns = n_pub + tail
    parent = list(range(-1, ns - 1))
    parent[0] = 0
    for s in range(n_pub - 1, -1, -1):       # pre-order: the deepest publisher's leaf comes first
        parent.append(s)
    return np.array(parent, np.uint32), {ns - 1: 300}


@functools.lru_cache(maxsize=None)
def shape_parent(name):
    """(parent array in DFS pre-order, {node: change count} overrides of the cycle)"""
    if name == "single_empty":
        return np.zeros(1, np.uint32), {0: 0}
    if name == "single_300":
        return np.zeros(1, np.uint32), {0: 300}
    if name == "path":                                  # one chain, nothing published, 2,000 levels
        return np.maximum(np.arange(2000) - 1, 0).astype(np.uint32), {0: 1}
    if name == "star":                                  # more chains than a grid has waves; nearly every chain has one node
        return np.zeros(5001, np.uint32), {0: 1023}
    if name == "caterpillar":                           # the worst case for publishing: every spine node has a waiting leaf
        par, over = _spine(2000, 0)
        over = {0: 1024}
        return par, over
    if name.startswith("spine_"):
        _, p, v = name.split("_")
        par, over = _spine(int(p), 1 if v == "end" else 5)
        over[0] = CYCLE[(int(p) * 5) % len(CYCLE)]
        return par, over
    if name == "broom":                                 # chains of 1 .. 8 nodes: around the prefetch depth PMX_CHAIN_AHEAD + 2
        parent = [0]
        for rep in range(3):
            for ln in range(1, 9):
                parent.append(0)
                parent.extend(range(len(parent) - 1, len(parent) - 1 + ln - 1))
        return np.array(parent, np.uint32), {0: 0}
    if name == "binary":                                # 12 full levels
        n = 2 ** 12 - 1
        heap = np.maximum((np.arange(n) - 1) // 2, 0)
        return _preorder(heap), {0: 1025}
    if name == "random":
        # A random recursive tree: node i hangs under a random earlier node.  Under the uniform law half the nodes are leaves
        # (3,000 chains of 6,000 nodes); the chains must outnumber three times the waves of a 256-CU grid (3,072), so the draw
        # leans towards early nodes (parent = i * u^4), which leaves about 70 % of the nodes childless.
        rng = np.random.default_rng(5)
        n = 6000
        par = np.zeros(n, np.int64)
        par[1:] = (np.arange(1, n) * rng.random(n - 1) ** 4).astype(np.int64)
        return _preorder(par), {0: 2049}
    raise KeyError(name)


class Tree:
    def __init__(self, name, parent, offsets, hashes, pc, cc):
        self.name, self.parent, self.offsets, self.hash, self.parent_count, self.child_count = name, parent, offsets, hashes, pc, cc
        self.n_nodes, self.n_changes = len(parent), len(hashes)

    def arrays(self):
        return dict(parent=self.parent, offsets=self.offsets, hash=self.hash, parent_count=self.parent_count, child_count=self.child_count)

    def reversed_lists(self):
        """every node's change list back to front: the same tree, the additions in another order"""
        off = self.offsets.astype(np.int64)
        node = np.repeat(np.arange(self.n_nodes), np.diff(off))
        idx = off[node] + off[node + 1] - 1 - np.arange(self.n_changes, dtype=np.int64)
        return Tree(self.name + "/reversed", self.parent, self.offsets, self.hash[idx], self.parent_count[idx], self.child_count[idx])

    def index(self, pmx):
        return pmx.Index.from_arrays(K, S, 0, L, False, self.parent, self.offsets, self.hash, self.parent_count, self.child_count)


COUNT_VALUES = np.array([0, 1, 2, 3, -1, 1000, 32767])     # -1: a small count, 4 .. 40


@functools.lru_cache(maxsize=None)
def tree(name):
    """the shape's index arrays.  A node's parent_count for a hash is what the nearest ancestor that touched the hash left (0
    if none did): one depth-first walk keeps the counts of the current root path and undoes a node's changes on the way back
    up.  About 3 % of the entries have child == parent (both sides skip them); no other entry does."""
    parent, over = shape_parent(name)
    n = len(parent)
    rng = np.random.default_rng(sum(name.encode()))
    n_ch = np.array([CYCLE[i % len(CYCLE)] for i in range(n)], np.int64)
    for nd, v in over.items():
        n_ch[nd] = v
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(n_ch)
    m = int(offsets[-1])
    h_idx, pc, cc = np.zeros(m, np.int64), np.zeros(m, np.int16), np.zeros(m, np.int16)
    cur = np.zeros(POOL, np.int16)
    stack = []                               # (node, its slice of the arrays) along the current root path
    for i in range(n):
        while stack and stack[-1][0] != parent[i]:
            _, a, b = stack.pop()
            cur[h_idx[a:b]] = pc[a:b]
        assert i == 0 or stack, "ids are not in DFS pre-order"
        a, b = int(offsets[i]), int(offsets[i + 1])
        k = b - a
        if k:
            idx = (int(rng.integers(0, POOL)) + int(rng.integers(1, POOL)) * np.arange(k, dtype=np.int64)) % POOL
            was = cur[idx]
            new = COUNT_VALUES[rng.integers(0, len(COUNT_VALUES), k)]
            new = np.where(new < 0, rng.integers(4, 41, k), new).astype(np.int16)
            new = np.where(new == was, np.where(was == 5, 6, 5), new).astype(np.int16)
            new = np.where(rng.random(k) < 0.03, was, new).astype(np.int16)
            h_idx[a:b], pc[a:b], cc[a:b] = idx, was, new
            cur[idx] = new
        stack.append((i, a, b))
    return Tree(name, parent, offsets, pool()[h_idx], pc, cc)


def check_consistent(t):
    """the generator's own conditions, restated naively: parent[i] < i in DFS pre-order, counts in 0 .. 32767, no hash twice in
    a node, and parent_count == the count the nearest ancestor that touched the hash left"""
    n = t.n_nodes
    assert t.parent[0] == 0 and np.all(t.parent[1:] < np.arange(1, n))
    assert t.parent_count.min(initial=0) >= 0 and t.child_count.min(initial=0) >= 0
    assert t.parent_count.max(initial=0) <= 32767 and t.child_count.max(initial=0) <= 32767
    path, state = [], {}
    for i in range(n):
        while path and path[-1][0] != t.parent[i]:
            for h, was in reversed(path.pop()[1]):
                state[h] = was
        assert i == 0 or path, "ids are not in DFS pre-order"      # (the parent is on the current root path)
        a, b = int(t.offsets[i]), int(t.offsets[i + 1])
        hs = t.hash[a:b].tolist()
        assert len(set(hs)) == len(hs), i
        undo = []
        for h, p, c in zip(hs, t.parent_count[a:b].tolist(), t.child_count[a:b].tolist()):
            assert state.get(h, 0) == p, (i, h, p, state.get(h, 0))
            undo.append((h, p))
            state[h] = c
        path.append((i, undo))


# ------------------------------------------------------------------------------------------------ decomposition
@functools.lru_cache(maxsize=None)
def decomposition(name):
    """numpy restatement of pmx_place_create's heavy-path decomposition: weight of a node = own changes + 64, summed over its
    subtree; the heaviest child continues the chain (the first child wins a tie); chain heads in (depth, id) order.
    -> dict(chains: list of node lists, publish: bool per node (two or more children), n_levels, n_children)"""
    t = tree(name)
    n, parent = t.n_nodes, t.parent.astype(np.int64)
    sw = np.diff(t.offsets.astype(np.int64)) + 64
    depth, n_child, heavy = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for i in range(n - 1, 0, -1):
        sw[parent[i]] += sw[i]
    for i in range(1, n):
        p = parent[i]
        depth[i] = depth[p] + 1
        n_child[p] += 1
        if heavy[p] < 0 or sw[i] > sw[heavy[p]]:
            heavy[p] = i
    chains = []
    for hd in np.lexsort((np.arange(n), depth)):
        if hd != 0 and heavy[parent[hd]] == hd:
            continue
        chain, v = [], int(hd)
        while v >= 0:
            chain.append(v)
            v = int(heavy[v])
        chains.append(chain)
    assert sum(len(c) for c in chains) == n
    return dict(chains=chains, publish=n_child >= 2, n_children=n_child, n_levels=int(depth.max()) + 1,
                n_chains=len(chains), max_chain_len=max(len(c) for c in chains))


# ------------------------------------------------------------------------------------------------ the oracle's answer
def _want(t, hist, mask_fraction, min_support, force_leaf):
    from oracle import oracle
    keys, counts = histogram(hist)
    kh, kl, st = oracle.finalize_reads(keys, counts, K, mask_fraction, min_support)
    sc, met, cts, wc = oracle.score_nodes(t.parent, t.offsets, t.hash, t.parent_count, t.child_count, kh, kl, st)
    best, bidx, ties = oracle.best_ties(t.parent, sc, force_leaf)
    for a in (keys, counts, kh, kl, sc, met, cts):
        a.setflags(write=False)
    return dict(hist_hash=keys, hist_count=counts, kept_hash=kh, kept_log=kl, state=st, scores=sc, metrics=met, counts=cts, wc_den=wc,
                best=best, best_idx=bidx, ties=ties)


@functools.lru_cache(maxsize=None)
def want(name, hist="A", mask_fraction=0.0, min_support=-1, force_leaf=False):
    """what oracle.place would report for this tree and histogram (shared and read-only)"""
    return _want(tree(name), hist, mask_fraction, min_support, force_leaf)


def want_reversed(name, hist="A"):
    return _want(tree(name).reversed_lists(), hist, 0.0, -1, False)


def order_sensitive_share(name, hist="A"):
    """share of the nodes with at least one accumulator whose bits change when every change list is added back to front"""
    a, b = want(name, hist)["metrics"], want_reversed(name, hist)["metrics"]
    return float(np.mean(np.any(a.view(np.uint64) != b.view(np.uint64), axis=1)))


# ------------------------------------------------------------------------------------------------ the comparison
def assert_place_matches(placer, res, want):
    """everything a scored placer reports against the oracle's dict (oracle.place): seeds, kept seeds, the read-side scalars,
    node accumulators / scores / counts bit for bit, best score, best index and tie lists of the five metrics"""
    hh, hc = placer.histogram()
    assert np.array_equal(hh, want["hist_hash"]), "seed set differs"
    assert np.array_equal(hc, want["hist_count"]), "seed counts differ"
    kh, kl = placer.kept_seeds()
    assert np.array_equal(kh, want["kept_hash"])
    assert np.array_equal(kl.view(np.uint64), want["kept_log"].view(np.uint64)), "log1p(count) not bit-equal"
    st = want["state"]
    assert res.min_support == st.min_support and res.readUniqueSeedCount == st.n_kept
    assert res.totalReadSeedFrequency == st.total_freq and res.n_unique_seeds == st.n_unique_in
    assert np.float64(res.readMagnitude).view(np.uint64) == np.float64(st.log_magnitude).view(np.uint64)
    assert np.float64(res.logContainmentDenominator).view(np.uint64) == np.float64(st.log_cont_den).view(np.uint64)
    assert np.float64(res.weightedContainmentDenominator).view(np.uint64) == np.float64(want["wc_den"]).view(np.uint64)
    sc, met, cts = placer.node_outputs()
    assert np.array_equal(cts, want["counts"])
    assert np.array_equal(met.view(np.uint64), want["metrics"].view(np.uint64)), "node accumulators not bit-equal"
    assert np.array_equal(sc.view(np.uint64), want["scores"].view(np.uint64)), "node scores not bit-equal"
    for m in range(5):
        assert res.best_score[m] == want["best"][m] and res.best_index[m] == want["best_idx"][m]
        assert np.array_equal(res.tied_indices[m], want["ties"][m])
