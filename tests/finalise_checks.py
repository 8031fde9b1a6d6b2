"""Crafted histograms for the place stage's seed table and read-side finalise step, and the oracle's answer to each
(tests/test_place_finalise_gpu.py on the GPU, tests/test_place_finalise_families.py for the cases themselves).  A case is a
list of steps for one Placer -- merges of (keys, counts) arrays, resets, histogram() and score() calls between them -- with the
TraversalParams of the final score() and the name of a three-node index.  Four families:
  A  the seed table: duplicates inside one merge, growth by rehash, every branch of the reservation after reset(), probe runs
     that share one home slot or wrap the table's end;
  B  the read filters: homopolymer seeds, the truncation of seedMaskFraction * alive, ties at the mask cut, the automatic and
     the explicit minReadSupport;
  C  the canonical summation order at every tail of its blocks, chunks and unrolled loops;
  D  the probe table of the kept seeds and the weighted-containment denominator over the root's change list.
Everything comes from fixed seeds; counts are >= 1 and no key is the all-ones empty mark.  Nothing here touches a GPU."""
import functools

import numpy as np

import place_tree_checks as tc

K = tc.K
M64 = (1 << 64) - 1
EMPTY_KEY = M64
_C1, _C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)
SUM_BLOCK = 1024                       # PMX_SUM_BLOCK / ORC_SUM_BLOCK
TABLE_FLOOR = 1 << 16                  # table_reserve never makes a smaller table
CLUSTER_BITS = 20                      # the clusters share these low bits of mix64: one home slot at every capacity up to 2^20
HOME = 0x5A5A5                         # the home slot (mod capacity) of the one-slot clusters
MID = 100                              # misses are homed this far inside a cluster
LAST4 = tuple(range((1 << CLUSTER_BITS) - 4, 1 << CLUSTER_BITS))   # homes of the clusters that wrap the table's end


# ------------------------------------------------------------------------------------------------ mixing
def mix64(x):
    """device/pmx_math.h mix64 in Python integers"""
    x ^= x >> 33
    x = x * _C1 & M64
    x ^= x >> 33
    x = x * _C2 & M64
    return x ^ x >> 33


def unmix64(v):
    """the inverse: an xor-shift by 33 is its own inverse, the multipliers are odd"""
    v ^= v >> 33
    v = v * _I2 & M64
    v ^= v >> 33
    v = v * _I1 & M64
    return v ^ v >> 33


def mix64_array(a):
    x = np.asarray(a, np.uint64).copy()
    s = np.uint64(33)
    x ^= x >> s
    x *= np.uint64(_C1)
    x ^= x >> s
    x *= np.uint64(_C2)
    x ^= x >> s
    return x


def keys_homed(low_values, n, seed):
    """n distinct keys whose mix64 value has its low CLUSTER_BITS bits in low_values (cycled): home = low & (cap - 1)"""
    rng = np.random.default_rng(seed)
    high = np.unique(rng.integers(1, 1 << (64 - CLUSTER_BITS - 1), 2 * n + 8))
    high = high[rng.permutation(len(high))][:n]
    assert len(high) == n
    low = [low_values[i % len(low_values)] for i in range(n)]
    out = np.array([unmix64(int(h) << CLUSTER_BITS | lo) for h, lo in zip(high, low)], np.uint64)
    assert len(np.unique(out)) == n and EMPTY_KEY not in out
    return out


@functools.lru_cache(maxsize=None)
def homopolymer_hashes(k=K):
    from oracle import oracle
    return tuple(min(oracle.hash_seq(b * k)) for b in (b"A", b"C", b"G", b"T"))


def homopolymer_keys(k=K):
    """the distinct ones: a run of A is the reverse complement of a run of T, so the four canonical hashes are two values"""
    return np.array(sorted(set(homopolymer_hashes(k))), np.uint64)


# ------------------------------------------------------------------------------------------------ generators
@functools.lru_cache(maxsize=None)
def pool():
    """distinct random keys; every B, C and D histogram takes a prefix, so the indexes below hit all of them"""
    v = np.unique(np.random.default_rng(21).integers(1, 2 ** 63, 300000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1))
    v = v[np.random.default_rng(22).permutation(len(v))]
    assert len(v) > 290000 and EMPTY_KEY not in v
    v.setflags(write=False)
    return v


def other_keys(n, start=0):
    """keys of no B, C or D histogram (the pool's far end)"""
    return pool()[200000 + start:200000 + start + n]


def spread_counts(n, seed):
    """counts from 1 to just under 2^40, evenly over the magnitudes: sums of their log1p depend on the order"""
    c = np.floor(2.0 ** np.random.default_rng(seed).uniform(0.0, 40.0, n)).astype(np.int64)
    return np.maximum(c, 1)


def hist_sorted(keys, counts):
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.int64)
    o = np.argsort(keys)
    assert len(np.unique(keys)) == len(keys) and counts.min(initial=1) >= 1 and EMPTY_KEY not in keys
    return keys[o], counts[o]


def unique_sum(merges):
    """what the table must hold after these merges: np.unique of the keys with the counts summed"""
    if not merges:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    keys = np.concatenate([m[0] for m in merges])
    counts = np.concatenate([m[1] for m in merges])
    u, inv = np.unique(keys, return_inverse=True)
    s = np.zeros(len(u), np.int64)
    np.add.at(s, inv, counts)
    return u, s


def final_histogram(steps):
    merges = []
    for st in steps:
        if st[0] == "reset":
            merges = []
        elif st[0] == "merge":
            merges.append(st[1:])
    return unique_sum(merges)


# ------------------------------------------------------------------------------------------------ table model
def next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def table_model(steps):
    """table_reserve's sizing arithmetic restated: [(branch, capacity after)] for every merge step.  Branches:
    first_allocation; after a reset grow_after_reset / shrink / clear_and_keep; otherwise fits / first_rehash (the spare
    buffer pair is made) / rehash_into_spares (it is reused)"""
    cap, spare, needs_clear, present, out = 0, False, False, np.zeros(0, np.uint64), []
    for st in steps:
        if st[0] == "reset":
            needs_clear, present = cap != 0, np.zeros(0, np.uint64)
        if st[0] != "merge" or len(st[1]) == 0:
            continue
        n = len(st[1])
        if needs_clear or cap == 0:
            need = max(next_pow2(int(n / 0.7) + 1024), TABLE_FLOOR)
            needs_clear = False
            branch = "first_allocation" if cap == 0 else "grow_after_reset" if cap < need else "shrink" if cap > 4 * need else "clear_and_keep"
            if branch != "clear_and_keep":
                cap = need
        else:
            need = max(next_pow2(int((len(present) + n) / 0.7) + 1024), TABLE_FLOOR)
            if cap >= need:
                branch = "fits"
            else:
                branch, spare, cap = "rehash_into_spares" if spare else "first_rehash", True, need
        present = np.union1d(present, st[1])
        out.append((branch, cap))
    return out


def probe_table_cap(n_kept):
    """sums_and_probe_table's sizing of the kept seeds' table"""
    return next_pow2(2 * max(n_kept, 1) + 64)


def fill_table(keys, cap):
    """linear probing from mix64(key) & (cap - 1): the occupied slots (whatever the order of the inserts) -> bool array"""
    occ = np.zeros(cap, bool)
    for h in (mix64_array(keys) & np.uint64(cap - 1)).tolist():
        while occ[h]:
            h = (h + 1) & (cap - 1)
        occ[h] = True
    return occ


def run_through(occ, slot):
    """(first slot, length, wraps) of the run of occupied slots through `slot`; no probe inside it walks further"""
    cap = len(occ)
    assert occ[slot] and not occ.all()
    a = slot
    while occ[(a - 1) % cap]:
        a = (a - 1) % cap
    n = 0
    while occ[(a + n) % cap]:
        n += 1
    return a, n, a + n > cap


def probes_of_miss(occ, key):
    """occupied slots a lookup of an absent key walks before it meets the empty one"""
    cap = len(occ)
    h, n = mix64(int(key)) & (cap - 1), 0
    while occ[h]:
        h, n = (h + 1) & (cap - 1), n + 1
    return n


# ------------------------------------------------------------------------------------------------ small indexes
def small_tree(name, root_hashes, root_cc=None, seed=0):
    """three nodes (0 <- 1 <- 2): the root's change list is root_hashes in this order with child_count root_cc (0 allowed:
    such an entry changes nothing); node 1 changes the first half of them again and adds five hashes of no histogram; node 2
    changes every third.  Satisfies place_tree_checks.check_consistent."""
    rng = np.random.default_rng(1000 + seed)
    h0 = np.asarray(root_hashes, np.uint64)
    m = len(h0)
    assert len(np.unique(h0)) == m
    c0 = np.asarray(root_cc, np.int16) if root_cc is not None else rng.integers(1, 41, m).astype(np.int16)
    na = (m + 1) // 2
    c1 = np.where(rng.random(na) < 0.2, 0, rng.integers(1, 1000, na)).astype(np.int16)
    c1 = np.where(c1 == c0[:na], c1 + 1, c1).astype(np.int16)
    fresh = other_keys(5, 60000 + 5 * seed)
    assert not np.isin(fresh, h0).any()
    state = c0.copy()
    state[:na] = c1
    third = np.arange(0, m, 3)
    p2 = state[third]
    c2 = np.where(p2 < 32767, p2 + 1, 5).astype(np.int16)
    hashes = np.concatenate([h0, h0[:na], fresh, h0[third]])
    pc = np.concatenate([np.zeros(m, np.int16), c0[:na], np.zeros(5, np.int16), p2]).astype(np.int16)
    cc = np.concatenate([c0, c1, np.array([3, 1, 40, 2, 32767], np.int16), c2]).astype(np.int16)
    offsets = np.array([0, m, m + na + 5, m + na + 5 + len(third)], np.uint64)
    return tc.Tree(name, np.array([0, 0, 1], np.uint32), offsets, hashes, pc, cc)


def small_index(pmx, root_hashes, root_cc=None, seed=0):
    return small_tree("small", root_hashes, root_cc, seed).index(pmx)


ROOT_LENGTHS = (1, 7, 8, 9, 1023, 1024, 1025, 2049)      # around k_wc_denominator's 8-way add and its 1,024-wide tile
N_ROOT_HIST = 3000                                         # seeds of the histogram the root-list cases score
SIZE_BOUNDARY = (1, 480, 481)                              # 2 * n_kept + 64 reaches 1,024 at 480: 481 doubles the probe table
N_CLUSTER_D = 200


@functools.lru_cache(maxsize=None)
def cluster_keys(n, which, seed):
    return keys_homed((HOME,) if which == "home" else LAST4, n, seed)


def _mixed(parts, seed):
    v = np.concatenate(parts)
    return v[np.random.default_rng(seed).permutation(len(v))]


@functools.lru_cache(maxsize=None)
def tree(name):
    """the indexes of the cases, by name"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "default":                   # 20 of the pool's first keys (every histogram has some of them) and 20 misses
        return small_tree(name, _mixed([pool()[:20], other_keys(20)], 1))
    if name == "sizes":                     # 150 keys of the 480 / 481-seed histograms, the single seed among them, 150 misses
        return small_tree(name, _mixed([pool()[0:300:2], other_keys(150)], 2), seed=2)
    if name == "clusters":
        # hits inside both clusters and outside them; misses homed on the one-slot cluster's home, MID slots inside it, on
        # the table's last slot (the wrapping cluster starts there at the latest) and anywhere
        hits = [cluster_keys(N_CLUSTER_D, "home", 41)[::4], cluster_keys(N_CLUSTER_D, "end", 42)[::4], pool()[:100]]
        miss = [keys_homed((HOME,), 30, 43), keys_homed((HOME + MID,), 30, 44), keys_homed((LAST4[-1],), 30, 45), other_keys(110)]
        return small_tree(name, _mixed(hits + miss, 3), seed=3)
    if name.startswith("root_"):            # about half the list kept, about a tenth of the entries with child_count 0
        m = int(name.split("_")[1])
        n_hit = (m + 1) // 2
        hit = pool()[:N_ROOT_HIST][rng.permutation(N_ROOT_HIST)[:n_hit]]
        cc = np.where(rng.random(m) < 0.1, 0, rng.integers(1, 41, m))
        if m == 1:
            cc[:] = 3
        return small_tree(name, _mixed([hit, other_keys(m - n_hit, 1000)], 4 + m), cc, seed=4 + m)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    def __init__(self, name, steps, tree="default", expect=None, **params):
        self.name, self.family, self.steps, self.tree, self.params, self.expect = name, name[0], steps, tree, params, expect or {}

    def traversal_params(self, pmx):
        return pmx.TraversalParams(**self.params)

    def merges(self):
        return [st for st in self.steps if st[0] == "merge"]


def _merge(keys, counts):
    keys, counts = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(counts, np.int64)
    assert len(keys) == len(counts) and counts.min(initial=1) >= 1 and EMPTY_KEY not in keys
    keys.setflags(write=False)
    counts.setflags(write=False)
    return ("merge", keys, counts)


def _one(keys, counts):
    return [_merge(*hist_sorted(keys, counts))]


def _with_homopolymers(keys, counts, hp_counts):
    hp = homopolymer_keys()
    return np.concatenate([keys, hp]), np.concatenate([counts, np.asarray(hp_counts, np.int64)[:len(hp)]])


# ---- A: the seed table
GROWTH_WANT = ["first_allocation", "first_rehash", "rehash_into_spares", "fits", "rehash_into_spares"]
GROWTH_CAPS = [1 << 16, 1 << 17, 1 << 18, 1 << 18, 1 << 19]
N_CLUSTER_A, N_RANDOM_A = 600, 30000


def _growth_merges():
    """40,000 + 40,000 new keys, two merges of 60,000 that half-overlap what is there, and 45,000 keys that are all there
    already: the reservation counts a merge's length, so the last one grows the table without a new key"""
    p = pool()[:140000]
    rng = np.random.default_rng(31)
    parts = [p[:40000], p[40000:80000], _mixed([p[50000:80000], p[80000:110000]], 32), _mixed([p[80000:110000], p[110000:140000]], 33),
             p[rng.permutation(140000)[:45000]]]
    return [_merge(k, spread_counts(len(k), 34 + i)) for i, k in enumerate(parts)]


def _cases_a():
    out = {}
    # 1. duplicates in one call
    keys = pool()[:20000]
    rng = np.random.default_rng(51)
    hs = np.repeat(keys, rng.integers(1, 6, len(keys)))
    cn = spread_counts(len(hs), 52)
    cn[rng.permutation(len(hs))[:200]] = 2 ** 40
    o = rng.permutation(len(hs))
    out["A_duplicates"] = Case("A_duplicates", [_merge(hs[o], cn[o]), ("histogram",)])
    # 2. growth on one placer; the table is finalised (histogram(), once score()) and merged into again
    g = _growth_merges()
    out["A_growth"] = Case("A_growth", [g[0], ("histogram",), g[1], ("histogram",), ("score",), g[2], ("histogram",), g[3], ("histogram",), g[4],
                                        ("histogram",)])
    # 3. the reservation after reset() at the high-water capacity of 2^19: 80,000 keys want 2^17, a quarter, and the table is
    # cleared whole and kept; 100 keys want the floor and it shrinks; 30,000 keep the floor; 120,000 grow it again
    p = pool()
    again = [_mixed([p[130000:140000], p[150000:220000]], 61), p[139950:140050], _mixed([p[:15000], p[230000:245000]], 62), p[100000:220000]]
    steps = list(g)
    for i, k in enumerate(again):
        steps += [("histogram",), ("reset",), _merge(k, spread_counts(len(k), 63 + i))]
    out["A_after_reset"] = Case("A_after_reset", steps + [("histogram",)])
    # 4. clusters: every key three times, so that the reservation (which counts a merge's length) makes 2^17 slots -- at the
    # floor of 2^16 the 30,000 random keys would stretch a 600-key cluster's run past 1,000 slots
    halves = []
    for half in range(2):
        k = np.concatenate([cluster_keys(N_CLUSTER_A, "home", 71)[half::2], cluster_keys(N_CLUSTER_A, "end", 72)[half::2],
                            pool()[half * 15000:(half + 1) * 15000]])
        k = _mixed([k, k, k], 73 + half)
        halves.append(_merge(k, spread_counts(len(k), 75 + half)))
    out["A_clusters"] = Case("A_clusters", [halves[0], ("histogram",), halves[1], ("histogram",)])
    return out


# ---- B: the read filters
MASK_CUTS = (          # (alive, fraction, n_mask, a round-to-nearest would differ)
    (100, 0.29, 28, True), (100, 0.07, 7, False), (300, 0.01, 3, False), (9, 0.1, 0, True), (10, 0.999, 9, True), (10, 1.0, 10, False),
    (10, 1.5, 10, False))
TIE_RUNS = ((2, 100, 0.05, 5, 4), (50, 200, 0.15, 30, 10))      # (run, alive, fraction, n_mask, distinct larger counts above the run)
AUTO_SUPPORT = (       # name, counts, estimate, support, n_kept
    ("all3", [3] * 10, 3.0, 1, 10), ("alt24", [2, 4] * 5, 3.0, 1, 10), ("nine3_one4", [3] * 9 + [4], 3.1, 2, 10),
    ("all1", [1] * 10, 0.0, 1, 10), ("nine1_one4", [1] * 9 + [4], 4.0, 2, 1))


def _cases_b():
    out = {}
    hp = homopolymer_keys()
    assert not np.isin(hp, pool()).any()

    def add(name, steps, expect=None, **params):
        out[name] = Case(name, steps, "default", expect, **params)
    # homopolymer seeds with the largest counts of the histogram
    rng = np.random.default_rng(81)
    keys, counts = _with_homopolymers(pool()[:300], rng.integers(1, 50, 300), [2 ** 40, 10 ** 6, 10 ** 7, 10 ** 6 + 1])
    for frac in (0.0, 0.01, 1.0, 1.5):
        add("B_homopolymer_mask_%g" % frac, _one(keys, counts), dict(alive=300, n_mask=min(int(frac * 300), 300)), seedMaskFraction=frac)
    for frac in (0.0, 1.0):
        add("B_homopolymer_only_mask_%g" % frac, _one(hp, [2 ** 40, 5, 1, 3][:len(hp)]), dict(alive=0, n_mask=0), seedMaskFraction=frac)
    # the mask cut: all counts distinct, so exactly the n_mask largest die; the homopolymer seeds are there and not alive
    for alive, frac, n_mask, differs in MASK_CUTS:
        counts = np.random.default_rng(82).permutation(alive) + 5
        keys, counts = _with_homopolymers(pool()[:alive], counts, [2 ** 30] * 4)
        add("B_mask_%d_%g" % (alive, frac), _one(keys, counts), dict(alive=alive, fraction=frac, n_mask=n_mask, round_differs=differs),
            seedMaskFraction=frac, minReadSupport=1)
    counts = np.random.default_rng(83).choice([5, 3, 2], 70000, p=[0.004, 0.5, 0.496])
    add("B_mask_70000_ties", _one(pool()[:70000], counts), dict(alive=70000, fraction=0.01, n_mask=700, round_differs=False, all_ties=True),
        seedMaskFraction=0.01, minReadSupport=1)
    # ties at the cut: `above` distinct larger counts, then a run of equal ones that the cut divides, smaller ones below
    for run, alive, frac, n_mask, above in TIE_RUNS:
        counts = np.concatenate([1000 + np.arange(above), np.full(run, 500), np.random.default_rng(84).integers(1, 400, alive - above - run)])
        counts = counts[np.random.default_rng(85).permutation(alive)]
        add("B_tie_run_%d" % run, _one(pool()[:alive], counts), dict(alive=alive, fraction=frac, n_mask=n_mask, round_differs=False, tie_run=run),
            seedMaskFraction=frac, minReadSupport=1)
    # automatic support
    for name, counts, est, support, n_kept in AUTO_SUPPORT:
        add("B_auto_" + name, _one(pool()[:len(counts)], counts), dict(estimate=est, support=support, n_kept=n_kept))
    add("B_auto_2pow40", _one(pool()[:1000], 2 ** 40 + np.arange(1000)), dict(support=2, n_kept=1000))
    counts = np.concatenate([np.full(10, 100), np.tile([2, 4], 495)])[np.random.default_rng(86).permutation(1000)]
    add("B_auto_flip_unmasked", _one(pool()[:1000], counts), dict(estimate=3.97, support=2, n_kept=1000))
    add("B_auto_flip_masked", _one(pool()[:1000], counts), dict(estimate=3.0, support=1, n_kept=990), seedMaskFraction=0.01)
    # explicit support: counts at the threshold, one below it and above
    counts = np.tile(np.arange(1, 8), 10)
    for s in (1, 2, 5):
        add("B_support_%d" % s, _one(pool()[:70], counts), dict(support=s, n_kept=int((counts >= s).sum())), minReadSupport=s)
    return out


# ---- C: canonical sums
# (tails of 4, 5 and 6 values after the 8-way add need sizes of their own; so do 7, 8 and 9 blocks -- k_sequential_sums'
# unrolled add alone, with and without its tail: 7 * 1024 - 5, 8 * 1024 and 8 * 1024 + 1)
SUM_SIZES = (1, 2, 4, 5, 6, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 7 * 1024 - 5, 8 * 1024, 8 * 1024 + 1, 63 * 1024,
             64 * 1024, 64 * 1024 + 1, 65 * 1024 + 9, 128 * 1024 + 1)
SUM_SEEDS = {8: 22, 9: 10, 63: 1, 64: 1, 65: 1, 127: 2, 128: 1, 129: 3}   # size -> seed of its counts, where seed 0 gives a sum that the reverse order reproduces


def _cases_c():
    return {"C_sum_%d" % n: Case("C_sum_%d" % n, _one(pool()[:n], spread_counts(n, [SUM_SEEDS.get(n, 0), n])), minReadSupport=1)
            for n in SUM_SIZES}


# ---- D: probe table and weighted-containment denominator
def _cases_d():
    out = {}
    for n in SIZE_BOUNDARY:
        out["D_size_%d" % n] = Case("D_size_%d" % n, _one(pool()[:n], spread_counts(n, 91) + 1), "sizes", dict(n_kept=n), minReadSupport=1)
    keys = np.concatenate([cluster_keys(N_CLUSTER_D, "home", 41), cluster_keys(N_CLUSTER_D, "end", 42), pool()[:2600]])
    out["D_clusters"] = Case("D_clusters", _one(keys, spread_counts(len(keys), 92)), "clusters", dict(n_kept=len(keys)), minReadSupport=1)
    for m in ROOT_LENGTHS:
        out["D_root_%d" % m] = Case("D_root_%d" % m, _one(pool()[:N_ROOT_HIST], spread_counts(N_ROOT_HIST, 93)), "root_%d" % m,
                                    dict(n_kept=N_ROOT_HIST), minReadSupport=1)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for fam in (_cases_a, _cases_b, _cases_c, _cases_d):
        out.update(fam())
    out["empty"] = Case("empty", [])
    assert list(out) == [n for f in "ABCD" for n in names(f)] + ["empty"]
    return out


def names(family):
    """the case names of a family, from the tables alone (collecting the tests builds no case and needs no oracle)"""
    return {"A": ["A_duplicates", "A_growth", "A_after_reset", "A_clusters"],
            "B": (["B_homopolymer_mask_%g" % f for f in (0.0, 0.01, 1.0, 1.5)] + ["B_homopolymer_only_mask_%g" % f for f in (0.0, 1.0)] +
                  ["B_mask_%d_%g" % (a, f) for a, f, _, _ in MASK_CUTS] + ["B_mask_70000_ties"] + ["B_tie_run_%d" % t[0] for t in TIE_RUNS] +
                  ["B_auto_" + t[0] for t in AUTO_SUPPORT] + ["B_auto_2pow40", "B_auto_flip_unmasked", "B_auto_flip_masked"] +
                  ["B_support_%d" % s for s in (1, 2, 5)]),
            "C": ["C_sum_%d" % n for n in SUM_SIZES],
            "D": ["D_size_%d" % n for n in SIZE_BOUNDARY] + ["D_clusters"] + ["D_root_%d" % m for m in ROOT_LENGTHS]}[family]


# ------------------------------------------------------------------------------------------------ the oracle's answer
@functools.lru_cache(maxsize=None)
def want(name, tree_name=None):
    """what the oracle reports for the case's final histogram, its parameters and its index (or another one); read-only"""
    from oracle import oracle
    c = cases()[name]
    t = tree(tree_name or c.tree)
    keys, counts = final_histogram(c.steps)
    kh, kl, st = oracle.finalize_reads(keys, counts, K, c.params.get("seedMaskFraction", 0.0), c.params.get("minReadSupport", -1))
    sc, met, cts, wc = oracle.score_nodes(t.parent, t.offsets, t.hash, t.parent_count, t.child_count, kh, kl, st)
    best, bidx, ties = oracle.best_ties(t.parent, sc, False)
    for a in (keys, counts, kh, kl, sc, met, cts):
        a.setflags(write=False)
    return dict(hist_hash=keys, hist_count=counts, kept_hash=kh, kept_log=kl, state=st, scores=sc, metrics=met, counts=cts, wc_den=wc,
                best=best, best_idx=bidx, ties=ties)


def mask_model(keys, counts, fraction, descending_ties=False):
    """the seeds that survive the homopolymer erase and the top-fraction mask, restated: count descending, equal counts by
    ascending hash (the canonical rule) or by descending hash -> (surviving keys ascending, alive before the mask, n_mask)"""
    live = ~np.isin(keys, homopolymer_keys())
    k, c = keys[live], counts[live]
    alive = len(k)
    n_mask = min(int(fraction * alive), alive)
    order = sorted(range(alive), key=lambda i: (-int(c[i]), -int(k[i]) if descending_ties else int(k[i])))
    gone = np.zeros(alive, bool)
    gone[order[:n_mask]] = True
    return k[~gone], alive, n_mask


def plain_sums(kept_log):
    """(readMagnitude, logContainmentDenominator) summed front to back and back to front, one addition after the other"""
    out = []
    for v in (kept_log, kept_log[::-1]):
        out.append((float(np.sqrt(np.cumsum(v * v)[-1])), float(np.cumsum(v)[-1])))
    return out
