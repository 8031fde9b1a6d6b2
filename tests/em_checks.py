"""--meta scoring and EM on crafted inputs: the inputs, the choice of a case and the EM restatement that
tests/test_meta_em_families.py (on the restatement alone) and tests/test_meta_em_crafted_gpu.py (against the device) share.
No product code in here: seedmers come from oracle_meta.seedmers, the node side from index arrays alone, the all-node
score matrix from assign_checks.restate.

  * wide family: one tree of 16,000 nodes in DFS pre-order (every node's parent among the 40 nodes before it, so subtrees
    are bit ranges of many lengths).  The root holds every seedmer of the read set in the reads' orientation; every other
    node loses or regains one to four of them, or gains one in the other orientation.  At least 10,300 of its score columns
    are pairwise different over all merged reads -- and 10,241 over the 300 reads of the EM cases beyond 10,240 columns,
    which is what asks for 16,000 nodes rather than 12,000.
  * read sets: the windows of assign_checks.crafted_reads(), step-1 windows of further random sequences (those that give
    a new seedmer list), copies, reverse complements, short random reads that match nothing, the 1,200-base read and its
    prefixes with 127 and 128 seedmers.  The "short" set is the same without the reads of 128 or more seedmers.
  * a Sample is a sub-list of a restated read set with its merged reads in the device's order;
    pick_case chooses candidates with exactly n_cols distinct columns and a sample that keeps exactly n_rows rows.
  * em_restated restates oracle_meta.square_em with the parameters of _lib.MetaParams, in float64 or longdouble, and
    returns every iteration's proportions, log-likelihoods and choice."""
import functools

import numpy as np

import assign_checks as ac
from oracle import oracle_meta as om

K, S, L = ac.K, ac.S, ac.L
XOR = om.ORIENT_XOR
HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 2e-19)
LONGDOUBLE_REASON = "np.longdouble is no wider than float64 here: no higher-precision reference for the EM"
EM_MAX_SEEDMERS = 64          # reads in the EM cases: err^n stays far above the smallest float64


# ------------------------------------------------------------------------------------------------ read sets
def _seedmers(r):
    return tuple(om.seedmers(r, K, S, L))


@functools.lru_cache(maxsize=None)
def wide_reads():
    """(long read set, short read set, the random reads): the short set is the long one without reads of >= 128 seedmers"""
    rng = np.random.default_rng(4242)
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    base, _, base_random = ac.crafted_reads()
    reads = [r for r in base if r not in base_random]            # windows, copies, reverse complements, the long reads
    seen = {_seedmers(r) for r in reads}
    while len(seen) < 2350:                                      # step-1 windows: those that give a new seedmer list
        q = rnd(1000)
        for i in range(len(q) - 149):
            w = q[i:i + 150]
            x = _seedmers(w)
            if x and x not in seen:
                seen.add(x)
                reads.append(ac.revcomp(w) if i % 7 == 3 else w)
    reads += [reads[i] for i in rng.integers(0, len(reads), 300)]                     # copies: multiplicities of 2 or more
    random_reads = [rnd(int(rng.integers(30, 46))) for _ in range(len(reads) // 9 + 1)]   # 10 %, short: few hashes of their own
    reads += random_reads
    reads = [reads[i] for i in rng.permutation(len(reads))]
    short = [r for r in reads if len(_seedmers(r)) < 128]
    return reads, short, frozenset(random_reads)


# ------------------------------------------------------------------------------------------------ the wide tree
def wide_tree(n_nodes, seed):
    rng = np.random.default_rng(seed)
    reads, _, random_reads = wide_reads()
    entries = sorted({(h, int(rev)) for r in reads if r not in random_reads for h, rev in _seedmers(r)})
    children = [[] for _ in range(n_nodes)]
    for v in range(1, n_nodes):
        children[int(rng.integers(max(0, v - 40), v))].append(v)
    parent = ac._preorder(children)
    plan = {0: {e: "toggle" for e in entries}}                   # the root: every read scores its full n there
    for v in range(1, n_nodes):
        d = plan.setdefault(v, {})
        for _ in range(int(rng.integers(1, 5))):
            h, o = entries[int(rng.integers(len(entries)))]
            x = rng.random()
            if x < 0.06:
                d.setdefault((h, o), "bump")
                continue
            key = (h, 1 - o) if x < 0.26 else (h, o)             # the other orientation, or lost / regained
            if d.get(key) == "toggle":
                del d[key]
            else:
                d[key] = "toggle"
    return ac.tree_from_plan("wide%d" % n_nodes, parent, plan, rng)


def column_classes(sc):
    """(first, cls): cls[c] numbers the columns of `sc` [rows][columns] so that equal columns share a number, first[k] is the
    first column of class k"""
    t = np.ascontiguousarray(np.asarray(sc).T.astype(np.int16))
    if t.shape[1] == 0:
        return np.zeros(min(1, t.shape[0]), np.int64), np.zeros(t.shape[0], np.int64)
    v = t.view(np.dtype((np.void, t.shape[1] * 2))).ravel()
    _, first, cls = np.unique(v, return_index=True, return_inverse=True)
    return first, cls.ravel()


def distinct_columns(sc):
    """the columns of `sc` that differ from every earlier one, ascending: what the device's digests keep"""
    return np.sort(column_classes(sc)[0])


WIDE_DISTINCT = 10300


@functools.lru_cache(maxsize=None)
def wide_family():
    """(tree, restatement over the long read set): nodes are added until WIDE_DISTINCT score columns differ"""
    n_nodes = 16000                                              # (12,000 give the columns over all reads, not over 300 of them)
    while True:
        tree = wide_tree(n_nodes, 99)
        R = ac.restate(tree.oriented, wide_reads()[0], 2.0)      # (--discard 2: no read assigned, no LCA walks; scores only)
        R.scores = R.scores.astype(np.int16)
        if len(distinct_columns(R.scores)) >= WIDE_DISTINCT:
            return tree, R
        n_nodes += 2000


# ------------------------------------------------------------------------------------------------ samples and cases
class Sample:
    """a sub-list of a restated read set: `reads` for set_reads, `rows` its merged reads as rows of R.scores in the device's
    order, `n` their seedmer counts, `mult` their multiplicities, `lists` their seedmer lists"""

    def __init__(self, R, all_reads, chosen):
        self.reads = [all_reads[i] for i in chosen]
        m = R.merged[np.asarray(chosen, np.int64)]
        self.rows, self.mult = np.unique(m[m >= 0], return_counts=True)
        self.lists = [R.lists[i] for i in self.rows]
        self.n = np.array([len(x) for x in self.lists], np.int64)

    def scores(self, R, cands):
        return R.scores[np.ix_(self.rows, np.asarray(cands, np.int64))]


def sample_of(R, all_reads, sub_reads):
    """the Sample of the reads of `all_reads` that are in `sub_reads` (a subset, copies included)"""
    sub = set(sub_reads)
    return Sample(R, all_reads, [i for i, r in enumerate(all_reads) if r in sub])


# the read sets of the scoring tests by the seedmers of their longest read: 16 planes, 16 planes at the threshold itself
# (a 128-seedmer read counted on 7 planes would wrap to 0), 7 planes with the counter full
READ_CAPS = {"planes16": None, "planes16_at_128": 128, "planes7": 127}


def capped_sample(R, all_reads, cap):
    """the Sample of the reads with at most `cap` seedmers (None: all of them); reads without a merged read stay in"""
    return Sample(R, all_reads, [i for i, m in enumerate(R.merged) if cap is None or m < 0 or len(R.lists[m]) <= cap])


def kept_rows(sc, n, discard):
    return om.discard_rows(sc.max(axis=1) if sc.shape[1] else np.zeros(len(sc), np.int64), n, discard)


def pick_case(R, all_reads, n_cols, n_rows, discard=0.0, dups=0, pool=None, seed=0):
    """(candidates, Sample): the candidates (ascending) have exactly n_cols distinct score columns over the sample's merged
    reads plus `dups` columns equal to an earlier one; of the sample's merged reads exactly n_rows are kept by
    oracle_meta.discard_rows.  Reads of more than EM_MAX_SEEDMERS seedmers stay out; the other merged reads that the
    candidates do not keep (discarded ones, random ones) all stay in: they tell columns apart and carry no weight.
    Everything is judged on the restatement R.  Raises if the family cannot give the case."""
    rng = np.random.default_rng([seed, n_cols, n_rows])
    n_nodes = R.scores.shape[1]
    pool = np.arange(n_nodes) if pool is None else np.asarray(pool, np.int64)
    n_all = np.array([len(x) for x in R.lists], np.int64)
    usable = n_all <= EM_MAX_SEEDMERS
    raw_of = [[] for _ in R.lists]
    for i, m in enumerate(R.merged):
        if m >= 0:
            raw_of[m].append(i)
    copies = np.array([len(x) > 1 for x in raw_of])
    cands = np.sort(rng.choice(pool, n_cols, replace=False))
    for _ in range(40):
        keep = kept_rows(R.scores[:, cands], n_all, discard) & usable
        kept = np.nonzero(keep)[0]
        if len(kept) < n_rows or not copies[kept].any():
            raise AssertionError("%d reads kept, %d wanted" % (len(kept), n_rows))
        rows_kept = kept[np.unique(np.linspace(0, len(kept) - 1, n_rows).astype(np.int64))]
        assert len(rows_kept) == n_rows
        if not copies[rows_kept].any():                          # a multiplicity above 1 in every case
            rows_kept = np.sort(np.concatenate([rows_kept[1:], kept[copies[kept]][:1]]))
        rows = np.sort(np.concatenate([rows_kept, np.nonzero(~keep & usable)[0]]))
        first, cls = column_classes(R.scores[np.ix_(rows, pool)])
        if len(first) < n_cols:
            raise AssertionError("%d distinct columns over these rows, %d wanted" % (len(first), n_cols))
        mine = np.unique(cls[np.searchsorted(pool, cands)])
        if len(mine) == n_cols:
            break
        others = np.setdiff1d(np.arange(len(first)), mine)
        cands = np.sort(pool[first[np.concatenate([mine, rng.choice(others, n_cols - len(mine), replace=False)])]])
    else:
        raise AssertionError("no %d distinct columns with %d kept rows" % (n_cols, n_rows))
    if dups:
        sub = R.scores[np.ix_(rows, np.arange(n_nodes))]
        have = {sub[:, c].tobytes() for c in cands}
        extra = [int(v) for v in range(n_nodes) if v not in set(cands.tolist()) and sub[:, v].tobytes() in have][:dups]
        if len(extra) != dups:
            raise AssertionError("no %d duplicate columns" % dups)
        cands = np.sort(np.concatenate([cands, extra]))
    chosen = []
    for m in rows:
        chosen += raw_of[m]
    sample = Sample(R, all_reads, sorted(chosen))
    assert np.array_equal(sample.rows, rows)
    sc = sample.scores(R, cands)
    assert int(kept_rows(sc, sample.n, discard).sum()) == n_rows and len(distinct_columns(sc)) == n_cols
    return cands.astype(np.uint32), sample


# the fixed-iteration cases of the EM: (distinct columns, kept rows, --discard)
COLUMN_CASES = [(c, 300, 0.0) for c in (1, 2, 63, 64, 65, 192, 193, 256, 257, 449, 513)]
ROW_CASES = [(65, 1, 0.9)] + [(65, r, 0.0) for r in (255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)]
LDS_CASES = [(c, 300, 0.0) for c in (4096, 4097, 10239, 10240, 10241)]
FIXED_CASES = COLUMN_CASES + ROW_CASES + LDS_CASES
FIXED_ITERATIONS = (1, 3, 17)
# One column, two columns and one read are at their fixed point after an iteration or two: with the default convergence
# threshold such a run stops by itself before 17 iterations, whatever the sample.  Every other case reaches the cap.
STOP_EARLY = {(1, 300, 0.0), (2, 300, 0.0), (65, 1, 0.9)}
# seeds of pick_case under which the restatement reaches the cap with every choice far from rounding (0 where not named)
CASE_SEEDS = {(63, 300): 6, (64, 300): 3, (193, 300): 1, (513, 300): 3, (65, 255): 6, (65, 256): 1, (65, 257): 5, (65, 1024): 1,
              (65, 1025): 3, (65, 2047): 1, (65, 2048): 2, (10239, 300): 2, (10240, 300): 1}


@functools.lru_cache(maxsize=None)
def fixed_case(n_cols, n_rows, discard):
    """(candidates, Sample, kept score matrix [n_rows][n_cols], n, weight) of a fixed-iteration case on the wide family"""
    tree, R = wide_family()
    pool = None
    if discard > 0:                                              # deep nodes only: reads fall below the threshold there
        depth = np.zeros(len(tree.parent), np.int64)
        for v in range(1, len(depth)):
            depth[v] = depth[tree.parent[v]] + 1
        pool = np.nonzero(depth >= np.quantile(depth, 0.7))[0]
    cands, sample = pick_case(R, wide_reads()[0], n_cols, n_rows, discard, pool=pool, seed=CASE_SEEDS.get((n_cols, n_rows), 0))
    cols, _, sc, n, w = em_inputs(R, cands, sample, discard)
    assert len(cols) == n_cols
    return cands, sample, sc, n, w


# ------------------------------------------------------------------------------------------------ the EM restatement
class EmParams:
    """the fields of _lib.MetaParams the EM reads, with its defaults"""

    def __init__(self, error_rate=0.005, em_convergence=1e-5, em_delta_threshold=0.0, prop_threshold=0.005, discard=0.0,
                 em_max_iterations=1000, em_max_rounds=5):
        self.error_rate, self.em_convergence, self.em_delta_threshold = error_rate, em_convergence, em_delta_threshold
        self.prop_threshold, self.discard = prop_threshold, discard
        self.em_max_iterations, self.em_max_rounds = em_max_iterations, em_max_rounds


class EmResult:
    """cols (indices into the columns given), props, rounds, iterations, llh: as pmx_meta_em_info and the haplotypes report
    them; trace[round][iteration] = dict(props, llh2, llh_sq, took_sq, margin) with margin = llh_sq - (llh2 - convergence);
    dropped[round]: whether the round ended with columns below prop_threshold"""

    def order(self):
        """positions in cols / props in the order the haplotypes are published: by proportion, descending, stable"""
        return np.argsort(-self.props.astype(np.float64), kind="stable")


def em_restated(scores, n_seedmers, weight, params, dtype=np.float64):
    """oracle_meta.square_em (updateProps / normalizeProps / getExp / runSquareEM / removeLowPropNodes) with `params`
    (anything with the fields of _lib.MetaParams), computed in `dtype`; `scores` [kept rows][merged columns]"""
    T = dtype
    scores = np.asarray(scores, np.int64)
    n = np.asarray(n_seedmers, np.int64)[:, None]
    err = T(params.error_rate)
    probs = np.power(err, (n - scores).astype(T)) * np.power(T(1) - err, scores.astype(T))
    w = np.asarray(weight).astype(T)
    inv_total = T(1) / w.sum()
    eta, delta, floor = T(params.em_convergence), T(params.em_delta_threshold), T(1e-12)
    cols = np.arange(scores.shape[1])
    out = EmResult()
    out.trace, out.dropped, out.rounds, out.iterations, out.llh = [], [], 0, 0, T(0)
    props = np.zeros(0, T)

    def normalize(p):
        p = np.where(p <= 0, floor, p)
        return p / p.sum()

    for _ in range(max(1, int(params.em_max_rounds))):
        P = np.ascontiguousarray(probs[:, cols])
        k = len(cols)
        props = np.full(k, T(1) / T(k), T)

        def step(p):
            inv = T(1) / (P @ p)
            return ((w * inv) @ P) * p * inv_total

        def llh_of(p):
            return (w * np.log(P @ p)).sum()
        llh = T(0)
        its = []
        for _it in range(int(params.em_max_iterations)):
            p0 = props
            p1 = normalize(step(p0))
            p2 = normalize(step(p1))
            r = p1 - p0
            v = (p2 - p1) - r
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = -np.sqrt((r * r).sum()) / np.sqrt((v * v).sum())
                sq = normalize(p0 - T(2) * alpha * r + alpha * alpha * v)
                l2, lsq = llh_of(p2), llh_of(sq)
                took_sq = bool(lsq > l2 - eta)
            props, now = (sq, lsq) if took_sq else (p2, l2)
            diff, llh = now - llh, now
            its.append(dict(props=props, llh2=l2, llh_sq=lsq, took_sq=took_sq, margin=lsq - (l2 - eta), llh=now))
            if delta == 0:
                if abs(diff) < eta:
                    break
            elif np.abs(props - p0).max() < delta:
                break
        out.trace.append(its)
        out.rounds += 1
        out.iterations += len(its)
        out.llh = llh
        keep = props >= T(params.prop_threshold)
        out.dropped.append(not keep.all())
        if keep.all():
            break
        cols = cols[keep]
        props = np.full(len(cols), T(1) / T(len(cols)), T) if len(cols) else np.zeros(0, T)
        if not len(cols):
            break
    out.cols, out.props = cols, props
    return out


def cut(res, n_iterations):
    """a one-round run without any drop, as it stands after its first n_iterations iterations: the run with
    em_max_iterations = n_iterations (the loop is the same up to there; tests/test_meta_em_families.py checks it)"""
    assert res.rounds == 1 and not res.dropped[0]
    n_iterations = min(n_iterations, len(res.trace[0]))          # (a run that stopped by itself stays as it is)
    out = EmResult()
    it = res.trace[0][n_iterations - 1]
    out.trace, out.dropped, out.rounds, out.iterations, out.llh = [res.trace[0][:n_iterations]], [False], 1, n_iterations, it["llh"]
    out.cols, out.props = res.cols, it["props"]
    return out


@functools.lru_cache(maxsize=None)
def fixed_restated(n_cols, n_rows, discard, dtype_name):
    """the fixed-iteration case run to the largest of FIXED_ITERATIONS in one round, nothing dropped"""
    _, _, sc, n, w = fixed_case(n_cols, n_rows, discard)
    # (columns equal on the kept rows stay apart: the device merges on whole columns, and pick_case made those differ)
    p = EmParams(em_max_iterations=max(FIXED_ITERATIONS), em_max_rounds=1, prop_threshold=0.0, discard=discard)
    return em_restated(sc, n, w, p, getattr(np, dtype_name))


# ------------------------------------------------------------------------------------------------ mask events
def mask_events(arrays, cands, uniq):
    """what k_meta_mask_events sees for candidates `cands` (ascending DFS indices): per count change of a seedmer the reads
    carry (`uniq`: their distinct hashes) that is a present / absent transition, the bit range [lo, hi) of its node's
    subtree among the candidates, the hash and the orientation; and the number of changes without a transition (bumps)"""
    parent, off = arrays["parent"], arrays["offsets"]
    n = len(parent)
    end = np.arange(n)
    for v in range(n - 1, 0, -1):
        end[parent[v]] = max(end[parent[v]], end[v])
    node = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    keys = np.asarray(arrays["hash"], np.uint64)
    uniq = np.asarray(uniq, np.uint64)
    if len(uniq) == 0 or len(keys) == 0:
        z = np.zeros(0, np.int64)
        return dict(lo=z, hi=z, hash=z.astype(np.uint64), rev=z, bumps=0)

    def among(kk):
        pos = np.minimum(np.searchsorted(uniq, kk), len(uniq) - 1)
        return uniq[pos] == kk
    fwd = among(keys)
    rev = ~fwd & among(keys ^ np.uint64(XOR))
    carried = fwd | rev
    was, now = arrays["parent_count"] > 0, arrays["child_count"] > 0
    ev = carried & (was != now)
    cands = np.asarray(cands, np.int64)
    lo = np.searchsorted(cands, node[ev])
    hi = np.searchsorted(cands, end[node[ev]] + 1)
    return dict(lo=lo, hi=hi, hash=np.where(rev[ev], keys[ev] ^ np.uint64(XOR), keys[ev]), rev=rev[ev].astype(np.int64),
                bumps=int((carried & was & now).sum()))


def event_classes(ev):
    """which of the word-edge cases of the range arithmetic the events reach"""
    lo, hi = ev["lo"], ev["hi"]
    some = hi > lo
    last = hi - 1
    both = set(ev["hash"][ev["rev"] == 0].tolist()) & set(ev["hash"][ev["rev"] == 1].tolist())
    return dict(lo_on_word=bool((some & (lo % 64 == 0)).any()), hi_on_word=bool((some & (hi % 64 == 0)).any()),
                one_word_to_bit_63=bool((some & (lo // 64 == last // 64) & (last % 64 == 63)).any()),
                three_words=bool((some & (last // 64 - lo // 64 >= 2)).any()), empty=bool((hi == lo).any()),
                both_orientations=bool(both), bump=ev["bumps"] > 0)


# the candidate sets of the scoring tests: per crafted tree all of its nodes and two subsets; the wide tree's counts
WIDE_CANDIDATE_COUNTS = (63, 64, 65, 127, 128, 129, 4097)


def crafted_candidate_sets(n_nodes, seed):
    """all nodes; every third node (subtrees without a candidate: empty ranges); a random half"""
    rng = np.random.default_rng(seed)
    sets = [np.arange(n_nodes)]
    if n_nodes >= 3:
        sets.append(np.arange(1, n_nodes, 3))
        sets.append(np.sort(rng.choice(n_nodes, n_nodes // 2, replace=False)))
    return [s.astype(np.uint32) for s in sets]


def wide_candidate_set(n_nodes, count):
    """`count` nodes spread over the wide tree, the root and the last node among them"""
    return np.unique(np.concatenate([[0, n_nodes - 1], np.random.default_rng(count).choice(np.arange(1, n_nodes - 1), count - 2, replace=False)])).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ whole runs on small mixtures
def em_inputs(R, cands, sample, discard):
    """(merged columns as positions in cands, members per column, kept scores [rows][columns], n, weight): what the EM runs on"""
    sc = sample.scores(R, cands)
    first, cls = column_classes(sc)
    cols = np.sort(first)
    members = [[int(cands[j]) for j in np.nonzero(cls == cls[c])[0] if j != c] for c in cols]
    keep = kept_rows(sc, sample.n, discard)
    return cols, members, sc[np.ix_(keep, cols)], sample.n[keep], sample.mult[keep]


STAR71 = 2                    # assign_checks.crafted_trees()[2]


class SmallCase:
    """a whole run: `family` "wide" or the index of a crafted tree, the candidates, the Sample, the parameters, and
    `expect(res)`, the property its restatement `res` (float64) has to show"""

    def __init__(self, family, R, cands, sample, params, expect):
        self.family, self.R, self.cands, self.sample, self.params, self.expect = family, R, cands, sample, params, expect

    def inputs(self):
        return em_inputs(self.R, self.cands, self.sample, self.params.discard)

    @functools.lru_cache(maxsize=None)
    def restated(self):
        _, _, sc, n, w = self.inputs()
        return em_restated(sc, n, w, self.params, np.float64)


@functools.lru_cache(maxsize=None)
def small_cases():
    tree, R = wide_family()
    reads = wide_reads()[0]
    out = {}

    def wide(name, n_cols, seed, params, expect, dups=0):
        cands, sample = pick_case(R, reads, n_cols, 200, params.discard, dups=dups, seed=seed)
        out[name] = SmallCase("wide", R, cands, sample, params, expect)

    def drop_then_none(res):
        assert res.dropped == [True, False] and res.rounds == 2 and len(res.cols) >= 2

    def uniform_published(res):
        k = len(res.cols)
        assert res.dropped == [True] and res.rounds == 1 and 2 <= k < 20 and (res.props == 1.0 / k).all()

    def delta_rule(res):
        other = SmallCase("wide", R, out["delta_threshold"].cands, out["delta_threshold"].sample, EmParams(), None).restated()
        assert [len(t) for t in res.trace] != [len(t) for t in other.trace]          # the rule decides where the rounds stop
        assert all(len(t) < 1000 for t in res.trace)

    def grouped(res):
        _, members, _, _, _ = out["duplicate_columns"].inputs()
        assert sum(len(m) for m in members) == 3 and len(res.cols) == 20             # (prop_threshold 0: every group is reported)

    def at_and_below(res):
        c = out["discard_half"]
        sc = c.sample.scores(c.R, c.cands)
        mx, thr = sc.max(axis=1), (c.sample.n.astype(np.float64) * 0.5).astype(np.int64)
        keep = kept_rows(sc, c.sample.n, 0.5)
        assert ((mx == thr) & keep).any() and ((mx == thr - 1) & (mx > 0) & ~keep).any() and 6 <= len(c.inputs()[0]) <= 40

    def one_column(res):
        assert len(res.cols) == 1 and res.props[0] == 1.0 and len(res.trace[-1][0]["props"]) == 1
        assert np.isnan(res.trace[-1][0]["llh_sq"]) and not res.trace[-1][0]["took_sq"] and np.isfinite(res.llh)

    wide("drop_then_none", 20, 8, EmParams(), drop_then_none)
    wide("one_round_with_a_drop", 20, 8, EmParams(em_max_rounds=1), uniform_published)
    wide("delta_threshold", 20, 10, EmParams(em_delta_threshold=1e-5), delta_rule)
    wide("duplicate_columns", 20, 1, EmParams(prop_threshold=0.0), grouped, dups=3)
    wide("one_column", 20, 0, EmParams(), one_column)
    Rc, creads = ac.crafted_restated(STAR71), ac.crafted_reads()[0]
    usable = [r for r, m in zip(creads, Rc.merged) if m >= 0 and len(Rc.lists[m]) <= EM_MAX_SEEDMERS]
    out["discard_half"] = SmallCase(STAR71, Rc, np.arange(71, dtype=np.uint32), sample_of(Rc, creads, usable), EmParams(discard=0.5), at_and_below)
    return out
