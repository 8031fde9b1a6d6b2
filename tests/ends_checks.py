"""--mask-read-ends, --em-leaves-only and --write-ocranks of --meta: the read family, the restatements and the comparison the
tests share.  No product code in here: seedmers and DUST scores come from oracle_meta, trimming is a Python slice.

--mask-read-ends N (extractReadSequences, src/mgsr.cpp:1274-1280, 1304-1310): a read of length L becomes read[N : L - N] when
L > 2N and the empty read otherwise, before anything else looks at it.  The library does not cut strings: the seeding
kernels' per-end trim keeps the k-mers that lie inside that slice.  The tests hold the two to each other: every output of a
Meta after set_mask_read_ends(N) + set_reads(family) must equal, bit for bit, the output after set_mask_read_ends(0) +
set_reads(the family trimmed here), and the merged lists must equal oracle_meta's seedmers of the trimmed strings.

The family of one N (family(N)), k = 19:
  * lengths 0, 1, 2N-1, 2N, 2N+1, 2N+k-1, 2N+k, 2N+k+1: nothing left, one base left, one base short of a k-mer, one k-mer, two;
  * trimmed lengths 31, 32, 33, 63, 64, 65: the 2-bit packing holds 32 bases a word, so the trimmed read ends on and off a word
    edge, and with N = 31, 32, 33 it starts on and off one;
  * a window and four copies of it with `N` at N-1, N, L-N-1 and L-N: the outer two lose their `N` to the trim and are the
    window again, the inner two keep it as their first / last base;
  * twins: a window and copies that differ from it inside the trimmed ends only -- one merged read of multiplicity >= 4;
  * two DUST reads around DUST_THRESHOLD: one above it before trimming and not after, one the other way round;
  * 100 reads tiled over two genomes of rsv_4K, every third reverse-complemented, as assign_checks.rsv_reads() tiles them.

--em-leaves-only (squareEM::squareEM, src/mgsr.cpp:8018-8037): leaves_candidates restates the rule from the overlap
coefficients, the ids and the heads.  --write-ocranks (writeOCRanks, src/main.cpp:430-444): ocranks_text."""
import functools

import numpy as np

import assign_checks as ac
import mask_checks as mc
from oracle import oracle_meta as om

K, S, L = ac.K, ac.S, ac.L
NS = (1, 5, 31, 32, 33)
DUST_THRESHOLD = 20.0
EDGE_LENGTHS = (31, 32, 33, 63, 64, 65)


def trim(read: bytes, n: int) -> bytes:
    return read[n:len(read) - n] if len(read) > 2 * n else b""


def trimmed(reads, n):
    return [trim(r, n) for r in reads]


def short_lengths(n):
    return (0, 1, 2 * n - 1, 2 * n, 2 * n + 1, 2 * n + K - 1, 2 * n + K, 2 * n + K + 1)


def _other(base):
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def _dust_reads(n, rng, window):
    """(down, up): get_dust(down) > T >= get_dust(trim(down)) and get_dust(up) <= T < get_dust(trim(up)).  `down` is a run of
    A, random bases and a genome window: it has seedmers either way, so the filter shows in the lists.  `up` is a run of A
    between random bases.  Both are found by a seeded scan over the length of the run."""
    rnd = lambda m: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), m))
    down = up = None
    for e in range(40):                     # the score grows with the run: the first run that crosses the threshold, flank by flank
        head, tail = rnd(n + e), rnd(n + e)
        for run in range(3, 90):
            q = b"A" * run + tail + window      # the trim shortens the run
            if down is None and om.get_dust(q) > DUST_THRESHOLD:
                if om.get_dust(trim(q, n)) <= DUST_THRESHOLD:
                    down = q
                break
        for run in range(3, 90):
            q = head + b"A" * run + tail        # the trim takes random bases away from around the run
            if up is None and om.get_dust(trim(q, n)) > DUST_THRESHOLD:
                if om.get_dust(q) <= DUST_THRESHOLD:
                    up = q
                break
        if down is not None and up is not None:
            break
    assert down is not None and up is not None, n
    return down, up


class Family:
    """reads: the raw reads in a shuffled order; the named members are the reads themselves"""


@functools.lru_cache(maxsize=None)
def family(n):
    rng = np.random.default_rng(1274 + n)
    a, b = mc.genomes()
    F = Family()
    F.n = n
    F.short = [a[500:500 + m] for m in short_lengths(n)]
    F.edges = [a[900 + 70 * i:900 + 70 * i + m + 2 * n] for i, m in enumerate(EDGE_LENGTHS)]
    w = a[2000:2000 + 150 + 2 * n]
    F.window = w
    F.with_n = []
    for p in (n - 1, n, len(w) - n - 1, len(w) - n):
        q = bytearray(w)
        q[p] = ord("N")
        F.with_n.append(bytes(q))
    t = a[5000:5000 + 150 + 2 * n]
    ends = list(range(n)) + list(range(len(t) - n, len(t)))
    first, last, every = bytearray(t), bytearray(t), bytearray(t)
    first[0] = _other(t[0])
    last[-1] = _other(t[-1])
    for p in ends:
        every[p] = _other(t[p])
    F.twins = [t, bytes(first), bytes(last), bytes(every)]
    F.dust_down, F.dust_up = _dust_reads(n, rng, a[4000:4120])
    tiles = ac._tile(a.decode(), 60) + ac._tile(b.decode(), 40)
    F.tiles = [ac.revcomp(r) if i % 3 == 0 else r for i, r in enumerate(tiles)]
    assert all(set(r) <= set(b"ACGT") for r in F.short + F.edges + [w, t])   # (the genome has stretches of N: some tiles hold them)
    reads = F.short + F.edges + [w] + F.with_n + F.twins + [F.dust_down, F.dust_up] + F.tiles
    F.reads = [reads[i] for i in rng.permutation(len(reads))]
    return F


@functools.lru_cache(maxsize=None)
def crafted_sample(n):
    """the family of n and 80 reads of the crafted family of assign_checks: what a crafted tree has something to score with
    (its reads of 150 bases only: the EM's err^n underflows for the hundreds of seedmers of its 1,200-base read)"""
    return family(n).reads + [r for r in ac.crafted_reads()[0] if len(r) == 150][:80]


def kept_by_dust(reads, dust):
    """the reads --dust keeps (src/mgsr.cpp:1593-1594: a read with a non-zero score above the threshold leaves)"""
    if not dust < 100.0:
        return [True] * len(reads)
    return [not (d != 0 and d > dust) for d in (om.get_dust(r) for r in reads)]


def merged_from_strings(reads, dust=100.0):
    """(offsets, hashes, orientations, multiplicities, raw -> merged) of these very strings, from oracle_meta alone: the
    distinct non-empty seedmer lists of the reads --dust keeps, in the order of (hash list, orientation list)"""
    keep = kept_by_dust(reads, dust)
    off, h, v, mult, raw = mc.merge_lists([r if kp else b"" for r, kp in zip(reads, keep)])
    return off, h, v, mult, raw


@functools.lru_cache(maxsize=None)
def family_expected(n, dust=100.0, crafted=False):
    return merged_from_strings(trimmed(crafted_sample(n) if crafted else family(n).reads, n), dust)


# ------------------------------------------------------------------------------------------------ two runs of one Meta
def bits(x):
    """doubles as their bit patterns"""
    return np.atleast_1d(np.asarray(x, np.float64)).copy().view(np.uint64)


def run(meta, reads, ends, params, dust=100.0, mask_reads=0, top_oc=1000):
    """one sample through a Meta -> everything the issue compares, doubles as bit patterns"""
    meta.set_mask_read_ends(ends)
    meta.set_dust(dust)
    meta.set_masks(reads=mask_reads)
    meta.set_reads(reads)
    out = dict(seedmers=meta.read_seedmers(), info=meta.read_info(), raw_to_merged=meta.raw_to_merged(), oc=bits(meta.overlap_coefficients()))
    meta.score(top_oc=top_oc)
    out["candidates"], out["scores"] = meta.candidates(), meta.scores()
    out["haplotypes"] = [(node, int(bits(p)[0]), members) for node, p, members in meta.em(params)]
    info = meta.em_info()
    out["em_info"] = (info["rounds"], info["iterations"], int(bits(info["log_likelihood"])[0]))
    return out


def assert_same(got, want, label=""):
    """two results of run(): exactly equal"""
    for i, name in enumerate(("offsets", "hashes", "orientations")):
        assert np.array_equal(got["seedmers"][i], want["seedmers"][i]), (label, name)
    for i, name in enumerate(("n_seedmers", "multiplicity")):
        assert np.array_equal(got["info"][i], want["info"][i]), (label, name)
    for name in ("raw_to_merged", "oc", "candidates", "scores"):
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (label, name)
    assert got["haplotypes"] == want["haplotypes"], (label, "haplotypes")
    assert got["em_info"] == want["em_info"], (label, "em_info", got["em_info"], want["em_info"])


def assert_lists(got, expected, label=""):
    """a result of run() against merged_from_strings of the trimmed strings"""
    off, h, v, mult, raw = expected
    assert np.array_equal(got["seedmers"][0], off) and np.array_equal(got["seedmers"][1], h) and np.array_equal(got["seedmers"][2], v), label
    assert np.array_equal(got["info"][1], mult) and np.array_equal(got["raw_to_merged"], raw), label


# ------------------------------------------------------------------------------------------------ --em-leaves-only
def is_sample(node_id: str) -> bool:
    return not node_id.startswith("node_")


def eligible_nodes(ids, heads):
    """a node is eligible when it, or a node folded onto the same head, is a sample"""
    heads = np.asarray(heads)
    sampled_heads = {int(heads[v]) for v in range(len(ids)) if is_sample(ids[v])}
    return np.array([int(heads[v]) in sampled_heads for v in range(len(ids))], bool)


def leaves_candidates(oc, ids, heads, top_oc):
    """the rule restated (src/mgsr.cpp:8021-8037): the nodes by falling coefficient, ascending DFS index within a value; a node
    that is not eligible is passed over before a rank is counted; stop when the eligible ranks exceed top_oc"""
    ok = eligible_nodes(ids, heads)
    order = sorted(range(len(oc)), key=lambda v: (-oc[v], v))
    out, ranks, cur = [], 0, None
    for v in order:
        if not ok[v]:
            continue
        if cur is None or oc[v] != cur:
            cur = oc[v]
            ranks += 1
            if ranks > top_oc:
                break
        out.append(v)
    return np.array(sorted(out), np.uint32)


def plain_candidates(oc, top_oc):
    """the rule without the switch: every node counts"""
    return leaves_candidates(oc, [""] * len(oc), np.arange(len(oc)), top_oc)


# ------------------------------------------------------------------------------------------------ --write-ocranks
def ocranks_text(oc, ids) -> str:
    """`<prefix>.overlapCoefficients.tsv` (writeOCRanks, src/main.cpp:430-444): id <TAB> coefficient with six decimals <TAB>
    rank, by falling coefficient (ascending DFS index within a value); the rank starts at 0 and goes up whenever the
    coefficient differs from the line before"""
    order = sorted(range(len(oc)), key=lambda v: (-oc[v], v))
    lines, rank, cur = [], 0, oc[order[0]] if order else 0.0
    for v in order:
        if oc[v] != cur:
            cur = oc[v]
            rank += 1
        lines.append("%s\t%.6f\t%d" % (ids[v], oc[v], rank))
    return "\n".join(lines) + ("\n" if lines else "")


# ------------------------------------------------------------------------------------------------ the tree of eight nodes
SMALL_IDS = ["node_1", "node_2", "S_a", "node_3", "S_b", "node_4", "node_5", "S_c"]
SMALL_PARENT = np.array([0, 0, 1, 0, 3, 3, 0, 6], np.uint32)


@functools.lru_cache(maxsize=None)
def small_tree():
    """Eight nodes in DFS pre-order, made through Index.from_arrays with ids:

        0 node_1 ── 1 node_2 ── 2 S_a
                 ├─ 3 node_3 ── 4 S_b
                 │           └─ 5 node_4
                 └─ 6 node_5 ── 7 S_c     (S_c carries no change: it folds onto node_5, which is eligible through the fold)

    Four sequences of 400 random bases X, Y, Z, W; the reads are windows of X, Y, Z (none of W), so a seedmer of W in a genome
    lowers its coefficient.  Gained: node_2 all of X's seedmers (coefficient 1, the best, and not eligible); S_a loses the last
    third of X's and gains 4 of W's; node_3 the first half of Y's and 2 of W's; S_b the rest of Y's and 10 of W's; node_4 20
    of W's; node_5 the first third of Z's and 6 of W's; the root holds nothing.  The tests check the order this gives.
    -> (tree, reads, ids)"""
    rng = np.random.default_rng(8018)
    rnd = lambda m: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), m))
    X, Y, Z, W = (rnd(400) for _ in range(4))
    sm = lambda q: [(h, int(v)) for h, v in dict.fromkeys(om.seedmers(q, K, S, L))]
    x, y, z, w = sm(X), sm(Y), sm(Z), sm(W)
    assert len(w) >= 42 and len({h for h, _ in x + y + z + w}) == len(x + y + z + w)
    toggle = lambda keys: {key: "toggle" for key in keys}
    plan = {1: toggle(x), 2: toggle(x[2 * len(x) // 3:] + w[:4]), 3: toggle(y[:len(y) // 2] + w[4:6]), 4: toggle(y[len(y) // 2:] + w[6:16]),
            5: toggle(w[16:36]), 6: toggle(z[:len(z) // 3] + w[36:42])}
    tree = ac.tree_from_plan("small8", SMALL_PARENT, plan, rng)
    reads = [q[i:i + 150] for q in (X, Y, Z) for i in range(0, 251, 25)]
    return tree, reads, SMALL_IDS


def small_indexes(pmx, ids):
    tree = small_tree()[0]
    a, o = tree.plain, tree.oriented
    return (pmx.Index.from_arrays(K, S, 0, L, False, tree.parent, a["offsets"], a["hash"], a["parent_count"], a["child_count"], node_ids=ids),
            pmx.Index.from_arrays(K, S, 0, L, False, tree.parent, o["offsets"], o["hash"], o["parent_count"], o["child_count"], oriented=True,
                                  node_ids=ids))
