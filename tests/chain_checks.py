"""Anchor lists for the sort / chaining probes (pmx_align_chain_probe, hs_chain_probe), a plain-Python restatement of the
reference's chain fill and backtrack that counts the events the families are named for, and the exact comparison.  No test
lives here: tests/test_chain_families.py (CPU) and tests/test_chain_probe_gpu.py import it.

Anchors are the reference's: x = strand << 63 | rid << 32 | ref_pos, y = seg << 48 | q_span << 32 | q_pos.

A Family is ONE probe call: an operation, the parameter overrides, and a batch of lists.  `expect` of a list:
  "equal"              served, status 0, n_u / u[] / anchors equal to the reference's
  "equal_or_overflow"  the same, or PMX_ST_OVERFLOW (the sort's pending stack)
  "unsupported"        the packed cells do not hold the positions: PMX_ST_UNSUPPORTED with n_a = 0 -- on the wave paths only
                       for n > 64 (the n <= 64 fill keeps whole anchors in registers), on the scalar forms at any n
Two rules sit above `expect` and come from the reported capacities and the reference's answer alone: a list longer than
caps.max_anchor is not served, and a list for which the reference accepts more than caps.max_reg * 4 chains carries
PMX_ST_OVERFLOW."""
import ctypes as C
import dataclasses
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

SEG_SHIFT = 48
ST_OVERFLOW, ST_UNSUPPORTED = 1, 2
OPS = {"SORT128": 0, "SORT64": 1, "CHAIN_DP": 2, "CHAIN_RMQ": 3}
INT_MIN = -(1 << 31)
DEFAULT = INT_MIN            # an integer parameter left to the preset (a float: NaN)
PARAM_FIELDS = ("bw", "bw_long", "max_gap", "max_chain_skip", "max_chain_iter", "min_cnt", "min_chain_score", "chn_pen_gap", "chn_pen_skip",
                "rmq_inner_dist", "rmq_size_cap", "max_dist_x", "max_dist_y", "n_seg")
PARAMS_DTYPE = np.dtype([(k, "<f4" if k.startswith("chn_pen") else "<i4") for k in PARAM_FIELDS])
RESULT_DTYPE = np.dtype([("served", "<i4"), ("status", "<u4"), ("n_a", "<i8"), ("n_u", "<i4"), ("pad", "<i4")])
CAPS_DTYPE = np.dtype([("max_anchor", "<i4"), ("max_reg", "<i4"), ("max_qlen", "<i4"), ("reserved", "<i4")])
PRESETS = {"150": 150, "1000": 1000}       # mean read length -> the short-read preset / map-ont
MAX_READ_LEN = 2000                        # what the wave layouts are planned from: 16,160 anchors, 128 chains


def params_record(overrides):
    p = np.zeros(1, PARAMS_DTYPE)
    for k in PARAM_FIELDS:
        p[k] = np.nan if k.startswith("chn_pen") else DEFAULT
    for k, v in overrides.items():
        p[k] = v
    return p


def mk(strand, rid, rpos, qpos, span=15, seg=0):
    return (strand << 63 | rid << 32 | rpos, seg << SEG_SHIFT | span << 32 | qpos)


def diag(strand, rid, r0, q0, n, step, span=15, seg=0, qstep=None):
    qstep = step if qstep is None else qstep
    return [mk(strand, rid, r0 + step * k, q0 + qstep * k, span, seg) for k in range(n)]


def as_list(anchors, sort=True):
    """(x, y) uint64 arrays, sorted by x (stable: what precedes in the input precedes among equal x)"""
    x = np.array([a[0] for a in anchors], np.uint64)
    y = np.array([a[1] for a in anchors], np.uint64)
    if sort and len(x):
        o = np.argsort(x, kind="stable")
        x, y = x[o], y[o]
    return x, y


@dataclasses.dataclass
class Family:
    name: str
    op: str
    lists: list                      # [(x, y)]
    params: dict = dataclasses.field(default_factory=dict)
    n_segs: int = 1                  # of the layout; params["n_seg"] follows it unless given
    qlen: list = None                # per list (q0, q1); None: (60000, 0) / (30000, 30000)
    expect: list = None              # per list; None: "equal"
    max_read_len: int = MAX_READ_LEN

    def __post_init__(self):
        n = len(self.lists)
        if self.qlen is None:
            self.qlen = [(60000, 0) if self.n_segs == 1 else (30000, 30000)] * n
        if self.expect is None:
            self.expect = ["equal"] * n
        self.params = dict(self.params)
        self.params.setdefault("n_seg", self.n_segs)

    def flat(self):
        off = np.zeros(len(self.lists) + 1, np.int64)
        if self.lists:
            off[1:] = np.cumsum([len(x) for x, _ in self.lists])
        a = np.zeros((max(int(off[-1]), 1), 2), np.uint64)
        for i, (x, y) in enumerate(self.lists):
            a[off[i]:off[i + 1], 0] = x
            a[off[i]:off[i + 1], 1] = y
        return a, off, np.ascontiguousarray(np.array(self.qlen, np.int32).reshape(-1, 2))


# ----------------------------------------------------------------------------------------- the reference, list by list
def reference(fam: Family, P):
    """the compiled reference on every list of the family; P: the parameters in force (a PARAMS_DTYPE record with no defaults left).
    -> [(x, y, u)] (sorts: u empty)"""
    out = []
    for x, y in fam.lists:
        if fam.op == "SORT128":
            sx, sy = orc.ref_radix_sort_128x(x, y)
            out.append((sx, sy, np.zeros(0, np.uint64)))
        elif fam.op == "SORT64":
            sx = orc.ref_radix_sort_64(x)
            out.append((sx, np.zeros(len(sx), np.uint64), np.zeros(0, np.uint64)))
        elif fam.op == "CHAIN_DP":
            out.append(orc.ref_lchain_dp(x, y, int(P["max_dist_x"]), int(P["max_dist_y"]), int(P["bw"]), int(P["max_chain_skip"]), int(P["max_chain_iter"]),
                                         int(P["min_cnt"]), int(P["min_chain_score"]), float(P["chn_pen_gap"]), float(P["chn_pen_skip"]), int(P["n_seg"])))
        else:
            out.append(orc.ref_lchain_rmq(x, y, int(P["max_gap"]), int(P["rmq_inner_dist"]), int(P["bw_long"]), int(P["max_chain_skip"]),
                                          int(P["rmq_size_cap"]), int(P["min_cnt"]), int(P["min_chain_score"]), float(P["chn_pen_gap"]),
                                          float(P["chn_pen_skip"])))
    return out


# ----------------------------------------------------------------------------------------- the compare function
def compare(fam: Family, got, caps, ref, wave: bool):
    """got: (results RESULT_DTYPE[n], anchors uint64 [total][2], u uint64 [total], offsets).  wave: a wave path (else a scalar form).
    -> None, or a message naming the first differing list with its family, index and n"""
    res, ga, gu, off = got
    max_anchor, max_chains = int(caps["max_anchor"]), int(caps["max_reg"]) * 4
    for i, (x, _) in enumerate(fam.lists):
        n = len(x)
        tag = "%s[%d] n=%d %s" % (fam.name, i, n, fam.op)
        r = res[i]
        if n > max_anchor:
            if r["served"]:
                return tag + ": served beyond max_anchor=%d" % max_anchor
            continue
        if not r["served"]:
            return tag + ": not served within max_anchor=%d" % max_anchor
        rx, ry, ru = ref[i]
        st = int(r["status"])
        exp = fam.expect[i]
        if exp == "unsupported" and n > 0 and (n > 64 or not wave):
            if st != ST_UNSUPPORTED or int(r["n_a"]) != 0:
                return tag + ": status %d n_a %d, PMX_ST_UNSUPPORTED with n_a 0 required" % (st, int(r["n_a"]))
            continue
        if fam.op.startswith("CHAIN") and len(ru) > max_chains:
            if st != ST_OVERFLOW:
                return tag + ": status %d, PMX_ST_OVERFLOW required (%d chains > %d)" % (st, len(ru), max_chains)
            continue
        if exp == "equal_or_overflow" and st == ST_OVERFLOW:
            continue
        if st != 0:
            return tag + ": status %d" % st
        if fam.op.startswith("CHAIN") and int(r["n_u"]) != len(ru):
            return tag + ": n_u %d, reference %d" % (int(r["n_u"]), len(ru))
        if int(r["n_a"]) != len(rx):
            return tag + ": n_a %d, reference %d" % (int(r["n_a"]), len(rx))
        o = int(off[i])
        for k in range(len(ru)):
            if int(gu[o + k]) != int(ru[k]):
                return tag + ": u[%d] = %#x, reference %#x" % (k, int(gu[o + k]), int(ru[k]))
        bad = np.nonzero((ga[o:o + len(rx), 0] != rx) | (ga[o:o + len(rx), 1] != ry))[0]
        if len(bad):
            k = int(bad[0])
            return tag + ": anchor %d = (%#x, %#x), reference (%#x, %#x)" % (k, int(ga[o + k, 0]), int(ga[o + k, 1]), int(rx[k]), int(ry[k]))
    return None


# ----------------------------------------------------------------------------------------- hs_chain_probe
_hs = {}


def hostsim(tpp: bool):
    if tpp not in _hs:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
        so = os.path.join(here, "libhostsim_tpp.so" if tpp else "libhostsim.so")
        import subprocess
        subprocess.run(["make", "-C", here], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        L = C.CDLL(so)
        L.hs_chain_probe.restype = C.c_int
        L.hs_chain_probe.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 4
        _hs[tpp] = L
    return _hs[tpp]


def run_hostsim(fam: Family, mean_read_len: int, tpp: bool):
    """-> (got as compare takes it, caps record, parameters in force)"""
    L = hostsim(tpp)
    a, off, ql = fam.flat()
    n = len(fam.lists)
    P = params_record(fam.params)
    caps = np.zeros(1, CAPS_DTYPE)
    res = np.zeros(max(n, 1), RESULT_DTYPE)
    oa = np.zeros_like(a)
    ou = np.zeros(len(a), np.uint64)
    rc = L.hs_chain_probe(mean_read_len, OPS[fam.op], fam.max_read_len, fam.n_segs, P.ctypes.data, a.ctypes.data, off.ctypes.data, ql.ctypes.data, n,
                          res.ctypes.data, oa.ctypes.data, ou.ctypes.data, caps.ctypes.data)
    assert rc == 0, rc
    return (res[:n], oa, ou, off), caps[0], P[0]


def preset_params(mean_read_len: int, overrides):
    """the parameters in force for a preset: the defaults come from the CPU build's make_opt"""
    L = hostsim(False)
    P = params_record(overrides)
    caps = np.zeros(1, CAPS_DTYPE)
    rc = L.hs_chain_probe(mean_read_len, 0, MAX_READ_LEN, 1, P.ctypes.data, None, None, None, 0, None, None, None, caps.ctypes.data)
    assert rc == 0, rc
    return P[0]


# ----------------------------------------------------------------------------------------- mg_lchain_dp in plain Python
def _mg_log2(x):   # mmpriv.h:118-126 on float32 arrays
    zi = x.view(np.uint32)
    log2 = (((zi >> np.uint32(23)) & np.uint32(255)).astype(np.int32) - 128).astype(np.float32)
    zf = ((zi & np.uint32(~(255 << 23) & 0xffffffff)) + np.uint32(127 << 23)).view(np.float32)
    return log2 + ((np.float32(-0.34484843) * zf + np.float32(2.02466578)) * zf - np.float32(0.67487759))


def _i32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def comput_sc(xi, yi, xs, ys, P):
    """comput_sc (lchain.c:113-138, is_cdna = 0) of anchor i against the anchors (xs, ys): int64 array, INT_MIN = rejected"""
    gap, skip = np.float32(P["chn_pen_gap"]), np.float32(P["chn_pen_skip"])
    mdx, mdy, bw, n_seg = P["mdx"], P["mdy"], P["bw"], P["n_seg"]
    qi = _i32(int(yi) & 0xffffffff)
    qj = _i32((ys & np.uint64(0xffffffff)).astype(np.int64))
    dq = _i32(qi - qj)
    dr = _i32((((int(xi) & 0xffffffff) - (xs & np.uint64(0xffffffff)).astype(np.int64))) & 0xffffffff)
    sidi = int(yi) >> SEG_SHIFT & 0xff
    same = ((ys >> np.uint64(SEG_SHIFT)) & np.uint64(0xff)).astype(np.int64) == sidi
    dd = np.abs(dr - dq)
    bad = (dq <= 0) | (dq > mdx) | (same & ((dr == 0) | (dq > mdy))) | (same & (dd > bw))
    if n_seg > 1:
        bad |= same & (dr > mdy)
    dg = np.minimum(dr, dq)
    span = ((ys >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    sc = np.minimum(span, dg)
    pen = (dd != 0) | (dg > span)
    ddc = np.clip(dd, 0, 1 << 30)
    lin = gap * ddc.astype(np.float32) + skip * np.clip(dg, -(1 << 30), 1 << 30).astype(np.float32)
    logp = np.where(ddc >= 1, _mg_log2((ddc + 1).astype(np.float32)), np.float32(0)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p_same = np.trunc(lin + np.float32(.5) * logp)
        p_diff = np.trunc(np.minimum(lin, logp))
    p_same = np.nan_to_num(p_same, nan=0.0, posinf=1e9, neginf=-1e9).astype(np.int64)
    p_diff = np.nan_to_num(p_diff, nan=0.0, posinf=1e9, neginf=-1e9).astype(np.int64)
    sc_pen = np.where(same, sc - p_same, np.where(dr == 0, sc + 1, sc - p_diff))
    sc = np.where(pen, sc_pen, sc)
    return np.where(bad, INT_MIN, sc)


def py_lchain_dp(x, y, P):
    """the fill loop of mg_lchain_dp (lchain.c:163-205) and mg_chain_backtrack + compact_a (:9-111) restated; the two sorts inside
    are the compiled reference's (their tie order is the sort families' subject).  P: the parameters in force.
    -> dict(f, p, x, y, u, ev) with ev the event counts"""
    n = len(x)
    bw = int(P["bw"])
    Q = dict(chn_pen_gap=float(P["chn_pen_gap"]), chn_pen_skip=float(P["chn_pen_skip"]), bw=bw, n_seg=int(P["n_seg"]),
             mdx=max(int(P["max_dist_x"]), bw), mdy=max(int(P["max_dist_y"]), bw))
    max_skip, max_iter, mdx = int(P["max_chain_skip"]), int(P["max_chain_iter"]), Q["mdx"]
    min_cnt, min_sc, max_drop = int(P["min_cnt"]), int(P["min_chain_score"]), bw
    ev = dict(breaks=0, breaks_inside=0, rescues=0, clamps=0, max_window=0, windows=set(), max_mark_dist=0, mii_before_st=0, strand_resets=0,
              ends_used=0, max_used_run=0, drop_cuts=0, rejected_marking=0, hit_used=0, end_ties=0, n_z=0, drop_exact=0)
    xi_ = [int(v) for v in x]
    f, p, t = [0] * n, [-1] * n, [0] * n
    st, max_ii = 0, -1
    M64 = (1 << 64) - 1
    for i in range(n):
        max_j, max_f, n_skip = -1, int(y[i]) >> 32 & 0xff, 0
        while st < i and (xi_[i] >> 32 != xi_[st] >> 32 or xi_[i] > xi_[st] + mdx):
            st += 1
        if i - st > max_iter:
            st = i - max_iter
            ev["clamps"] += 1
        ev["max_window"] = max(ev["max_window"], i - st)
        ev["windows"].add(i - st)
        end_j = st - 1
        if i > st:
            sc_all = comput_sc(x[i], y[i], x[st:i], y[st:i], Q)
            for jj in np.nonzero(sc_all != INT_MIN)[0][::-1]:
                j = st + int(jj)
                sc = int(sc_all[jj]) + f[j]
                if sc > max_f:
                    max_f, max_j = sc, j
                    if n_skip > 0:
                        n_skip -= 1
                elif t[j] == i:
                    n_skip += 1
                    if n_skip > max_skip:
                        end_j = j
                        ev["breaks"] += 1
                        if j > st:
                            ev["breaks_inside"] += 1
                        break
                if p[j] >= 0:
                    t[p[j]] = i
                    ev["max_mark_dist"] = max(ev["max_mark_dist"], j - p[j])
        if max_ii < 0 or ((xi_[i] - xi_[max_ii]) & M64) > mdx:
            if max_ii >= 0 and xi_[i] >> 63 != xi_[max_ii] >> 63:
                ev["strand_resets"] += 1
            mx, max_ii = INT_MIN, -1
            for j in range(i - 1, st - 1, -1):
                if mx < f[j]:
                    mx, max_ii = f[j], j
        if max_ii >= 0 and max_ii < end_j:
            if max_ii < st:
                ev["mii_before_st"] += 1
            tmp = int(comput_sc(x[i], y[i], x[max_ii:max_ii + 1], y[max_ii:max_ii + 1], Q)[0])
            if tmp != INT_MIN and max_f < tmp + f[max_ii]:
                max_f, max_j = tmp + f[max_ii], max_ii
                ev["rescues"] += 1
        f[i], p[i] = max_f, max_j
        if max_ii < 0 or (((xi_[i] - xi_[max_ii]) & M64) <= mdx and f[max_ii] < f[i]):
            max_ii = i
    # mg_chain_backtrack
    zi = [i for i in range(n) if f[i] >= min_sc]
    ev["n_z"] = len(zi)
    out = dict(f=f, p=p, ev=ev, x=np.zeros(0, np.uint64), y=np.zeros(0, np.uint64), u=np.zeros(0, np.uint64))
    if not zi:
        return out
    zx, zy = orc.ref_radix_sort_128x(np.array([f[i] for i in zi], np.int64).astype(np.uint64), np.array(zi, np.uint64))
    ev["end_ties"] = len(zx) - len(set(int(v) for v in zx))
    used = [0] * n          # 0 free, 1 in an accepted chain, 2 in a rejected one
    v, u = [], []
    run = 0
    for k in range(len(zx) - 1, -1, -1):
        i = int(zy[k])
        if used[i]:
            ev["ends_used"] += 1
            run += 1
            ev["max_used_run"] = max(ev["max_used_run"], run)
            continue
        run = 0
        zf = _i32(int(zx[k]) & 0xffffffff)
        # mg_chain_bk_end
        max_s, max_i, walk, j = 0, i, [], i
        while True:
            walk.append(j)
            j = p[j]
            s = zf if j < 0 else zf - f[j]
            if s > max_s:
                max_s, max_i = s, j
            elif max_s - s > max_drop:
                ev["drop_cuts"] += 1
                break
            elif max_s - s == max_drop:
                ev["drop_exact"] += 1
            if not (j >= 0 and used[j] == 0):
                if j >= 0:
                    ev["hit_used"] += 1
                    if used[j] == 2:
                        ev["rejected_marking"] += 1
                break
        chain = []
        j = i
        while j != max_i:
            chain.append(j)
            j = p[j]
        sc = zf if j < 0 else zf - f[j]
        ok = sc >= min_sc and len(chain) > 0 and len(chain) >= min_cnt
        for j in chain:
            used[j] = 1 if ok else 2
        if ok:
            v.append(chain[::-1])
            u.append(sc << 32 | len(chain))
    if not u:
        return out
    # compact_a
    starts, k = [], 0
    for c in v:
        starts.append(k)
        k += len(c)
    wx, wy = orc.ref_radix_sort_128x(np.array([int(x[c[0]]) for c in v], np.uint64), np.array([starts[i] << 32 | i for i in range(len(v))], np.uint64))
    order = [int(w) & 0xffffffff for w in wy]
    idx = [j for i in order for j in v[i]]
    out.update(x=x[idx], y=y[idx], u=np.array([u[i] for i in order], np.uint64))
    return out


# ----------------------------------------------------------------------------------------- sort families
def sort_families(op):
    rnd = random.Random(20240607)
    fams = []

    def pay(keys):     # distinct payloads: the order of equal keys is visible (SORT64 has none: equal keys are equal words)
        return (np.array(keys, np.uint64), np.arange(len(keys), dtype=np.uint64) + np.uint64(1000))

    def fam(name, key_lists, expect=None, max_read_len=MAX_READ_LEN):
        fams.append(Family(name, op, [pay(k) for k in key_lists], expect=expect, max_read_len=max_read_len))

    r64 = lambda: rnd.getrandbits(64)
    fam("sizes", [[r64() for _ in range(n)] for n in (0, 1, 2, 63, 64, 65, 66, 128, 129, 1000)])
    fam("all_equal", [[0x1234567800abcdef] * 65, [77] * 200, [0] * 66])
    b0 = [[0xaabbccddeeff1100 | rnd.randrange(256) for _ in range(n)] for n in (65, 300)]
    b7 = [[rnd.randrange(256) << 56 | 0x00bbccddeeff1122 for _ in range(n)] for n in (65, 300)]
    b07 = [[rnd.randrange(256) << 56 | 0x00bbccddeeff1100 | rnd.randrange(256) for _ in range(n)] for n in (65, 300, 1000)]
    # (bytes 0 and 7 only: a byte-7 bucket of more than 64 elements must still be sorted on byte 0 -- 4 top bytes over 400 elements)
    b07.append([rnd.randrange(4) << 56 | 0x00bbccddeeff1100 | rnd.randrange(256) for _ in range(400)])
    fam("single_byte", b0 + b7 + b07)
    d8 = [r64() for _ in range(8)]
    fam("heavy_duplicates", [[d8[rnd.randrange(8)] for _ in range(500)], [d8[rnd.randrange(2)] for _ in range(130)]])
    # second-level buckets of exactly 64 and 65: one top byte, second byte k holds 64 / 65 elements that differ further down
    lv2 = []
    for m in (64, 65):
        keys = [0x55 << 56 | b << 48 | rnd.getrandbits(48) for b in range(3) for _ in range(m)]
        rnd.shuffle(keys)
        lv2.append(keys)
    fam("level2_buckets", lv2)
    base = sorted(r64() for _ in range(300))
    fam("orders", [base, base[::-1], [r64() for _ in range(300)], sorted(rnd.randrange(50) for _ in range(300)), sorted((rnd.randrange(50) for _ in range(300)), reverse=True)])
    # chain-end-like keys: small positive scores, the top six bytes equal
    fam("chain_ends", [[rnd.randrange(25, 3000) for _ in range(n)] for n in (64, 65, 200, 1800)] + [[rnd.randrange(40, 60) for _ in range(500)]])
    # the stack edge: 70 first-level buckets of 65 elements each (more pending ranges than the 64-entry stack holds), and 64 x 65 below it
    edge = []
    for nb in (64, 70):
        keys = [b << 56 | rnd.getrandbits(56) for b in range(nb) for _ in range(65)]
        rnd.shuffle(keys)
        edge.append(keys)
    fam("stack_edge", edge, expect=["equal", "equal_or_overflow"])
    return fams


# ----------------------------------------------------------------------------------------- CHAIN_DP families
def _pad(anchors, n_pad):
    """n_pad anchors of a clean diagonal on another target in front: the list takes the n > 64 forms, the windows stay the same"""
    return diag(0, 0, 100, 100, n_pad, 20) + anchors


def mixture(rnd, n, rid=1, n_diag=None, span=15, n_seg=1, both_strands=True, noise=0.3, qmax=60000, rmax=60000):
    """n anchors: a few diagonals with jitter and gaps, plus noise"""
    out = []
    n_noise = int(n * noise * rnd.random())
    n_d = n_diag or rnd.randint(1, 4)
    left = n - n_noise
    for d in range(n_d):
        m = left if d == n_d - 1 else rnd.randint(0, left)
        left -= m
        strand = rnd.randint(0, 1) if both_strands else 0
        r0, q0 = rnd.randrange(1000, rmax // 2), rnd.randrange(100, qmax // 2)
        step = rnd.choice((3, 7, 15, 20, 40))
        r, q = r0, q0
        for _ in range(m):
            seg = 0 if n_seg == 1 else int(q > qmax // 3)
            out.append(mk(strand, rid, r, q, span, seg))
            s = step + rnd.choice((0, 0, 0, 1, -1, 5, 60))
            r += max(s, 1) + rnd.choice((0, 0, 0, 0, 2, 30))
            q += max(s, 1)
            if r >= rmax or q >= qmax:
                r, q = r0 + rnd.randrange(50), q0 + rnd.randrange(50)
    for _ in range(n - len(out)):
        out.append(mk(rnd.randint(0, 1) if both_strands else 0, rid, rnd.randrange(1000, rmax), rnd.randrange(100, qmax), span,
                      0 if n_seg == 1 else rnd.randint(0, 1)))
    return as_list(out)


def dp_families(P0):
    """P0: the preset's parameters in force (no overrides)"""
    bw, gap = int(P0["bw"]), int(P0["max_gap"])
    rnd = random.Random(77)
    fams = []
    NS = (2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 257)
    wide = dict(max_dist_x=6000, max_dist_y=6000)

    # colinear: one clean diagonal, both strands, one and two segments; min_cnt on either side of n
    for n_seg in (1, 2):
        ls = []
        for n in (1,) + NS:
            d = diag(n & 1, 1, 1000, 100, n, 20)
            if n_seg == 2:
                d = [(ax, ay | (int(k >= n // 2) << SEG_SHIFT)) for k, (ax, ay) in enumerate(d)]
            ls.append(as_list(d))
        fams.append(Family("colinear_seg%d" % n_seg, "CHAIN_DP", ls, dict(wide), n_segs=n_seg))
    for n in (3, 64, 65, 129):
        fams.append(Family("colinear_min_cnt%d" % n, "CHAIN_DP", [as_list(diag(m & 1, 1, 1000, 100, m, 20)) for m in (n - 1, n, n + 1)], dict(wide, min_cnt=n)))

    # windows: anchors every 10 bases, max_dist_x = 10 W + 5: the predecessor window i - st is exactly W from anchor W on
    for W in (63, 64, 65, 128, 129):
        for skip in (100000, None):
            par = dict(max_dist_x=10 * W + 5, max_dist_y=10 * W + 5)
            if skip:
                par["max_chain_skip"] = skip
            fams.append(Family("window%d%s" % (W, "" if skip else "_skip"), "CHAIN_DP",
                               [as_list(diag(s, 1, 1000, 100, W + 40, 10)) for s in (0, 1)] + [mixture(rnd, W + 60, n_diag=2, both_strands=False, rmax=3000, qmax=3000)], par))

    # iter clamp: 300 anchors all in range
    for it in (64, 65, 70):
        for skip in (100000, None):
            par = dict(wide, max_chain_iter=it, bw=300)
            if skip:
                par["max_chain_skip"] = skip
            # (the last list: a chain A, then 150 anchors that are predecessors of nothing but successors of A's last anchor -- once the
            #  clamp has moved st past it, max_ii still names it: max_ii lies BEFORE st, and only the rescue chains them to it)
            lone = diag(0, 1, 1000, 100, 20, 20) + [mk(0, 1, 1400 + k, 800) for k in range(150)]
            fams.append(Family("iter_clamp%d%s" % (it, "" if skip else "_skip"), "CHAIN_DP",
                               [as_list(diag(0, 1, 1000, 100, 300, 5)), as_list(diag(1, 1, 1000, 100, 300, 7, qstep=6)),
                                mixture(rnd, 300, n_diag=3, both_strands=False, rmax=3000, qmax=3000), as_list(lone)], par))

    # skip break: a long diagonal A, a run of a second diagonal B 50 off it (entered from A at a penalty, one base per anchor: it never
    # scores above A's last anchor), A again -- B's run ends the scan before it reaches A's last anchor, which max_ii then supplies;
    # and interleaved diagonals with noise
    for skip in (1, 2, None):
        ls = []
        for run in (5, 28):
            for lead in (10, 60):
                a1 = diag(0, 1, 1000, 100, lead, 20)
                bx = 1000 + 20 * lead
                b = [mk(0, 1, bx + k, bx + k - 900 - 50) for k in range(run)]
                ax = bx + run + 40
                ls.append(as_list(a1 + b + diag(0, 1, ax, ax - 900, 10, 20)))
        for _ in range(30):
            n_d, m = rnd.randint(2, 3), rnd.randint(20, 90)
            an = []
            for d in range(n_d):
                an += [mk(0, 1, 2000 + 6 * k + 2 * d + rnd.choice((0, 0, 1)), 1000 + 6 * k + 30 * d) for k in range(m)]
            an += [mk(0, 1, rnd.randrange(2000, 2000 + 6 * m), rnd.randrange(900, 1200 + 6 * m)) for _ in range(rnd.randint(0, 20))]
            ls.append(as_list(an))
        par = dict(max_dist_x=2000, max_dist_y=2000, bw=100, chn_pen_gap=1.0)
        if skip:
            par["max_chain_skip"] = skip
        fams.append(Family("skip_break%s" % (skip or "_preset"), "CHAIN_DP", ls, par))

    # far marks: i visits j1, whose predecessor j0 lies 71 anchors back (the fillers between them are on a far diagonal: rejected
    # before they leave a mark); j0 is then visited marked and not better, and with max_chain_skip = 0 the scan ends before it reaches
    # the chain P that would have been best.  H keeps max_ii on an anchor that is no predecessor of i, so nothing rescues P.
    ls = []
    for n_fill in (62, 63, 64, 70, 130):
        H = [mk(0, 1, 100 + 20 * k, 3100 + 20 * k) for k in range(15)]
        Pc = diag(0, 1, 1000, 1500, 5, 20)
        j0 = mk(0, 1, 1100, 990)
        fill = [mk(0, 1, 1101 + m, 7101 + 2 * m) for m in range(n_fill)]
        j1 = mk(0, 1, 1102 + n_fill + 5, 990 + n_fill + 7)
        ai = mk(0, 1, 1102 + n_fill + 40, 1102 + n_fill + 40 + 500)
        ls.append(as_list(H + Pc + [j0] + fill + [j1, ai]))
    fams.append(Family("far_marks", "CHAIN_DP", ls, dict(max_dist_x=5000, max_dist_y=5000, bw=1000, chn_pen_gap=0.01, max_chain_skip=0, min_cnt=1,
                                                         min_chain_score=10)))

    # strand change: a forward block, then a reverse block
    ls = []
    for nf, nr in ((10, 10), (30, 34), (40, 40), (100, 100), (3, 70)):
        ls.append(as_list(diag(0, 1, 1000, 100, nf, 20) + diag(1, 1, 900, 150, nr, 20)))
        ls.append(as_list(diag(0, 1, 5000, 100, nf, 20) + diag(1, 1, 900, 150, nr, 20)))
    fams.append(Family("strand_change", "CHAIN_DP", ls, dict(wide)))

    # score edges: a lead of three anchors, then T at (dr, dq) from the last of them, every pair of the edge values; then a follower
    for n_seg in (1, 2):
        for span in (15, 255):
            mdy = gap
            vals = sorted({0, 1, span - 1, span, span + 1, bw - 1, bw, bw + 1, mdy - 1, mdy, mdy + 1, mdy + bw, mdy + bw + 1})
            ls = []
            for pad in (0, 70):
                for dr in vals:
                    for dq in [-5] + vals:
                        for tseg in range(n_seg):
                            lead = diag(0, 1, 1000, 20000, 3, 20, span)
                            T = mk(0, 1, 1040 + dr, 20040 + dq, span, tseg)
                            fol = mk(0, 1, 1040 + dr + 12, 20040 + dq + 12, span, tseg)
                            ls.append(as_list(_pad(lead + [T, fol], pad)))
            fams.append(Family("score_edges_seg%d_span%d" % (n_seg, span), "CHAIN_DP", ls, dict(max_dist_x=gap + 2 * bw, max_dist_y=mdy, min_cnt=1, min_chain_score=10),
                               n_segs=n_seg))

    # positions at the top of the packed cells' 16 bits; a read-length sum the packed cells cannot hold
    for n_seg in (1, 2):
        ls, ql, ex = [], [], []
        for n in (10, 64, 65, 200):
            d = as_list(diag(0, 1, 1000, 65535 - 20 * (n - 1), n, 20, seg=n_seg - 1))
            for q, e in (((65535, 0) if n_seg == 1 else (32767, 32768), "equal"), ((65536, 0) if n_seg == 1 else (32768, 32768), "unsupported")):
                ls.append(d); ql.append(q); ex.append(e)
        fams.append(Family("qlen_sum_seg%d" % n_seg, "CHAIN_DP", ls, dict(wide), n_segs=n_seg, qlen=ql, expect=ex))

    # backtrack
    ls = []
    for trunk, pad in ((10, 0), (10, 70), (40, 0)):          # three diagonals that share a trunk
        an = diag(0, 1, 1000, 100, trunk, 20)
        ex_, eq = 1000 + 20 * trunk, 100 + 20 * trunk
        for d, m in ((0, 12), (6, 9), (-6, 7)):
            an += [mk(0, 1, ex_ + 20 * k + (d if d > 0 else 0), eq + 20 * k + (-d if d < 0 else 0)) for k in range(m)]
        ls.append(as_list(_pad(an, pad)))
    fams.append(Family("bt_shared_trunk", "CHAIN_DP", ls, dict(wide)))
    ls = []
    for pad in (0, 70):                                       # a dip of more than max_drop = bw = 30 inside a chain
        for na, nb in ((20, 3), (20, 8), (5, 3)):
            an = diag(0, 1, 1000, 100, na, 20)
            jx = 1000 + 20 * na
            an += [mk(0, 1, jx + 25 + 20 * k, 100 + 20 * na + 20 * k) for k in range(nb + 1)]
            ls.append(as_list(_pad(an, pad)))
    # ... and a dip of exactly max_drop, which does not cut (J is 35 / 14 bases on: min(span, 14) - (int)(2 * 21 + log2(22) / 2) = -30)
    for pad, na in ((0, 10), (70, 10), (0, 70), (0, 130)):
        an = diag(0, 1, 1000, 100, na, 20)
        jx, jq = 1000 + 20 * (na - 1) + 35, 100 + 20 * (na - 1) + 14
        an += [mk(0, 1, jx + 20 * k, jq + 20 * k) for k in range(4)]
        ls.append(as_list(_pad(an, pad)))
    fams.append(Family("bt_max_drop", "CHAIN_DP", ls, dict(wide, bw=30, chn_pen_gap=2.0)))
    # every f below min_chain_score
    fams.append(Family("bt_none", "CHAIN_DP", [as_list(diag(0, 1, 1000, 100, n, 400)) for n in (1, 5, 64, 65, 100)], dict(wide, min_chain_score=10000)))
    # 64, 65 and 129 used chain ends in a row before a free one: one chain of L anchors, then a pair scoring 27
    ls = []
    for run in (20, 62, 63, 64, 65, 128, 129, 130):
        ls.append(as_list(diag(0, 1, 1000, 100, run + 2, 20) + diag(0, 2, 1000, 100, 2, 12)))
    fams.append(Family("bt_used_run", "CHAIN_DP", ls, dict(wide, min_cnt=2, min_chain_score=25)))
    # more accepted chains than u[] holds (caps.max_reg * 4: 128 on the wave layouts, 20 on the thread-per-pair layout)
    ls = [as_list([a for c in range(nc) for a in diag(c & 1, 1 + c, 1000, 100, 2, 20)]) for nc in (19, 20, 21, 30, 127, 128, 129, 140)]
    fams.append(Family("bt_many_chains", "CHAIN_DP", ls, dict(wide, min_cnt=2, min_chain_score=25)))
    return fams


def dp_selected_families(P0, find):
    """random mixtures kept for the backtrack events they show under the reference's rules (find(fam) -> per-list event counts):
    walks that run into a used anchor, into one a REJECTED chain marked, chains cut by max_drop, tied chain-end scores"""
    rnd = random.Random(4242)
    out = []
    for name, par, key in (("bt_hit_used", dict(max_dist_x=6000, max_dist_y=6000), "hit_used"),
                           ("bt_rejected_marks", dict(max_dist_x=6000, max_dist_y=6000, min_cnt=6), "rejected_marking"),
                           ("bt_drop_cut", dict(max_dist_x=6000, max_dist_y=6000, bw=30, chn_pen_gap=1.5), "drop_cuts"),
                           ("bt_end_ties", dict(max_dist_x=6000, max_dist_y=6000), "end_ties")):
        cand = Family(name, "CHAIN_DP", [mixture(rnd, rnd.choice((30, 60, 64, 65, 90, 150)), n_diag=rnd.randint(2, 4), both_strands=False, rmax=4000, qmax=4000)
                                         for _ in range(120)], par)
        evs = find(cand)
        keep = [i for i, e in enumerate(evs) if e[key] > 0][:24]
        out.append(Family(name, "CHAIN_DP", [cand.lists[i] for i in keep], par))
    return out


def dp_random_family(n_seg=1):
    rnd = random.Random(1000 + n_seg)
    return Family("random_seg%d" % n_seg, "CHAIN_DP", [mixture(rnd, rnd.randint(1, 600), n_seg=n_seg) for _ in range(300)], n_segs=n_seg,
                  params=dict(max_dist_x=5000, max_dist_y=5000))


# ----------------------------------------------------------------------------------------- CHAIN_RMQ families
def rmq_inner_off(P0):
    return max(int(P0["max_gap"]), int(P0["bw_long"]))


def rmq_inner_on(P0):
    return min(1000, rmq_inner_off(P0) // 2)


def rmq_families(P0):
    max_gap = int(P0["max_gap"])
    rnd = random.Random(99)
    fams = []

    def gapped(n, strand=0, rid=1, r0=1000, q0=100):
        an, r, q = [], r0, q0
        for k in range(n):
            an.append(mk(strand, rid, r, q))
            g = rnd.choice((20, 20, 20, 35, 300, 2500))
            r += g + rnd.choice((0, 0, 3, 200))
            q += g
            if q > 60000 or r > 2000000000:
                break
        return an

    fams.append(Family("rmq_sizes", "CHAIN_RMQ", [as_list(diag(0, 1, 1000, 100, n, 23)) for n in (1, 2, 64, 65)] +
                       [as_list([mk(0, 1, 1000 + 29 * k + rnd.choice((0, 0, 7)), 100 + 29 * k) for k in range(n)]) for n in (300, 2000)]))
    # runs of equal x (an anchor enters the trees only once the position moves on)
    ls = []
    for n in (30, 64, 65, 200):
        an = []
        for k in range(n // 4):
            for m in range(rnd.choice((1, 2, 4, 7))):
                an.append(mk(0, 1, 1000 + 40 * k, 100 + 40 * k + 3 * m))
        ls.append(as_list(an))
    fams.append(Family("rmq_equal_x", "CHAIN_RMQ", ls))
    # identical disjoint sub-chains mirrored about an anti-diagonal: equal f and equal x + y, hence equal priorities in the tree
    ls = []
    for m, D in ((5, 200), (20, 600), (40, 30), (70, 1000)):
        an = []
        for c in range(3):
            an += [mk(0, 1, 5000 + c * D + 20 * k, 5000 - c * D + 20 * k) for k in range(m)]
        an += [mk(0, 1, 5000 + 3 * D + 20 * m + 500 + 10 * k, 5000 + 20 * m + 500 + 10 * k) for k in range(6)]
        ls.append(as_list(an))
    fams.append(Family("rmq_priority_ties", "CHAIN_RMQ", ls))
    # spans beyond max_dist: one node or many nodes leave the tree per step
    ls = [as_list(diag(0, 1, 1000, 100, 40, 20) + diag(0, 1, 1000 + 40 * 20 + rmq_inner_off(P0) + 100, 1000, 40, 20)),
          as_list([mk(0, 1, 1000 + (rmq_inner_off(P0) // 3) * k, 100 + 50 * k) for k in range(100)]),
          as_list(gapped(150)), as_list(gapped(400))]
    fams.append(Family("rmq_beyond_max_dist", "CHAIN_RMQ", ls))
    # a strand (and target) change empties the tree
    ls = [as_list(diag(0, 1, 1000, 100, nf, 20) + diag(1, 1, 900, 150, nr, 20) + diag(1, 2, 900, 150, 10, 20)) for nf, nr in ((10, 10), (40, 40), (64, 1), (100, 100))]
    fams.append(Family("rmq_strand_change", "CHAIN_RMQ", ls))
    dense = [as_list([mk(0, 1, 1000 + 9 * k + rnd.choice((0, 0, 4)), 100 + 9 * k + rnd.choice((0, 0, 0, 150))) for k in range(n)]) for n in (40, 64, 65, 300)]
    dense += [mixture(rnd, n, n_diag=3, both_strands=False, rmax=6000, qmax=6000) for n in (100, 300)]
    # (a chain, 100 anchors that precede nothing at 25 positions, the chain again 40 bases on: its best predecessor is 101 anchors back)
    dense.append(as_list(diag(0, 1, 1000, 100, 20, 20) + [mk(0, 1, 1381 + k // 4, 30000 + 3 * k) for k in range(100)] + diag(0, 1, 1420, 520, 20, 20)))
    # interleaved diagonals (the skip-break lists of the fill): candidates of the inner loop that are marked and no better
    inter = []
    for _ in range(12):
        n_d, m = rnd.randint(2, 3), rnd.randint(20, 90)
        an = []
        for d in range(n_d):
            an += [mk(0, 1, 2000 + 6 * k + 2 * d + rnd.choice((0, 0, 1)), 1000 + 6 * k + 30 * d) for k in range(m)]
        inter.append(as_list(an))
    inter += [mixture(rnd, 200, n_diag=3, both_strands=False, rmax=3000, qmax=3000) for _ in range(12)]
    for cap in (8, 64):
        fams.append(Family("rmq_size_cap%d" % cap, "CHAIN_RMQ", dense, dict(rmq_size_cap=cap)))
    # the inner tree: off at 0, on below max(max_gap, bw_long) (mg_lchain_rmq raises max_dist to the bandwidth), off again from there on
    for inner in sorted({0, rmq_inner_on(P0), 1000, max_gap, rmq_inner_off(P0)}):
        fams.append(Family("rmq_inner%d" % inner, "CHAIN_RMQ", dense + inter, dict(rmq_inner_dist=inner)))
    fams.append(Family("rmq_skip1", "CHAIN_RMQ", dense + inter, dict(max_chain_skip=1, rmq_inner_dist=rmq_inner_on(P0))))
    fams.append(Family("rmq_random", "CHAIN_RMQ", [mixture(rnd, rnd.randint(1, 400), both_strands=True) for _ in range(200)]))
    # more anchors than the 16-bit links of the trees hold: no layout of the tests admits the list, so it is not served
    big = as_list(diag(0, 1, 1000, 100, 65534, 1))
    fams.append(Family("rmq_64k", "CHAIN_RMQ", [big]))
    return fams


def rmq_input(fam: Family, P):
    """what map_frag feeds chain_rmq: the anchors mg_lchain_dp keeps, sorted by x again (map.c:289-290)"""
    ls = []
    for x, y in fam.lists:
        cx, cy, _ = orc.ref_lchain_dp(x, y, int(P["max_gap"]), int(P["max_gap"]), int(P["bw"]), int(P["max_chain_skip"]), int(P["max_chain_iter"]),
                                      int(P["min_cnt"]), int(P["min_chain_score"]), float(P["chn_pen_gap"]), float(P["chn_pen_skip"]), 1)
        ls.append(orc.ref_radix_sort_128x(cx, cy))
    return dataclasses.replace(fam, name=fam.name + "_chained", lists=ls)


# ----------------------------------------------------------------------------------------- every family of a preset, once
_families = {}


def families(preset, restate=False):
    """{name:op -> (family, parameters in force, the reference's answers, the restatement's or None)} of PRESETS[preset]; computed
    once and shared by the tests (restate: mg_lchain_dp in Python on every CHAIN_DP list as well -- tens of seconds)"""
    ent = _families.get(preset)
    if ent is None:
        mean = PRESETS[preset]
        P0 = preset_params(mean, {})
        ent = {}

        def add(fam):
            P = preset_params(mean, fam.params)
            ent[fam.name + ":" + fam.op] = [fam, P, reference(fam, P), None]

        for op in ("SORT128", "SORT64"):
            for fam in sort_families(op):
                add(fam)
        for fam in dp_families(P0):
            add(fam)
        for fam in dp_selected_families(P0, lambda f: [py_lchain_dp(x, y, preset_params(mean, f.params))["ev"] for x, y in f.lists]):
            add(fam)
        for n_seg in (1, 2):
            add(dp_random_family(n_seg))
        for fam in rmq_families(P0):
            add(fam)
            if fam.name in ("rmq_random", "rmq_beyond_max_dist"):
                add(rmq_input(fam, P0))
        _families[preset] = ent
    if restate:
        for e in ent.values():
            if e[0].op == "CHAIN_DP" and e[3] is None:
                e[3] = [py_lchain_dp(x, y, e[1]) for x, y in e[0].lists]
    return ent
