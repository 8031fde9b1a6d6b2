"""Request families for the device DP kernels and their comparison with the reference DP (tests/test_dp_wave_gpu.py on the GPU,
tests/test_dp_families.py for the families themselves).  A family is a list of requests (query, target, w, zdrop, end_bonus, flag)
of nt4 codes; the reference side is ksw_extd2_sse / ksw_ll_i16 of the compiled reference through oracle.ref_ksw_extd2 /
oracle.ref_ksw_ll, computed once per (family, preset) and shared by every test of a session."""
import functools

import numpy as np

APPROX_MAX, EXTZ_ONLY, RIGHT, REV_CIGAR = 0x08, 0x40, 0x02, 0x80
KINDS = (APPROX_MAX, 0, EXTZ_ONLY, EXTZ_ONLY | RIGHT | REV_CIGAR)     # gap fill, its second pass after a Z-drop, right / left extension
FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "n_cigar", "reach_end")   # == test_dp_service_gpu.FIELDS
EXACT_BIT = 0x20     # PMX_DP_PATH_EXACT
SEQ_BYTES, REQ_MAX_CIGAR, SMALL_SIDE = 480, 20, 192     # a posted request's sequences / CIGAR operations; sides of the register class

# mean read length -> the DP scoring of the preset it selects (mm_mapopt_t: sr, map-ont, map-hifi); Aligner.scoring() must agree
PRESETS = {
    150: dict(a=2, b=8, q=12, e=2, q2=24, e2=1, sc_ambi=1, zdrop=100, zdrop_inv=100, end_bonus=10),
    3000: dict(a=2, b=4, q=4, e=2, q2=24, e2=1, sc_ambi=1, zdrop=400, zdrop_inv=200, end_bonus=-1),
    10000: dict(a=1, b=4, q=6, e=2, q2=26, e2=1, sc_ambi=1, zdrop=400, zdrop_inv=200, end_bonus=-1),
}


class Family:
    def __init__(self):
        self.q, self.t, self.w, self.z, self.eb, self.f, self.name = [], [], [], [], [], [], []

    def add(self, q, t, w, z, eb, f, name=None):
        self.q.append(q); self.t.append(t); self.w.append(int(w)); self.z.append(int(z)); self.eb.append(int(eb)); self.f.append(int(f))
        self.name.append(name)

    def __len__(self):
        return len(self.q)

    def describe(self, i):
        return dict(i=i, name=self.name[i], qlen=len(self.q[i]), tlen=len(self.t[i]), w=self.w[i], zdrop=self.z[i], end_bonus=self.eb[i],
                    flag=hex(self.f[i]), q=self.q[i] if len(self.q[i]) <= 64 else "...", t=self.t[i] if len(self.t[i]) <= 64 else "...")


def tb_bytes(qlen, tlen, w):
    """dp_request_tb_bytes (csrc/align_kernel.h): bytes of the traceback matrix, n_col as ksw2_extd2_sse.c:95-98"""
    if w < 0:
        w = max(qlen, tlen)
    return (qlen + tlen - 1) * (((min(qlen, tlen, w + 1) + 15) // 16 + 1) * 16)


def band_cuts(qlen, tlen, w):
    return 0 <= w < max(qlen, tlen) - 1


def _draws(rng, sc):
    return (int(rng.choice([-1, 20, 50, sc["zdrop"], sc["zdrop_inv"]])), int(rng.choice([-1, 0, 5, sc["end_bonus"], 40])))


def _related(rng, t, qlen, suffix):
    """the target's prefix or suffix at the query's length, <= 3 substitutions and one indel of 1-4 bases"""
    tl = len(t)
    if qlen <= tl:
        q = list(t[tl - qlen:] if suffix else t[:qlen])
    else:
        extra = [int(x) for x in rng.integers(0, 4, qlen - tl)]
        q = extra + list(t) if suffix else list(t) + extra
    for _ in range(int(rng.integers(0, 4))):
        p = int(rng.integers(0, len(q)))
        q[p] = (q[p] + 1 + int(rng.integers(0, 3))) % 4
    n, p = int(rng.integers(1, 5)), int(rng.integers(0, len(q)))
    if rng.random() < 0.5:
        q = q[:p] + [int(x) for x in rng.integers(0, 4, n)] + q[p:]
    elif len(q) > n:
        q = q[:p] + q[p + n:]
    q = q[:qlen]
    q += [int(x) for x in rng.integers(0, 4, qlen - len(q))]
    return q


def _table(rng, sc, tlens, qlens, bands, fits):
    fam = Family()
    for tl in tlens:
        t = [int(x) for x in rng.integers(0, 4, tl)]
        for ql in qlens:
            if not fits(ql, tl):
                continue
            L = max(ql, tl)
            ws = []
            for w in bands(ql, tl, L):
                if w >= -1 and w not in ws:
                    ws.append(w)
            for w in ws:
                for k, kind in enumerate(KINDS):
                    z, eb = _draws(rng, sc)
                    fam.add(_related(rng, t, ql, suffix=bool((k + w) & 1)), t, w, z, eb, kind)
    return fam


def fits_request(ql, tl):
    return ((ql + 15) & ~15) + tl <= SEQ_BYTES


def boundary_table(preset):
    """test 1: the NC 64/65 and 128/129 edges of the register kernel, the 192/193 class edge, bands from none to st > en, the 8 KB and
    12 KB traceback areas straddled; then the named regression cases"""
    sc, rng = PRESETS[preset], np.random.default_rng(1000 + preset)
    fam = _table(rng, sc, (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 300), (1, 16, 17, 64, 150, 192),
                 lambda ql, tl, L: (-1, L - 1, L - 2, 0, 1, 15, 16, 17, abs(ql - tl), abs(ql - tl) - 1, (ql + tl) // 4), fits_request)
    for ql, tl in ((51, 51), (52, 52), (30, 226), (30, 230)):       # 8,080 | 8,240 bytes (class 1: 8,192); 12,240 | 12,432 (class 2: 12,288)
        t = [int(x) for x in rng.integers(0, 4, tl)]
        for kind in KINDS:
            z, eb = _draws(rng, sc)
            fam.add(_related(rng, t, ql, False), t, -1, z, eb, kind, "tb_straddle_%dx%d" % (ql, tl))
    assert (tb_bytes(51, 51, -1), tb_bytes(52, 52, -1), tb_bytes(30, 226, -1), tb_bytes(30, 230, -1)) == (8080, 8240, 12240, 12432)
    return fam


def long_boundary_table(preset):
    """test 3: the SW 256/257, 512/513, 768/769 edges of the rows kernel, its tlen 1024/1025 limit, the dp_fast 608/609 limit"""
    sc, rng = PRESETS[preset], np.random.default_rng(3000 + preset)
    return _table(rng, sc, (255, 256, 257, 511, 512, 513, 607, 608, 609, 767, 768, 769, 1023, 1024, 1025, 1500), (1, 64, 300, 607, 608, 609, 1100),
                  lambda ql, tl, L: (-1, L - 1, L - 2, 500, 751), lambda ql, tl: True)


def _mutate(rng, seq, sub, indel):
    out = []
    for c in seq:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out += [c, int(rng.integers(0, 4))]
        elif r < indel + sub:
            out.append(int((c + 1 + rng.integers(0, 3)) % 4))
        else:
            out.append(int(c))
    return out or [0]


def _random(rng, sc, n, max_t, max_q, fits):
    fam = Family()
    i = 0
    while len(fam) < n:
        kind = KINDS[i % 4]
        mode = i % 6
        i += 1
        tl = int(rng.integers(1, max_t + 1))
        t = [int(x) for x in rng.integers(0, 4, tl)]
        if mode == 0:
            q = [int(x) for x in rng.integers(0, 4, int(rng.integers(1, max_q + 1)))]              # unrelated
        elif mode == 1:
            q = _mutate(rng, t, 0.25, 0.1)                                                         # diverged: Z-drops fire
        elif mode == 2:
            q = _mutate(rng, t, 0.02, 0.0)                                                         # one gap of 5-60 bases
            g, p = int(rng.integers(5, 61)), int(rng.integers(0, len(q)))
            q = q[:p] + q[p + g:] if rng.random() < 0.5 and len(q) > g + 1 else q[:p] + [int(x) for x in rng.integers(0, 4, g)] + q[p:]
        else:
            step = (i // 6) % 4                                                                    # a ladder of mild divergence
            q = _mutate(rng, t, 0.01 * (step + 1), 0.004 * step)
        if kind & EXTZ_ONLY and rng.random() < 0.5:
            q = q[:max(1, len(q) // 2)]                                                            # the target overhangs
        q = q[:max_q]
        if mode == 4 or rng.random() < 0.05:
            for _ in range(int(rng.integers(1, 4))):
                (q if rng.random() < 0.5 else t)[int(rng.integers(0, min(len(q), len(t))))] = 4    # the odd N
        if not fits(len(q), tl):
            continue
        L = max(len(q), tl)
        w = int(rng.integers(0, L)) if rng.random() < 0.5 else (-1 if rng.random() < 0.4 else L - 1 + int(rng.integers(0, 200)))
        z, eb = _draws(rng, sc)
        fam.add(q, t, w, z, eb, kind)
    return fam


def random_requests(preset):
    """test 2: ~3,000 requests with both sides <= 192 and ~1,500 with targets up to 440"""
    sc, rng = PRESETS[preset], np.random.default_rng(2000 + preset)
    a, b = _random(rng, sc, 3000, 192, 192, fits_request), _random(rng, sc, 1500, 440, 192, fits_request)
    for x in ("q", "t", "w", "z", "eb", "f", "name"):
        getattr(a, x).extend(getattr(b, x))
    return a


def long_random_requests(preset):
    """test 4: ~300 requests with tlen <= 1024, qlen <= 1100"""
    return _random(np.random.default_rng(4000 + preset), PRESETS[preset], 300, 1024, 1100, lambda ql, tl: True)


def sw_ll_shapes(preset):
    """test 5: (query, target) pairs; qlen around the 8-position stripes and the 64-lane steps of sw_ll"""
    rng, out = np.random.default_rng(5000 + preset), []
    for ql in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 500):
        for tl in (1, 2, 64, 500):
            base = [int(x) for x in rng.integers(0, 4, max(ql, tl))]
            for mode in range(4):
                t = base[:tl]
                q = base[:ql] if mode == 0 else (_mutate(rng, base, 0.1, 0.05) + base)[:ql] if mode == 1 else [int(x) for x in rng.integers(0, 4, ql)]
                if mode == 3:
                    q = list(base[:ql])
                    q[int(rng.integers(0, ql))] = 4
                    t = list(t)
                    t[int(rng.integers(0, tl))] = 4
                out.append((q, t))
    return out


FAMILIES = {"boundary_table": boundary_table, "random_requests": random_requests, "long_boundary_table": long_boundary_table,
            "long_random_requests": long_random_requests}


@functools.lru_cache(maxsize=None)
def family(name, preset):
    return FAMILIES[name](preset)


@functools.lru_cache(maxsize=None)
def reference(name, preset):
    """ksw_extd2_sse of the compiled reference on every request of the family: a tuple of dicts, never modified"""
    from oracle import oracle
    sc, fam = PRESETS[preset], family(name, preset)
    mat = oracle.simple_mat(sc["a"], sc["b"], sc["sc_ambi"])
    return tuple(oracle.ref_ksw_extd2(fam.q[i], fam.t[i], mat, sc["q"], sc["e"], sc["q2"], sc["e2"], fam.w[i], fam.z[i], fam.eb[i], fam.f[i])
                 for i in range(len(fam)))


def over_capacity(qlen, tlen, w, caps):
    """the request exceeds a capacity the entry point returned: a side, or the traceback matrix (ksw_extd2_t's own check; the area in LDS
    counts when the layout has one)"""
    t16 = (tlen + 15) // 16 * 16
    return (qlen > caps["max_qlen"] or tlen > caps["max_tlen"] or t16 > caps["max_tlen"] or qlen > caps["max_tlen"] or
            tb_bytes(qlen, tlen, w) > max(int(caps["tb_cap"]), int(caps["tb_fast_cap"])))


def compare(fam, want, got, arena, caps, small_class):
    """every served request equals the reference field by field and CIGAR by CIGAR; an unserved one exceeds a returned capacity: more
    CIGAR operations in the reference than max_cigar (20 on the request paths), a side, or the traceback matrix.  Nothing else may be
    unserved, in the tables and the random families alike.  small_class: the path has the register class (caps[1]), which takes
    sides up to 192 whose traceback fits its slab whatever caps[0] says.  -> (served, set of path_taken)"""
    max_cigar = int(caps[0]["max_cigar"])
    bad, refused, served, paths = [], [], 0, set()
    for i in range(len(fam)):
        g, r = got[i], want[i]
        ql, tl, w = len(fam.q[i]), len(fam.t[i]), fam.w[i]
        if not g["served"]:
            small = small_class and ql <= SMALL_SIDE and tl <= SMALL_SIDE and tb_bytes(ql, tl, w) <= int(caps[1]["tb_cap"])
            over = not small and over_capacity(ql, tl, w, caps[0])
            if not (over or r["n_cigar"] > max_cigar):
                refused.append((fam.describe(i), "reference n_cigar %d" % r["n_cigar"]))
            continue
        served += 1
        paths.add(int(g["path_taken"]))
        off, n = int(g["cigar_off"]), int(g["n_cigar"])
        diff = {f: (int(g[f]), r[f]) for f in FIELDS if int(g[f]) != r[f]}
        if diff or [int(x) for x in arena[off:off + n]] != r["cigar"]:
            bad.append((fam.describe(i), hex(int(g["path_taken"])), diff or "cigar", [int(x) for x in arena[off:off + n]][:8], r["cigar"][:8]))
    assert not bad, (len(bad), bad[:3])
    assert not refused, (len(refused), refused[:3])
    return served, paths
