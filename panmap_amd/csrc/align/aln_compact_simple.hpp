// ALIGN stage, COMPACT tier: pairs whose mates do not overlap on the reference, chained from registers.
//
// compact_chain_pair (aln_compact.hpp) keeps a pair's anchors, chain cells and index lists in LDS because the general pair
// needs them: the heap's tie order where the mates share minimizers, a predecessor loop per anchor, a backtrack over
// arbitrary chains.  A pair whose mates lie apart on the reference needs none of that, and compact_chain_simple restates
// what compact_chain_pair computes for it from the pair's hand-over words (CSeedOutT) alone -- no CMemT block.  Every
// statement below is about compact_chain_pair; that function is the one proved against the reference.
//
// WHAT IS VERIFIED (anything else returns PMX_C_BAIL and the pair goes to the second form, which finishes a superset of
// the first form's pairs with the same records):
//   (a) both mates have a seed, at most PMX_C_CAP1 seeds together, no bit above TANDEM in a query word, SEG = the mate;
//   (b) every seed has one strand relation rel = (position word ^ query word) & 1 (all anchors forward, or all reverse);
//   (c) inside a mate, from one seed to the next (query order): 0 < dq <= run_lim and the reference position moves by
//       +dq (rel = 0) or -dq (rel = 1): one diagonal, no indel;
//   (d) the mates' position ranges are disjoint, and the mate that lies below on the reference (run A; the other: run B)
//       is also the one with the smaller query positions: mate 0 when rel = 0, mate 1 when rel = 1;
//   (e) use_tab (the tabulated gap penalties; the closed forms of the fill hold under it).
//
// SORT.  By (c) the position words of a mate are strictly monotone, by (d) no two words of the pair are equal: the heap
// of map.c:102-166 pops them in ascending order whatever its shape.  With (b) all anchors are on one strand, so anchor t
// of the pair is the t-th position in ascending order: run A's anchors 0 .. nA-1, then run B's nA .. n-1, each mate in
// seed order (rel = 0) or in reversed seed order (rel = 1; the anchor's query position is qlen_sum - (qp + 1 - k) - 1, which
// rises as qp falls).  In anchor order a run has dq = dr > 0 from one anchor to the next, the same numbers as in (c).
// The query positions of the two mates lie in disjoint intervals (mate 0 below qlen0 <= mate 1, mirrored for rel = 1), so
// with (d) every anchor of B lies above every anchor of A in x and in q.
//
// FILL, run A (anchors i = 0 .. nA-1).  Anchor 0: no predecessor, f = k, the loop does not run, so it is FULL and `above`
// (names of the comment in compact_chain_pair).  Anchor i >= 1: `extends` holds by (c) and (e) (st <= i - 1 because
// x_i - x_{i-1} <= run_lim <= max_dist_x), and `dom` holds with i' = i - 1: dl_i = i - 1 >= st, the flag pair of the mate
// is FULL | above by induction (the closed form never sets `stop`; q rises strictly and x differs), d = dq, and the other
// mate has no anchor yet (o_hi = -1).  So f[i] = f[i-1] + min(dq, k), p[i] = i - 1, the loop is not entered, and, f rising
// strictly with steps of at most max_dist_x, max_ii = i after every anchor: the max_ii test cannot fire.
//
// FILL, an anchor i of B against the anchors j of A.  Write sc_i(j) = f[j] + comput_sc(i, j).  The pair (i, j) is of
// different mates, so comput_sc rejects it only for dq <= 0 (never, by (d)) or dq > max_dist_x, the loop reaches j only
// while dr <= max_dist_x (st), and the penalty depends on dd = |dr - dq| = |diagonal of B - diagonal of A|: ONE number pen
// for all (i, j); dr > 0, so the dr == 0 case of mates never arises.  Hence sc_i(j) = f[j] + min(dg, k) - pen with
// dg = min(dr, dq).
//   (1) Down run A, from j to j - 1 with step d: dq, dr and therefore dg grow by d and f falls by min(d, k);
//       min(dg + d, k) <= min(dg, k) + min(d, k), so sc_i(j - 1) <= sc_i(j).  The anchors the loop can reach and score are
//       a top segment of A (both limits only get worse downwards) and the topmost, nA - 1, is the best of them.
//   (2) Up run B, from i - 1 to i with step d: seen from nA - 1, dq, dr and dg grow by d again, so
//       sc_i(nA - 1) <= sc_{i-1}(nA - 1) + min(d, k); and if nA - 1 is out of reach for i - 1 it is for i.
// Junction (i = nA): `extends` and `dom` fail (first anchor of its mate), the loop starts at nA - 1 with max_f = k.  If
// nA - 1 is within both limits and sc_nA(nA - 1) > k it is taken (f = that, p = nA - 1) and by (1) no lower anchor is
// better (`better` is strict), whatever marks, run skips and the max_skip break do below it; otherwise nothing is: f = k,
// p = none.  The max_ii test cannot fire: max_ii is nA - 1 >= end_j, or the rescan found nothing (st = nA).
// Run B (i > nA): `extends` holds as in run A, so max_f starts at f[i-1] + min(dq, k) with p = i - 1 -- in the `dom` form
// (no loop) or in the `extends` form, whose loop, and whose max_ii test after a break, can only score anchors of A or
// lower anchors of B.  By (2) and induction from f[nA] >= sc_nA(nA - 1), f[i-1] + min(dq, k) >= sc_i(nA - 1) >= sc_i(j)
// for every j of A; a lower anchor t of B is not better by the run inequality of compact_chain_pair's comment.  So
// f[i] = f[i-1] + min(dq, k), p[i] = i - 1 whether or not an earlier loop took the max_skip break.
// f rises along both runs, so "f outside 0 .. 1023" is a test of f[nA-1] and f[n-1].
//
// BACKTRACK.  Chain ends are taken by descending (f, index) among unused anchors with f >= min_sc; inside a run s rises
// with every step down (f falls), so keep == walk.  fA = f[nA-1], fB = f[n-1], fJ = f[nA].
//   * not linked (p[nA] = none): two chains, A (score fA, nA anchors) and B (fB, nB); an end under min_sc is never
//     picked, a picked end with fewer than min_cnt anchors is rejected.
//   * linked, followed only when fJ > fA (then the step from anchor nA to nA - 1 raises s too, and fB >= fJ > fA: B's
//     end is picked first): one chain of all n anchors with score fB.
//
// REGIONS.  Every mate's list lies on one diagonal, so mm_fix_bad_ends changes nothing (mx - mn = 0), the bad-seed count
// is 0, and c_align1 reads only the list's first and last anchor and whether it has more than one: it is called on a list
// of those two.  c_reg_set_coor's outputs are all overwritten by c_align1 and read by nothing before it but
// mm_fix_bad_ends' loops, which do not run here.  From there on (filter, mapq, pairing, record) the code is shared.
//
// RANGES, NOT EXTENTS.  (d) is about the mates' position ranges: the reference positions of their SEEDS.  The mates'
// extents -- where the reads themselves lie, each projected from its first seed -- may overlap: mates that overlap by at
// most k - 1 bases cannot share a k-mer, so they share no minimizer, and every seed of the lower mate still lies below
// every seed of the upper one; the same holds for a longer overlap as far as neither mate has a seed inside it.  No step
// above reads an extent:
//   * SORT needs the position words distinct and the runs in order: (c) and (d).
//   * FILL, across the mates: comput_sc on a pair of anchors of different mates tests dq and dr against 0 and max_dist_x
//     and nothing else.  dr > 0 by (d), dq > 0 because the mates' query intervals are disjoint whatever the reference
//     says; a dr below k (the runs' ends closer than a seed: the seeds themselves overlap on the reference) only makes
//     dg = min(dr, dq) small, and (1), (2) are statements about min(dg, k) for any dg > 0.  The penalty is the one number
//     pen for dd = |dr - dq|: with extents that overlap by v bases dr - dq = -v at every cross pair.
//   * the junction is c_chain_score_tab on those two anchors -- the function compact_chain_pair's fill calls; a chain
//     linked across overlapping extents is the chain the first form finds.
//   * REGIONS: one region per mate from its own run's two ends; c_align1's end extensions run along the mate's own
//     diagonal to the read's ends and take no notice of the other mate's region.  Pairing and the record are shared code.
//
// CLASSES.  Two sets of pairs come here, both on the simple list:
//   * marked by the seeding (compact_seed_pair's `simple`, PMX_C_NSEED_SIMPLE in the hand-over count): the extents lie
//     apart.  Extents are all the seeds kernel has in registers; its code does not change.
//   * the near class, decided in k_compact_classes_near16/32 (registers to spare) by compact_near_class below for a pair
//     without the mark: both mates have a seed, n <= PMX_C_CAP1, and the junction seeds -- mate 0's last, mate 1's first --
//     have one strand relation and lie in the order (d) implies for it: rel = 0: pos(seed n0 - 1) < pos(seed n0); rel = 1:
//     pos(seed n0) < pos(seed n0 - 1).  For a pair that satisfies (b) and (c) that IS (d), since each mate's positions are
//     monotone; for any other pair it is a guess, and the pass over the words finds (b), (c) violated and returns
//     PMX_C_BAIL.  A wrong class costs a detour through the second form, never a record.
//     Third condition: the junction's link gains, min(dg, k) > pen.  Junction seeds of overlapping extents lie a few bases
//     apart (dr small) while dd is the overlap, so the link often gains nothing: fJ <= fA, which BACKTRACK above does not
//     follow -- in the host model every bail of a near pair that the first form finishes was this one (4 % of the class).
// The kernel counts what it finishes of the two in separate counters (simple_chain_items, near_chain_items).
#pragma once
#include "aln_compact.hpp"

namespace pmx {
namespace aln {

// a region's first and last anchor as c_align1 reads a list (x: reference position, y: query position in the mate)
struct CEnds {
    int32_t x0, y0, xl, yl;
    PMX_HD int32_t x(int i) const { return i ? xl : x0; }
    PMX_HD int32_t y(int i) const { return i ? yl : y0; }
    PMX_HD uint32_t rev(int) const { return 0u; }   // (read by c_align1<MULTI>'s fence scan only, which this list never reaches)
};

// The near class (see CLASSES above): the junction seeds of a pair the seeding did not mark -- mate 0's last seed and mate
// 1's first, adjacent hand-over words -- have one strand relation, lie in the order (d) asks of them, and the link between
// them would raise the score.  `out`: the pair's hand-over words (CSeedOutT<PT>::out).  Not complete and not meant to be:
// compact_chain_simple checks (a) - (e) itself.
template <class PT>
PMX_HD bool compact_near_class(const c_g32* out, int n_s, int n_s0, const Opt& o) {
    const int n0 = n_s0, n1 = n_s - n_s0;
    if (n0 < 1 || n1 < 1 || n_s > PMX_C_CAP1) return false;
    uint32_t xa, ya, xb, yb;   // a: seed n0 - 1, b: seed n0
    if (sizeof(PT) == 2) {
        const uint32_t a = out[n0 - 1], b = out[n0];
        xa = a & 0xffffu; ya = a >> 16; xb = b & 0xffffu; yb = b >> 16;
    } else {
        xa = out[2 * n0 - 2]; ya = out[2 * n0 - 1]; xb = out[2 * n0]; yb = out[2 * n0 + 1];
    }
    const uint32_t rel = (xa ^ ya) & 1u;
    if (((xb ^ yb) & 1u) != rel) return false;
    // the junction as compact_chain_simple sees it: the anchors' dq is the seeds' on either strand (both query positions
    // are mirrored), dr their distance on the reference in the order of (d)
    const int32_t dr = rel ? (int32_t)(xa >> 1) - (int32_t)(xb >> 1) : (int32_t)(xb >> 1) - (int32_t)(xa >> 1);
    const int32_t dq = (int32_t)((yb & 0x3ffu) >> 1) - (int32_t)((ya & 0x3ffu) >> 1);
    if (dr <= 0 || dq <= 0) return false;
    // min(dg, k) - pen > 0 (comput_sc for anchors of different mates, the values the penalty table holds): with seeds this
    // close the link often gains nothing, and a linked junction with fJ <= fA is one the path does not follow
    const int32_t dd = dr > dq ? dr - dq : dq - dr, dg = dr < dq ? dr : dq;
    if (dd >= PMX_C_PEN_DIFF) return false;
    int ps, pd;
    c_pen_values(o.chn_pen_gap, dd, &ps, &pd);
    return (dg < o.k ? dg : o.k) > (pd < 255 ? pd : 255);
}

template <class PT>
PMX_HD int compact_chain_simple(const CSeedOutT<PT>& so, const Opt& o, const RefIndex& ri, const CRead* rd, int n_s, int n_s0, CResult& out,
                                 const CPenTab& pen_tab, bool want_edits = false) {
    out.mapped = 0;
    const int k = o.k;
    const int qlen0 = rd[0].len, qlen1 = rd[1].len, qlen_sum = qlen0 + qlen1;
    out.edit[0] = qlen0; out.edit[1] = qlen1;
    const int n0 = n_s0, n1 = n_s - n_s0;
    if (n0 < 1 || n1 < 1 || n_s > PMX_C_CAP1) return PMX_C_BAIL;   // (a)

    int max_chain_gap_ref;
    if (o.max_gap_ref > 0) max_chain_gap_ref = o.max_gap_ref;
    else if (o.max_frag_len > 0) {
        max_chain_gap_ref = o.max_frag_len - qlen_sum;
        if (max_chain_gap_ref < o.max_gap) max_chain_gap_ref = o.max_gap;
    } else max_chain_gap_ref = o.max_gap;
    const int bw = o.bw, min_cnt = o.min_cnt, min_sc = o.min_chain_score;
    int32_t max_dist_x = max_chain_gap_ref, max_dist_y = o.max_gap;
    if (max_dist_x < bw) max_dist_x = bw;
    if (max_dist_y < bw) max_dist_y = bw;
    const bool use_tab = pen_tab.same != nullptr && o.chn_pen_skip == 0.0f && bw < PMX_C_PEN_SAME && max_dist_x < PMX_C_PEN_DIFF;
    if (!use_tab) return PMX_C_BAIL;   // (e)
    const int32_t run_lim = max_dist_x < max_dist_y ? max_dist_x : max_dist_y;

    // ---------------------------------------------------------------- (a) - (c): one pass over the hand-over words
    // per mate: first and last seed (reference position, query position of the pair) and S = sum of min(dq, k)
    uint32_t rel = 0;
    int32_t r0f = 0, q0f = 0, r0l = 0, q0l = 0, S0 = 0;
    int32_t cf_r = 0, cf_q = 0, pr = 0, pq = 0, cS = 0;
    bool have = false, ok = true;
    for (int i0 = 0; i0 < n_s; i0 += 4) {
        uint32_t xw[4], yw[4];
        so.get4(i0, xw, yw);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int idx = i0 + b;
            if (idx >= n_s) continue;
            if (idx == n0) { r0f = cf_r; q0f = cf_q; r0l = pr; q0l = pq; S0 = cS; have = false; cS = 0; }
            const int32_t rp = (int32_t)(xw[b] >> 1), qp = (int32_t)((yw[b] & 0x3ffu) >> 1);
            const uint32_t r = (xw[b] ^ yw[b]) & 1u;
            if (idx == 0) rel = r;
            ok = ok && (yw[b] & ~0xfffu) == 0u && ((yw[b] >> 10) & 1u) == (idx >= n0 ? 1u : 0u) && r == rel;
            if (have) {
                const int32_t dq = qp - pq, dr = rp - pr;
                ok = ok && dq > 0 && dq <= run_lim && dr == (rel ? -dq : dq);
                cS += dq < k ? dq : k;
            } else { cf_r = rp; cf_q = qp; }
            pr = rp; pq = qp; have = true;
        }
    }
    if (!ok) return PMX_C_BAIL;
    const int32_t r1f = cf_r, q1f = cf_q, r1l = pr, q1l = pq, S1 = cS;
    // seeds -> anchors (to_anchor of compact_chain_pair); a mate's first anchor is its first seed (rel = 0) or its last
    const int32_t qmir = qlen_sum + k - 2;   // reverse: qlen_sum - (qp + 1 - k) - 1
    const int32_t x0a = rel ? r0l : r0f, y0a = rel ? qmir - q0l : q0f, x0z = rel ? r0f : r0l, y0z = rel ? qmir - q0f : q0l;
    const int32_t x1a = rel ? r1l : r1f, y1a = rel ? qmir - q1l : q1f, x1z = rel ? r1f : r1l, y1z = rel ? qmir - q1f : q1l;
    // ---------------------------------------------------------------- (d): run A below run B, in x and in q
    int mA;
    if (x0z < x1a) mA = 0;
    else if (x1z < x0a) mA = 1;
    else return PMX_C_BAIL;
    if (mA != (int)rel) return PMX_C_BAIL;
    const int nA = mA ? n1 : n0, nB = mA ? n0 : n1;
    const int32_t xA0 = mA ? x1a : x0a, yA0 = mA ? y1a : y0a, xAl = mA ? x1z : x0z, yAl = mA ? y1z : y0z;
    const int32_t xB0 = mA ? x0a : x1a, yB0 = mA ? y0a : y1a, xBl = mA ? x0z : x1z, yBl = mA ? y0z : y1z;
    const int32_t fA = k + (mA ? S1 : S0), SB = mA ? S0 : S1;

    // ---------------------------------------------------------------- the junction: anchor nA against anchor nA - 1
    int32_t fJ = k;
    bool linked = false;
    {
        const int32_t dq = yB0 - yAl, dr = xB0 - xAl;   // both > 0 by (d)
        if (dq <= max_dist_x && dr <= max_dist_x) {     // valid for comput_sc (mates: no other limit), and not below st
            const int32_t sc = fA + c_chain_score_tab(pen_tab, (uint32_t)xB0, yB0, 1 - mA, (uint32_t)xAl, yAl, mA, k, max_dist_x, max_dist_y, bw);
            if (sc > k) { fJ = sc; linked = true; }
        }
    }
    const int32_t fB = fJ + SB;
    if (fA > 1023 || fB > 1023) return PMX_C_BAIL;

    // ---------------------------------------------------------------- backtrack -> per mate: the chain's score
    int32_t scA, scB;
    if (!linked) {
        const bool okA = fA >= min_sc && nA >= min_cnt, okB = fB >= min_sc && nB >= min_cnt;
        if (!okA && !okB) return PMX_C_DONE;                           // no chain: unmapped
        if (!okA || !okB) return want_edits ? PMX_C_BAIL : PMX_C_DONE;   // a mate without a region: unmapped
        scA = fA; scB = fB;
    } else {
        if (fJ <= fA) return PMX_C_BAIL;
        if (fB < min_sc) return PMX_C_DONE;                            // nothing is picked
        if (nA + nB < min_cnt) return PMX_C_BAIL;
        scA = scB = fB;
    }

    // ---------------------------------------------------------------- one region per mate, aligned from its two ends
    CReg R0, R1;
    CEnds E0, E1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const bool isA = s == mA;
        CReg& r = s == 0 ? R0 : R1;
        CEnds& e = s == 0 ? E0 : E1;
        const int32_t shift = s == 0 ? (rel ? qlen_sum - qlen0 : 0) : (rel ? 0 : qlen0);   // hit.c:381
        e.x0 = isA ? xA0 : xB0; e.y0 = (isA ? yA0 : yB0) - shift;
        e.xl = isA ? xAl : xBl; e.yl = (isA ? yAl : yBl) - shift;
        r.cnt = isA ? nA : nB;
        r.score = isA ? scA : scB;
        r.rev = (int32_t)rel;
        r.has_p = 0; r.dp_score = r.dp_max = 0; r.mapq = 0; r.proper_frag = 0; r.m_len = 0;
        r.mlen = r.blen = 0;
    }
    {
        bool kept;
        const int32_t cnt0 = R0.cnt, cnt1 = R1.cnt;
        R0.cnt = cnt0 < 2 ? cnt0 : 2;
        if (c_align1(E0, o, ri, rd[0], qlen0, R0) != PMX_C_DONE) return PMX_C_BAIL;
        R0.cnt = cnt0;
        if (c_filter_mapq(o, ri, qlen0, R0, &kept) != PMX_C_DONE) return PMX_C_BAIL;
        if (!kept) return want_edits ? PMX_C_BAIL : PMX_C_DONE;
        R1.cnt = cnt1 < 2 ? cnt1 : 2;
        if (c_align1(E1, o, ri, rd[1], qlen1, R1) != PMX_C_DONE) return PMX_C_BAIL;
        R1.cnt = cnt1;
        if (c_filter_mapq(o, ri, qlen1, R1, &kept) != PMX_C_DONE) return PMX_C_BAIL;
        if (!kept) return want_edits ? PMX_C_BAIL : PMX_C_DONE;
    }
    c_pair_record(o, R0, R1, max_chain_gap_ref, out);
    return PMX_C_DONE;
}

}  // namespace aln
}  // namespace pmx
