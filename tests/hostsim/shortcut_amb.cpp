// CPU build of the DP shortcuts (panmap_amd/csrc/align/aln_ksw.hpp, PMX_W = 1) for the property check of their
// closed forms over ambiguous bases (tests/test_shortcut_ambiguous_host.py).  TEST INFRASTRUCTURE: never linked into
// libpanmap_amd.so.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align/aln_host.hpp"

using namespace pmx::aln;

static uint64_t am_state;
static inline uint32_t am_rand() {
    am_state ^= am_state << 13; am_state ^= am_state >> 7; am_state ^= am_state << 17;
    return (uint32_t)(am_state >> 11);
}

// Random extension / gap-fill problems rich in ambiguous bases: runs of 1-40 N on the query only, the target only or
// both at the same positions, at the start, the middle or the end, with 0-3 substitutions, small alphabets and tandem
// repeats; right and left extensions (the left ones with right-aligned gaps), gap fills with left- and right-aligned
// gaps.  Whenever ksw_shortcut answers, ksw_extd2 must give the same fields: zdropped, the CIGAR, the score of a fill;
// max, max_t, max_q, mqe, mqe_t, reach_end of an extension, and mte, mte_q when the target is as long as the query.
// counts: [0] declined, [1] agreed, [2] disagreed, [3] agreed on a problem with an ambiguous base.
extern "C" int hs_amb_shortcut_fuzz(uint64_t seed, int64_t n_cases, int64_t* counts, int verbose) {
    am_state = seed * 0x9E3779B97F4A7C15ULL + 1;
    Opt o = make_opt(150);
    gen_simple_mat(o.mat, (int8_t)o.a, (int8_t)o.b, (int8_t)o.sc_ambi);
    Layout L = plan_layout(256, 2, o, (size_t)1 << 30);
    std::vector<uint8_t> fast(L.fast_bytes + 64), slow(L.slow_bytes + 64);
    Work W;
    memset(&W, 0, sizeof(W));
    bind_work(W, L, fast.data(), slow.data());
    std::vector<uint32_t> cig1(256);
    for (int i = 0; i < 4; ++i) counts[i] = 0;
    uint8_t q[256], t[256];
    for (int64_t it = 0; it < n_cases; ++it) {
        const int mode = (int)(am_rand() % 4);   // 0 right extension, 1 left extension, 2 / 3 gap fill with left- / right-aligned gaps
        // every other problem sits at the bounds' edges: homopolymer runs or a period-1..3 tandem (where a one-base gap costs
        // nothing but its penalty), a real mismatch and short N runs next to each other near the query end, a one-base
        // indel there (the inserted base often an N), an N at the query's last position, and as often as not a target no
        // longer than the query
        const bool edge = (am_rand() & 1) != 0;
        const int alpha = 2 + (int)(am_rand() % 3);
        const int qlen = edge ? 6 + (int)(am_rand() % 60) : 3 + (int)(am_rand() % 150);
        const int period = edge ? 1 + (int)(am_rand() % 3) : (am_rand() & 3) == 0 ? 1 + (int)(am_rand() % 6) : 0;
        const int tlen = mode >= 2 || (edge && (am_rand() & 1)) ? qlen : qlen + (int)(am_rand() % (edge ? 4 : 40));
        const bool runs = edge && (am_rand() & 1);   // homopolymer runs of 1-6 bases instead of a tandem
        for (int i = 0; i < tlen; ++i) {
            if (runs) t[i] = (uint8_t)(i > 0 && am_rand() % 6 != 0 ? t[i - 1] : am_rand() % alpha);
            else t[i] = (uint8_t)(period && i >= period ? t[i - period] : am_rand() % alpha);
        }
        for (int i = 0; i < qlen; ++i) q[i] = t[i];
        if (edge) {
            const int p = qlen - 1 - (int)(am_rand() % (qlen < 8 ? qlen : 8));   // near the query end
            const int indel = (int)(am_rand() % 4);   // a one-base indel at p: none, a base (N half the time) inserted into
            const uint8_t ins = (am_rand() & 1) ? 4 : (uint8_t)(am_rand() % alpha);   // the query / the target, a query base deleted
            if (indel == 1) { for (int i = qlen - 1; i > p; --i) q[i] = q[i - 1]; q[p] = ins; }
            else if (indel == 2) { for (int i = tlen - 1; i > p; --i) t[i] = t[i - 1]; t[p] = ins; }
            else if (indel == 3) { for (int i = p; i < qlen - 1; ++i) q[i] = q[i + 1]; q[qlen - 1] = tlen > qlen ? t[qlen] : (uint8_t)(am_rand() % alpha); }
            if (am_rand() & 1) {   // an N at the query's last position, on either side or both
                const int side = (int)(am_rand() % 3);
                if (side != 1) q[qlen - 1] = 4;
                if (side != 0) t[qlen - 1] = 4;
            }
            const int n_mut = (int)(am_rand() % 3);
            for (int m = 0; m < n_mut; ++m) {
                const int pm = p - (int)(am_rand() % 4);
                if (pm >= 0) q[pm] = (uint8_t)((q[pm] + 1 + am_rand() % 3) % 4);
            }
            const int n_runs = 1 + (int)(am_rand() % 2);
            for (int k = 0; k < n_runs; ++k) {
                const int len = 1 + (int)(am_rand() % 4);
                int at = p - 3 + (int)(am_rand() % 7);
                if (at < 0) at = 0;
                const int side = (int)(am_rand() % 3);
                for (int i = at; i < at + len && i < qlen; ++i) {
                    if (side != 1) q[i] = 4;
                    if (side != 0) t[i] = 4;
                }
            }
        }
        const int n_mut = edge ? 0 : (int)(am_rand() % 4);
        for (int m = 0; m < n_mut; ++m) {
            const int p = (int)(am_rand() % qlen);
            q[p] = (uint8_t)((q[p] + 1 + am_rand() % 3) % 4);
        }
        const int n_runs = edge ? 0 : 1 + (int)(am_rand() % 3);
        for (int k = 0; k < n_runs; ++k) {
            const int len = 1 + (int)(am_rand() % 40);
            const int where = (int)(am_rand() % 3);   // start, middle, end (of the query)
            int at = where == 0 ? 0 : where == 2 ? qlen - len : (int)(am_rand() % qlen);
            if (at < 0) at = 0;
            const int side = (int)(am_rand() % 3);   // query only, target only, both
            for (int i = at; i < at + len && i < tlen; ++i) {
                if (side != 1 && i < qlen) q[i] = 4;
                if (side != 0) t[i] = 4;
            }
        }
        bool has_amb = false;
        for (int i = 0; i < qlen; ++i) has_amb = has_amb || q[i] > 3 || t[i] > 3;
        const int flag = mode == 0 ? PMX_EZ_EXTZ_ONLY
                         : mode == 1 ? (PMX_EZ_EXTZ_ONLY | PMX_EZ_RIGHT | PMX_EZ_REV_CIGAR)
                         : mode == 2 ? PMX_EZ_APPROX_MAX : (PMX_EZ_APPROX_MAX | PMX_EZ_RIGHT);
        const int end_bonus = mode >= 2 ? -1 : o.end_bonus;
        const int w = (am_rand() & 1) ? -1 : (int)(o.bw * 1.5 + 1.);
        Ez e1, e2;
        W.status = 0;
        const bool took = ksw_shortcut(W, qlen, q, tlen, t, o.mat, (int8_t)o.q, (int8_t)o.e, (int8_t)o.q2, (int8_t)o.e2, w, o.zdrop, end_bonus, flag, e1);
        if (!took) { ++counts[0]; continue; }
        for (int i = 0; i < e1.n_cigar; ++i) cig1[(size_t)i] = W.cig_tmp[i];
        ksw_extd2(W, qlen, q, tlen, t, o.mat, (int8_t)o.q, (int8_t)o.e, (int8_t)o.q2, (int8_t)o.e2, w, o.zdrop, end_bonus, flag, e2);
        bool same = e1.zdropped == e2.zdropped && e1.n_cigar == e2.n_cigar;
        if (mode >= 2) same = same && e1.score == e2.score;
        else {
            same = same && e1.max == e2.max && e1.max_t == e2.max_t && e1.max_q == e2.max_q && e1.reach_end == e2.reach_end &&
                   e1.mqe == e2.mqe && e1.mqe_t == e2.mqe_t;
            if (tlen == qlen) same = same && e1.mte == e2.mte && e1.mte_q == e2.mte_q;
        }
        for (int i = 0; same && i < e1.n_cigar; ++i) same = cig1[(size_t)i] == W.cig_tmp[i];
        if (same) {
            ++counts[1];
            if (has_amb) ++counts[3];
        } else {
            if (verbose && counts[2] < 5) {
                fprintf(stderr, "shortcut mismatch mode=%d qlen=%d tlen=%d w=%d: max %u/%u max_t %d/%d max_q %d/%d reach %d/%d mqe %d/%d mqe_t %d/%d mte %d/%d score %d/%d ncig %d/%d\n  q=",
                        mode, qlen, tlen, w, e1.max, e2.max, e1.max_t, e2.max_t, e1.max_q, e2.max_q, e1.reach_end, e2.reach_end, e1.mqe, e2.mqe, e1.mqe_t,
                        e2.mqe_t, e1.mte, e2.mte, e1.score, e2.score, e1.n_cigar, e2.n_cigar);
                for (int i = 0; i < qlen; ++i) fputc("ACGTN"[q[i]], stderr);
                fprintf(stderr, "\n  t=");
                for (int i = 0; i < tlen; ++i) fputc("ACGTN"[t[i]], stderr);
                fputc('\n', stderr);
            }
            ++counts[2];
        }
    }
    return 0;
}

// Gap fills over N runs through the fill step of align1 (aln_align.hpp): the first pass (the shortcut when it answers,
// fill_zdrop_skip, test_zdrop unless skipped, the second pass after a Z-drop) against the same step with the shortcut
// off.  preset: 0 short reads (make_opt(150)), 1 long reads (make_opt(1000)).  Fills of real bases around an N run of
// 1..max_run bases on the query, the target or both, with 0-2 substitutions; the band of a plain fill or of a long join.
// counts: [0] fills the shortcut answered, [1] results that differ from the DP path, [2] skips whose test_zdrop would
// not have returned 0, [3] answered fills on which test_zdrop fired.
extern "C" int hs_amb_fill_zdrop(uint64_t seed, int64_t n_cases, int preset, int max_run, int64_t* counts, int verbose) {
    am_state = seed * 0x9E3779B97F4A7C15ULL + 7;
    Opt o = make_opt(preset ? 1000 : 150);
    gen_simple_mat(o.mat, (int8_t)o.a, (int8_t)o.b, (int8_t)o.sc_ambi);
    const int max_len = 2 * 80 + max_run;
    Layout L = plan_layout(max_len, 1, o, (size_t)1 << 31);
    std::vector<uint8_t> fast(L.fast_bytes + 64), slow(L.slow_bytes + 64);
    Work W;
    memset(&W, 0, sizeof(W));
    bind_work(W, L, fast.data(), slow.data());
    std::vector<uint32_t> cig_s((size_t)max_len * 2 + 8);
    std::vector<uint8_t> q((size_t)max_len), t((size_t)max_len);
    for (int i = 0; i < 4; ++i) counts[i] = 0;
    // the fill step of align1, with or without the shortcut; the final Ez and CIGAR land in ez / W.cig_tmp
    auto fill = [&](int n, int bw1, bool shortcut, Ez& ez) {
        W.status = 0;
        bool decided = false;
        if (shortcut) {
            FwdBases<ByteReader> qf{ByteReader(Ptr<const uint8_t>(q.data()))};
            FwdBases<ByteReader> tf{ByteReader(Ptr<const uint8_t>(t.data()))};
            decided = try_shortcut_direct(W, o, n, qf, n, tf, bw1, -1, o.zdrop, PMX_EZ_APPROX_MAX, ez);
        }
        if (!decided) {
            W.skip_shortcut = 1;
            align_pair(W, o, n, q.data(), n, t.data(), bw1, -1, o.zdrop, PMX_EZ_APPROX_MAX, ez);
            W.skip_shortcut = 0;
        }
        const bool skip = fill_zdrop_skip(W, o, n, ez);
        if (decided) {
            ++counts[0];
            const int code = test_zdrop(W, o, q.data(), t.data(), ez.n_cigar, W.cig_tmp);
            if (skip && code != 0) ++counts[2];
            if (code != 0) ++counts[3];
        }
        const int code = skip ? 0 : test_zdrop(W, o, q.data(), t.data(), ez.n_cigar, W.cig_tmp);
        if (code != 0) align_pair(W, o, n, q.data(), n, t.data(), bw1, -1, code == 2 ? o.zdrop_inv : o.zdrop, 0, ez);
        return decided;
    };
    for (int64_t it = 0; it < n_cases; ++it) {
        const int left = 1 + (int)(am_rand() % 80), right = 1 + (int)(am_rand() % 80), run = 1 + (int)(am_rand() % max_run);
        const int n = left + run + right;
        for (int i = 0; i < n; ++i) t[(size_t)i] = (uint8_t)(am_rand() % 4);
        for (int i = 0; i < n; ++i) q[(size_t)i] = t[(size_t)i];
        const int side = (int)(am_rand() % 3);   // query only, target only, both
        for (int i = left; i < left + run; ++i) {
            if (side != 1) q[(size_t)i] = 4;
            if (side != 0) t[(size_t)i] = 4;
        }
        const int n_mut = (int)(am_rand() % 3);
        for (int m = 0; m < n_mut; ++m) {
            const int p = (int)(am_rand() % n);
            if (q[(size_t)p] <= 3) q[(size_t)p] = (uint8_t)((q[(size_t)p] + 1 + am_rand() % 3) % 4);
        }
        const int bw1 = (am_rand() & 1) ? o.bw_long : n;   // the band of a fill, or of one closing a long join
        Ez e1, e2;
        if (!fill(n, bw1, true, e1)) continue;
        const int n1 = e1.n_cigar;
        for (int i = 0; i < n1; ++i) cig_s[(size_t)i] = W.cig_tmp[i];
        fill(n, bw1, false, e2);
        bool same = e1.zdropped == e2.zdropped && e1.n_cigar == e2.n_cigar;
        if (same && e1.zdropped) same = e1.max == e2.max && e1.max_t == e2.max_t && e1.max_q == e2.max_q;
        else if (same) same = e1.score == e2.score;
        for (int i = 0; same && i < n1; ++i) same = cig_s[(size_t)i] == W.cig_tmp[i];
        if (!same) {
            if (verbose && counts[1] < 5)
                fprintf(stderr, "fill mismatch preset=%d n=%d run=%d side=%d: zdropped %d/%d score %d/%d max_t %d/%d ncig %d/%d\n", preset, n, run, side,
                        e1.zdropped, e2.zdropped, e1.score, e2.score, e1.max_t, e2.max_t, e1.n_cigar, e2.n_cigar);
            ++counts[1];
        }
    }
    return 0;
}
