// Device pileup of the genotype stage (gfx950).
//
// The reference forks `bcftools mpileup -Ou -B` on the BAM it wrote (src/conversion.cpp:83-128).  What that program hands to
// its error model at a position is a multiset of (base, strand, capped quality) -- nothing else of a read survives
// bcf_call_glfgen (src/3rdparty/bcftools/bam2bcf.c:248-573) -- so the pileup is kept as INTEGER counters per position:
//   hist[pos][q][strand][base]   the bases bcf_call_glfgen pushes into bca->bases (q as it caps it, base A C G T N)
//   aux[pos][0..3]               raw depth (ori_depth), sum of the capped mapping qualities of those bases (I16[8]+I16[10]),
//                                bases of MQ-0 reads (mq0), reads that cover the position with a deletion
// Two kernels:
//   k_pileup_quals   one thread per read pair: the base qualities in BAM orientation, with htslib's reconciliation of
//                    overlapping mates (tweak_overlap_quality, htslib-1.20/sam.c:5824-5963) applied;
//   k_pileup_bias    a second pass for a list of sites (the records that get written): the histograms mpileup's rank tests
//                    read -- position in the read, soft-clip length, mapping and base quality by ref/alt, mapping quality
//                    by strand (bam2bcf.c:488-527) -- over exactly the bases the window kernel counted.  One block per
//                    site, counters in LDS, plain stores; integers only.
//   k_pileup_window  one block per window of PLP_WINDOW positions: the admitted reads that reach the window (a contiguous
//                    run of the BAM order) are walked along their CIGARs, the counters accumulate in LDS, and the window is
//                    written to global memory with plain stores -- a window has one owner, so there is no global atomic at
//                    all, the counters are integers, and the tables do not depend on the order the reads are visited in.
// Which reads are in the pileup (mplp_func's filters, the depth cap of bam_plp_push) is decided by one host sweep over the
// records in BAM order (api_genotype.hip) and arrives as one byte per read.
#include "pileup_kernels.h"

#include <hip/hip_runtime.h>

namespace pmx {
namespace {

enum { CIG_M = 0, CIG_I = 1, CIG_D = 2, CIG_N = 3, CIG_S = 4, CIG_H = 5, CIG_P = 6, CIG_EQ = 7, CIG_X = 8 };

// one read as the BAM record shows it (build_bam_from_result, src/conversion.cpp:288-388): forward-strand sequence, CIGAR
// with the soft clips of the unaligned query ends in front and behind
struct ReadView {
    const uint32_t* ops;
    int n_ops;          // with the clips
    uint32_t c5, c3;
    int len;
    int64_t off;
    int m2rc;           // a mate 2 the pipeline reverse-complements before it aligns (seeding::reverseComplement)
    int rev;            // placed on the other strand of what was aligned
    int flipseq;        // m2rc ^ rev: BAM query index i is base len-1-i of the uploaded read
    int rs;
    __device__ uint32_t op(int k) const {
        if (c5) { if (k == 0) return c5 << 4 | CIG_S; --k; }
        const int inner = n_ops - (c5 ? 1 : 0) - (c3 ? 1 : 0);
        return k < inner ? ops[k] : (c3 << 4 | CIG_S);
    }
};

__device__ ReadView view_of(const PileupArgs& a, int64_t r) {
    const pmx_aln_record& rec = a.recs[r];
    ReadView v;
    v.off = a.off[r];
    v.len = (int)(a.off[r + 1] - a.off[r]);
    v.ops = a.cigars + rec.cigar_off;
    int c5 = rec.rev ? v.len - rec.qe : rec.qs, c3 = rec.rev ? rec.qs : v.len - rec.qe;
    v.c5 = c5 > 0 ? (uint32_t)c5 : 0;
    v.c3 = c3 > 0 ? (uint32_t)c3 : 0;
    v.n_ops = rec.n_cigar + (v.c5 ? 1 : 0) + (v.c3 ? 1 : 0);
    v.m2rc = (a.revcomp_mate2 && (r & 1)) ? 1 : 0;
    v.rev = rec.rev ? 1 : 0;
    v.flipseq = v.m2rc ^ v.rev;
    v.rs = rec.rs;
    return v;
}

// htslib's seq_nt16_table: "=ACMGRSVTWYHKDBN", either case, every other byte N = 15 (the letters' codes as nibbles A..P, Q..Z)
__device__ int nt16_of(uint8_t c) {
    const uint32_t l = (uint32_t)(c | 0x20) - 'a';   // 0..25 for a letter of either case
    if (l >= 26u) return c == '=' ? 0 : 15;
    const uint64_t tab = l < 16u ? 0xFFF3FCFFB4FFD2E1ull : 0xFAF97F865Full;
    return (int)((tab >> (4u * (l & 15u))) & 0xfu);
}

// The 4-bit code the BAM record holds for query base i.  seeding::reverseComplement (src/seeding.cpp:271-284) complements
// the upper-case A C G T of a mate 2 and leaves every other byte; build_bam_from_result (src/conversion.cpp:288-388) keeps
// the letters of a read placed as aligned -- ambiguity codes included, R is not N -- and, for a read placed on the other
// strand, complements A C G T of either case and writes N for everything else.  tweak_overlap_quality compares these codes.
__device__ int base16(const PileupArgs& a, const ReadView& v, int i) {
    const uint8_t c = a.ascii[v.off + (v.flipseq ? v.len - 1 - i : i)];
    int code = nt16_of(c);
    const bool acgt = code != 0 && (code & (code - 1)) == 0;                     // 1 2 4 8; their complement is the code's bits reversed
    if (v.m2rc && acgt && c < 'a') code = (int)(__brev((unsigned)code) >> 28);     // upper case only
    if (v.rev) code = acgt ? (int)(__brev((unsigned)code) >> 28) : 15;
    return code;
}

// cigar_iref2iseq_set / cigar_iref2iseq_next (htslib-1.20/sam.c:5750-5816) over an index instead of a pointer:
// 0 = on a match base, -1 = no more CIGAR / position not covered, -2 = an operation the walk does not know
struct CigPos { int ci; int64_t icig, iseq, iref; };

__device__ int cig_set(const ReadView& v, CigPos& s) {
    int64_t pos = s.iref;
    if (pos < 0) return -1;
    s.icig = s.iseq = s.iref = 0;
    while (s.ci < v.n_ops) {
        const uint32_t c = v.op(s.ci);
        const int op = (int)(c & 0xf);
        const int64_t n = c >> 4;
        if (op == CIG_S) { ++s.ci; s.iseq += n; s.icig = 0; continue; }
        if (op == CIG_H || op == CIG_P) { ++s.ci; s.icig = 0; continue; }
        if (op == CIG_M || op == CIG_EQ || op == CIG_X) {
            pos -= n;
            if (pos < 0) { s.icig = n + pos; s.iseq += s.icig; s.iref += s.icig; return 0; }
            ++s.ci; s.iseq += n; s.icig = 0; s.iref += n;
            continue;
        }
        if (op == CIG_I) { ++s.ci; s.iseq += n; s.icig = 0; continue; }
        if (op == CIG_D || op == CIG_N) {
            pos -= n;
            if (pos < 0) pos = 0;
            ++s.ci; s.icig = 0; s.iref += n;
            continue;
        }
        return -2;
    }
    s.iseq = -1;
    return -1;
}

__device__ int cig_next(const ReadView& v, CigPos& s) {
    while (s.ci < v.n_ops) {
        const uint32_t c = v.op(s.ci);
        const int op = (int)(c & 0xf);
        const int64_t n = c >> 4;
        if (op == CIG_M || op == CIG_EQ || op == CIG_X) {
            if (s.icig >= n - 1) { s.icig = -1; ++s.ci; continue; }
            ++s.iseq; ++s.icig; ++s.iref;
            return 0;
        }
        if (op == CIG_D || op == CIG_N) { ++s.ci; s.iref += n; s.icig = -1; continue; }
        if (op == CIG_I || op == CIG_S) { ++s.ci; s.iseq += n; s.icig = -1; continue; }
        if (op == CIG_H || op == CIG_P) { ++s.ci; s.icig = -1; continue; }
        return -2;
    }
    s.iseq = -1;
    s.iref = -1;
    return -1;
}

__device__ inline uint8_t q08(int q) { return (uint8_t)(q * 4 / 5); }   // (uint8_t)(q * 0.8): 0.8 rounds up, the product never reaches the next integer

// tweak_overlap_quality (htslib-1.20/sam.c:5824-5963): a = the mate that came first in BAM order, b = the second.  Where
// both cover a reference base: equal bases -> one mate gets the sum (at most 200), the other 0; different bases -> the
// better one keeps 0.8 of its quality, the other gets 0.  Which mate keeps the agreeing bases is a hash of the read name
// (a_keeps; the host computes it).
__device__ void reconcile(const PileupArgs& a, const ReadView& va, const ReadView& vb, int a_keeps) {
    uint8_t* aq = a.effq + va.off;
    uint8_t* bq = a.effq + vb.off;
    const int amul = a_keeps ? 1 : 0, bmul = a_keeps ? 0 : 1;
    int64_t iref = vb.rs;
    CigPos sa{0, 0, 0, iref - va.rs}, sb{0, 0, 0, iref - vb.rs};
    int a_ret = cig_set(va, sa);
    if (a_ret < 0) return;
    int b_ret = cig_set(vb, sb);
    if (b_ret < 0) return;
    for (int64_t guard = 4 * ((int64_t)va.len + vb.len) + 64; guard > 0; --guard) {
        while (a_ret >= 0 && sa.iref >= 0 && sa.iref < iref - va.rs) a_ret = cig_next(va, sa);
        if (a_ret < 0) break;
        while (b_ret >= 0 && sb.iref >= 0 && sb.iref < iref - vb.rs) b_ret = cig_next(vb, sb);
        if (b_ret < 0) break;
        if (iref < sa.iref + va.rs) iref = sa.iref + va.rs;
        if (iref < sb.iref + vb.rs) iref = sb.iref + vb.rs;
        ++iref;
        if (sa.iref + va.rs != sb.iref + vb.rs) {
            // a deletion in one mate: the other catches up, its bases under the deletion lose like mismatches
            if (sa.iref + va.rs < sb.iref + vb.rs && sb.ci > 0 && (vb.op(sb.ci - 1) & 0xf) == CIG_D) {
                do {
                    if (sa.iseq >= va.len) return;
                    aq[sa.iseq] = amul ? q08(aq[sa.iseq]) : 0;
                    a_ret = cig_next(va, sa);
                    if (a_ret < 0) return;
                } while (sa.iref + va.rs < sb.iref + vb.rs);
            } else if (sa.ci > 0 && (va.op(sa.ci - 1) & 0xf) == CIG_D) {
                do {
                    if (sb.iseq >= vb.len) return;
                    bq[sb.iseq] = bmul ? q08(bq[sb.iseq]) : 0;
                    b_ret = cig_next(vb, sb);
                    if (b_ret < 0) return;
                } while (sb.iref + vb.rs < sa.iref + va.rs);
            } else continue;
        }
        if (sa.iseq >= va.len || sb.iseq >= vb.len) return;
        const int qa = aq[sa.iseq], qb = bq[sb.iseq];
        if (base16(a, va, (int)sa.iseq) == base16(a, vb, (int)sb.iseq)) {
            const int sum = qa + qb > 200 ? 200 : qa + qb;
            aq[sa.iseq] = (uint8_t)(amul * sum);
            bq[sb.iseq] = (uint8_t)(bmul * sum);
        } else if (qa > qb) {
            aq[sa.iseq] = q08(qa);
            bq[sb.iseq] = 0;
        } else if (qa < qb) {
            bq[sb.iseq] = q08(qb);
            aq[sa.iseq] = 0;
        } else {
            aq[sa.iseq] = amul ? q08(qa) : 0;
            bq[sb.iseq] = bmul ? q08(qb) : 0;
        }
    }
}

// The quality mpileup gives query base i of a read (bam2bcf.c:425-435): the lower of the base's reconciled quality and its
// neighbours' + delta_baseq -- the right neighbour of base `late` as it stood before the reconciliation (k_pileup_quals) --
// dropped (-1) below min_baseq, at most max_baseq.  This is `baseQ`; the window kernel goes on to cap it by the mapping
// quality.  Both table kernels take a base's quality from here, so they count the same bases.
__device__ inline int base_quality(const PileupArgs& a, const uint8_t* eq, int len, int i, int late, int late_q) {
    int q = eq[i];
    if (i > 0 && q > eq[i - 1] + a.delta_baseq) q = eq[i - 1] + a.delta_baseq;
    if (i + 1 < len) {
        const int qr = i == late ? late_q : eq[i + 1];
        if (q > qr + a.delta_baseq) q = qr + a.delta_baseq;
    }
    if (q < a.min_baseq) return -1;
    return q > a.max_baseq ? a.max_baseq : q;
}

// seq_nt16_int of the BAM code: A C G T -> 0..3, everything else 4
__device__ inline int base4_of(int b16) { return b16 == 1 ? 0 : b16 == 2 ? 1 : b16 == 4 ? 2 : b16 == 8 ? 3 : 4; }

// get_position (bam2bcf.c:144-193) and the two scalings of :493-498 for query base i of a read with soft clips c5 / c3:
// epos = place in the aligned part scaled to 0..98, scl = 15 * nearest clip's length / (distance + 1), at most 99.  Where
// both ends are clipped and the left clip is not the nearer one, the reference leaves the clip length unset (0).  Doubles,
// in the reference's order of operations (the build does not contract).
__device__ inline void read_position(int i, int len, int c5, int c3, int& epos, int& scl) {
    const int pos = i + 1 - c5, aligned = len - c5 - c3;
    epos = (int)((double)pos / (aligned + 1) * (PLB_NPOS - 1));
    const int left = c5 ? i + 1 - c5 : -1, right = c3 ? len - c3 - i : -1;
    int sc_len = 0, sc_dist = 0;
    if (left >= 0) {
        if (right < 0 || left < right) { sc_len = c5; sc_dist = left; }
    } else if (right >= 0) { sc_len = c3; sc_dist = right; }
    scl = 0;
    if (sc_len) {
        scl = (int)(15.0 * sc_len / (sc_dist + 1));
        if (scl > PLB_NPOS - 1) scl = PLB_NPOS - 1;
    }
    epos = min(max(epos, 0), PLB_NPOS - 1);   // the reference asserts both ranges (:499-500); a counter never leaves its block
    scl = max(scl, 0);
}

}  // namespace

__global__ void k_pileup_quals(PileupArgs a) {
    const int64_t unit = a.paired ? 2 : 1;
    const int64_t n_units = a.n_reads / unit;
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x) {
        for (int64_t r = u * unit; r < (u + 1) * unit; ++r) {
            a.late_idx[r] = -1;
            a.late_q[r] = 0;
            if (!(a.rinfo[r] & PLP_ADMIT)) continue;
            const ReadView v = view_of(a, r);
            for (int i = 0; i < v.len; ++i) {   // bam_qual of build_bam_from_result: Phred+33 minus 33, missing qualities 'I'
                int q = a.qual ? a.qual[v.off + (v.flipseq ? v.len - 1 - i : i)] : 'I';
                if (q == 0) q = 'I';
                q -= 33;
                a.effq[v.off + i] = (uint8_t)(q < 0 ? 0 : q);
            }
        }
        if (!a.paired) continue;
        const int64_t r1 = 2 * u, r2 = r1 + 1;
        if (!(a.rinfo[r1] & PLP_TWEAK) || !(a.rinfo[r2] & PLP_TWEAK)) continue;
        const int64_t ra = (a.rinfo[r1] & PLP_SECOND) ? r2 : r1, rb = ra == r1 ? r2 : r1;
        const ReadView va = view_of(a, ra), vb = view_of(a, rb);
        // The pileup of a position is taken as soon as a read that starts behind it has been pushed
        // (bam_plp64_next, sam.c:6034), the reconciliation when b is pushed (overlap_push, sam.c:5969-6003).  The last base of
        // a in front of b's start looks at its right neighbour's quality (bam2bcf.c:427-432), which the reconciliation may
        // change: it sees the changed value only if b is the first admitted read that starts behind that base.
        int p_last = -1, q_last = -1;
        {
            int x = va.rs, y = 0;
            for (int k = 0; k < va.n_ops && x < vb.rs; ++k) {
                const uint32_t c = va.op(k);
                const int op = (int)(c & 0xf), n = (int)(c >> 4);
                if (op == CIG_M || op == CIG_EQ || op == CIG_X) {
                    const int cover = min(n, vb.rs - x);
                    p_last = x + cover - 1;
                    q_last = y + cover - 1;
                    x += n; y += n;
                } else if (op == CIG_I || op == CIG_S) y += n;
                else if (op == CIG_D || op == CIG_N) x += n;
            }
        }
        uint8_t neighbour = 0;
        const bool has_neighbour = q_last >= 0 && q_last + 1 < va.len;
        if (has_neighbour) neighbour = a.effq[va.off + q_last + 1];
        reconcile(a, va, vb, (a.rinfo[ra] & PLP_KEEP) ? 1 : 0);
        if (has_neighbour) {
            const int at = min(p_last + 1, a.ref_len + 1);
            if (a.first_ge[at] != a.rank[rb]) { a.late_idx[ra] = q_last; a.late_q[ra] = neighbour; }
        }
    }
}

__global__ void __launch_bounds__(256) k_pileup_window(PileupArgs a) {
    __shared__ uint32_t tab[PLP_WINDOW * PLP_CELLS];
    for (int w0 = blockIdx.x * PLP_WINDOW; w0 < a.ref_len; w0 += gridDim.x * PLP_WINDOW) {
        const int w1 = min(w0 + PLP_WINDOW, a.ref_len);
        for (int i = threadIdx.x; i < PLP_WINDOW * PLP_CELLS; i += blockDim.x) tab[i] = 0;
        __syncthreads();
        // the admitted reads that can reach the window: starts in [w0 - max_span, w1) -- one run of the BAM order
        int64_t lo = 0, hi = a.n_sorted;
        {
            const int from = w0 - a.max_span;
            int64_t l = 0, h = a.n_sorted;
            while (l < h) { const int64_t m = (l + h) >> 1; if (a.s_rs[m] < from) l = m + 1; else h = m; }
            lo = l;
            h = a.n_sorted;
            while (l < h) { const int64_t m = (l + h) >> 1; if (a.s_rs[m] < w1) l = m + 1; else h = m; }
            hi = l;
        }
        for (int64_t k = lo + threadIdx.x; k < hi; k += blockDim.x) {
            const int64_t r = a.s_idx[k];
            const pmx_aln_record& rec = a.recs[r];
            if (rec.re <= w0) continue;
            const ReadView v = view_of(a, r);
            const uint8_t* eq = a.effq + v.off;
            const int strand = (a.paired && (r & 1)) ? !rec.rev : (rec.rev != 0);   // bam_is_rev of the written record
            int mapq = rec.mapq < 255 ? rec.mapq : 20;                               // DEF_MAPQ (bam2bcf.c:449)
            const bool mq0 = mapq == 0;
            if (mapq > a.cap_mapq) mapq = a.cap_mapq;
            const int late = a.late_idx[r], late_q = a.late_q[r];
            int x = v.rs, y = 0;
            for (int ci = 0; ci < v.n_ops && x < w1; ++ci) {
                const uint32_t c = v.op(ci);
                const int op = (int)(c & 0xf), n = (int)(c >> 4);
                if (op == CIG_M || op == CIG_EQ || op == CIG_X) {
                    for (int p = max(x, w0); p < min(x + n, w1); ++p) {
                        const int i = y + (p - x);
                        if (i >= v.len) break;
                        uint32_t* cell = tab + (p - w0) * PLP_CELLS;
                        atomicAdd(cell + PLP_HIST + 0, 1u);   // ori_depth: every read that shows a base here (bam2bcf.c:298-308)
                        int q = base_quality(a, eq, v.len, i, late, late_q);
                        if (q < 0) continue;
                        if (q > mapq) q = mapq;               // bam2bcf.c:456-460
                        if (q > 63) q = 63;
                        if (q < 4) q = 4;
                        const int b = base4_of(base16(a, v, i));
                        atomicAdd(cell + (q * 2 + strand) * PLP_NBASE + b, 1u);
                        atomicAdd(cell + PLP_HIST + 1, (uint32_t)mapq);
                        if (mq0) atomicAdd(cell + PLP_HIST + 2, 1u);
                    }
                    x += n; y += n;
                } else if (op == CIG_I || op == CIG_S) y += n;
                else if (op == CIG_D) {
                    for (int p = max(x, w0); p < min(x + n, w1); ++p) atomicAdd(tab + (p - w0) * PLP_CELLS + PLP_HIST + 3, 1u);
                    x += n;
                } else if (op == CIG_N) x += n;
            }
        }
        __syncthreads();
        const int n_pos = w1 - w0;
        for (int i = threadIdx.x; i < n_pos * PLP_HIST; i += blockDim.x) {
            const int p = i / PLP_HIST, c = i - p * PLP_HIST;
            a.hist[(int64_t)(w0 + p) * PLP_HIST + c] = tab[p * PLP_CELLS + c];
        }
        for (int i = threadIdx.x; i < n_pos * PLP_AUX; i += blockDim.x) {
            const int p = i / PLP_AUX, c = i - p * PLP_AUX;
            a.aux[(int64_t)(w0 + p) * PLP_AUX + c] = tab[p * PLP_CELLS + PLP_HIST + c];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_pileup_bias(PileupBiasArgs b) {
    __shared__ uint32_t tab[PLB_CELLS];
    const PileupArgs& a = b.run;
    for (int64_t s = blockIdx.x; s < b.n_sites; s += gridDim.x) {
        const int p = b.sites[s];
        for (int i = threadIdx.x; i < PLB_CELLS; i += blockDim.x) tab[i] = 0;
        __syncthreads();
        // is_diff of bam2bcf.c:438: a base is "ref" only against a reference letter A C G T
        const int r16 = nt16_of(b.ref_bases[s]);
        const int ref4 = base4_of(r16);
        // the admitted reads that can reach the site: starts in [p - max_span, p] -- the window kernel's two searches
        int64_t lo, hi;
        {
            const int from = p - a.max_span;
            int64_t l = 0, h = a.n_sorted;
            while (l < h) { const int64_t m = (l + h) >> 1; if (a.s_rs[m] < from) l = m + 1; else h = m; }
            lo = l;
            h = a.n_sorted;
            while (l < h) { const int64_t m = (l + h) >> 1; if (a.s_rs[m] < p + 1) l = m + 1; else h = m; }
            hi = l;
        }
        for (int64_t k = lo + threadIdx.x; k < hi; k += blockDim.x) {
            const int64_t r = a.s_idx[k];
            const pmx_aln_record& rec = a.recs[r];
            if (rec.re <= p) continue;
            const ReadView v = view_of(a, r);
            // the query base on the site, if the read shows one there
            int i = -1;
            {
                int x = v.rs, y = 0;
                for (int ci = 0; ci < v.n_ops && x <= p; ++ci) {
                    const uint32_t c = v.op(ci);
                    const int op = (int)(c & 0xf), n = (int)(c >> 4);
                    if (op == CIG_M || op == CIG_EQ || op == CIG_X) {
                        if (p < x + n) { i = y + (p - x); break; }
                        x += n; y += n;
                    } else if (op == CIG_I || op == CIG_S) y += n;
                    else if (op == CIG_D || op == CIG_N) x += n;
                }
            }
            if (i < 0 || i >= v.len) continue;
            int bq = base_quality(a, a.effq + v.off, v.len, i, a.late_idx[r], a.late_q[r]);
            if (bq < 0) continue;
            if (bq > PLB_NQUAL - 1) bq = PLB_NQUAL - 1;
            int mq = rec.mapq < 255 ? rec.mapq : 20;
            if (mq > a.cap_mapq) mq = a.cap_mapq;
            if (mq > PLB_NQUAL - 1) mq = PLB_NQUAL - 1;
            const int strand = (a.paired && (r & 1)) ? !rec.rev : (rec.rev != 0);
            const int alt = (ref4 < 4 && base4_of(base16(a, v, i)) == ref4) ? 0 : 1;
            int epos, scl;
            read_position(i, v.len, (int)v.c5, (int)v.c3, epos, scl);
            atomicAdd(tab + PLB_POS + alt * PLB_NPOS + epos, 1u);
            atomicAdd(tab + PLB_SCL + alt * PLB_NPOS + scl, 1u);
            atomicAdd(tab + PLB_MQ + alt * PLB_NQUAL + mq, 1u);
            atomicAdd(tab + PLB_BQ + alt * PLB_NQUAL + bq, 1u);
            atomicAdd(tab + PLB_MQS + strand * PLB_NQUAL + mq, 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < PLB_CELLS; i += blockDim.x) b.out[s * PLB_CELLS + i] = tab[i];
        __syncthreads();
    }
}

}  // namespace pmx
