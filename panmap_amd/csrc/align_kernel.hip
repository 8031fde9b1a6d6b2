// ALIGN stage, tier-2 (general) kernels for gfx950: work arrays may live in LDS or in the per-wave HBM
// slab (generic pointers).  Used for pairs that exceed the tier-1 capacities and for long reads.
// Integer hashing + int8 DP + a little fp32: VALU/LDS work, no MFMA.
#include "align_kernel_body.hpp"

namespace pmx {
namespace aln {

// two register budgets of the same body: 256 VGPRs (2 waves/SIMD) and 128 VGPRs (4 waves/SIMD)
__global__ void __launch_bounds__(64, 2) k_align_reads(AlignArgs A) { align_reads_body<2>(A); }
__global__ void __launch_bounds__(64, 4) k_align_reads_w4(AlignArgs A) { align_reads_body<4>(A); }


// pmx_align_dp_probe: one DP request per wave on a layout of the wave-per-read kernels -- the request's sequences staged
// where align1 keeps them (query: qseq, target: tseq; LDS or the wave's slab, by the layout), then ksw_extd2 (or sw_ll)
// exactly as align1 calls it.  A side beyond the layout's capacities is left unserved before anything is staged.
__global__ void __launch_bounds__(64, 2) k_align_dp_probe(DpProbeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    Work& W = *reinterpret_cast<Work*>(lds);
    uint8_t* fast = lds + PMX_ALIGN_WORK_BYTES;
    uint8_t* slow = A.slow_base + (size_t)blockIdx.x * A.slow_stride;
    const int lane = (int)(threadIdx.x & 63u);
    for (int64_t it = blockIdx.x; it < A.n; it += gridDim.x) {
        __syncthreads();
        bind_work(W, A.layout, fast, slow);
        W.n_segs = 1;
        W.prof = nullptr;
        W.no_rows_dp = A.no_rows_dp;
        W.mv_ready = 0;
        W.dp_path = 0;
        const int64_t ql = A.q_off[it + 1] - A.q_off[it], tl = A.t_off[it + 1] - A.t_off[it];
        DpProbeOut o;
        memset(&o, 0, sizeof(o));
        __syncthreads();
        if (ql < 1 || tl < 1 || ql > A.layout.caps.max_qlen || tl > A.layout.caps.max_tlen) {
            if (lane == 0) A.out[it] = o;
            continue;
        }
        const int qlen = (int)ql, tlen = (int)tl;
        uint8_t* qs = W.qseq[0][0];
        uint8_t* ts = W.tseq;
        for (int i = lane; i < qlen; i += 64) qs[i] = A.seqs[A.q_off[it] + i];
        for (int i = lane; i < tlen; i += 64) ts[i] = A.seqs[A.t_off[it] + i];
        __syncthreads();
        if (A.sw_ll) {
            auto qf = [&](int k) { return (int)qs[k]; };
            auto tf = [&](int k) { return (int)ts[k]; };
            int qe = -1, te = -1;
            bool ok = false;
            o.ez.score = sw_ll(W, A.opt, qlen, qf, tlen, tf, &qe, &te, &ok);
            o.served = ok ? 1 : 0;
            o.ok = ok ? 1 : 0;
            o.qe = qe;
            o.te = te;
        } else {
            Ez ez;
            ksw_extd2(W, qlen, (const uint8_t*)qs, tlen, (const uint8_t*)ts, A.opt.mat, (int8_t)A.opt.q, (int8_t)A.opt.e, (int8_t)A.opt.q2, (int8_t)A.opt.e2,
                      A.w[it], A.zdrop[it], A.end_bonus[it], A.flag[it], ez);
            __syncthreads();
            o.ez = ez;
            o.path = W.dp_path;
            o.served = !(W.status & PMX_ST_OVERFLOW) && ez.n_cigar >= 0 && ez.n_cigar <= W.caps.max_cigar ? 1 : 0;
            if (o.served) {
                const uint32_t* cg = W.cig_tmp;
                uint32_t* dst = A.cigars + (size_t)it * (size_t)A.layout.caps.max_cigar;
                for (int i = lane; i < ez.n_cigar; i += 64) dst[i] = cg[i];
            }
        }
        if (lane == 0) A.out[it] = o;
    }
}

// pmx_align_chain_probe: one anchor list per wave on a layout of the wave-per-read kernels -- the list copied to where map_frag
// keeps its anchors (W.a; LDS or the wave's slab, by the layout), then one operation of the sort / chaining code exactly as
// map_frag calls it (aln_chain_probe.hpp).  A list beyond the layout's anchor capacity is left unserved before anything is copied.
__global__ void __launch_bounds__(64, 2) k_align_chain_probe(ChainProbeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    Work& W = *reinterpret_cast<Work*>(lds);
    uint8_t* fast = lds + PMX_ALIGN_WORK_BYTES;
    uint8_t* slow = A.slow_base + (size_t)blockIdx.x * A.slow_stride;
    const int lane = (int)(threadIdx.x & 63u);
    for (int64_t it = blockIdx.x; it < A.n; it += gridDim.x) {
        __syncthreads();
        bind_work(W, A.layout, fast, slow);
        W.n_segs = A.n_segs;
        W.prof = nullptr;
        W.no_rows_dp = 0;
        W.mv_ready = 0;
        W.dp_path = 0;
        const int64_t a0 = A.a_off[it], na = A.a_off[it + 1] - a0;
        W.qlen[0] = A.qlen ? A.qlen[2 * it] : 0;
        W.qlen[1] = A.qlen ? A.qlen[2 * it + 1] : 0;
        W.n_a = na;
        W.n_u = 0;
        __syncthreads();
        if (na < 0 || na > A.layout.caps.max_anchor) continue;
        A128* a = W.a;
        if (A.op == PMX_CP_SORT64) {
            uint64_t* v = reinterpret_cast<uint64_t*>(a);
            for (int64_t i = lane; i < na; i += 64) v[i] = A.anchors[a0 + i].x;
        } else {
            for (int64_t i = lane; i < na; i += 64) a[i] = A.anchors[a0 + i];
        }
        __syncthreads();
        chain_probe_run(W, A.opt, A.op, A.max_dist_x, A.max_dist_y, A.n_seg);
        __syncthreads();
        ChainProbeOut o;
        o.served = 1;
        o.status = W.status;
        o.n_a = W.n_a;
        o.n_u = W.n_u;
        o.pad = 0;
        // (what the operation may leave: at most the anchors it was given, at most one chain per anchor)
        const int64_t n_out = o.n_a < 0 ? 0 : (o.n_a > na ? na : o.n_a), u_out = o.n_u < 0 ? 0 : ((int64_t)o.n_u > na ? na : (int64_t)o.n_u);
        if (A.op == PMX_CP_SORT64) {
            const uint64_t* v = reinterpret_cast<const uint64_t*>(a);
            for (int64_t i = lane; i < n_out; i += 64) { A128 e; e.x = v[i]; e.y = 0; A.out_anchors[a0 + i] = e; }
        } else {
            for (int64_t i = lane; i < n_out; i += 64) A.out_anchors[a0 + i] = a[i];
        }
        const uint64_t* u = W.u;
        for (int64_t i = lane; i < u_out; i += 64) A.out_u[a0 + i] = u[i];
        if (lane == 0) A.out[it] = o;
    }
}

}  // namespace aln
}  // namespace pmx
