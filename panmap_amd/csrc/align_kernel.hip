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

}  // namespace aln
}  // namespace pmx
