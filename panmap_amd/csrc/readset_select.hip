// A read set made from a subset of another, for gfx950 (wave64): pmx_readset_select (include/panmap_amd.h).  It replaces the
// nodeSeqs / nodeQuals copies of alignAssignedReads (src/main.cpp:691-699): there the reads of one node are copied string by
// string on the host; here the reads stay on the device and a node's subset is one gather of an uploaded set.
//
// Steps, all on the context's stream:
//   k_select_lengths   len[i] = off[idx[i] + 1] - off[idx[i]], nwords[i] = its 32-base words, entry n of both = 0, stats[0] = the
//                      longest picked read.  One thread per picked read.
//   two exclusive scans (rocprim) of n + 1 entries: the byte offsets and the word offsets (pmx_readset_pack needs both).
//   one 24-byte read-back (total bases, total words, longest read): the only synchronisation, it sizes the output.
//   k_select_copy      one wave per picked read: bases and, when present, qualities.  Source and destination byte addresses are
//                      arbitrary, so a wave takes the widest piece (16, 8, 4 bytes) for which the two ADDRESSES are congruent,
//                      copies the bytes ahead of the destination's first aligned piece and behind its last one singly, and
//                      falls back to bytes when the addresses differ by an odd amount.  A read longer than a wave's step (64
//                      pieces) is a loop.  Plain vector loads and stores only.
// Only bytes inside [off[idx[i]], off[idx[i] + 1]) of the source and [out_off[i], out_off[i + 1]) of the result are touched.
// Algorithmic HBM bytes: 2 x the selected bytes (one read, one write); 4 x with qualities.  The 16 bytes of offsets per read are
// noise for reads of 100 bases and more.
// Resources (hipcc --offload-arch=gfx950 -O3 --save-temps, .vgpr_count / .sgpr_count / .group_segment_fixed_size /
// .private_segment_fixed_size): k_select_lengths 16 VGPR, 26 SGPR; k_select_copy 58 VGPR, 48 SGPR (the piece loops unrolled);
// both LDS 0, scratch 0, no spills.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include <rocprim/rocprim.hpp>

#include "device/dev_util.hpp"
#include "readset.hpp"

namespace pmx {
namespace {

__global__ void __launch_bounds__(256)
k_select_lengths(const int64_t* __restrict__ off, const int64_t* __restrict__ idx, int64_t n, int64_t* __restrict__ len, int64_t* __restrict__ nwords,
                 unsigned long long* stats) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (t == 0) { len[n] = 0; nwords[n] = 0; }
    unsigned long long mx = 0;
    for (int64_t i = t; i < n; i += stride) {
        const int64_t r = idx[i], l = off[r + 1] - off[r];
        len[i] = l;
        nwords[i] = (l + 31) >> 5;
        mx = (unsigned long long)l > mx ? (unsigned long long)l : mx;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)mx, d);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&stats[0], mx);
}

// `body` bytes in pieces of type V, the piece v of a wave's step to lane v
template <class V>
__device__ __forceinline__ void copy_pieces(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t body, int lane) {
    const V* __restrict__ sv = reinterpret_cast<const V*>(s);
    V* __restrict__ dv = reinterpret_cast<V*>(d);
    const int64_t nv = body / (int64_t)sizeof(V);
    for (int64_t v = lane; v < nv; v += 64) dv[v] = sv[v];
}

// len bytes from s to d by one wave: W = the widest piece for which s and d are congruent; the bytes ahead of d's first W-aligned
// address and behind its last one go singly (fewer than W each: one lane per byte)
__device__ __forceinline__ void copy_span(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t len, int lane) {
    const uintptr_t diff = (uintptr_t)s ^ (uintptr_t)d;
    const int W = !(diff & 15u) ? 16 : !(diff & 7u) ? 8 : !(diff & 3u) ? 4 : 1;
    if (W == 1) {
        for (int64_t i = lane; i < len; i += 64) d[i] = s[i];
        return;
    }
    int64_t head = (int64_t)((0 - (uintptr_t)d) & (uintptr_t)(W - 1));
    head = head < len ? head : len;
    const int64_t body = (len - head) & ~(int64_t)(W - 1), tail = len - head - body;
    if (lane < head) d[lane] = s[lane];
    if (W == 16) copy_pieces<uint4>(s + head, d + head, body, lane);
    else if (W == 8) copy_pieces<uint2>(s + head, d + head, body, lane);
    else copy_pieces<uint32_t>(s + head, d + head, body, lane);
    if (lane < tail) d[head + body + lane] = s[head + body + lane];
}

__global__ void __launch_bounds__(256)
k_select_copy(const uint8_t* __restrict__ ascii, const uint8_t* __restrict__ qual, const int64_t* __restrict__ off, const int64_t* __restrict__ idx, int64_t n,
              const int64_t* __restrict__ out_off, uint8_t* __restrict__ out_ascii, uint8_t* __restrict__ out_qual) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave; i < n; i += n_waves) {
        const int64_t s = off[idx[i]], d = out_off[i], len = out_off[i + 1] - d;
        if (len <= 0) continue;
        copy_span(ascii + s, out_ascii + d, len, lane);
        if (qual) copy_span(qual + s, out_qual + d, len, lane);
    }
}

}  // namespace
}  // namespace pmx

using namespace pmx;

extern "C" int pmx_readset_select(pmx_ctx* ctx, const pmx_readset* src, const int64_t* idx, int64_t n, pmx_readset** out) {
    if (!ctx || !src || !out || n < 0 || (n > 0 && !idx)) return fail(PMX_ERR_ARG, "pmx_readset_select: a null argument or a negative count");
    if (*out == src) return fail(PMX_ERR_ARG, "pmx_readset_select: the result cannot be the source read set");
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= src->n)
            return fail(PMX_ERR_ARG, "pmx_readset_select: index " + std::to_string(idx[i]) + " (entry " + std::to_string(i) + ") is outside the " + std::to_string(src->n) + " reads of the source");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<pmx_readset> fresh;
    pmx_readset* dst = *out;
    if (!dst) { fresh.reset(new pmx_readset()); dst = fresh.get(); }
    dst->packed = false;
    dst->has_order = false;
    dst->has_pair_order = false;
    dst->has_pair_map = false;
    dst->packed_ranges.clear();
    dst->ordered_ranges.clear();
    dst->has_qual = false;
    dst->has_recs = false;
    dst->hpc = src->hpc;
    dst->n = n;
    dst->total = 0;
    dst->max_len = 0;
    dst->n_words = 0;
    dst->off0 = 0;
    own_ensure(dst->off, (size_t)n + 1);
    dst->sel_idx.ensure((size_t)n + 1);
    dst->len_tmp.ensure((size_t)n + 1);
    dst->nw_tmp.ensure((size_t)n + 1);
    dst->woff.ensure((size_t)n + 1);
    dst->stats.ensure(2);
    PMX_ZERO(dst->stats, 2, ctx->stream);
    PMX_H2D(dst->sel_idx, idx, n, ctx->stream);
    PMX_LAUNCH(k_select_lengths, dim3(grid_for(n + 1, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, src->off.p, dst->sel_idx.p, n, dst->len_tmp.p,
               dst->nw_tmp.p, dst->stats.p);
    PMX_ROCPRIM(dst->scan_tmp, exclusive_scan, dst->len_tmp.p, dst->off.p, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), ctx->stream);
    PMX_ROCPRIM(dst->scan_tmp, exclusive_scan, dst->nw_tmp.p, dst->woff.p, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), ctx->stream);
    struct { int64_t total, n_words; unsigned long long st[2]; } h = {0, 0, {0, 0}};
    PMX_D2H(&h.total, pmx::at(dst->off, n), 1, ctx->stream);
    PMX_D2H(&h.n_words, pmx::at(dst->woff, n), 1, ctx->stream);
    PMX_D2H_SYNC(h.st, dst->stats, ctx->stream);   // (sizes the output; `idx` has been read by now)
    own_ensure(dst->ascii, (size_t)h.total + 32);
    if (src->has_qual) dst->qual.ensure((size_t)h.total + 32);
    dst->words.ensure((size_t)std::max<int64_t>(h.n_words, 1));
    dst->amb.ensure((size_t)std::max<int64_t>(h.n_words, 1));
    const bool recs = n > 0 && (int64_t)h.st[0] <= 160;
    if (recs) dst->recs.ensure((size_t)n * 64);
    if (h.total > 0) {
        timer_begin(ctx, "select");
        PMX_LAUNCH(k_select_copy, dim3(grid_for(n, 4, ctx->n_cu * 32)), dim3(256), 0, ctx->stream, src->ascii.p, src->has_qual ? src->qual.p : (const uint8_t*)nullptr,
                   src->off.p, dst->sel_idx.p, n, dst->off.p, dst->ascii.p, src->has_qual ? dst->qual.p : (uint8_t*)nullptr);
        timer_end(ctx, "select", 1);
    } else {
        timer_cancel(ctx, "select");
    }
    dst->total = h.total;
    dst->n_words = h.n_words;
    dst->max_len = (int64_t)h.st[0];
    dst->has_qual = src->has_qual;
    dst->has_recs = recs;
    if (fresh) *out = fresh.release();
    return PMX_OK;
    PMX_CATCH
}
