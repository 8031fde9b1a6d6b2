// C ABI, device part 4: --meta (haplotype deconvolution of a mixed sample; BASELINE config 5).
//
// What the reference does (src/main.cpp:1192-1313 runDeconvolution; src/mgsr.cpp):
//   1. every read becomes its list of k-min-mers ("seedmers": hash + orientation), identical lists are merged with a
//      multiplicity (initializeQueryData, mgsr.cpp:1774-2237);
//   2. every node gets an overlap coefficient: distinct read seedmer hashes its genome holds / its distinct seedmers
//      (computeOverlapCoefficients, :5685-5790); the nodes of the best `top_oc` distinct values are the candidates
//      (squareEM::squareEM, :8010-8060);
//   3. every (read, candidate) pair gets a parsimony score: with f = the read's seedmers the node's genome holds in the
//      read's orientation and r = those it holds in the other one, the score is max(f, r) (scoreReadsHelper, :7225-7455,
//      a DFS that applies and reverts per-node seed deltas);
//   4. candidates with identical score columns are merged, P(read | node) = err^(n - s) * (1 - err)^s with n = the read's
//      seedmers, and a SQUAREM-accelerated EM estimates the mixture proportions (:8100-8160, :4341-4443); nodes below
//      0.5 % are dropped and the EM is run again, up to five rounds (:4445-4490, main.cpp:1263-1271).
// Here, MI355X-first:
//   * the node side is the ORIENTED seed index (pmx_index_build_ex mode | PMX_INDEX_ORIENTED): a count-change index like
//     the place stage's, keyed hash ^ PMX_ORIENT_XOR for right-to-left k-min-mers.  Nodes are in DFS pre-order, so "seedmer
//     becomes present / absent at node v" holds for the contiguous index range [v, end(v)] of v's subtree: presence at any
//     node is the XOR of the ranges that cover it.  No tree walk, no per-node state: k_meta_mask_events toggles, for every
//     transition of a seedmer the reads carry, a bit range of that seedmer's row in a (seedmer x candidate) bit matrix.
//   * k_meta_scores: one thread per (read, 64 candidates).  The read's seedmers are added as bit planes (a carry-save
//     counter per candidate bit: 64 candidates advance with a handful of 64-bit ops per seedmer), for both orientations;
//     max(f, r) per candidate goes out as a 16-bit score.
//   * step 2 reuses the place stage: the overlap coefficient's two counts are its per-node intersection / genome seed counts.
//   * the EM runs on the score matrix, P(read | node) gathered from a table of the few distinct (n, s) pairs (computed on
//     the host with the libm the oracle uses), FP64 throughout, every reduction in a fixed order (bit-stable runs):
//     k_meta_denoms (a wave per read), k_meta_colsum (a thread per candidate over a chunk of reads; chunk partials added in
//     chunk order).  HBM-bound: 2 B per (read, candidate) per pass, six passes per SQUAREM iteration.
// --filter-and-assign (every read against EVERY node, no score matrix) is meta_assign.hip, on the state of meta_state.hpp;
// --mask-reads / --mask-seeds (merged reads or list entries with low-coverage k-min-mers leave the sample) is meta_mask.hip.
// --mask-read-ends is the seeding kernels' per-end trim (seedmer_lists, overlap_place_params; DUST scores the same slice);
// --em-leaves-only is a filter in select_candidates.
// Read-side seedmer extraction is host C++ here (threads; the k-min-mer definitions of host/seed_host.hpp); moving it into
// the seeding kernel is the next step.  parity: the reference's own MGSR index and EM cannot be built here (panman / TBB /
// Eigen / abseil are absent): scores and EM are checked by the test suite against a direct restatement (per-node seed
// sets by walking the tree, numpy EM), the end result against the reference's e2e expectation on rsv_4K (70 / 30 mixture
// recovered within its ranges, src/test/e2e/run_e2e.sh:182-204).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "api_internal.hpp"
#include "device/dev_util.hpp"
#include "host/index_build.hpp"
#include "host/seed_host.hpp"
#include "meta_state.hpp"
#include "place_kernels.h"
#include "readset.hpp"

using namespace pmx;

namespace {
// the EM's two fixed-order reductions: reads per partial column sum (k_meta_colsum) and values per block sum (k_meta_sum_blocks)
constexpr int64_t kColsumChunk = 256;
constexpr int64_t kSumBlock = 1024;
// reads per launch of the seeding kernel in list mode: bounds the list arrays (one slot per base)
constexpr int64_t kListChunk = 2000000;

// first position in the ascending array a[0..n) whose value is >= v
__device__ __forceinline__ int lower_bound_u32(const uint32_t* __restrict__ a, int n, uint32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Every count change of the oriented index whose seedmer becomes present (parent count 0) or absent (child count 0) and
// whose hash the reads carry toggles the candidates inside the node's subtree in that seedmer's row: bits [lo, hi) of
// mask[orientation][uid].  Candidates are sorted by DFS index, so the subtree is one bit range.
__global__ void k_meta_mask_events(const uint64_t* __restrict__ ch_key, const int16_t* __restrict__ ch_pc, const int16_t* __restrict__ ch_cc,
                                   const uint32_t* __restrict__ ch_node, int64_t n_changes, const uint32_t* __restrict__ subtree_end,
                                   const uint64_t* __restrict__ uniq, int64_t n_uniq, const uint32_t* __restrict__ cand_dfs, int n_cand, int words,
                                   unsigned long long* mask_fwd, unsigned long long* mask_rev) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_changes; c += (int64_t)gridDim.x * blockDim.x) {
        const bool was = ch_pc[c] > 0, is = ch_cc[c] > 0;
        if (was == is) continue;
        const uint64_t key = ch_key[c];
        int64_t uid = find_sorted(uniq, n_uniq, key);
        unsigned long long* row = mask_fwd;
        if (uid < 0) { uid = find_sorted(uniq, n_uniq, key ^ PMX_ORIENT_XOR); row = mask_rev; }
        if (uid < 0) continue;
        const uint32_t v = ch_node[c];
        const int lo = lower_bound_u32(cand_dfs, n_cand, v), hi = lower_bound_u32(cand_dfs, n_cand, subtree_end[v] + 1u);
        if (hi <= lo) continue;
        row += (size_t)uid * (size_t)words;
        for (int w = lo >> 6; w <= (hi - 1) >> 6; ++w) {
            const int b0 = w == (lo >> 6) ? (lo & 63) : 0, b1 = w == ((hi - 1) >> 6) ? ((hi - 1) & 63) : 63;
            const unsigned long long bits = (b1 == 63 ? ~0ULL : ((1ULL << (b1 + 1)) - 1ULL)) & ~((1ULL << b0) - 1ULL);
            atomicXor(&row[w], bits);
        }
    }
}

// One thread per (read, word of 64 candidates).  seed_uid / seed_rev: the read's seedmers as row indices + orientation.
// score[read][cand] = max(#seedmers present in the read's orientation, #present in the other one).
template <int PLANES>
__global__ void k_meta_scores(const int64_t* __restrict__ read_off, const uint32_t* __restrict__ seed_uid, const uint8_t* __restrict__ seed_rev,
                              int64_t n_reads, const unsigned long long* __restrict__ mask_fwd, const unsigned long long* __restrict__ mask_rev,
                              int words, int n_cand, uint16_t* __restrict__ score) {
    const int64_t total = n_reads * (int64_t)words;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / words;
        const int w = (int)(t - r * words);
        unsigned long long same[PLANES], other[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) { same[p] = 0; other[p] = 0; }
        for (int64_t i = read_off[r]; i < read_off[r + 1]; ++i) {
            const size_t row = (size_t)seed_uid[i] * (size_t)words + (size_t)w;
            const unsigned long long f = mask_fwd[row], b = mask_rev[row];
            const bool rev = seed_rev[i] != 0;
            planes_add<PLANES>(same, rev ? b : f);    // the genome holds it the way the read does
            planes_add<PLANES>(other, rev ? f : b);
        }
        const int c0 = w * 64;
        for (int b = 0; b < 64 && c0 + b < n_cand; ++b) {
            uint32_t s = 0, o = 0;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) { s |= (uint32_t)((same[p] >> b) & 1ULL) << p; o |= (uint32_t)((other[p] >> b) & 1ULL) << p; }
            score[(size_t)r * (size_t)n_cand + (size_t)(c0 + b)] = (uint16_t)(s > o ? s : o);
        }
    }
}

// 128-bit digest of every candidate's score column (candidates with equal columns are merged before the EM)
__global__ void k_meta_column_digest(const uint16_t* __restrict__ score, int64_t n_reads, int n_cand, uint64_t* digest) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cand; c += gridDim.x * blockDim.x) {
        uint64_t a = 0x9e3779b97f4a7c15ULL, b = 0xc2b2ae3d27d4eb4fULL;
        for (int64_t r = 0; r < n_reads; ++r) {
            const uint64_t v = (uint64_t)score[(size_t)r * (size_t)n_cand + (size_t)c] + 1ULL;
            a = (a ^ v) * 0xff51afd7ed558ccdULL; a ^= a >> 29;
            b = (b + v * 0x9e3779b97f4a7c15ULL) * 0xc4ceb9fe1a85ec53ULL; b ^= b >> 31;
        }
        digest[2 * (size_t)c] = a;
        digest[2 * (size_t)c + 1] = b;
    }
}

// --gpus N, pass A of the EM rows: each read's best score over the candidates and whether the --discard rule of pmx_meta_em
// keeps it (the same integer arithmetic as the host loop of the one-rank path, which downloads the whole matrix instead).
// A wave per read; the maximum is order-free.
__global__ void k_meta_row_keep(const uint16_t* __restrict__ score, int64_t n_reads, int n_cand, const int64_t* __restrict__ read_off,
                                double discard, uint8_t* __restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const uint16_t* srow = score + (size_t)r * (size_t)n_cand;
        int mx = 0;
        for (int c = lane; c < n_cand; c += 64) mx = max(mx, (int)srow[c]);
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
        if (lane == 0) {
            const int64_t n_seed = read_off[r + 1] - read_off[r];
            keep[r] = (mx == 0 || mx < (int)((double)n_seed * discard)) ? 0 : 1;
        }
    }
}

// EM pass 1: denom[j] = 1 / sum_i P(j, i) * props[i] over the kept columns, in column order (lanes stride the columns, a fixed
// butterfly adds the lanes); llh[j] = weight[j] * log(denom[j]).  A wave per read.
__global__ void k_meta_denoms(const uint16_t* __restrict__ score, int n_cand, const int* __restrict__ cols, int n_cols, const double* __restrict__ props,
                              const int64_t* __restrict__ rows, int64_t n_rows, const uint32_t* __restrict__ tab_off, const double* __restrict__ tab,
                              const double* __restrict__ weight, double* denom, double* llh, const int* done) {
    if (done && *done) return;   // (the SQUAREM loop runs ahead of the host: launches queued past convergence do nothing)
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t j = wave; j < n_rows; j += n_waves) {
        const int64_t r = rows[j];
        const uint16_t* srow = score + (size_t)r * (size_t)n_cand;
        const double* t = tab + tab_off[j];
        double acc = 0.0;
        // (same order of additions; four columns' loads are in flight at a time -- each entry is a chain of three dependent loads,
        //  and one at a time the pass ran at an eighth of the HBM rate)
        int i = lane;
        for (; i + 192 < n_cols; i += 256) {
            const int c0 = cols[i], c1 = cols[i + 64], c2 = cols[i + 128], c3 = cols[i + 192];
            const uint16_t s0 = srow[c0], s1 = srow[c1], s2 = srow[c2], s3 = srow[c3];
            const double p0 = props[i], p1 = props[i + 64], p2 = props[i + 128], p3 = props[i + 192];
            const double t0 = t[s0], t1 = t[s1], t2 = t[s2], t3 = t[s3];
            acc += t0 * p0;
            acc += t1 * p1;
            acc += t2 * p2;
            acc += t3 * p3;
        }
        for (; i < n_cols; i += 64) acc += t[srow[cols[i]]] * props[i];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) { denom[j] = 1.0 / acc; llh[j] = weight[j] * log(acc); }   // (the reciprocal: pass 2 multiplies every entry of the row by it -- a division per entry before)
    }
}

// EM pass 2: part[chunk][i] = sum over the chunk's reads j (in order) of weight[j] * (P(j, i) * props[i] * (1 / denom[j])).
// A thread per column; the chunks are added in chunk order by k_meta_fold.
__global__ void k_meta_colsum(const uint16_t* __restrict__ score, int n_cand, const int* __restrict__ cols, int n_cols, const double* __restrict__ props,
                              const int64_t* __restrict__ rows, int64_t n_rows, int64_t chunk, const uint32_t* __restrict__ tab_off,
                              const double* __restrict__ tab, const double* __restrict__ weight, const double* __restrict__ denom, double* part,
                              const int* done) {
    if (done && *done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cols) return;
    const int64_t j0 = (int64_t)blockIdx.y * chunk, j1 = j0 + chunk < n_rows ? j0 + chunk : n_rows;
    const int c = cols[i];
    const double pi = props[i];
    double acc = 0.0;
    int64_t j = j0;
    for (; j + 3 < j1; j += 4) {   // (same order of additions, four reads' loads in flight)
        const int64_t r0 = rows[j], r1 = rows[j + 1], r2 = rows[j + 2], r3 = rows[j + 3];
        const uint32_t o0 = tab_off[j], o1 = tab_off[j + 1], o2 = tab_off[j + 2], o3 = tab_off[j + 3];
        const uint16_t s0 = score[(size_t)r0 * (size_t)n_cand + (size_t)c], s1 = score[(size_t)r1 * (size_t)n_cand + (size_t)c],
                       s2 = score[(size_t)r2 * (size_t)n_cand + (size_t)c], s3 = score[(size_t)r3 * (size_t)n_cand + (size_t)c];
        const double t0 = tab[o0 + s0], t1 = tab[o1 + s1], t2 = tab[o2 + s2], t3 = tab[o3 + s3];
        acc += weight[j] * (t0 * pi * denom[j]);
        acc += weight[j + 1] * (t1 * pi * denom[j + 1]);
        acc += weight[j + 2] * (t2 * pi * denom[j + 2]);
        acc += weight[j + 3] * (t3 * pi * denom[j + 3]);
    }
    for (; j < j1; ++j) acc += weight[j] * (tab[tab_off[j] + score[(size_t)rows[j] * (size_t)n_cand + (size_t)c]] * pi * denom[j]);   // denom = 1 / denominator
    part[(size_t)blockIdx.y * (size_t)n_cols + (size_t)i] = acc;
}

// the seedmer lists of a chunk of reads from their slot stretches (k_seed_histogram, list mode: entry e of read r at
// woff[r] * 32 + e) to contiguous arrays; eight lanes per read
__global__ void __launch_bounds__(256) k_meta_gather_lists(const uint64_t* __restrict__ list_hash, const uint8_t* __restrict__ list_rev,
                                                          const int64_t* __restrict__ woff, const int64_t* __restrict__ out_off, int64_t n_reads,
                                                          uint64_t* __restrict__ out_hash, uint8_t* __restrict__ out_rev) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_thr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = gid >> 3; r < n_reads; r += n_thr >> 3) {
        const int64_t src = woff[r] * 32, dst = out_off[r], n = out_off[r + 1] - dst;
        for (int64_t e = gid & 7; e < n; e += 8) { out_hash[dst + e] = list_hash[src + e]; out_rev[dst + e] = list_rev[src + e]; }
    }
}

__global__ void k_meta_fold(const double* __restrict__ part, int n_chunks, int n_cols, double scale, double* out, const int* done) {
    if (done && *done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cols) return;
    double acc = 0.0;
    int c = 0;
    for (; c + 8 <= n_chunks; c += 8) {   // (same order of additions, eight loads in flight)
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(c + u) * (size_t)n_cols + (size_t)i];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; c < n_chunks; ++c) acc += part[(size_t)c * (size_t)n_cols + (size_t)i];
    out[i] = acc * scale;
}

// sums of 1,024 contiguous values each, a wave per block in a FIXED order (lane l adds v[l], v[l + 64], ... in order, a fixed
// butterfly adds the lanes); the host adds the block sums in order.  (One thread per block took 104 us per likelihood.)
__global__ void k_meta_sum_blocks(const double* __restrict__ v, int64_t n, double* block_sums, const int* done) {
    if (done && *done) return;
    const int lane = threadIdx.x & 63;
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t lo = b * kSumBlock, hi = lo + kSumBlock < n ? lo + kSumBlock : n;
    if (lo >= n) return;
    double acc = 0.0;
    for (int64_t i = lo + lane; i < hi; i += 64) acc += v[i];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) block_sums[b] = acc;
}

// ---- the SQUAREM iteration's vector arithmetic on the device (runSquareEM, src/mgsr.cpp:4394-4443).  The vectors have a few
// thousand entries; every sum runs in index order on one thread, exactly as the host loop they replace did, so the results are
// the same numbers -- what is gone is four host round trips per iteration.  One block of 256 threads each.
struct EmCtl {
    double llh, llh2, llh_sq, difference;
    int done, iterations;
};
// v <- v with non-positive entries raised to 1e-12, divided by its sum (normalizeProps, :4374-4383); src may equal dst
// (the in-order sums run on one thread over a copy of the vector in LDS: straight from global memory a dependent load per
//  element made each of them ~130 us)
__device__ __forceinline__ double em_sum_in_order(const double* lds_v, int n) {
    double s = 0.0;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        const double a0 = lds_v[i], a1 = lds_v[i + 1], a2 = lds_v[i + 2], a3 = lds_v[i + 3], a4 = lds_v[i + 4], a5 = lds_v[i + 5], a6 = lds_v[i + 6], a7 = lds_v[i + 7];
        s += a0; s += a1; s += a2; s += a3; s += a4; s += a5; s += a6; s += a7;
    }
    for (; i < n; ++i) s += lds_v[i];
    return s;
}
__global__ void k_em_normalize(const double* src, double* dst, int n, const EmCtl* ctl, double* work) {
    if (ctl->done) return;
    extern __shared__ double em_lds_[];
    double* em_lds = work ? work : em_lds_;   // (more columns than LDS holds: a scratch vector in global memory)
    __shared__ double s_sum;
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const double x = src[i]; em_lds[i] = x <= 0 ? 1e-12 : x; }
    __syncthreads();
    if (threadIdx.x == 0) s_sum = em_sum_in_order(em_lds, n);
    __syncthreads();
    const double s = s_sum;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = em_lds[i] / s;
}
__global__ void k_em_copy(const double* src, double* dst, int n, const EmCtl* ctl) {
    if (ctl->done) return;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
// the squared-extrapolation point: alpha = -|r| / |v|, sq = p0 - 2 alpha r + alpha^2 v, normalised
__global__ void k_em_extrapolate(const double* p0, const double* p1, const double* p2, double* sq, int n, const EmCtl* ctl, double* work) {
    if (ctl->done) return;
    extern __shared__ double em_lds_[];   // r*r, then v*v, then the extrapolated point: n entries each
    double* em_lds = work ? work : em_lds_;
    __shared__ double s_alpha, s_sum;
    double* rr = em_lds;
    double* vv = em_lds + n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double r = p1[i] - p0[i], v = (p2[i] - p1[i]) - r;
        rr[i] = r * r;
        vv[i] = v * v;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_alpha = -sqrt(em_sum_in_order(rr, n)) / sqrt(em_sum_in_order(vv, n));
    __syncthreads();
    const double alpha = s_alpha;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double r = p1[i] - p0[i], v = (p2[i] - p1[i]) - r;
        const double x = p0[i] - 2.0 * alpha * r + alpha * alpha * v;
        rr[i] = x <= 0 ? 1e-12 : x;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_sum = em_sum_in_order(rr, n);
    __syncthreads();
    const double s = s_sum;
    for (int i = threadIdx.x; i < n; i += blockDim.x) sq[i] = rr[i] / s;
}
// the block sums of a likelihood pass, added in order (getExp, :4385-4388): which = 0 -> llh2, 1 -> llh_sq
__global__ void k_em_store_llh(const double* bsum, int64_t n_bsum, EmCtl* ctl, int which) {
    if (ctl->done || threadIdx.x != 0) return;
    double s = 0.0;
    for (int64_t i = 0; i < n_bsum; ++i) s += bsum[i];
    if (which == 0) ctl->llh2 = s; else ctl->llh_sq = s;
}
// keep the extrapolated point unless it lost likelihood; count the iteration; test convergence (:4424-4441)
__global__ void k_em_choose(const double* p0, const double* p2, const double* sq, double* props, int n, EmCtl* ctl, double convergence, double delta_threshold) {
    if (ctl->done) return;
    __shared__ int s_take_sq;
    if (threadIdx.x == 0) s_take_sq = ctl->llh_sq > ctl->llh2 - convergence ? 1 : 0;
    __syncthreads();
    const double* from = s_take_sq ? sq : p2;
    for (int i = threadIdx.x; i < n; i += blockDim.x) props[i] = from[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        const double now = s_take_sq ? ctl->llh_sq : ctl->llh2;
        const double difference = now - ctl->llh;
        ctl->difference = difference;
        ctl->llh = now;
        ++ctl->iterations;
        if (delta_threshold == 0) {
            if (fabs(difference) < convergence) ctl->done = 1;
        } else {
            double mc = 0.0;
            for (int i = 0; i < n; ++i) { const double d = fabs(from[i] - p0[i]); mc = mc > d ? mc : d; }   // (a maximum: any order)
            if (mc < delta_threshold) ctl->done = 1;
        }
    }
}
}  // namespace

namespace {
// the order of merged reads: lexicographic on the hash list, then on the orientation list (the order the vector comparisons gave)
int cmp_lists(const uint64_t* xh, const uint8_t* xv, int64_t xn, const uint64_t* yh, const uint8_t* yv, int64_t yn) {
    const int64_t nmin = std::min(xn, yn);
    for (int64_t i = 0; i < nmin; ++i)
        if (xh[i] != yh[i]) return xh[i] < yh[i] ? -1 : 1;
    if (xn != yn) return xn < yn ? -1 : 1;
    const int c = memcmp(xv, yv, (size_t)xn);
    return c < 0 ? -1 : c > 0 ? 1 : 0;
}

// --gpus N: every rank's merged run (sorted, distinct lists with multiplicities) to every rank -- the counts first, then one
// max-padded all-gather of the bytes -- and a k-way merge into the whole sample's run, multiplicities added.  Equal to what
// one rank makes of all the reads: a sort of the union with equal lists merged.  to_whole: for every merged read of THIS rank's
// run (before the merge) the index of the whole sample's merged read that took it.
void merge_runs_over_ranks(pmx_meta* m, const std::vector<int64_t>& counts, int k, std::vector<int64_t>& to_whole) {
    pmx_ctx* ctx = m->ctx;
    const int world = (int)(counts.size() / (size_t)k);
    const bool amps = m->amp_on;   // (the same on every rank: merge_over_ranks checked); then the amplicon of every read ends the run
    auto amp_at = [](int64_t nr, int64_t ns) { return (size_t)(16 * nr + 8 * ns + ((ns + 7) & ~(int64_t)7)); };
    auto run_bytes = [&](int64_t nr, int64_t ns) { return amp_at(nr, ns) + (amps ? (size_t)((4 * nr + 7) & ~(int64_t)7) : 0); };
    size_t mx = 8;
    for (int r = 0; r < world; ++r) mx = std::max(mx, run_bytes(counts[(size_t)r * k + 3], counts[(size_t)r * k + 4]));
    // this rank's run: lengths, multiplicities (int64), hashes (uint64), orientations (bytes)
    const int64_t nr = m->n_reads, ns = m->n_seedmers;
    const int rank = pmx_dist_rank(m->dist);
    to_whole.assign((size_t)nr, -1);
    std::vector<char> mine(mx, 0);
    for (int64_t i = 0; i < nr; ++i) {
        const int64_t len = m->h_read_off[(size_t)i + 1] - m->h_read_off[(size_t)i];
        memcpy(mine.data() + 8 * i, &len, 8);
    }
    if (nr > 0) memcpy(mine.data() + 8 * nr, m->h_mult.data(), 8 * (size_t)nr);
    if (ns > 0) {
        memcpy(mine.data() + 16 * nr, m->h_seed_hash.data(), 8 * (size_t)ns);
        memcpy(mine.data() + 16 * nr + 8 * ns, m->h_seed_rev.data(), (size_t)ns);
    }
    if (amps && nr > 0) memcpy(mine.data() + amp_at(nr, ns), m->h_read_amp.data(), 4 * (size_t)nr);
    DevBuf<char> d_mine, d_all;
    d_mine.alloc(mx);
    d_all.alloc(mx * (size_t)world);
    std::vector<char> all(mx * (size_t)world);
    PMX_H2D(d_mine, mine, mx, ctx->stream);
    dist_all_gather(m->dist, d_mine.p, mx, d_all.p);
    PMX_D2H_SYNC(all, d_all, ctx->stream);
    struct Run { const int64_t *len, *mult; const uint64_t* h; const uint8_t* v; const int32_t* amp; int64_t n, i, at; };
    std::vector<Run> runs;
    for (int r = 0; r < world; ++r) {
        const char* b = all.data() + (size_t)r * mx;
        const int64_t rn = counts[(size_t)r * k + 3], rs = counts[(size_t)r * k + 4];
        runs.push_back(Run{(const int64_t*)b, (const int64_t*)(b + 8 * rn), (const uint64_t*)(b + 16 * rn), (const uint8_t*)(b + 16 * rn + 8 * rs),
                           amps ? (const int32_t*)(b + amp_at(rn, rs)) : nullptr, rn, 0, 0});
    }
    auto cmp_heads = [amps](const Run& x, const Run& y) {
        if (amps && x.amp[x.i] != y.amp[y.i]) return x.amp[x.i] < y.amp[y.i] ? -1 : 1;
        return cmp_lists(x.h + x.at, x.v + x.at, x.len[x.i], y.h + y.at, y.v + y.at, y.len[y.i]);
    };
    m->h_read_off.assign(1, 0);
    m->h_seed_hash.clear(); m->h_seed_rev.clear(); m->h_mult.clear();
    std::vector<int32_t> merged_amp;
    for (;;) {
        int lo = -1;
        for (int r = 0; r < world; ++r)
            if (runs[r].i < runs[r].n && (lo < 0 || cmp_heads(runs[r], runs[lo]) < 0)) lo = r;
        if (lo < 0) break;
        const Run head = runs[lo];
        const int64_t len = head.len[head.i];
        m->h_seed_hash.insert(m->h_seed_hash.end(), head.h + head.at, head.h + head.at + len);
        m->h_seed_rev.insert(m->h_seed_rev.end(), head.v + head.at, head.v + head.at + len);
        m->h_read_off.push_back((int64_t)m->h_seed_hash.size());
        if (amps) merged_amp.push_back(head.amp[head.i]);
        int64_t mult = 0;
        for (int r = lo; r < world; ++r) {   // (a run holds a list once; the ranks below `lo` hold greater heads)
            Run& x = runs[r];
            if (x.i < x.n && (r == lo || cmp_heads(x, head) == 0)) {
                mult += x.mult[x.i];
                if (r == rank) to_whole[(size_t)x.i] = (int64_t)m->h_mult.size();   // (the merged read made by this turn of the loop)
                x.at += x.len[x.i];
                ++x.i;
            }
        }
        m->h_mult.push_back(mult);
    }
    m->h_read_amp.swap(merged_amp);
    m->n_reads = (int64_t)m->h_mult.size();
    m->n_seedmers = (int64_t)m->h_seed_hash.size();
}

// scores of merged reads [first, first + count) against the candidates (the masks of pmx_meta_score) into out[count][n_cand]
void score_rows(pmx_ctx* ctx, pmx_meta* m, int64_t first, int64_t count, uint16_t* out) {
    if (count <= 0) return;
    const int n_cand = (int)m->cand.size(), words = (n_cand + 63) / 64;
    const int64_t threads = count * (int64_t)words;
    const dim3 grid(grid_for(threads, 256, ctx->n_cu * 16)), block(256);
    meta_with_planes(m->longest, [&](auto planes) {
        PMX_LAUNCH(k_meta_scores<decltype(planes)::value>, grid, block, 0, ctx->stream, m->d_read_off.p + first, m->d_seed_uid.p, m->d_seed_rev.p, count,
                   m->mask_fwd.p, m->mask_rev.p, words, n_cand, out);
    });
}

// a read set made inside a step: released when the step ends, on every way out of it (the step's caller has set the device)
using ReadSetGuard = std::unique_ptr<pmx_readset>;

// the place stage's parameters for the overlap coefficients: every read seed kept, of the reads without their masked ends
pmx_place_params overlap_place_params(const pmx_meta* m) {
    pmx_place_params pp;
    memset(&pp, 0, sizeof(pp));
    pp.min_read_support = 1;
    pp.trim_start = pp.trim_end = meta_read_end_trim(m);
    return pp;
}

// One call of pmx_meta_set_reads: one function per step, in the order the entry point calls them.  A step that calls into the
// read-set or place API returns that API's code; the others throw (HipError).
struct MetaReads {
    pmx_ctx* const ctx;
    pmx_meta* const m;
    // the sample: the caller's reads, after drop_dusty the kept ones (kept_concat / kept_off hold them when any read was dropped)
    const char* concat;
    const int64_t* offsets;
    int64_t n_reads;
    std::string kept_concat;
    std::vector<int64_t> kept_off;
    std::vector<int64_t> kept_raw;    // kept read -> the caller's read (filled when any read was dropped)
    const int64_t n_raw;              // reads the caller passed
    int64_t n_dusty = 0;              // of them, dropped by --dust
    int64_t n_kept_all;               // kept reads of the whole sample (--gpus N: over all ranks)
    // seedmer_lists: the flat seedmer lists of the kept reads, read r at [r_off[r], r_off[r + 1])
    std::vector<int64_t> r_off;
    std::vector<uint64_t> r_hash;
    std::vector<uint8_t> r_rev;
    // what the chunks of seedmer_lists share, for as long as that step runs: the launch plan and the device arrays
    struct ListChunks {
        SeedParams sp;
        size_t lds = 0;                    // dynamic LDS of k_seed_histogram
        DevBuf<uint64_t> d_lh, d_oh;       // hashes: per slot / gathered
        DevBuf<uint8_t> d_lr, d_or;        // orientations: per slot / gathered
        DevBuf<uint32_t> d_ln;             // seedmers per read
        DevBuf<int64_t> d_ooff;            // offsets of the gathered lists
        DevBuf<unsigned long long> d_ctr;  // the seeding kernel's counters (not read here)
    };

    // amplicons (pmx_meta_set_amplicons): whether they are set; then m->amp_of_raw holds the amplicon of every read the caller passed
    const bool amplicons;

    MetaReads(pmx_ctx* c, pmx_meta* mm, const char* cc, const int64_t* off, int64_t n)
        : ctx(c), m(mm), concat(cc), offsets(off), n_reads(n), n_raw(n), n_kept_all(n), amplicons(mm->amp_set) {}
    int32_t amp_of(int64_t kept) const { return m->amp_of_raw[(size_t)(kept_raw.empty() ? kept : kept_raw[(size_t)kept])]; }
    struct ListView { const uint64_t* h; const uint8_t* v; int64_t n; };
    ListView list(int64_t r) const { return ListView{r_hash.data() + r_off[(size_t)r], r_rev.data() + r_off[(size_t)r], r_off[(size_t)r + 1] - r_off[(size_t)r]}; }
    // (lexicographic on the hash list, then on the orientation list: the order the vector comparisons gave)
    int cmp(int64_t a, int64_t b) const { const ListView x = list(a), y = list(b); return cmp_lists(x.h, x.v, x.n, y.h, y.v, y.n); }

    int check_settings() const;
    void drop_dusty();
    int seedmer_lists();
    int seedmer_lists_chunk(ListChunks& lc, int64_t c0, int64_t nc);
    void merge_equal_lists();
    void amplicon_tallies();
    int merge_over_ranks();
    void upload_lists();
    int overlap_coefficients();
};

// The masking parameters and the amplicons as the setters left them (src/mgsr.cpp:2049-2053; a relative parameter without
// amplicons would do nothing in the reference, whose single group is the unlisted one: refused).  Reads: them, n_raw.
// Leaves nothing: PMX_OK, or the refusal.
int MetaReads::check_settings() const {
    if (meta_masks_above_zero(m->lowcov_reads, m->lowcov_seeds, m->lowcov_reads_rf, m->lowcov_seeds_rf) > 1)
        return fail(PMX_ERR_ARG, "Only one masking parameter can be set at a time");
    if ((m->lowcov_reads_rf > 0 || m->lowcov_seeds_rf > 0) && !m->amp_set)
        return fail(PMX_ERR_ARG, "pmx_meta_set_reads: a relative-frequency mask needs amplicons (pmx_meta_set_amplicons): its threshold is a share of "
                                 "the reads of an amplicon group, and without groups every read is unlisted and takes no relative threshold");
    if (m->amp_set && (int64_t)m->amp_of_raw.size() != n_raw)
        return fail(PMX_ERR_ARG, "pmx_meta_set_reads: " + std::to_string(n_raw) + " reads, but pmx_meta_set_amplicons named the amplicons of " +
                                     std::to_string(m->amp_of_raw.size()));
    return PMX_OK;
}

// --dust.  Reads: the caller's reads, m->dust_threshold, m->mask_read_ends.  Leaves: concat / offsets / n_reads describe the kept reads only
// (re-concatenated when any was dropped), n_dusty, n_kept_all.  Nothing below knows about DUST.
void MetaReads::drop_dusty() {
    const double dust_thr = m->dust_threshold;
    if (!(dust_thr < 100.0)) return;
    // src/mgsr.cpp:1593-1594: a read with a non-zero score above the threshold is left out
    // --mask-read-ends: the score is the trimmed read's, a slice of the caller's bytes; a read trimmed to nothing scores 0 and stays
    const int64_t ends = m->mask_read_ends;
    std::vector<uint8_t> dusty((size_t)n_reads, 0);
    unsigned n_thr = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n_reads < 4096) n_thr = 1;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < n_thr; ++t)
        pool.emplace_back([&, t]() {
            for (int64_t r = (int64_t)t; r < n_reads; r += n_thr) {
                const int64_t len = offsets[r + 1] - offsets[r];
                const double d = ends > 0 && len <= 2 * ends ? 0.0 : pmx_read_dust(concat + offsets[r] + ends, len - 2 * ends, 64);
                if (d != 0 && d > dust_thr) dusty[(size_t)r] = 1;
            }
        });
    for (auto& th : pool) th.join();
    // the dusty reads leave the sample altogether (src/mgsr.cpp:1590-1597: they never enter seqToIndexVec), the overlap
    // coefficients included: everything below sees the kept reads only
    for (uint8_t d : dusty) n_dusty += d;
    if (n_dusty == 0) return;
    kept_off.push_back(0);
    for (int64_t r = 0; r < n_reads; ++r) {
        if (dusty[(size_t)r]) continue;
        kept_concat.append(concat + offsets[r], (size_t)(offsets[r + 1] - offsets[r]));
        kept_off.push_back((int64_t)kept_concat.size());
        kept_raw.push_back(r);
    }
    concat = kept_concat.data();
    offsets = kept_off.data();
    n_reads = n_kept_all = (int64_t)kept_off.size() - 1;
}

// The reads' seedmer lists ON THE DEVICE (round 4; src/mgsr.cpp:1774-2237): the reads are packed 2 bit/base like any read set
// and the generic seeding kernel runs in its list mode (k_seed_histogram: same syncmers, same k-min-mers as the place stage,
// orientation = R < F); a gather makes the lists contiguous.  Chunks of reads bound the list arrays (one slot per base).
// Reads: concat / offsets / n_reads.  Leaves: r_off / r_hash / r_rev.
int MetaReads::seedmer_lists() {
    const SyncmerParams& p = m->params;
    ListChunks lc;
    SeedParams& sp = lc.sp;
    // --mask-read-ends: the kernel's per-end trim keeps the k-mers inside read[n : len - n] -- the trimmed string's -- and its
    // k-min-mer windows run over those alone; the reads themselves are uploaded whole
    sp.k = p.k; sp.s = p.s; sp.t = p.t; sp.l = p.l; sp.open = p.open ? 1 : 0; sp.trim_start = sp.trim_end = meta_read_end_trim(m);
    const int w = sp.k - sp.s + 1;
    const size_t lds = lc.lds = (size_t)(2 * w + p.l) * PMX_SEED_BLOCK * sizeof(uint64_t) + (size_t)(PMX_SEED_BLOCK / 64) * (PMX_SEED_QCAP * sizeof(uint64_t) + 8);
    if (lds > 160 * 1024) return fail(PMX_ERR_UNSUPPORTED, "k-s+1 too large for the LDS ring");
    if (lds > 64 * 1024) PMX_HIP(hipFuncSetAttribute((const void*)k_seed_histogram, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    r_off.assign((size_t)n_reads + 1, 0);
    lc.d_ctr.alloc(PMX_CTR_N);
    PMX_ZERO(lc.d_ctr, PMX_CTR_N, ctx->stream);
    for (int64_t c0 = 0; c0 < n_reads; c0 += kListChunk) {
        const int rc = seedmer_lists_chunk(lc, c0, std::min(n_reads, c0 + kListChunk) - c0);
        if (rc != PMX_OK) return rc;
    }
    return PMX_OK;
}

// One chunk: upload and pack reads [c0, c0 + nc), the seeding kernel in list mode (entry e of read r in slot woff[r] * 32 + e,
// the count in d_ln[r]), the counts to the host for the offsets, the gather, the lists to the host.
// Leaves: r_off (c0, c0 + nc], r_hash / r_rev grown by the chunk's seedmers.
int MetaReads::seedmer_lists_chunk(ListChunks& lc, int64_t c0, int64_t nc) {
    pmx_readset* rs = nullptr;
    int rc = pmx_readset_upload(ctx, concat, offsets + c0, nc, &rs);
    if (rc != PMX_OK) return rc;
    const ReadSetGuard rs_guard(rs);
    rc = pmx_readset_pack(ctx, rs);
    if (rc != PMX_OK) return rc;
    const size_t slots = (size_t)std::max<int64_t>(rs->n_words, 1) * 32;
    lc.d_lh.ensure(slots); lc.d_lr.ensure(slots); lc.d_ln.ensure((size_t)nc);
    PMX_ZERO(lc.d_ln, nc, ctx->stream);
    PMX_LAUNCH(k_seed_histogram, dim3(grid_for(nc, PMX_SEED_BLOCK, ctx->n_cu * 16)), dim3(PMX_SEED_BLOCK), lc.lds, ctx->stream, rs->words.p, rs->amb.p,
               rs->woff.p, rs->off.p, (int64_t)0, nc, lc.sp, (uint64_t*)nullptr, (unsigned long long*)nullptr, (uint64_t)0, lc.d_ctr.p,
               (const uint8_t*)nullptr, (const uint8_t*)nullptr, 0, lc.d_lh.p, lc.d_lr.p, lc.d_ln.p);
    std::vector<uint32_t> h_n((size_t)nc);
    PMX_D2H_SYNC(h_n, lc.d_ln, nc, ctx->stream);
    std::vector<int64_t> o_off((size_t)nc + 1, 0);
    for (int64_t i = 0; i < nc; ++i) o_off[(size_t)i + 1] = o_off[(size_t)i] + (int64_t)h_n[(size_t)i];
    const int64_t tot = o_off[(size_t)nc];
    const size_t base = r_hash.size();
    r_hash.resize(base + (size_t)tot);
    r_rev.resize(base + (size_t)tot);
    if (tot > 0) {
        lc.d_ooff.ensure((size_t)nc + 1); lc.d_oh.ensure((size_t)tot); lc.d_or.ensure((size_t)tot);
        PMX_H2D(lc.d_ooff, o_off, (size_t)nc + 1, ctx->stream);
        PMX_LAUNCH(k_meta_gather_lists, dim3(grid_for(nc * 8, 256, ctx->n_cu * 16)), dim3(256), 0, ctx->stream, lc.d_lh.p, lc.d_lr.p, rs->woff.p,
                   lc.d_ooff.p, nc, lc.d_oh.p, lc.d_or.p);
        PMX_D2H(r_hash.data() + base, lc.d_oh, tot, ctx->stream);
        PMX_D2H_SYNC(r_rev.data() + base, lc.d_or, tot, ctx->stream);
    }
    for (int64_t i = 0; i < nc; ++i) r_off[(size_t)(c0 + i) + 1] = (int64_t)base + o_off[(size_t)i + 1];
    return PMX_OK;
}

// Reads with the same seedmer list (hash and orientation, in order) are one read with a multiplicity; a read without
// seedmers scores 0 everywhere and carries no weight in the EM (src/mgsr.cpp:8170-8173): dropped here.
// Reads: r_off / r_hash / r_rev.  Leaves: m->h_read_off / h_seed_hash / h_seed_rev / h_mult, sorted by cmp_lists, with
// m->n_reads / n_seedmers, this rank's raw and dropped counts, and m->h_raw_to_merged (the caller's read -> its merged read).
void MetaReads::merge_equal_lists() {
    std::vector<int64_t> order;
    for (int64_t r = 0; r < n_reads; ++r)
        if (r_off[(size_t)r + 1] > r_off[(size_t)r]) order.push_back(r);
    // amplicons: reads are merged within their amplicon only, the amplicon is the first key of the order; N_g counts the reads
    // the caller passed (readSequencesByGroup[groupId].size(): before DUST, reads without seedmers included)
    m->amp_on = amplicons;
    m->n_amp = amplicons ? m->amp_n_groups + 1 : 0;
    m->h_read_amp.clear();
    m->ampc_group.clear(); m->ampc_hash.clear(); m->ampc_count.clear();
    m->amp_raw.assign((size_t)m->n_amp, 0);
    m->amp_thr.assign((size_t)m->n_amp, 0);
    std::vector<int32_t> group;   // per kept read
    if (amplicons) {
        for (int32_t g : m->amp_of_raw) ++m->amp_raw[(size_t)g];
        group.resize((size_t)n_reads);
        for (int64_t r = 0; r < n_reads; ++r) group[(size_t)r] = amp_of(r);
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            if (group[(size_t)a] != group[(size_t)b]) return group[(size_t)a] < group[(size_t)b];
            const int c = cmp(a, b);
            return c < 0 || (c == 0 && a < b);
        });
    } else {
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { const int c = cmp(a, b); return c < 0 || (c == 0 && a < b); });
    }
    m->n_raw_reads = n_raw;
    m->n_dust_dropped = n_dusty;
    m->h_read_off.assign(1, 0);
    m->h_seed_hash.clear(); m->h_seed_rev.clear(); m->h_mult.clear();
    m->h_raw_to_merged.assign((size_t)n_raw, -1);
    for (size_t i = 0; i < order.size(); ++i) {
        const bool copy = i > 0 && (!amplicons || group[(size_t)order[i - 1]] == group[(size_t)order[i]]) && cmp(order[i - 1], order[i]) == 0;
        if (amplicons && !copy) m->h_read_amp.push_back(group[(size_t)order[i]]);
        const int64_t raw = kept_raw.empty() ? order[i] : kept_raw[(size_t)order[i]];
        m->h_raw_to_merged[(size_t)raw] = (int64_t)m->h_mult.size() - (copy ? 1 : 0);   // the merged read made last, or the one made now
        if (copy) { ++m->h_mult.back(); continue; }
        const ListView o = list(order[i]);
        m->h_seed_hash.insert(m->h_seed_hash.end(), o.h, o.h + o.n);
        m->h_seed_rev.insert(m->h_seed_rev.end(), o.v, o.v + o.n);
        m->h_read_off.push_back((int64_t)m->h_seed_hash.size());
        m->h_mult.push_back(1);
    }
    m->n_reads = (int64_t)m->h_mult.size();
    m->n_seedmers = (int64_t)m->h_seed_hash.size();
    amplicon_tallies();
}

// the merged reads of every amplicon, before a mask (and left, until a mask says otherwise)
void MetaReads::amplicon_tallies() {
    m->amp_before.assign((size_t)m->n_amp, 0);
    for (int32_t g : m->h_read_amp) ++m->amp_before[(size_t)g];
    m->amp_left = m->amp_before;
}

// --gpus N: the ranks' runs become the whole sample's; the raw, DUST-dropped and kept read counts are summed, with amplicons
// also the raw reads of every amplicon (the run carries the amplicon of every merged read, and the merge compares it first).
// The sixth count is the rank's number of amplicon groups + 1 (0 without amplicons): ranks that disagree all return
// PMX_ERR_ARG here, after the exchange that showed it to each of them and before any further collective.
// Reads and leaves what merge_equal_lists left, now for the whole sample, on every rank.
int MetaReads::merge_over_ranks() {
    const int k = 6;
    const int64_t mine[k] = {n_raw, n_dusty, n_reads, m->n_reads, m->n_seedmers, (int64_t)m->n_amp};
    const std::vector<int64_t> counts = dist_exchange_counts(m->dist, mine, k);
    const size_t world = counts.size() / k;
    for (size_t r = 0; r < world; ++r)
        if (counts[k * r + 5] != counts[5])
            return fail(PMX_ERR_ARG, "pmx_meta_set_reads: the ranks disagree on the amplicon groups (rank " + std::to_string(r) + " has " +
                                         std::to_string(counts[k * r + 5] - 1) + ", rank 0 has " + std::to_string(counts[5] - 1) + "; -1 = none set)");
    m->n_raw_reads = m->n_dust_dropped = n_kept_all = 0;
    for (size_t r = 0; r < world; ++r) { m->n_raw_reads += counts[k * r]; m->n_dust_dropped += counts[k * r + 1]; n_kept_all += counts[k * r + 2]; }
    if (amplicons) {
        const std::vector<int64_t> raw = dist_exchange_counts(m->dist, m->amp_raw.data(), m->n_amp);
        m->amp_raw.assign((size_t)m->n_amp, 0);
        for (size_t r = 0; r < world; ++r)
            for (int32_t g = 0; g < m->n_amp; ++g) m->amp_raw[(size_t)g] += raw[r * (size_t)m->n_amp + (size_t)g];
    }
    std::vector<int64_t> to_whole;
    merge_runs_over_ranks(m, counts, k, to_whole);
    amplicon_tallies();
    // (the merged reads are the whole sample's now: this rank's raw reads, in shard order, name them through the merge)
    for (int64_t& to : m->h_raw_to_merged)
        if (to >= 0) to = to_whole[(size_t)to];
    return PMX_OK;
}

// Reads: the merged lists in m->h_*.  Leaves: m->h_uniq (the distinct hashes, ascending) and, on the device, the offsets,
// every seedmer as its index into h_uniq with its orientation, and h_uniq itself.
void MetaReads::upload_lists() {
    m->h_uniq = m->h_seed_hash;
    std::sort(m->h_uniq.begin(), m->h_uniq.end());
    m->h_uniq.erase(std::unique(m->h_uniq.begin(), m->h_uniq.end()), m->h_uniq.end());
    std::vector<uint32_t>& uid = m->h_seed_uid;
    uid.resize((size_t)m->n_seedmers);
    for (int64_t i = 0; i < m->n_seedmers; ++i)
        uid[(size_t)i] = (uint32_t)(std::lower_bound(m->h_uniq.begin(), m->h_uniq.end(), m->h_seed_hash[(size_t)i]) - m->h_uniq.begin());
    m->d_read_off.ensure((size_t)m->n_reads + 1);
    m->d_seed_uid.ensure((size_t)std::max<int64_t>(m->n_seedmers, 1));
    m->d_seed_rev.ensure((size_t)std::max<int64_t>(m->n_seedmers, 1));
    m->d_uniq.ensure(std::max<size_t>(m->h_uniq.size(), 1));
    PMX_H2D(m->d_read_off, m->h_read_off, (size_t)m->n_reads + 1, ctx->stream);
    if (m->n_seedmers > 0) {
        PMX_H2D(m->d_seed_uid, uid, m->n_seedmers, ctx->stream);
        PMX_H2D(m->d_seed_rev, m->h_seed_rev, m->n_seedmers, ctx->stream);
        PMX_H2D(m->d_uniq, m->h_uniq, ctx->stream);
    }
    PMX_HIP(hipStreamSynchronize(ctx->stream));
}

// Overlap coefficients through the place stage: seed the reads on the device, score the tree with every read seed kept
// (--gpus N: each rank seeds its kept reads, the histograms are merged, and every rank scores the tree with the whole
//  sample's kept-read count -- the coefficients, and so the candidates, are the same on every rank).
// Reads: concat / offsets / n_reads, n_kept_all.  Leaves: m->oc.
int MetaReads::overlap_coefficients() {
    m->oc.assign((size_t)m->n_nodes, 0.0);
    if (n_kept_all <= 0) return PMX_OK;
    pmx_readset* rs = nullptr;
    int rc = pmx_readset_upload(ctx, concat, offsets, n_reads, &rs);
    if (rc != PMX_OK) return rc;
    ReadSetGuard rs_guard(rs);
    const pmx_place_params pp = overlap_place_params(m);
    rc = pmx_readset_pack(ctx, rs);
    if (rc == PMX_OK) rc = pmx_place_reset(ctx, m->placer);
    if (rc == PMX_OK) rc = pmx_place_add_reads(ctx, m->placer, rs, &pp);
    if (rc == PMX_OK && m->dist) rc = pmx_dist_merge_histograms(m->dist, m->placer);
    return meta_overlap_from_histogram(ctx, m, rc, n_kept_all, &rs_guard);
}

// ---- pmx_meta_score's steps

// --em-leaves-only (no HIP), one flag per node: the node is a sampled genome -- its id does not begin with `node_`
// (src/mgsr.cpp:8023) -- or pmx_index_node_heads folds it onto the same head as one, which stands for the reference's "or one
// of its identicalNodeIdentifiers" (:8024-8026).  The ids are the plain index's (what the abundance file prints); an index
// adopted from arrays without ids names every node "", a sample.
std::vector<uint8_t> sampled_or_folded_with_one(const pmx_meta* m) {
    const size_t n = (size_t)m->n_nodes;
    std::vector<uint32_t> head(n);
    if (pmx_index_node_heads(m->idx_oriented, head.data()) != PMX_OK) throw std::runtime_error(pmx_last_error());
    std::vector<uint8_t> group_sampled(n, 0), eligible(n, 0);
    for (size_t v = 0; v < n; ++v) {
        const char* id = pmx_index_node_id(m->idx_std, (int64_t)v);
        if (!id || strncmp(id, "node_", 5) != 0) group_sampled[head[v]] = 1;
    }
    for (size_t v = 0; v < n; ++v) eligible[v] = group_sampled[head[v]];
    return eligible;
}

// The candidates (no HIP): the nodes of the `top_oc` best distinct overlap coefficients, or exactly the nodes of the
// override; ascending DFS indices, each once.  False: an override node out of range.  `eligible` (--em-leaves-only, one flag
// per node; null: every node): a node that is not eligible is passed over BEFORE a new rank is counted, so the ranks are those
// of the eligible nodes' coefficients (squareEM::squareEM, src/mgsr.cpp:8021-8037); an override is taken as it is.
bool select_candidates(const std::vector<double>& oc, int64_t n_nodes, int64_t top_oc, const uint32_t* cand_override, int64_t n_override,
                       const uint8_t* eligible, std::vector<uint32_t>& cand) {
    cand.clear();
    if (n_override > 0) {
        cand.assign(cand_override, cand_override + n_override);
        for (uint32_t v : cand)
            if ((int64_t)v >= n_nodes) return false;
    } else {
        std::vector<uint32_t> by_oc((size_t)n_nodes);
        std::iota(by_oc.begin(), by_oc.end(), 0u);
        std::stable_sort(by_oc.begin(), by_oc.end(), [&](uint32_t a, uint32_t b) { return oc[a] > oc[b]; });
        int64_t ranks = 0;
        double cur = -1.0;
        for (uint32_t v : by_oc) {
            if (eligible && !eligible[v]) continue;
            if (oc[v] != cur) {
                cur = oc[v];
                if (++ranks > top_oc) break;
            }
            cand.push_back(v);
        }
    }
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    return true;
}


// Reads: m->cand, the oriented index, m->d_uniq.  Leaves: m->d_cand and the two (seedmer x candidate) bit matrices,
// enqueued on the context's stream.
void build_masks(pmx_ctx* ctx, pmx_meta* m) {
    const int n_cand = (int)m->cand.size(), words = (n_cand + 63) / 64;
    m->d_cand.ensure((size_t)n_cand);
    PMX_H2D(m->d_cand, m->cand, n_cand, ctx->stream);
    const size_t mask_words = m->h_uniq.size() * (size_t)words;
    m->mask_fwd.ensure(std::max<size_t>(mask_words, 1));
    m->mask_rev.ensure(std::max<size_t>(mask_words, 1));
    PMX_ZERO(m->mask_fwd, std::max<size_t>(mask_words, 1), ctx->stream);
    PMX_ZERO(m->mask_rev, std::max<size_t>(mask_words, 1), ctx->stream);
    if (m->n_changes > 0)
        PMX_LAUNCH(k_meta_mask_events, dim3(grid_for(m->n_changes, 256, ctx->n_cu * 8)), dim3(256), 0, ctx->stream, m->ch_key.p, m->ch_pc.p,
                   m->ch_cc.p, m->ch_node.p, m->n_changes, m->subtree_end.p, m->d_uniq.p, (int64_t)m->h_uniq.size(), m->d_cand.p, n_cand, words,
                   m->mask_fwd.p, m->mask_rev.p);
}

// ---- pmx_meta_em's steps

// One call of pmx_meta_em, for a sample with candidates and reads: one function per step, in the order the entry point
// calls them; what a step leaves is constant afterwards.
struct EmStage {
    pmx_ctx* const ctx;
    pmx_meta* const m;
    const pmx_meta_params* const mp;
    const hipStream_t st;
    const int n_cand;
    const int64_t n_reads;
    const int world;
    // group_columns: one column per distinct score column
    std::vector<int> col_cand;                         // column -> candidate position of its representative (the group's first)
    std::vector<std::vector<uint32_t>> col_members;    // column -> the other candidates (DFS indices) with that score column
    // kept_rows_*: the merged reads the EM runs on, ascending
    DevBuf<uint64_t> d_dig;                            // the one-rank path's column digests (made on both paths)
    std::vector<int64_t> rows;
    int64_t n_rows = 0;
    // likelihood_tables, per kept row j: P(read | node) with score s at tab[tab_off[j] + s], the read's multiplicity
    std::vector<double> tab, weight;
    std::vector<uint32_t> tab_off;
    double inv_total = 0.0;                            // 1 / the sum of the weights
    int n_chunks = 0;                                  // partial column sums (kColsumChunk rows each) over all kept rows
    int64_t n_bsum = 0;                                // block sums (kSumBlock rows each) over all kept rows
    // own_em_rows: kept rows [e_first, e_first + e_count) are this rank's, as rows loc_rows[] of the matrix score_p
    int64_t e_first = 0, e_count = 0, per = 0;         // per: rows per rank in the gathers
    const uint16_t* score_p = nullptr;
    std::vector<int64_t> loc_rows;
    int loc_chunks = 0;
    int64_t loc_bsum = 0, slot_chunks = 0, slot_bsum = 0;   // this rank's partials and block sums; per rank in the gathers
    // upload_rows: device buffers of the call (the per-column ones grow in EmRound)
    DevBuf<int64_t> d_rows;
    DevBuf<uint32_t> d_tab_off;
    DevBuf<double> d_tab, d_weight, d_denom, d_llh, d_props, d_out, d_part, d_bsum, d_gpart, d_gbsum;
    DevBuf<int> d_cols;
    const double* bsum_all = nullptr;                  // the block sums of all rows: d_bsum, or (--gpus N) the gathered d_gbsum

    EmStage(pmx_ctx* c, pmx_meta* mm, const pmx_meta_params* p)
        : ctx(c), m(mm), mp(p), st(c->stream), n_cand((int)mm->cand.size()), n_reads(mm->n_reads), world(mm->dist ? pmx_dist_world(mm->dist) : 1) {
        d_dig.alloc(2 * (size_t)n_cand);
    }
    void group_columns(const std::vector<uint64_t>& digests, int n_ranks);
    void kept_rows_one_rank();
    void kept_rows_dist();
    void likelihood_tables();
    void own_em_rows();
    void upload_rows();
    void publish_groups(const std::vector<int>& cols, const std::vector<std::vector<uint32_t>>& members, const std::vector<double>& props);
};

// Columns: one per distinct score column, in the order of their first candidates.  digests[2 * (r * n_cand + c)], + 1: the
// 128-bit digest of candidate c's column over rank r's rows.  Two columns are equal iff they are equal on every rank's rows:
// the key of a column is its digests in rank order (one rank: its one digest).  The map is only asked `find` and `emplace`,
// never walked, so its ordering of the keys plays no part: a column joins the group of the first candidate with its key.
// Leaves: col_cand / col_members.
void EmStage::group_columns(const std::vector<uint64_t>& digests, int n_ranks) {
    std::map<std::vector<uint64_t>, int> first_of;
    std::vector<uint64_t> key(2 * (size_t)n_ranks);
    for (int c = 0; c < n_cand; ++c) {
        for (int r = 0; r < n_ranks; ++r) memcpy(&key[2 * (size_t)r], &digests[2 * ((size_t)r * (size_t)n_cand + (size_t)c)], 2 * sizeof(uint64_t));
        auto it = first_of.find(key);
        if (it == first_of.end()) { first_of.emplace(key, (int)col_cand.size()); col_cand.push_back(c); col_members.emplace_back(); }
        else col_members[(size_t)it->second].push_back(m->cand[(size_t)c]);
    }
}

// One rank: the column digests, then the whole score matrix to the host for the rows.
// Reads: m->score.  Leaves: the columns and `rows`, the reads that score somewhere (the others carry no weight,
// src/mgsr.cpp:8170-8173) and that --discard keeps.
void EmStage::kept_rows_one_rank() {
    PMX_LAUNCH(k_meta_column_digest, dim3((n_cand + 63) / 64), dim3(64), 0, st, m->score.p, n_reads, n_cand, d_dig.p);
    std::vector<uint64_t> dig(2 * (size_t)n_cand);
    PMX_D2H_SYNC(dig, d_dig, st);
    group_columns(dig, 1);
    std::vector<uint16_t> h_score((size_t)n_reads * (size_t)n_cand);
    PMX_D2H_SYNC(h_score, m->score, st);
    for (int64_t r = 0; r < n_reads; ++r) {
        int mx = 0;
        for (int c = 0; c < n_cand; ++c) mx = std::max<int>(mx, h_score[(size_t)r * (size_t)n_cand + (size_t)c]);
        const int64_t n_seed = m->h_read_off[(size_t)r + 1] - m->h_read_off[(size_t)r];
        // --discard (src/main.cpp:1229-1240): the threshold is TRUNCATED to an integer there,
        // `maxScore < static_cast<int>(seedmers * discard)`, so a read with int(n * d) <= max < n * d stays in the EM
        if (mx == 0 || mx < (int)((double)n_seed * mp->discard)) continue;
        rows.push_back(r);
    }
    n_rows = (int64_t)rows.size();
}

// --gpus N, pass A: the column digests of this rank's slice and its reads' --discard flags (k_meta_row_keep), one
// all-gather of both.  The groups (and their order: by first candidate) are the one-rank groups, see group_columns.
// Reads: m->score (this rank's slice).  Leaves: the columns and `rows`, the same on every rank.
void EmStage::kept_rows_dist() {
    const int64_t max_slice = (n_reads + world - 1) / world;
    const size_t dig_bytes = sizeof(uint64_t) * 2 * (size_t)n_cand, part_bytes = dig_bytes + (((size_t)max_slice + 7) & ~(size_t)7);
    DevBuf<char> d_mine, d_all;
    d_mine.alloc(part_bytes);
    d_all.alloc(part_bytes * (size_t)world);
    PMX_ZERO(d_mine, part_bytes, st);
    PMX_LAUNCH(k_meta_column_digest, dim3((n_cand + 63) / 64), dim3(64), 0, st, m->score.p, m->row_count, n_cand, (uint64_t*)d_mine.p);
    if (m->row_count > 0)
        PMX_LAUNCH(k_meta_row_keep, dim3(grid_for(m->row_count * 64, 256, ctx->n_cu * 8)), dim3(256), 0, st, m->score.p, m->row_count, n_cand,
                   m->d_read_off.p + m->row_first, mp->discard, (uint8_t*)(d_mine.p + dig_bytes));
    dist_all_gather(m->dist, d_mine.p, part_bytes, d_all.p);
    std::vector<char> all(part_bytes * (size_t)world);
    PMX_D2H_SYNC(all, d_all, st);
    std::vector<uint64_t> dig(2 * (size_t)n_cand * (size_t)world);
    for (int r = 0; r < world; ++r) memcpy(&dig[2 * (size_t)n_cand * (size_t)r], all.data() + (size_t)r * part_bytes, dig_bytes);
    group_columns(dig, world);
    for (int r = 0; r < world; ++r) {
        const int64_t f = n_reads * r / world, n = n_reads * (r + 1) / world - f;
        const uint8_t* keep = (const uint8_t*)(all.data() + (size_t)r * part_bytes + dig_bytes);
        for (int64_t i = 0; i < n; ++i)
            if (keep[i]) rows.push_back(f + i);
    }
    n_rows = (int64_t)rows.size();
}

// P(read | node) = err^(n - s) * (1 - err)^s for the distinct n of the reads: tables computed with the host libm.
// Reads: rows, the reads' lengths and multiplicities.  Leaves: tab / tab_off / weight / inv_total, n_chunks / n_bsum.
void EmStage::likelihood_tables() {
    std::map<int64_t, uint32_t> off_of_n;
    tab_off.resize((size_t)n_rows);
    weight.resize((size_t)n_rows);
    double total_weight = 0.0;
    for (int64_t j = 0; j < n_rows; ++j) {
        const int64_t r = rows[(size_t)j], n_seed = m->h_read_off[(size_t)r + 1] - m->h_read_off[(size_t)r];
        auto it = off_of_n.find(n_seed);
        if (it == off_of_n.end()) {
            it = off_of_n.emplace(n_seed, (uint32_t)tab.size()).first;
            for (int64_t s = 0; s <= n_seed; ++s) tab.push_back(std::pow(mp->error_rate, (double)(n_seed - s)) * std::pow(1.0 - mp->error_rate, (double)s));
        }
        tab_off[(size_t)j] = it->second;
        weight[(size_t)j] = (double)m->h_mult[(size_t)r];
        total_weight += weight[(size_t)j];   // (integers: exact in any order)
    }
    inv_total = 1.0 / total_weight;
    // (kColsumChunk reads per partial column sum; with 2,048: 2,200 waves for 3,000 columns x 90k reads, each a serial walk: 373 us per pass)
    n_chunks = (int)((n_rows + kColsumChunk - 1) / kColsumChunk);
    n_bsum = (n_rows + kSumBlock - 1) / kSumBlock;
}

// This rank's EM rows: all of them, or (--gpus N, pass B) a contiguous range whose bounds are multiples of both
// reduction widths -- the rank's chunk partials and block sums are then whole global ones, at global positions
// rank * per / width of the all-gathered arrays, and the one-rank fold and store kernels add them in the one-rank order.
// Reads: rows.  Leaves: e_first / e_count / per, score_p / loc_rows and the counts of partials and block sums.
void EmStage::own_em_rows() {
    e_first = 0; e_count = per = n_rows;
    score_p = m->score.p;
    loc_rows = rows;
    if (m->dist) {
        const int rank = pmx_dist_rank(m->dist);
        const int64_t align = std::lcm(kColsumChunk, kSumBlock);
        per = ((n_rows + world - 1) / world + align - 1) / align * align;
        e_first = std::min<int64_t>(n_rows, per * rank);
        e_count = std::min<int64_t>(n_rows, e_first + per) - e_first;
        // pass B: the merged reads of the range, scored again into a matrix of their own
        const int64_t r_lo = e_count > 0 ? rows[(size_t)e_first] : 0, r_hi = e_count > 0 ? rows[(size_t)(e_first + e_count - 1)] + 1 : 0;
        m->score_em.ensure((size_t)std::max<int64_t>(r_hi - r_lo, 1) * (size_t)n_cand);
        score_rows(ctx, m, r_lo, r_hi - r_lo, m->score_em.p);
        score_p = m->score_em.p;
        loc_rows.assign((size_t)e_count, 0);
        for (int64_t j = 0; j < e_count; ++j) loc_rows[(size_t)j] = rows[(size_t)(e_first + j)] - r_lo;
    }
    loc_chunks = (int)((e_count + kColsumChunk - 1) / kColsumChunk);
    loc_bsum = (e_count + kSumBlock - 1) / kSumBlock;
    slot_chunks = (per + kColsumChunk - 1) / kColsumChunk;
    slot_bsum = (per + kSumBlock - 1) / kSumBlock;
}

// Reads: loc_rows and this rank's range of tab_off / weight, tab.  Leaves: them on the device, with room for the
// denominators, the log-likelihood terms and the block sums.
void EmStage::upload_rows() {
    d_rows.alloc((size_t)e_count); d_tab_off.alloc((size_t)e_count); d_tab.alloc(tab.size()); d_weight.alloc((size_t)e_count);
    d_denom.alloc((size_t)e_count); d_llh.alloc((size_t)e_count);
    if (e_count > 0) {
        PMX_H2D(d_rows, loc_rows, e_count, st);
        PMX_H2D(d_tab_off, tab_off.data() + e_first, e_count, st);
        PMX_H2D(d_weight, weight.data() + e_first, e_count, st);
    }
    PMX_H2D(d_tab, tab, st);
    d_bsum.alloc((size_t)slot_bsum);
    if (m->dist) d_gbsum.alloc((size_t)slot_bsum * (size_t)world);
    bsum_all = m->dist ? d_gbsum.p : d_bsum.p;
}

// Reads: the columns the rounds left, with their proportions.  Leaves: m->groups, by proportion, descending.
void EmStage::publish_groups(const std::vector<int>& cols, const std::vector<std::vector<uint32_t>>& members, const std::vector<double>& props) {
    for (size_t i = 0; i < cols.size(); ++i) {
        pmx_meta_group g;
        g.node = m->cand[(size_t)cols[i]];
        g.members = members[i];
        g.prop = props[i];
        m->groups.push_back(std::move(g));
    }
    std::stable_sort(m->groups.begin(), m->groups.end(), [](const pmx_meta_group& a, const pmx_meta_group& b) { return a.prop > b.prop; });
}

// One round of the EM over the columns `cols`: its device vectors, then the SQUAREM loop.
// The whole SQUAREM loop stays on the device: the proportion vectors never leave it, the small vector arithmetic runs in
// single-block kernels with the host loop's own order of operations, and the host only looks at the convergence flag
// every 16 iterations (launches queued past convergence return at once).  Per iteration: 6 passes over the score
// matrix (4 x k_meta_denoms, 2 x k_meta_colsum) and 13 small launches; before, 4 host round trips.  --gpus N: the
// passes run over the rank's rows, and 4 all-gathers per iteration (chunk partials x 2, block sums x 2) bring every
// rank the global arrays; the single-block kernels then run replicated on identical inputs, so the convergence flag
// and the iteration count agree on every rank and every rank issues the same sequence of collectives (queued past
// convergence too).
struct EmRound {
    EmStage* const S;
    pmx_meta* const m;
    const hipStream_t st;
    const int n_cols;
    DevBuf<double> d_p0, d_p1, d_p2, d_sq;
    DevBuf<EmCtl> d_ctl;
    DevBuf<double> d_em_work;
    double* em_work = nullptr;           // the small kernels' scratch vector in global memory, when LDS cannot hold it
    const double* part_all = nullptr;    // the chunk partials of all rows: d_part, or (--gpus N) the gathered d_gpart
    const int* d_done = nullptr;
    EmCtl h_ctl;                         // as of the last look; after run, the round's iterations and log-likelihood

    EmRound(EmStage* stage, const std::vector<int>& cols);
    void denoms(const double* pr);
    void em_step(const double* from, double* to);
    void log_likelihood(const double* pr, int which);
    void run(std::vector<double>& props);
};

// Reads: the round's columns.  Leaves: them on the device, the control block zeroed, the LDS attribute of the small kernels.
EmRound::EmRound(EmStage* stage, const std::vector<int>& cols) : S(stage), m(stage->m), st(stage->st), n_cols((int)cols.size()) {
    S->d_cols.ensure((size_t)n_cols); S->d_props.ensure((size_t)n_cols); S->d_out.ensure((size_t)n_cols); S->d_part.ensure((size_t)S->slot_chunks * (size_t)n_cols);
    if (m->dist) S->d_gpart.ensure((size_t)S->slot_chunks * (size_t)n_cols * (size_t)S->world);
    part_all = m->dist ? S->d_gpart.p : S->d_part.p;
    PMX_H2D(S->d_cols, cols, n_cols, st);
    d_p0.alloc((size_t)n_cols); d_p1.alloc((size_t)n_cols); d_p2.alloc((size_t)n_cols); d_sq.alloc((size_t)n_cols);
    d_ctl.alloc(1);
    memset(&h_ctl, 0, sizeof(h_ctl));
    PMX_H2D(d_ctl, &h_ctl, 1, st);
    d_done = &d_ctl.p->done;
    // the in-order sums of the small kernels read a copy of the vector in LDS (2 x n_cols doubles at most); beyond 160 KB a
    // scratch vector in global memory stands in.  The 160 KB of a workgroup hold the kernels' static __shared__ words too
    // (s_alpha and s_sum of k_em_extrapolate): at exactly 10,240 columns the dynamic part alone fills them, and a launch
    // that asks for more is not refused with an error: the queue aborts (HSA_STATUS_ERROR_INVALID_ALLOCATION)
    const size_t em_lds = 2 * sizeof(double) * (size_t)n_cols;
    hipFuncAttributes fa_norm, fa_extra;
    PMX_HIP(hipFuncGetAttributes(&fa_norm, (const void*)k_em_normalize));
    PMX_HIP(hipFuncGetAttributes(&fa_extra, (const void*)k_em_extrapolate));
    const size_t em_static = std::max<size_t>({fa_norm.sharedSizeBytes, fa_extra.sharedSizeBytes, 2 * sizeof(double)});
    if (em_lds + em_static > (size_t)160 * 1024) { d_em_work.alloc(2 * (size_t)n_cols); em_work = d_em_work.p; }
    else if (em_lds > (size_t)64 * 1024) {
        PMX_HIP(hipFuncSetAttribute((const void*)k_em_normalize, hipFuncAttributeMaxDynamicSharedMemorySize, (int)em_lds));
        PMX_HIP(hipFuncSetAttribute((const void*)k_em_extrapolate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)em_lds));
    }
}

void EmRound::denoms(const double* pr) {
    PMX_LAUNCH(k_meta_denoms, dim3(grid_for(S->e_count * 64, 256, S->ctx->n_cu * 8)), dim3(256), 0, st, S->score_p, S->n_cand, S->d_cols.p, n_cols, pr,
               S->d_rows.p, S->e_count, S->d_tab_off.p, S->d_tab.p, S->d_weight.p, S->d_denom.p, S->d_llh.p, d_done);
}

// updateProps (src/mgsr.cpp:4341-4372) + normalizeProps
void EmRound::em_step(const double* from, double* to) {
    if (S->e_count > 0) {
        denoms(from);
        PMX_LAUNCH(k_meta_colsum, dim3((n_cols + 63) / 64, S->loc_chunks), dim3(64), 0, st, S->score_p, S->n_cand, S->d_cols.p, n_cols, from, S->d_rows.p,
                   S->e_count, kColsumChunk, S->d_tab_off.p, S->d_tab.p, S->d_weight.p, S->d_denom.p, S->d_part.p, d_done);
    }
    if (m->dist) dist_all_gather(m->dist, S->d_part.p, sizeof(double) * (size_t)S->slot_chunks * (size_t)n_cols, S->d_gpart.p);
    PMX_LAUNCH(k_meta_fold, dim3((n_cols + 63) / 64), dim3(64), 0, st, part_all, S->n_chunks, n_cols, S->inv_total, S->d_out.p, d_done);
    PMX_LAUNCH(k_em_normalize, dim3(1), dim3(256), em_work ? 0 : sizeof(double) * (size_t)n_cols, st, S->d_out.p, to, n_cols, d_ctl.p, em_work);
}

// getExp (src/mgsr.cpp:4385-4388)
void EmRound::log_likelihood(const double* pr, int which) {
    if (S->e_count > 0) {
        denoms(pr);
        PMX_LAUNCH(k_meta_sum_blocks, dim3((unsigned)((S->loc_bsum + 3) / 4)), dim3(256), 0, st, S->d_llh.p, S->e_count, S->d_bsum.p, d_done);
    }
    if (m->dist) dist_all_gather(m->dist, S->d_bsum.p, sizeof(double) * (size_t)S->slot_bsum, S->d_gbsum.p);
    PMX_LAUNCH(k_em_store_llh, dim3(1), dim3(64), 0, st, S->bsum_all, S->n_bsum, d_ctl.p, which);
}

// runSquareEM (src/mgsr.cpp:4394-4443) from uniform proportions, in batches of 16 iterations between two looks at the convergence flag.
// Leaves: props, h_ctl.
void EmRound::run(std::vector<double>& props) {
    const pmx_meta_params* mp = S->mp;
    props.assign((size_t)n_cols, 1.0 / (double)n_cols);
    PMX_H2D(S->d_props, props, n_cols, st);
    const int look_every = 16;
    for (int iter = 0; iter < mp->em_max_iterations;) {
        const int batch = std::min(look_every, mp->em_max_iterations - iter);
        for (int b = 0; b < batch; ++b) {
            PMX_LAUNCH(k_em_copy, dim3(1), dim3(256), 0, st, S->d_props.p, d_p0.p, n_cols, d_ctl.p);
            em_step(d_p0.p, d_p1.p);
            em_step(d_p1.p, d_p2.p);
            PMX_LAUNCH(k_em_extrapolate, dim3(1), dim3(256), em_work ? 0 : 2 * sizeof(double) * (size_t)n_cols, st, d_p0.p, d_p1.p, d_p2.p, d_sq.p, n_cols, d_ctl.p, em_work);
            log_likelihood(d_p2.p, 0);
            log_likelihood(d_sq.p, 1);
            PMX_LAUNCH(k_em_choose, dim3(1), dim3(256), 0, st, d_p0.p, d_p2.p, d_sq.p, S->d_props.p, n_cols, d_ctl.p, mp->em_convergence,
                       mp->em_delta_threshold);
        }
        PMX_D2H_SYNC(&h_ctl, d_ctl, 1, st);
        iter += batch;
        if (h_ctl.done) break;
    }
    PMX_D2H_SYNC(props, S->d_props, n_cols, st);
}

// removeLowPropNodes (src/mgsr.cpp:4445-4490), called after EVERY round including the last allowed one (src/main.cpp:1263-1271):
// when it removes anything the surviving nodes' proportions are reset to uniform, and if that was the last round
// the uniform vector is what the abundance file reports -- mirrored, not "fixed".  (No HIP.)  True: a column was dropped.
bool drop_low_proportions(std::vector<int>& cols, std::vector<std::vector<uint32_t>>& members, std::vector<double>& props, double prop_threshold) {
    std::vector<int> keep;
    for (int i = 0; i < (int)cols.size(); ++i)
        if (props[(size_t)i] >= prop_threshold) keep.push_back(i);
    if (keep.size() == cols.size()) return false;
    std::vector<int> cols2;
    std::vector<std::vector<uint32_t>> members2;
    for (int i : keep) { cols2.push_back(cols[(size_t)i]); members2.push_back(members[(size_t)i]); }
    cols.swap(cols2);
    members.swap(members2);
    props.assign(cols.size(), cols.empty() ? 0.0 : 1.0 / (double)cols.size());
    return true;
}
}  // namespace

// (declared in meta_state.hpp: MetaReads::overlap_coefficients and meta_mask.hip's path end here)
int meta_overlap_from_histogram(pmx_ctx* ctx, pmx_meta* m, int rc, int64_t n_kept, ReadSetGuard* seeded) {
    const pmx_place_params pp = overlap_place_params(m);
    pmx_place_result res;
    if (rc == PMX_OK) rc = pmx_place_score(ctx, m->placer, &pp, n_kept, &res);
    if (seeded) seeded->reset();
    if (rc != PMX_OK) return rc;
    std::vector<int64_t> counts2((size_t)m->n_nodes * 2);
    rc = pmx_place_node_outputs(ctx, m->placer, nullptr, nullptr, counts2.data());
    if (rc != PMX_OK) return rc;
    for (int64_t v = 0; v < m->n_nodes; ++v)
        m->oc[(size_t)v] = counts2[2 * (size_t)v + 1] > 0 ? (double)counts2[2 * (size_t)v] / (double)counts2[2 * (size_t)v + 1] : 0.0;
    return PMX_OK;
}

extern "C" {

int pmx_meta_create(pmx_ctx* ctx, const pmx_index* idx_std, const pmx_index* idx_oriented, pmx_meta** out) {
    if (!ctx || !idx_std || !idx_oriented || !out) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const LiteIndex* S = pmx_index_internal(idx_std);
    const LiteIndex* O = pmx_index_internal(idx_oriented);
    if (!O->params.oriented) return fail(PMX_ERR_ARG, "the second index must be built with PMX_INDEX_ORIENTED");
    if (S->params.oriented || S->parent != O->parent || S->params.k != O->params.k || S->params.s != O->params.s || S->params.l != O->params.l ||
        S->params.t != O->params.t || S->params.open != O->params.open)
        return fail(PMX_ERR_ARG, "the two indexes must cover the same tree with the same seeding parameters");
    std::unique_ptr<pmx_meta> m(new pmx_meta());
    m->ctx = ctx;
    m->idx_std = idx_std;
    m->idx_oriented = idx_oriented;
    m->params = O->params;
    const int64_t n = (int64_t)O->parent.size(), c = (int64_t)O->hash.size();
    m->n_nodes = n;
    m->n_changes = c;
    // nodes are in DFS pre-order: the subtree of v is the index range [v, end(v)]
    std::vector<uint32_t> end((size_t)n);
    for (int64_t v = 0; v < n; ++v) end[v] = (uint32_t)v;
    for (int64_t v = n - 1; v > 0; --v) end[O->parent[v]] = std::max(end[O->parent[v]], end[v]);
    m->h_parent = O->parent;
    m->h_subtree_end = end;
    std::vector<uint32_t> node((size_t)c);
    for (int64_t v = 0; v < n; ++v)
        for (uint64_t q = O->offsets[v]; q < O->offsets[v + 1]; ++q) node[q] = (uint32_t)v;
    m->ch_key.alloc((size_t)c); m->ch_pc.alloc((size_t)c); m->ch_cc.alloc((size_t)c); m->ch_node.alloc((size_t)c); m->subtree_end.alloc((size_t)n);
    if (c > 0) {
        PMX_H2D(m->ch_key, O->hash, c, ctx->stream);
        PMX_H2D(m->ch_pc, O->parent_count, c, ctx->stream);
        PMX_H2D(m->ch_cc, O->child_count, c, ctx->stream);
        PMX_H2D(m->ch_node, node, c, ctx->stream);
    }
    // (copies on the context's stream: synchronous null-stream copies against its blocking CU-masked queue are a suspect of
    //  the unexplained stalls)
    PMX_H2D(m->subtree_end, end, n, ctx->stream);
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    const int rc = pmx_place_create(ctx, idx_std, &m->placer);
    if (rc != PMX_OK) return rc;
    *out = m.release();
    return PMX_OK;
    PMX_CATCH
}

void pmx_meta_free(pmx_ctx* ctx, pmx_meta* m) {
    if (!m) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (m->placer) pmx_place_free(ctx, m->placer);
    delete m;
}

int pmx_meta_attach_dist(pmx_meta* m, pmx_dist* d) {
    if (!m || !d) return PMX_ERR_ARG;
    if (dist_ctx(d) != m->ctx) return fail(PMX_ERR_ARG, "pmx_meta_attach_dist: the dist must be made on the meta's context");
    if (m->reads_set) return fail(PMX_ERR_ARG, "pmx_meta_attach_dist: attach before pmx_meta_set_reads");
    m->dist = d;
    return PMX_OK;
}

int pmx_meta_row_range(const pmx_meta* m, int64_t* first, int64_t* count) {
    if (!m) return PMX_ERR_ARG;
    if (first) *first = m->row_first;
    if (count) *count = m->row_count;
    return PMX_OK;
}

// Step 1 + 2: the reads' seedmer lists (the seeding kernel in list mode), merged by list; the overlap coefficient of every
// node (place stage).  The host only filters by DUST (integer state, a few operations per base) and merges equal lists.
int pmx_meta_set_reads(pmx_ctx* ctx, pmx_meta* m, const char* concat, const int64_t* offsets, int64_t n_reads) {
    if (!ctx || !m || !offsets || n_reads < 0 || (!concat && n_reads > 0)) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    MetaReads R(ctx, m, concat, offsets, n_reads);
    int rc = R.check_settings();
    if (rc != PMX_OK) return rc;
    R.drop_dusty();
    rc = R.seedmer_lists();
    if (rc != PMX_OK) return rc;
    R.merge_equal_lists();
    if (m->dist) {
        rc = R.merge_over_ranks();
        if (rc != PMX_OK) return rc;
    }
    if (m->amp_on && meta_masks_above_zero(m->lowcov_reads, m->lowcov_seeds, m->lowcov_reads_rf, m->lowcov_seeds_rf) > 0 && m->n_seedmers >= (int64_t)UINT32_MAX)
        return fail(PMX_ERR_CAPACITY, "pmx_meta_set_reads: a mask within amplicons indexes the list entries with 32 bits; the merged reads hold 2^32 - 1 or more");
    R.upload_lists();
    // the low-coverage masks (src/mgsr.cpp:2049-2139), when one is set: the reads that survive are the sample from here on
    rc = meta_apply_masks(ctx, m) ? meta_masked_overlap_coefficients(ctx, m) : R.overlap_coefficients();
    if (rc != PMX_OK) return rc;
    m->cand.clear();
    m->groups.clear();
    m->assigned = false;
    m->best_done = m->active_built = false;
    m->row_first = 0;
    m->row_count = m->dist ? 0 : m->n_reads;
    m->read_ends_masked = m->mask_read_ends;
    m->reads_set = true;
    return PMX_OK;
    PMX_CATCH
}

// Step 2 (selection) + 3: the nodes of the `top_oc` best distinct overlap coefficients become the candidates
// (cand_override / n_override > 0: exactly these nodes instead -- tests); every (read, candidate) score.
int pmx_meta_score(pmx_ctx* ctx, pmx_meta* m, int64_t top_oc, const uint32_t* cand_override, int64_t n_override) {
    if (!ctx || !m || (n_override > 0 && !cand_override)) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    std::vector<uint8_t> eligible;
    if (m->em_leaves_only && n_override <= 0) {
        eligible = sampled_or_folded_with_one(m);
        if (std::find(eligible.begin(), eligible.end(), (uint8_t)1) == eligible.end())
            return fail(PMX_ERR_ARG, "pmx_meta_score: --em-leaves-only, and every node of the tree is named node_...: no sampled genome to choose the candidates among");
    }
    if (!select_candidates(m->oc, m->n_nodes, top_oc, cand_override, n_override, eligible.empty() ? nullptr : eligible.data(), m->cand))
        return fail(PMX_ERR_ARG, "candidate node out of range");
    m->groups.clear();
    meta_own_row_slice(m);
    if (m->cand.empty() || m->n_reads == 0) return PMX_OK;
    m->score.ensure((size_t)m->row_count * m->cand.size());
    const int rc = meta_longest_read(m);
    if (rc != PMX_OK) return rc;
    timer_begin(ctx, "meta_score");
    build_masks(ctx, m);
    score_rows(ctx, m, m->row_first, m->row_count, m->score.p);
    timer_end(ctx, "meta_score", 1);
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
    PMX_CATCH
}

int64_t pmx_meta_num_reads(const pmx_meta* m) { return m ? m->n_reads : 0; }
int64_t pmx_meta_num_candidates(const pmx_meta* m) { return m ? (int64_t)m->cand.size() : 0; }
int pmx_meta_candidates(const pmx_meta* m, uint32_t* out, int64_t cap) {
    if (!m || cap < (int64_t)m->cand.size()) return PMX_ERR_ARG;
    std::copy(m->cand.begin(), m->cand.end(), out);
    return PMX_OK;
}
int pmx_meta_overlap_coefficients(const pmx_meta* m, double* out, int64_t cap) {
    if (!m || cap < (int64_t)m->oc.size()) return PMX_ERR_ARG;
    std::copy(m->oc.begin(), m->oc.end(), out);
    return PMX_OK;
}
// the merged reads: seedmers per read (n) and multiplicities; either pointer may be NULL
int pmx_meta_read_info(const pmx_meta* m, int64_t* n_seedmers, int64_t* multiplicity, int64_t cap) {
    if (!m || cap < m->n_reads) return PMX_ERR_ARG;
    for (int64_t r = 0; r < m->n_reads; ++r) {
        if (n_seedmers) n_seedmers[r] = m->h_read_off[(size_t)r + 1] - m->h_read_off[(size_t)r];
        if (multiplicity) multiplicity[r] = m->h_mult[(size_t)r];
    }
    return PMX_OK;
}
// the merged reads' seedmers (hash, orientation) with n_reads + 1 offsets -- what the checker recomputes scores from
int pmx_meta_read_seedmers(const pmx_meta* m, int64_t* offsets, uint64_t* hash, uint8_t* rev, int64_t cap_seedmers) {
    if (!m || cap_seedmers < m->n_seedmers || !offsets) return PMX_ERR_ARG;
    std::copy(m->h_read_off.begin(), m->h_read_off.end(), offsets);
    if (hash) std::copy(m->h_seed_hash.begin(), m->h_seed_hash.end(), hash);
    if (rev) std::copy(m->h_seed_rev.begin(), m->h_seed_rev.end(), rev);
    return PMX_OK;
}
int pmx_meta_scores(pmx_ctx* ctx, pmx_meta* m, uint16_t* out, int64_t cap) {
    if (!ctx || !m || !out) return PMX_ERR_ARG;
    const int64_t n = m->row_count * (int64_t)m->cand.size();
    if (cap < n) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (n > 0) {
        PMX_D2H_SYNC(out, m->score, n, ctx->stream);
    }
    return PMX_OK;
    PMX_CATCH
}

// Step 4: merge candidates with equal score columns, SQUAREM EM, drop nodes below prop_threshold, again (<= em_max_rounds).
int pmx_meta_em(pmx_ctx* ctx, pmx_meta* m, const pmx_meta_params* mp) {
    if (!ctx || !m || !mp) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    m->groups.clear();
    m->em_rounds = m->em_iterations = 0;
    m->llh = 0.0;
    if (m->cand.empty() || m->n_reads == 0) return PMX_OK;
    EmStage S(ctx, m, mp);
    if (m->dist) S.kept_rows_dist();
    else S.kept_rows_one_rank();
    if (S.n_rows == 0) return PMX_OK;
    S.likelihood_tables();
    S.own_em_rows();
    S.upload_rows();
    std::vector<int> cols = S.col_cand;       // current columns (candidate positions)
    std::vector<std::vector<uint32_t>> members = S.col_members;
    std::vector<double> props;
    for (int round = 0; round < std::max(1, mp->em_max_rounds); ++round) {
        EmRound R(&S, cols);
        R.run(props);
        m->em_iterations += R.h_ctl.iterations;
        m->llh = R.h_ctl.llh;
        ++m->em_rounds;
        if (!drop_low_proportions(cols, members, props, mp->prop_threshold) || cols.empty()) break;
    }
    S.publish_groups(cols, members, props);
    return PMX_OK;
    PMX_CATCH
}

int pmx_meta_set_dust(pmx_meta* m, double threshold) {
    if (!m || !(threshold <= 100.0)) return PMX_ERR_ARG;      // src/main.cpp:1353-1356: --dust must be <= 100
    m->dust_threshold = threshold;
    return PMX_OK;
}

// --mask-read-ends N (src/main.cpp:2065): kept for the next pmx_meta_set_reads, like the DUST threshold
int pmx_meta_set_mask_read_ends(pmx_meta* m, int64_t n) {
    if (!m || n < 0 || n > INT32_MAX) return PMX_ERR_ARG;
    m->mask_read_ends = n;
    return PMX_OK;
}

// --em-leaves-only (src/main.cpp:2053): for the pmx_meta_score calls that follow
int pmx_meta_set_em_leaves_only(pmx_meta* m, int on) {
    if (!m) return PMX_ERR_ARG;
    m->em_leaves_only = on != 0;
    return PMX_OK;
}

int64_t pmx_meta_num_haplotypes(const pmx_meta* m) { return m ? (int64_t)m->groups.size() : 0; }
int pmx_meta_haplotype(const pmx_meta* m, int64_t i, uint32_t* node, double* prop, int64_t* n_members, uint32_t* members, int64_t cap) {
    if (!m || i < 0 || i >= (int64_t)m->groups.size()) return PMX_ERR_ARG;
    const pmx_meta_group& g = m->groups[(size_t)i];
    if (node) *node = g.node;
    if (prop) *prop = g.prop;
    if (n_members) *n_members = (int64_t)g.members.size();
    if (members && cap >= (int64_t)g.members.size()) std::copy(g.members.begin(), g.members.end(), members);
    return PMX_OK;
}
int pmx_meta_em_info(const pmx_meta* m, int32_t* rounds, int32_t* iterations, double* log_likelihood) {
    if (!m) return PMX_ERR_ARG;
    if (rounds) *rounds = m->em_rounds;
    if (iterations) *iterations = m->em_iterations;
    if (log_likelihood) *log_likelihood = m->llh;
    return PMX_OK;
}

}  // extern "C"
