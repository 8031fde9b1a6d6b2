// Homopolymer compression of a read set for gfx950 (wave64): seeding::hpcCompressWithMapping (src/seeding.cpp:291-306) as the
// place stage applies it to every read before anything else (src/placement.cpp:1143-1165).
//
// Base 0 of a read is kept; base i > 0 is kept iff toupper(seq[i]) != toupper(seq[i-1]) -- a comparison of LETTERS (NNNN -> N,
// RY stays RY, aA -> a); the kept characters are copied as they are, and a run's quality is that of its first base.
//
// Both kernels: one wave per read, 64 consecutive bases per step (one byte per lane: a 64-byte contiguous read per step).  Lane
// i's predecessor comes from lane i-1; lane 0 takes the previous step's lane-63 letter, carried in a register.  A run never
// reaches across a read boundary: the first base of a read is kept whatever precedes it in the buffer.  Only bytes inside
// [off[r], off[r+1]) are touched, so nothing before the first or past the last byte of the buffer is read.
// Algorithmic HBM bytes: 2 B read (one per pass) + <= 1 B written per base; twice that with qualities.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "place_kernels.h"

namespace pmx {

namespace {
// toupper in the "C" locale: bytes outside a..z are unchanged
__device__ __forceinline__ uint32_t hpc_upper(uint32_t c) { return (c - 0x61u) < 26u ? c - 0x20u : c; }

// the keep flags of one 64-base step of a read: `idx` = this lane's byte, `b`/`e` = the read's byte range, `carry` = the letter
// of the base before the step (lane 63 of the previous step); returns the ballot and leaves this lane's character in `ch`
__device__ __forceinline__ unsigned long long hpc_step(const uint8_t* __restrict__ ascii, int64_t idx, int64_t b, int64_t e, uint32_t& carry, uint32_t& ch) {
    const int lane = (int)(threadIdx.x & 63u);
    const bool valid = idx < e;
    ch = valid ? (uint32_t)ascii[idx] : 0u;
    const uint32_t u = hpc_upper(ch);
    uint32_t prev = (uint32_t)__shfl_up((int)u, 1);
    if (lane == 0) prev = carry;
    const bool keep = valid && (idx == b || u != prev);
    carry = (uint32_t)__shfl((int)u, 63);
    return __ballot(keep);
}
}  // namespace

// len[r] = bases of the compressed read r, nwords[r] = its 32-base words; entry n_reads of both = 0 (the scans' last output is
// the total); stats[0] = the longest compressed read
__global__ void __launch_bounds__(256)
k_hpc_count(const uint8_t* __restrict__ ascii, const int64_t* __restrict__ off, int64_t n_reads, int64_t* __restrict__ len, int64_t* __restrict__ nwords,
            unsigned long long* stats) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (wave == 0 && lane == 0) { len[n_reads] = 0; nwords[n_reads] = 0; }
    unsigned long long mx = 0;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t b = off[r], e = off[r + 1];
        uint32_t carry = 0, ch;
        int64_t kept = 0;
        for (int64_t base = b; base < e; base += 64) kept += __popcll(hpc_step(ascii, base + lane, b, e, carry, ch));
        if (lane == 0) { len[r] = kept; nwords[r] = (kept + 31) >> 5; }
        mx = (unsigned long long)kept > mx ? (unsigned long long)kept : mx;
    }
    if (lane == 0 && mx) atomicMax(&stats[0], mx);
}

// the same flags again; a kept base goes to out_off[r] + (kept bases of the read's earlier steps) + (kept bases of the lanes
// below in this step): the writes of a step are contiguous.  qual / out_qual: null, or the qualities in lockstep.
__global__ void __launch_bounds__(256)
k_hpc_write(const uint8_t* __restrict__ ascii, const int64_t* __restrict__ off, const uint8_t* __restrict__ qual, int64_t n_reads,
            const int64_t* __restrict__ out_off, uint8_t* __restrict__ out_ascii, uint8_t* __restrict__ out_qual) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t b = off[r], e = off[r + 1];
        uint32_t carry = 0, ch;
        int64_t pos = out_off[r];
        const int64_t out_end = out_off[r + 1];
        for (int64_t base = b; base < e; base += 64) {
            const int64_t idx = base + lane;
            const unsigned long long m = hpc_step(ascii, idx, b, e, carry, ch);
            const int64_t at = pos + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (((m >> lane) & 1ULL) && at < out_end) {   // (at < out_end: the count pass saw the same bytes, so it always holds)
                out_ascii[at] = (uint8_t)ch;
                if (qual) out_qual[at] = qual[idx];
            }
            pos += __popcll(m);
        }
    }
}

}  // namespace pmx
