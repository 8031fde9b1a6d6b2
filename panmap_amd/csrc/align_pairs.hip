// ALIGN stage: what depends on the reads alone -- the pair order and the distinct-pair map of a packed, paired read set --
// and the fan-out of the representatives' results to their copies.
#include <hip/hip_runtime.h>

#include <string.h>

#include <rocprim/rocprim.hpp>

#include "align_stage.hpp"

using namespace pmx;
using namespace pmx::aln;

// pair key = locality key of mate 1 (fragment start) in the high half, of mate 2 (fragment end) in the low half
__global__ void k_pair_keys(const uint32_t* __restrict__ read_key, int64_t n_pairs, uint64_t* key, uint32_t* idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * blockDim.x) {
        key[i] = (uint64_t)read_key[2 * i] << 32 | (uint64_t)read_key[2 * i + 1];
        idx[i] = (uint32_t)i;
    }
}

// Distinct-pair map (readset_pair_map): a pair's content is its two 64-byte read records (bases, ambiguity words, length),
// 128 bytes side by side; what the align stage computes for a pair depends on them alone (the regions' hash: on the
// lengths).  Pairs are sorted by a 32-bit hash of the content (stable: equal keys keep input order), a pair whose content
// differs from its predecessor's starts a group, and every pair takes the first of its group as representative.  Equality
// is tested byte for byte, so a hash collision only costs a missed merge.
__global__ void k_pair_hashes(const uint8_t* __restrict__ recs, int64_t n_pairs, uint32_t* key, uint32_t* idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4* p = reinterpret_cast<const uint4*>(recs + (size_t)i * 128);
        uint64_t h = 0x9e3779b97f4a7c15ULL;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 v = p[k];
            h = mix64(h ^ ((uint64_t)v.y << 32 | v.x));
            h = mix64(h ^ ((uint64_t)v.w << 32 | v.z));
        }
        key[i] = (uint32_t)(h >> 32) ^ (uint32_t)h;
        idx[i] = (uint32_t)i;
    }
}
__device__ __forceinline__ bool pair_recs_equal(const uint8_t* __restrict__ recs, uint32_t a, uint32_t b) {
    const uint4* x = reinterpret_cast<const uint4*>(recs + (size_t)a * 128);
    const uint4* y = reinterpret_cast<const uint4*>(recs + (size_t)b * 128);
    bool eq = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 u = x[k], v = y[k];
        eq = eq && u.x == v.x && u.y == v.y && u.z == v.z && u.w == v.w;
    }
    return eq;
}
// sorted position p -> p when it starts a group, else 0 (an inclusive max-scan then gives every position its group's start)
__global__ void k_pair_group_starts(const uint8_t* __restrict__ recs, const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx, int64_t n,
                                    uint32_t* start) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const bool first = p == 0 || key[p] != key[p - 1] || !pair_recs_equal(recs, idx[p], idx[p - 1]);
        start[p] = first ? (uint32_t)p : 0u;
    }
}
// rep[pair] = the group's first pair; mult[rep] = pairs of the group (written by its last position; only reps get one)
__global__ void k_pair_reps(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ gs, int64_t n, uint32_t* rep, uint32_t* mult) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t g = gs[p], r = idx[g];
        rep[idx[p]] = r;
        if (p == n - 1 || gs[p + 1] != g) mult[r] = (uint32_t)(p - g + 1);
    }
}
struct IsPairRep {
    const uint32_t* rep;
    __host__ __device__ bool operator()(const uint32_t& i) const { return rep[i] == i; }
};
// the copies a list of representatives stands for: out += sum(mult[list[i]] - 1) over the first *n_list entries
__global__ void k_pair_dup_count(const uint32_t* __restrict__ list, const unsigned long long* __restrict__ n_list, const uint32_t* __restrict__ mult,
                                 unsigned long long* out) {
    const int64_t n = (int64_t)*n_list;
    unsigned long long sum = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) sum += mult[list[i]] - 1u;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(out, sum);
}
// Fan-out, after every tier: each copy takes its representative's two records, edit counts and CIGAR words.  A copy claims
// arena words of its own, so records never share words and an arena overflow is counted and flagged as it would have been
// had the copy been aligned itself.  The words are claimed with one atomic per wave and PMX_FANOUT_ROUNDS x 64 pairs (one
// per 64 pairs, as compact_emit claims them, put 78k atomics on one address per 10M reads: 0.9 ms for the kernel): a lane
// counts the words of its pairs first, then copies.  A copy whose representative overflowed the arena cannot know how many
// words it needs (the record's n_cigar is 0 then): counted in unknown[0], the host redoes the call without the map.
#define PMX_FANOUT_ROUNDS 16
__global__ void __launch_bounds__(256) k_pair_fanout(const uint32_t* __restrict__ rep, int64_t n_pairs, AlnRecord* records, int32_t* edits, uint32_t* cigars,
                                                     uint64_t cigar_cap, unsigned long long* cigar_used, unsigned long long* unknown) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t span = 64 * PMX_FANOUT_ROUNDS;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / 64;
    for (int64_t c0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64) * span; c0 < n_pairs; c0 += n_waves * span) {
        uint32_t mine = 0, lost = 0;
        for (int j = 0; j < PMX_FANOUT_ROUNDS; ++j) {
            const int64_t d = c0 + j * 64 + lane;
            if (d >= n_pairs) break;
            const uint32_t r = rep[d];
            if (r == (uint32_t)d) continue;
            for (int s = 0; s < 2; ++s) {
                const AlnRecord& x = records[2 * (size_t)r + s];
                if (x.flags & PMX_REC_HAS_ALN) {
                    mine += x.n_cigar;
                    if ((x.flags & PMX_REC_OVERFLOW) && x.n_cigar == 0) ++lost;
                }
            }
        }
        uint32_t incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        const uint32_t wave_total = __shfl(incl, 63);
        unsigned long long wave_base = 0;
        if (wave_total) {
            if (lane == 0) wave_base = atomicAdd(cigar_used, (unsigned long long)wave_total);
            wave_base = __shfl(wave_base, 0);
        }
        if (lost) atomicAdd(unknown, (unsigned long long)lost);
        uint64_t coff = wave_base + (incl - mine);
        for (int j = 0; j < PMX_FANOUT_ROUNDS; ++j) {
            const int64_t d = c0 + j * 64 + lane;
            if (d >= n_pairs) break;
            const uint32_t r = rep[d];
            if (r == (uint32_t)d) continue;
            for (int s = 0; s < 2; ++s) {
                AlnRecord rec = records[2 * (size_t)r + s];
                if (rec.flags & PMX_REC_HAS_ALN) {
                    const uint32_t src = rec.cigar_off, nw = rec.n_cigar;
                    rec.cigar_off = (uint32_t)coff;
                    if (coff + nw <= cigar_cap) {
                        for (uint32_t k = 0; k < nw; ++k) cigars[coff + k] = cigars[src + k];
                    } else {
                        rec.flags |= PMX_REC_OVERFLOW;
                        rec.n_cigar = 0;
                    }
                    coff += nw;
                }
                records[2 * (size_t)d + s] = rec;
                if (edits) edits[2 * (size_t)d + s] = edits[2 * (size_t)r + s];
            }
        }
    }
}

namespace pmx {
// Pair order of a paired read set: pairs sorted by (locality key of mate 1, of mate 2) -- the 64 pairs of a wave then start
// AND end within a few bases of each other.  side == nullptr: on the context's stream (or, when it was enqueued earlier on a
// side stream, the context's stream waits for it); side != nullptr: enqueued there, behind everything the context's stream
// holds now (the read order).  -> the permutation (device), or nullptr when the read set has no locality order.
const uint32_t* readset_pair_order(pmx_ctx* ctx, const pmx_readset* rs, hipStream_t side) {
    const int64_t n_items = rs->n / 2;
    if (rs->has_pair_order) {
        if (rs->pair_ev_pending && !side) { PMX_HIP(hipStreamWaitEvent(ctx->stream, rs->pair_ev, 0)); rs->pair_ev_pending = false; }
        return rs->pp_idx2.p;
    }
    if (!readset_locality_order(ctx, rs) || n_items < 1) return nullptr;
    rs->pp_key.ensure((size_t)n_items); rs->pp_key2.ensure((size_t)n_items); rs->pp_idx.ensure((size_t)n_items); rs->pp_idx2.ensure((size_t)n_items + 1);
    hipStream_t st = ctx->stream;
    if (side) {
        if (!rs->pair_ev) PMX_HIP(hipEventCreateWithFlags(&rs->pair_ev, hipEventDisableTiming));
        PMX_HIP(hipEventRecord(rs->pair_ev, ctx->stream));      // the read keys are in place behind this point
        PMX_HIP(hipStreamWaitEvent(side, rs->pair_ev, 0));
        st = side;
    }
    PMX_LAUNCH(k_pair_keys, dim3((unsigned)std::min<int64_t>((n_items + 255) / 256, (int64_t)ctx->n_cu * 8)), dim3(256), 0, st, rs->loc_key.p, n_items,
               rs->pp_key.p, rs->pp_idx.p);
    PMX_ROCPRIM(rs->pp_tmp, radix_sort_pairs, rs->pp_key.p, rs->pp_key2.p, rs->pp_idx.p, rs->pp_idx2.p, (size_t)n_items, 0, 64, st);
    // (the map, too, depends on the reads alone; below a million pairs the align stage seldom wants it -- PMX_ALIGN_DEDUP_DEPTH
    //  -- and makes it itself when it does)
    if (side && n_items >= ((int64_t)1 << 20) && !pmx::opt_str(pmx::O_ALIGN_NO_DEDUP)) readset_pair_map(ctx, rs, st);
    if (side) { PMX_HIP(hipEventRecord(rs->pair_ev, side)); rs->pair_ev_pending = true; }
    rs->has_pair_order = true;
    return rs->pp_idx2.p;
}

// Distinct-pair map of a packed, paired read set with read records (k_pair_hashes .. k_pair_reps): rs->pd_rep[pair] = its
// representative, rs->pd_mult[rep] = the pairs it stands for.  Enqueued on `st` (the side stream of the pair order, or the
// context's stream).  10M reads: one 128-byte line per pair read twice, a 32-bit four-pass sort, ~0.55 ms.
void readset_pair_map(pmx_ctx* ctx, const pmx_readset* rs, hipStream_t st) {
    const int64_t n = rs->n / 2;
    if (rs->has_pair_map || n < 1 || !rs->has_recs) return;
    rs->pd_key.ensure((size_t)n); rs->pd_key2.ensure((size_t)n); rs->pd_idx.ensure((size_t)n); rs->pd_idx2.ensure((size_t)n);
    rs->pd_gs.ensure((size_t)n); rs->pd_rep.ensure((size_t)n); rs->pd_mult.ensure((size_t)n);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->n_cu * 8);
    PMX_LAUNCH(k_pair_hashes, dim3(grid), dim3(256), 0, st, rs->recs.p, n, rs->pd_key.p, rs->pd_idx.p);
    PMX_ROCPRIM(rs->pd_tmp, radix_sort_pairs, rs->pd_key.p, rs->pd_key2.p, rs->pd_idx.p, rs->pd_idx2.p, (size_t)n, 0, 32, st);
    // (the unsorted keys are spent: their buffer takes the group starts before the scan)
    PMX_LAUNCH(k_pair_group_starts, dim3(grid), dim3(256), 0, st, rs->recs.p, rs->pd_key2.p, rs->pd_idx2.p, n, rs->pd_key.p);
    // (the sort and the scan share one temporary; the scan needs less of it, so it grows at the sort alone)
    PMX_ROCPRIM(rs->pd_tmp, inclusive_scan, rs->pd_key.p, rs->pd_gs.p, (size_t)n, rocprim::maximum<uint32_t>(), st);
    PMX_LAUNCH(k_pair_reps, dim3(grid), dim3(256), 0, st, rs->pd_idx2.p, rs->pd_gs.p, n, rs->pd_rep.p, rs->pd_mult.p);
    rs->has_pair_map = true;
}

int64_t pair_select_reps(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, const uint32_t* order, int64_t n_pairs) {
    if (rs->pair_ev_pending) { PMX_HIP(hipStreamWaitEvent(ctx->stream, rs->pair_ev, 0)); rs->pair_ev_pending = false; }
    readset_pair_map(ctx, rs, ctx->stream);   // (made beside the place stage with the pair order when the host asked for that)
    al->dd_list.ensure((size_t)n_pairs);
    const IsPairRep is_rep{rs->pd_rep.p};
    const rocprim::counting_iterator<uint32_t> every(0u);
    if (order) PMX_ROCPRIM(al->dd_tmp, select, order, al->dd_list.p, al->dd_count.p, (size_t)n_pairs, is_rep, ctx->stream);
    else PMX_ROCPRIM(al->dd_tmp, select, every, al->dd_list.p, al->dd_count.p, (size_t)n_pairs, is_rep, ctx->stream);
    unsigned long long h_reps = 0;
    PMX_D2H_SYNC(&h_reps, al->dd_count, 1, ctx->stream);
    return (int64_t)h_reps;
}

void pair_count_copies(pmx_ctx* ctx, pmx_aligner* al, const uint32_t* list, const unsigned long long* n_list, const uint32_t* mult, int64_t n_launch) {
    const unsigned dgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_launch + 255) / 256, (int64_t)ctx->n_cu * 8));
    PMX_LAUNCH(k_pair_dup_count, dim3(dgrid), dim3(256), 0, ctx->stream, list, n_list, mult, al->dd_count.p + 2);
}

void pair_fanout(pmx_ctx* ctx, pmx_aligner* al, const uint32_t* rep, int64_t n_pairs, int32_t* edits) {
    PMX_LAUNCH(k_pair_fanout, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_pairs + 256 * PMX_FANOUT_ROUNDS - 1) / (256 * PMX_FANOUT_ROUNDS), (int64_t)ctx->n_cu * 8))), dim3(256), 0,
               ctx->stream, rep, n_pairs, al->records.p, edits, al->cigars.p, (uint64_t)al->cigar_cap, al->cigar_used.p, al->dd_count.p + 1);
}
}  // namespace pmx


// Enqueue the align stage's pair order of a packed, paired read set NOW, on a side stream of the context: it depends on the
// reads alone, and made here it runs beside the place stage (scoring is latency-bound) instead of between the placement
// and the first align kernel (10M reads: ~1 ms).  Optional: an aligner that finds none makes it itself.
int pmx_readset_order_pairs(pmx_ctx* ctx, pmx_readset* rs) {
    if (!ctx || !rs) return PMX_ERR_ARG;
    if (rs->hpc) return fail(PMX_ERR_ARG, "the read set is homopolymer-compressed: the align stage's pair order is made of the uncompressed read set");
    if (!rs->packed) return fail(PMX_ERR_ARG, "read set is not packed");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (rs->n < 2 || rs->n / 2 >= (int64_t)UINT32_MAX) return PMX_OK;
    if (!ctx->pair_stream) ctx->pair_stream = create_dedicated_stream(ctx->n_cu);
    (void)readset_pair_order(ctx, rs, ctx->pair_stream);
    return PMX_OK;
    PMX_CATCH
}
