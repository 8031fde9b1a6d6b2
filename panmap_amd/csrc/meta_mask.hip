// --meta --mask-reads N / --mask-seeds N: the low-coverage k-min-mer masks (ThreadsManager::initializeQueryData,
// src/mgsr.cpp:2049-2139), a step of pmx_meta_set_reads between the upload of the merged lists and the overlap coefficients.
//
// The reference's rule, on the reads AFTER equal seedmer lists were merged into one read with a multiplicity:
//   count[h] = sum of the multiplicities of the merged reads that carry hash h -- a read adds its multiplicity ONCE per
//              distinct hash, however often its list repeats it (the loop is over uniqueSeedmers), either orientation;
//   mask-reads T > 0: a merged read with any list entry of count <= T is dropped (numMaskReads counts them);
//   mask-seeds T > 0 (only when mask-reads is off): every list entry of count <= T is removed, the rest keeps its order
//              (numMaskSeeds counts the removed entries); a read left empty is dropped; reads that became equal stay apart.
// Everything downstream -- the hash set of the overlap coefficients, the score rows, the EM's reads and weights -- sees the
// survivors only.
//
// Here, on the merged lists as upload_lists left them (offsets, every entry as its index `uid` into the ascending distinct
// hashes, orientations), a wave per merged read in every kernel, like k_meta_assign_max:
//   * k_meta_mask_count: the read's uids go to the wave's stretch of LDS; the lane that holds entry i adds mult[r] to
//     count[uid_i] with one 64-bit atomic iff no entry j < i of the read has the same uid (all lanes read the same j: a
//     broadcast, no bank conflict).  Quadratic in the read's entries, so only for reads of at most kMaskQuadratic entries
//     (short reads carry ~20; PMX_META_MASK_LONG lowers the bound for the tests).
//   * longer reads (a 20 kb read has ~3,300 entries, the limit is 65,534): k_meta_mask_long_keys writes (ordinal of the long
//     read << 32 | uid) per entry, one rocprim radix sort puts equal pairs next to each other, k_meta_mask_long_add adds the
//     read's multiplicity at the first key of every run.  n log n instead of n^2, and no LDS bound.
//   * k_meta_mask_flag: an entry is kept iff count[uid] > T.  mask-reads: the ballots of the read decide the whole read;
//     mask-seeds: the popcounts are its new length.  Writes the new length (0 = dropped), alive[r], used[uid] = 1 for every
//     surviving entry (plain stores of the same value) and feeds the two counters.
//   * exclusive scans (rocprim) of the new lengths, of alive[] and of used[]: new offsets, new read indices, new uids.
//   * k_meta_mask_compact: a wave per surviving read; ballot + popcount prefix place the surviving entries in their order;
//     hash, new uid, orientation per entry, offset and multiplicity per read.  k_meta_mask_compact_uniq: the surviving
//     distinct hashes with their counts.
// All sums are integers: nothing depends on the order of the atomics.
//
// With amplicons (--amplicon-depth; pmx_meta_set_amplicons; src/mgsr.cpp:1216-1342, :2062-2075) the rule holds within every
// amplicon: count[g][h] is over the merged reads of g, and a read of g is masked against the threshold of g -- the absolute
// parameter, or (size_t)(relative parameter * raw reads of g); the unlisted group, the last, always takes the absolute one.
// Then, and only then, the count key is the pair (amplicon, hash): k_meta_amp_keys writes amplicon << 32 | uid with the entry's
// index, one rocprim radix_sort_pairs sorts them, k_meta_amp_heads + an exclusive scan rank the distinct pairs (ascending by
// (amplicon, hash)), k_meta_amp_scatter gives every entry its pair's rank `pid` and fills the pair table.  The counting
// kernels run unchanged on the pids (within one read equal pids are exactly equal uids), k_meta_amp_totals adds every pair's
// count into its hash's total, and the GROUPED forms of k_meta_mask_flag / k_meta_mask_compact read the count through the pid
// and compare it with thr[amplicon of the read].  No launch depends on the number of amplicons and there is no
// amplicons x hashes table.  Without amplicons nothing of this runs or is allocated.
//
// The host side is MaskStage, a struct that lives for one call, one function per step; meta_apply_masks calls them in order:
//   reset_results      the results of a mask that removes nothing (host);
//   group_thresholds   amplicons: thr[] and m->amp_thr (host); a sample without merged reads ends here;
//   plan_sorted_path   the reads beyond the in-LDS bound, with the offsets of their keys (host);
//   upload             every allocation but the survivors', and the host-to-device copies;
//   clear_counters     the memsets, the first work inside the "meta_mask" span;
//   rank_pairs         amplicons: keys, the "meta_mask_sort" span, heads, scan, scatter;
//   count              the in-LDS kernel, the sorted path, k_meta_amp_totals with amplicons;
//   flag_and_size      k_meta_mask_flag, the three scans, the one synchronize that sizes the survivors;
//   compact            the survivors' buffers, k_meta_mask_compact, k_meta_mask_compact_uniq; the span ends;
//   publish            the host's copies, the (group, hash, count) triples, amp_left, h_raw_to_merged, the swaps, the numbers.
// The GROUPED kernels are launched from one argument list each: the amplicon buffers' pointers are null without amplicons.
// Resource report (gfx950): no kernel of this file uses scratch, all are at 8 waves/SIMD; the new ones take 10-18 VGPRs, the
// GROUPED forms 38 / 39 against 36 / 32 of the plain ones.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "api_internal.hpp"
#include "device/dev_util.hpp"
#include "meta_state.hpp"

using namespace pmx;

namespace {
constexpr int kMaskWaves = 4;             // waves per block (256 threads)
constexpr int kMaskQuadratic = 1024;      // entries a read may have on the in-LDS path: 4 KB of uids per wave, 16 KB per block

// (same-wave LDS traffic is ordered by the hardware; this pins the compiler)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(64 * kMaskWaves) k_meta_mask_count(const int64_t* __restrict__ read_off, const uint32_t* __restrict__ seed_uid,
                                                                     const int64_t* __restrict__ mult, int64_t n_reads, int bound,
                                                                     unsigned long long* count) {
    __shared__ uint32_t s_uid[kMaskWaves][kMaskQuadratic];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wave = (int64_t)blockIdx.x * kMaskWaves + wib, n_waves = (int64_t)gridDim.x * kMaskWaves;
    uint32_t* uids = s_uid[wib];
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t o = read_off[r], n64 = read_off[r + 1] - o;
        if (n64 > (int64_t)bound) continue;   // (bound <= kMaskQuadratic; the sorted path counts this read)
        const int n = (int)n64;
        const unsigned long long w = (unsigned long long)mult[r];
        for (int i = lane; i < n; i += 64) uids[i] = seed_uid[o + i];
        wave_lds_sync();
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const uint32_t u = i < n ? uids[i] : 0u;
            bool first = i < n;
            const int j1 = min(i0 + 63, n - 1);   // (the same in all lanes: every lane reads uids[j], one broadcast)
            for (int j = 0; j < j1; ++j) first &= !(j < i && uids[j] == u);
            if (first) atomicAdd(&count[u], w);
        }
        wave_lds_sync();
    }
}

// entry e of long read `ordinal` -> ordinal << 32 | uid at key[long_off[ordinal] + e]
__global__ void __launch_bounds__(256) k_meta_mask_long_keys(const int64_t* __restrict__ read_off, const uint32_t* __restrict__ seed_uid,
                                                             const uint32_t* __restrict__ long_read, const int64_t* __restrict__ long_off, int64_t n_long,
                                                             uint64_t* __restrict__ key) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t q = wave; q < n_long; q += n_waves) {
        const int64_t r = long_read[q], o = read_off[r], n = read_off[r + 1] - o, dst = long_off[q];
        for (int64_t e = lane; e < n; e += 64) key[dst + e] = ((uint64_t)q << 32) | (uint64_t)seed_uid[o + e];
    }
}

// the sorted keys: the first of every run of equal (read, uid) pairs adds the read's multiplicity
__global__ void k_meta_mask_long_add(const uint64_t* __restrict__ key, int64_t n_keys, const uint32_t* __restrict__ long_read,
                                     const int64_t* __restrict__ mult, unsigned long long* count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = key[i];
        if (i > 0 && key[i - 1] == k) continue;
        atomicAdd(&count[(uint32_t)k], (unsigned long long)mult[long_read[k >> 32]]);
    }
}

// whole_reads: --mask-reads (a read with an entry at or below the threshold goes as a whole), else --mask-seeds.
// ctr[0]: reads dropped by --mask-reads, ctr[1]: entries removed by --mask-seeds.
// GROUPED (amplicons): the count of entry e is count[seed_pid[e]], the count of its (amplicon, hash) pair, and the threshold is
// that of the read's amplicon, thr[read_amp[r]] (the same in all lanes); used[] stays per hash.  Else seed_pid / read_amp / thr
// are not read.
template <bool GROUPED>
__global__ void __launch_bounds__(256) k_meta_mask_flag(const int64_t* __restrict__ read_off, const uint32_t* __restrict__ seed_uid, int64_t n_reads,
                                                        const unsigned long long* __restrict__ count, unsigned long long threshold, int whole_reads,
                                                        int64_t* __restrict__ new_len, uint32_t* __restrict__ alive, uint32_t* used,
                                                        unsigned long long* ctr, const uint32_t* __restrict__ seed_pid,
                                                        const int32_t* __restrict__ read_amp, const unsigned long long* __restrict__ thr) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t o = read_off[r], n = read_off[r + 1] - o;
        if (GROUPED) threshold = thr[read_amp[r]];
        int64_t kept = 0;
        for (int64_t i0 = 0; i0 < n; i0 += 64) {
            const int64_t i = i0 + lane;
            const uint32_t u = i < n ? seed_uid[o + i] : 0u;
            const bool keep = i < n && count[GROUPED ? seed_pid[o + i] : u] > threshold;
            kept += __popcll(__ballot(keep));
            if (keep && !whole_reads) used[u] = 1u;
        }
        const int64_t len = whole_reads ? (kept == n ? n : 0) : kept;
        if (whole_reads && len > 0)
            for (int64_t i = lane; i < n; i += 64) used[seed_uid[o + i]] = 1u;
        if (lane == 0) {
            new_len[r] = len;
            alive[r] = len > 0 ? 1u : 0u;
            if (whole_reads && len == 0) atomicAdd(&ctr[0], 1ULL);
            if (!whole_reads && kept < n) atomicAdd(&ctr[1], (unsigned long long)(n - kept));
        }
    }
}

// new_off / read_pos / uid_pos: the exclusive scans of new_len / alive / used.  GROUPED: as in k_meta_mask_flag, and the
// amplicon of every surviving read goes to out_amp.
template <bool GROUPED>
__global__ void __launch_bounds__(256) k_meta_mask_compact(const int64_t* __restrict__ read_off, const uint32_t* __restrict__ seed_uid,
                                                           const uint8_t* __restrict__ seed_rev, const uint64_t* __restrict__ uniq,
                                                           const int64_t* __restrict__ mult, int64_t n_reads, const unsigned long long* __restrict__ count,
                                                           unsigned long long threshold, const int64_t* __restrict__ new_len,
                                                           const int64_t* __restrict__ new_off, const uint32_t* __restrict__ read_pos,
                                                           const uint32_t* __restrict__ uid_pos, int64_t* __restrict__ out_off,
                                                           uint64_t* __restrict__ out_hash, uint32_t* __restrict__ out_uid, uint8_t* __restrict__ out_rev,
                                                           int64_t* __restrict__ out_mult, const uint32_t* __restrict__ seed_pid,
                                                           const int32_t* __restrict__ read_amp, const unsigned long long* __restrict__ thr,
                                                           int32_t* __restrict__ out_amp) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (wave == 0 && lane == 0) out_off[read_pos[n_reads]] = new_off[n_reads];   // (the end of the last surviving read)
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        if (new_len[r] == 0) continue;
        const int64_t o = read_off[r], n = read_off[r + 1] - o;
        if (GROUPED) threshold = thr[read_amp[r]];
        int64_t at = new_off[r];   // (the read's entries go to [new_off[r], new_off[r] + new_len[r]): as many as are kept below)
        for (int64_t i0 = 0; i0 < n; i0 += 64) {
            const int64_t i = i0 + lane;
            const uint32_t u = i < n ? seed_uid[o + i] : 0u;
            const bool keep = i < n && count[GROUPED ? seed_pid[o + i] : u] > threshold;
            const unsigned long long b = __ballot(keep);
            if (keep) {
                const int64_t dst = at + __popcll(b & ((1ULL << lane) - 1ULL));
                out_hash[dst] = uniq[u];
                out_uid[dst] = uid_pos[u];
                out_rev[dst] = seed_rev[o + i];
            }
            at += __popcll(b);
        }
        if (lane == 0) {
            out_off[read_pos[r]] = new_off[r];
            out_mult[read_pos[r]] = mult[r];
            if (GROUPED) out_amp[read_pos[r]] = read_amp[r];
        }
    }
}

__global__ void k_meta_mask_compact_uniq(const uint64_t* __restrict__ uniq, const unsigned long long* __restrict__ count, const uint32_t* __restrict__ used,
                                         const uint32_t* __restrict__ uid_pos, int64_t n_uniq, uint64_t* __restrict__ out_uniq,
                                         int64_t* __restrict__ out_count) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_uniq; u += (int64_t)gridDim.x * blockDim.x) {
        if (!used[u]) continue;
        out_uniq[uid_pos[u]] = uniq[u];
        out_count[uid_pos[u]] = (int64_t)count[u];
    }
}

// ---- amplicons: the count key is (amplicon, hash).  Every entry gets the rank `pid` of its pair among the distinct pairs of
// the sample, ascending by (amplicon, hash); the counting kernels above then run on seed_pid in place of seed_uid (within one
// read equal pids are exactly equal uids).  The number of launches does not depend on the number of amplicons.

// a wave per merged read: entry e -> key[e] = amplicon << 32 | uid, val[e] = e (e < 2^32 - 1: the caller refuses more)
__global__ void __launch_bounds__(256) k_meta_amp_keys(const int64_t* __restrict__ read_off, const uint32_t* __restrict__ seed_uid,
                                                       const int32_t* __restrict__ read_amp, int64_t n_reads, uint64_t* __restrict__ key,
                                                       uint32_t* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t o = read_off[r], n = read_off[r + 1] - o;
        const uint64_t hi = (uint64_t)(uint32_t)read_amp[r] << 32;
        for (int64_t e = o + lane; e < o + n; e += 64) {
            key[e] = hi | (uint64_t)seed_uid[e];
            val[e] = (uint32_t)e;
        }
    }
}

// the sorted keys: head[i] = 1 at the first key of every run of equal pairs; head[n_keys] = 0 (the scan's total)
__global__ void k_meta_amp_heads(const uint64_t* __restrict__ key, int64_t n_keys, uint32_t* __restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_keys; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = i < n_keys && (i == 0 || key[i - 1] != key[i]) ? 1u : 0u;
}

// before: the exclusive scan of head.  The pair of sorted position i has rank before[i] + head[i] - 1 (< n_keys): to the entry
// val[i], and its key to the pair table
__global__ void k_meta_amp_scatter(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, const uint32_t* __restrict__ head,
                                   const uint32_t* __restrict__ before, int64_t n_keys, uint32_t* __restrict__ seed_pid,
                                   uint64_t* __restrict__ pair_key) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t pid = before[i] + head[i] - 1u;
        seed_pid[val[i]] = pid;
        if (head[i]) pair_key[pid] = key[i];
    }
}

// every pair's count into its hash's total over the amplicons (*n_pairs: the scan's total, on the device)
__global__ void k_meta_amp_totals(const uint64_t* __restrict__ pair_key, const unsigned long long* __restrict__ count,
                                  const uint32_t* __restrict__ n_pairs, unsigned long long* total) {
    const int64_t n = (int64_t)*n_pairs;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&total[(uint32_t)pair_key[p]], count[p]);
}

// entries a read may have on the in-LDS path: kMaskQuadratic, or what PMX_META_MASK_LONG lowers it to
int quadratic_bound() {
    int bound = kMaskQuadratic;
    if (const char* e = opt_str(O_META_MASK_LONG)) bound = (int)std::max<long long>(1, std::min<long long>(kMaskQuadratic, atoll(e)));
    return bound;
}

// the threshold of a group under a relative parameter (src/mgsr.cpp:2062-2075): the IEEE product, truncated
unsigned long long relative_threshold(double rf, int64_t n_raw) {
    const double t = rf * (double)n_raw;
    return t >= 18446744073709551615.0 ? ~0ULL : (unsigned long long)(size_t)t;
}
template <class F>
void with_grouped(bool grouped, F&& launch) {   // GROUPED as a compile-time constant: the launch is written once
    if (grouped) launch(std::true_type());
    else launch(std::false_type());
}

// One call of the mask step on a sample that has merged reads: one function per step, in the order meta_apply_masks calls
// them.  The device buffers live until the call ends; every step throws (HipError).
struct MaskStage {
    pmx_ctx* const ctx;
    pmx_meta* const m;
    const hipStream_t st;
    const int G;                              // blocks of a grid-stride launch at most
    const bool whole_reads, grouped;          // --mask-reads (else --mask-seeds); with amplicons
    const unsigned long long threshold;       // the absolute parameter
    const int64_t n_reads, n_seedmers, n_uniq;   // before masking
    std::vector<unsigned long long> thr;      // grouped: the threshold of every group
    // plan_sorted_path
    int bound = kMaskQuadratic;
    std::vector<uint32_t> long_read;
    std::vector<int64_t> long_off;
    int64_t n_long = 0, n_keys = 0;
    // upload: per merged read, per distinct hash, the sorted path's keys
    DevBuf<int64_t> d_mult, d_new_len, d_new_off, d_long_off;
    DevBuf<unsigned long long> d_count, d_ctr;
    DevBuf<uint32_t> d_alive, d_read_pos, d_used, d_uid_pos, d_long_read;
    DevBuf<uint64_t> d_key, d_key_sorted;
    DevBuf<char> tmp;
    // amplicons (null pointers otherwise): per entry its pair's rank, per pair its key and count (at most one pair per entry);
    // d_count above then holds the per-hash totals over the amplicons
    DevBuf<int32_t> d_read_amp, o_amp;
    DevBuf<unsigned long long> d_thr, d_pair_count;
    DevBuf<uint64_t> d_akey, d_akey_sorted, d_pair_key;
    DevBuf<uint32_t> d_aval, d_aval_sorted, d_head, d_before, d_seed_pid;
    const uint32_t* count_id = nullptr;       // what the counting kernels index their counters with: pids or uids
    unsigned long long* counters = nullptr;   // ... and the counters: per pair or per hash
    // flag_and_size: the survivors' sizes, the two counters of k_meta_mask_flag, the distinct pairs
    int64_t left_seedmers = 0;
    uint32_t left_reads = 0, left_uniq = 0, n_pairs = 0;
    unsigned long long h_ctr[2] = {0, 0};
    // compact: the survivors
    DevBuf<int64_t> o_off, o_mult, o_count;
    DevBuf<uint64_t> o_hash, o_uniq;
    DevBuf<uint32_t> o_uid;
    DevBuf<uint8_t> o_rev;

    MaskStage(pmx_ctx* c, pmx_meta* mm)
        : ctx(c), m(mm), st(c->stream), G(c->n_cu * 8), whole_reads(mm->lowcov_reads > 0 || mm->lowcov_reads_rf > 0), grouped(mm->amp_on),
          threshold((unsigned long long)(whole_reads ? mm->lowcov_reads : mm->lowcov_seeds)), n_reads(mm->n_reads), n_seedmers(mm->n_seedmers),
          n_uniq((int64_t)mm->h_uniq.size()) {}
    bool empty() const { return n_reads == 0 || n_seedmers == 0; }   // (merged reads have entries: both or neither)
    void reset_results();
    void group_thresholds();
    void plan_sorted_path();
    void upload();
    void clear_counters();
    void rank_pairs();
    void count();
    void flag_and_size();
    void compact();
    void publish();
};

// Reads: the sample before masking.  Leaves: m->masked and the results of a mask that removes nothing: the three numbers, the
// distinct hashes with zero counts.
void MaskStage::reset_results() {
    m->masked = true;
    m->lowcov_reads_dropped = m->lowcov_seeds_removed = 0;
    m->lowcov_reads_left = n_reads;
    m->lowcov_hash = m->h_uniq;
    m->lowcov_count.assign((size_t)n_uniq, 0);
}

// Amplicons only (host).  Reads: the parameters, m->amp_raw.  Leaves: thr[] and m->amp_thr: a share of the group's raw reads
// under a relative parameter, else the absolute parameter; the unlisted group, the last, always takes the absolute one.
void MaskStage::group_thresholds() {
    if (!grouped) return;
    const double rf = whole_reads ? m->lowcov_reads_rf : m->lowcov_seeds_rf;
    thr.assign((size_t)m->n_amp, threshold);
    if (rf > 0)
        for (int32_t g = 0; g + 1 < m->n_amp; ++g) thr[(size_t)g] = relative_threshold(rf, m->amp_raw[(size_t)g]);
    for (int32_t g = 0; g < m->n_amp; ++g) m->amp_thr[(size_t)g] = (int64_t)std::min<unsigned long long>(thr[(size_t)g], (unsigned long long)INT64_MAX);
}

// Host.  Reads: m->h_read_off.  Leaves: bound, and the reads with more entries than it, which the sorted path counts:
// long_read[q] with the offset long_off[q] of its keys, n_long, n_keys.
void MaskStage::plan_sorted_path() {
    bound = quadratic_bound();
    long_off.assign(1, 0);
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t n = m->h_read_off[(size_t)r + 1] - m->h_read_off[(size_t)r];
        if (n > bound) { long_read.push_back((uint32_t)r); long_off.push_back(long_off.back() + n); }
    }
    n_long = (int64_t)long_read.size();
    n_keys = long_off.back();
}

// Reads: the plan, thr[], m->h_mult / h_read_amp.  Leaves: every buffer of the call but the survivors', allocated; on the
// device the multiplicities, the long reads' plan and, with amplicons, the reads' amplicons and thr[]; count_id / counters.
// The amplicon buffers are made only when grouped.
void MaskStage::upload() {
    d_mult.alloc((size_t)n_reads); d_new_len.alloc((size_t)n_reads + 1); d_new_off.alloc((size_t)n_reads + 1);
    d_alive.alloc((size_t)n_reads + 1); d_read_pos.alloc((size_t)n_reads + 1);
    d_count.alloc((size_t)n_uniq); d_used.alloc((size_t)n_uniq + 1); d_uid_pos.alloc((size_t)n_uniq + 1);
    d_ctr.alloc(2);
    if (grouped) {
        d_read_amp.alloc((size_t)n_reads); d_thr.alloc(thr.size()); d_pair_count.alloc((size_t)n_seedmers); d_pair_key.alloc((size_t)n_seedmers);
        d_akey.alloc((size_t)n_seedmers); d_akey_sorted.alloc((size_t)n_seedmers); d_aval.alloc((size_t)n_seedmers); d_aval_sorted.alloc((size_t)n_seedmers);
        d_head.alloc((size_t)n_seedmers + 1); d_before.alloc((size_t)n_seedmers + 1); d_seed_pid.alloc((size_t)n_seedmers);
        PMX_H2D(d_read_amp, m->h_read_amp, n_reads, st);
        PMX_H2D(d_thr, thr, st);
    }
    count_id = grouped ? d_seed_pid.p : m->d_seed_uid.p;
    counters = grouped ? d_pair_count.p : d_count.p;
    PMX_H2D(d_mult, m->h_mult, n_reads, st);
    if (n_long > 0) {
        d_long_read.alloc((size_t)n_long); d_long_off.alloc((size_t)n_long + 1); d_key.alloc((size_t)n_keys); d_key_sorted.alloc((size_t)n_keys);
        PMX_H2D(d_long_read, long_read, n_long, st);
        PMX_H2D(d_long_off, long_off, (size_t)n_long + 1, st);
    }
}

// Leaves: zero in the counters of every hash (and pair), in used[], in the two counters of k_meta_mask_flag and in the entry
// past the last read of new_len[] / alive[] (the scans run over one entry more: their totals).
void MaskStage::clear_counters() {
    PMX_ZERO(d_count, n_uniq, st);
    PMX_ZERO(d_used, (size_t)n_uniq + 1, st);
    PMX_ZERO(d_ctr, 2, st);
    PMX_ZERO(pmx::at(d_new_len, n_reads), 1, st);
    PMX_ZERO(pmx::at(d_alive, n_reads), 1, st);
    if (grouped) PMX_ZERO(d_pair_count, n_seedmers, st);
}

// Amplicons only: the (amplicon, hash) pairs ranked.  Reads: the merged lists on the device, d_read_amp.  Leaves: d_seed_pid
// (per entry the rank of its pair, ascending by (amplicon, hash)), d_pair_key (per pair its key), d_before[n_seedmers] (the
// number of distinct pairs); the "meta_mask_sort" span around the key sort.
void MaskStage::rank_pairs() {
    PMX_LAUNCH(k_meta_amp_keys, dim3(grid_for(n_reads * 64, 256, G)), dim3(256), 0, st, m->d_read_off.p, m->d_seed_uid.p, d_read_amp.p, n_reads,
               d_akey.p, d_aval.p);
    unsigned end_bit = 32;   // (the uid, and the bits of the greatest amplicon)
    while (end_bit < 64 && ((uint64_t)(m->n_amp - 1) >> (end_bit - 32)) != 0) ++end_bit;
    timer_begin(ctx, "meta_mask_sort");   // (a span of its own inside "meta_mask": the share the key sort takes)
    PMX_ROCPRIM(tmp, radix_sort_pairs, d_akey.p, d_akey_sorted.p, d_aval.p, d_aval_sorted.p, (size_t)n_seedmers, 0u, end_bit, st);
    timer_end(ctx, "meta_mask_sort", 1);
    PMX_LAUNCH(k_meta_amp_heads, dim3(grid_for(n_seedmers + 1, 256, G)), dim3(256), 0, st, d_akey_sorted.p, n_seedmers, d_head.p);
    PMX_ROCPRIM(tmp, exclusive_scan, d_head.p, d_before.p, 0u, (size_t)n_seedmers + 1, rocprim::plus<uint32_t>(), st);
    PMX_LAUNCH(k_meta_amp_scatter, dim3(grid_for(n_seedmers, 256, G)), dim3(256), 0, st, d_akey_sorted.p, d_aval_sorted.p, d_head.p, d_before.p,
               n_seedmers, d_seed_pid.p, d_pair_key.p);
}

// Reads: count_id (uids, or pids), the multiplicities, the plan.  Leaves: counters[] = per hash (per pair) the sum of the
// multiplicities of the merged reads that carry it: the in-LDS kernel for the reads within the bound, keys + sort + add for the
// longer ones.  With amplicons also d_count[] = every hash's total over its pairs.
void MaskStage::count() {
    if (n_long < n_reads)
        PMX_LAUNCH(k_meta_mask_count, dim3(grid_for(n_reads * 64, 64 * kMaskWaves, G)), dim3(64 * kMaskWaves), 0, st, m->d_read_off.p, count_id,
                   d_mult.p, n_reads, bound, counters);
    if (n_long > 0) {
        PMX_LAUNCH(k_meta_mask_long_keys, dim3(grid_for(n_long * 64, 256, G)), dim3(256), 0, st, m->d_read_off.p, count_id, d_long_read.p,
                   d_long_off.p, n_long, d_key.p);
        unsigned end_bit = 33;   // (the uid, and the bits of the greatest ordinal)
        while (end_bit < 64 && ((uint64_t)(n_long - 1) >> (end_bit - 32)) != 0) ++end_bit;
        PMX_ROCPRIM(tmp, radix_sort_keys, d_key.p, d_key_sorted.p, (size_t)n_keys, 0u, end_bit, st);
        PMX_LAUNCH(k_meta_mask_long_add, dim3(grid_for(n_keys, 256, G)), dim3(256), 0, st, d_key_sorted.p, n_keys, d_long_read.p, d_mult.p, counters);
    }
    if (grouped)
        PMX_LAUNCH(k_meta_amp_totals, dim3(grid_for(n_seedmers, 256, G)), dim3(256), 0, st, d_pair_key.p, d_pair_count.p, d_before.p + n_seedmers,
                   d_count.p);
}

// Reads: counters[], the thresholds.  Leaves: per read its new length and alive[], per hash used[], their exclusive scans
// (d_new_off, d_read_pos, d_uid_pos) and, after the call's one synchronize before the compaction, the survivors' sizes
// left_seedmers / left_reads / left_uniq, h_ctr[] and n_pairs on the host.
void MaskStage::flag_and_size() {
    with_grouped(grouped, [&](auto g) {
        PMX_LAUNCH(k_meta_mask_flag<decltype(g)::value>, dim3(grid_for(n_reads * 64, 256, G)), dim3(256), 0, st, m->d_read_off.p, m->d_seed_uid.p,
                   n_reads, counters, threshold, whole_reads ? 1 : 0, d_new_len.p, d_alive.p, d_used.p, d_ctr.p, d_seed_pid.p, d_read_amp.p, d_thr.p);
    });
    PMX_ROCPRIM(tmp, exclusive_scan, d_new_len.p, d_new_off.p, (int64_t)0, (size_t)n_reads + 1, rocprim::plus<int64_t>(), st);
    PMX_ROCPRIM(tmp, exclusive_scan, d_alive.p, d_read_pos.p, 0u, (size_t)n_reads + 1, rocprim::plus<uint32_t>(), st);
    PMX_ROCPRIM(tmp, exclusive_scan, d_used.p, d_uid_pos.p, 0u, (size_t)n_uniq + 1, rocprim::plus<uint32_t>(), st);
    PMX_D2H(&left_seedmers, pmx::at(d_new_off, n_reads), 1, st);
    PMX_D2H(&left_reads, pmx::at(d_read_pos, n_reads), 1, st);
    PMX_D2H(&left_uniq, pmx::at(d_uid_pos, n_uniq), 1, st);
    PMX_D2H(h_ctr, d_ctr, st);
    if (grouped) PMX_D2H(&n_pairs, pmx::at(d_before, n_seedmers), 1, st);
    PMX_HIP(hipStreamSynchronize(st));
}

// Reads: the flags' scans and the sizes.  Leaves: the survivors in o_*: offsets, hash / new uid / orientation per entry,
// multiplicity (and amplicon) per read, the surviving distinct hashes with their counts before masking.
void MaskStage::compact() {
    o_off.alloc((size_t)left_reads + 1); o_mult.alloc((size_t)left_reads); o_count.alloc((size_t)left_uniq);
    o_hash.alloc((size_t)left_seedmers); o_uid.alloc((size_t)left_seedmers); o_rev.alloc((size_t)left_seedmers); o_uniq.alloc((size_t)left_uniq);
    if (grouped) o_amp.alloc((size_t)left_reads);
    with_grouped(grouped, [&](auto g) {
        PMX_LAUNCH(k_meta_mask_compact<decltype(g)::value>, dim3(grid_for(n_reads * 64, 256, G)), dim3(256), 0, st, m->d_read_off.p, m->d_seed_uid.p,
                   m->d_seed_rev.p, m->d_uniq.p, d_mult.p, n_reads, counters, threshold, d_new_len.p, d_new_off.p, d_read_pos.p, d_uid_pos.p, o_off.p,
                   o_hash.p, o_uid.p, o_rev.p, o_mult.p, d_seed_pid.p, d_read_amp.p, d_thr.p, o_amp.p);
    });
    PMX_LAUNCH(k_meta_mask_compact_uniq, dim3(grid_for(n_uniq, 256, G)), dim3(256), 0, st, m->d_uniq.p, d_count.p, d_used.p, d_uid_pos.p, n_uniq,
               o_uniq.p, o_count.p);
}

// Reads: o_*, d_count / d_read_pos, the pair table.  Leaves: the sample as its survivors -- the host's copies, which
// meta_assign.hip, the EM and the getters read, m->d_* (swapped with o_*), n_reads / n_seedmers, h_raw_to_merged rewritten
// through read_pos -- with the counts before masking (m->lowcov_count), the three numbers and, with amplicons, the
// (group, hash, count) triples before masking in pair order, the survivors' amplicons and amp_left.
void MaskStage::publish() {
    std::vector<uint32_t> read_pos((size_t)n_reads + 1);
    PMX_D2H(m->lowcov_count, d_count, n_uniq, st);
    PMX_D2H(read_pos, d_read_pos, (size_t)n_reads + 1, st);
    m->h_read_off.assign((size_t)left_reads + 1, 0);
    m->h_mult.resize((size_t)left_reads);
    m->h_seed_hash.resize((size_t)left_seedmers); m->h_seed_uid.resize((size_t)left_seedmers); m->h_seed_rev.resize((size_t)left_seedmers);
    m->h_uniq.resize((size_t)left_uniq);
    PMX_D2H(m->h_read_off, o_off, (size_t)left_reads + 1, st);
    if (left_reads > 0) {
        PMX_D2H(m->h_mult, o_mult, left_reads, st);
        PMX_D2H(m->h_seed_hash, o_hash, left_seedmers, st);
        PMX_D2H(m->h_seed_uid, o_uid, left_seedmers, st);
        PMX_D2H(m->h_seed_rev, o_rev, left_seedmers, st);
        PMX_D2H(m->h_uniq, o_uniq, left_uniq, st);
    }
    std::vector<uint64_t> pair_key((size_t)n_pairs);
    if (grouped) {
        m->ampc_count.resize((size_t)n_pairs);
        m->h_read_amp.resize((size_t)left_reads);
        PMX_D2H(pair_key, d_pair_key, n_pairs, st);
        PMX_D2H(m->ampc_count, d_pair_count, n_pairs, st);
        PMX_D2H(m->h_read_amp, o_amp, left_reads, st);
    }
    PMX_HIP(hipStreamSynchronize(st));
    if (grouped) {
        m->ampc_group.resize((size_t)n_pairs);
        m->ampc_hash.resize((size_t)n_pairs);
        for (size_t p = 0; p < (size_t)n_pairs; ++p) {
            m->ampc_group[p] = (int32_t)(pair_key[p] >> 32);
            m->ampc_hash[p] = m->lowcov_hash[(size_t)(uint32_t)pair_key[p]];
        }
        m->amp_left.assign((size_t)m->n_amp, 0);
        for (int32_t g : m->h_read_amp) ++m->amp_left[(size_t)g];
    }
    for (int64_t& to : m->h_raw_to_merged)
        if (to >= 0) to = read_pos[(size_t)to + 1] > read_pos[(size_t)to] ? (int64_t)read_pos[(size_t)to] : -1;
    m->d_read_off.swap(o_off); m->d_seed_uid.swap(o_uid); m->d_seed_rev.swap(o_rev); m->d_uniq.swap(o_uniq); m->d_uniq_count.swap(o_count);
    m->n_reads = left_reads;
    m->n_seedmers = left_seedmers;
    m->lowcov_reads_dropped = (int64_t)h_ctr[0];
    m->lowcov_seeds_removed = (int64_t)h_ctr[1];
    m->lowcov_reads_left = left_reads;
}
}  // namespace

// The mask step of pmx_meta_set_reads.  False when no mask is set: m->masked cleared, nothing launched or allocated.  Else the
// steps of MaskStage in order; a sample without merged reads ends after the host's resets, ahead of every allocation and
// launch.  Either way no "meta_mask" / "meta_mask_sort" span is left from an earlier call; a run that launches records its own.
bool meta_apply_masks(pmx_ctx* ctx, pmx_meta* m) {
    m->masked = false;
    timer_cancel(ctx, "meta_mask");
    timer_cancel(ctx, "meta_mask_sort");
    if (meta_masks_above_zero(m->lowcov_reads, m->lowcov_seeds, m->lowcov_reads_rf, m->lowcov_seeds_rf) == 0) return false;
    MaskStage S(ctx, m);
    S.reset_results();
    S.group_thresholds();
    if (S.empty()) return true;
    S.plan_sorted_path();
    S.upload();
    timer_begin(ctx, "meta_mask");
    S.clear_counters();
    if (S.grouped) S.rank_pairs();
    S.count();
    S.flag_and_size();
    S.compact();
    timer_end(ctx, "meta_mask", 1);
    S.publish();
    return true;
}

// Overlap coefficients after meta_apply_masks: their numerator set is the hashes the surviving lists hold
// (allSeedmerHashesSet, src/mgsr.cpp:5685-5768), so the placer's histogram is loaded with exactly those, from the device
// arrays the mask step left (each with its occurrence count before masking: at min_read_support 1 only its presence acts);
// the raw reads are not seeded again.  --gpus N: every rank holds the whole sample's survivors, nothing is exchanged.
// Reads: m->d_uniq / d_uniq_count / h_uniq / h_mult.  Leaves: m->oc.
int meta_masked_overlap_coefficients(pmx_ctx* ctx, pmx_meta* m) {
    m->oc.assign((size_t)m->n_nodes, 0.0);
    if (m->n_reads == 0) return PMX_OK;
    int64_t n_kept = 0;
    for (int64_t w : m->h_mult) n_kept += w;
    int rc = pmx_place_reset(ctx, m->placer);
    if (rc == PMX_OK) rc = pmx_place_histogram_merge_device(ctx, m->placer, m->d_uniq.p, m->d_uniq_count.p, (int64_t)m->h_uniq.size());
    return meta_overlap_from_histogram(ctx, m, rc, n_kept, nullptr);
}

extern "C" {

int pmx_meta_set_masks(pmx_meta* m, int64_t mask_reads, int64_t mask_seeds) {
    if (!m) return PMX_ERR_ARG;
    if (mask_reads < 0 || mask_seeds < 0) return fail(PMX_ERR_ARG, "pmx_meta_set_masks: a masking parameter must not be negative");
    if (meta_masks_above_zero(mask_reads, mask_seeds, m->lowcov_reads_rf, m->lowcov_seeds_rf) > 1)
        return fail(PMX_ERR_ARG, "Only one masking parameter can be set at a time");   // src/mgsr.cpp:2049-2053
    m->lowcov_reads = mask_reads;
    m->lowcov_seeds = mask_seeds;
    return PMX_OK;
}

int pmx_meta_set_relative_masks(pmx_meta* m, double reads_rf, double seeds_rf) {
    if (!m) return PMX_ERR_ARG;
    if (!(reads_rf >= 0) || !(seeds_rf >= 0)) return fail(PMX_ERR_ARG, "pmx_meta_set_relative_masks: a masking parameter must not be negative");
    if (meta_masks_above_zero(m->lowcov_reads, m->lowcov_seeds, reads_rf, seeds_rf) > 1)
        return fail(PMX_ERR_ARG, "Only one masking parameter can be set at a time");
    m->lowcov_reads_rf = reads_rf;
    m->lowcov_seeds_rf = seeds_rf;
    return PMX_OK;
}

int pmx_meta_set_amplicons(pmx_meta* m, const int32_t* group_of_read, int64_t n_reads, int32_t n_groups) {
    if (!m || n_reads < 0 || n_groups < 0) return PMX_ERR_ARG;
    if (!group_of_read) {   // cleared
        if (n_reads != 0) return PMX_ERR_ARG;
        m->amp_set = false;
        m->amp_n_groups = 0;
        m->amp_of_raw.clear();
        return PMX_OK;
    }
    for (int64_t r = 0; r < n_reads; ++r)
        if (group_of_read[r] < 0 || group_of_read[r] > n_groups)
            return fail(PMX_ERR_ARG, "pmx_meta_set_amplicons: the amplicon of read " + std::to_string(r) + " is not in [0, n_groups]");
    m->amp_set = true;
    m->amp_n_groups = n_groups;
    m->amp_of_raw.assign(group_of_read, group_of_read + n_reads);
    return PMX_OK;
}

int pmx_meta_read_amplicons(const pmx_meta* m, int32_t* amplicon, int64_t cap) {
    if (!m) return PMX_ERR_ARG;
    if (!m->amp_on) return fail(PMX_ERR_ARG, "pmx_meta_read_amplicons: the last pmx_meta_set_reads ran without amplicons");
    if (cap < m->n_reads) return PMX_ERR_ARG;
    if (amplicon) std::copy(m->h_read_amp.begin(), m->h_read_amp.end(), amplicon);
    return PMX_OK;
}

int32_t pmx_meta_num_amplicon_groups(const pmx_meta* m) { return m && m->amp_on ? m->n_amp : 0; }

int pmx_meta_amplicon_info(const pmx_meta* m, int64_t* raw_reads, int64_t* threshold, int64_t* merged_before, int64_t* merged_left, int64_t cap) {
    if (!m) return PMX_ERR_ARG;
    if (!m->amp_on) return fail(PMX_ERR_ARG, "pmx_meta_amplicon_info: the last pmx_meta_set_reads ran without amplicons");
    if (cap < (int64_t)m->n_amp) return PMX_ERR_ARG;
    if (raw_reads) std::copy(m->amp_raw.begin(), m->amp_raw.end(), raw_reads);
    if (threshold) std::copy(m->amp_thr.begin(), m->amp_thr.end(), threshold);
    if (merged_before) std::copy(m->amp_before.begin(), m->amp_before.end(), merged_before);
    if (merged_left) std::copy(m->amp_left.begin(), m->amp_left.end(), merged_left);
    return PMX_OK;
}

int64_t pmx_meta_amplicon_num_counts(const pmx_meta* m) { return m && m->amp_on && m->masked ? (int64_t)m->ampc_hash.size() : 0; }

int pmx_meta_amplicon_counts(const pmx_meta* m, int32_t* group, uint64_t* hash, int64_t* count, int64_t cap) {
    if (!m) return PMX_ERR_ARG;
    if (!m->amp_on || !m->masked) return fail(PMX_ERR_ARG, "pmx_meta_amplicon_counts: the last pmx_meta_set_reads ran without amplicons or without a mask");
    if (cap < (int64_t)m->ampc_hash.size()) return PMX_ERR_ARG;
    if (group) std::copy(m->ampc_group.begin(), m->ampc_group.end(), group);
    if (hash) std::copy(m->ampc_hash.begin(), m->ampc_hash.end(), hash);
    if (count) std::copy(m->ampc_count.begin(), m->ampc_count.end(), count);
    return PMX_OK;
}

int pmx_meta_mask_info(const pmx_meta* m, int64_t* reads_dropped, int64_t* seeds_removed, int64_t* reads_left) {
    if (!m) return PMX_ERR_ARG;
    if (reads_dropped) *reads_dropped = m->masked ? m->lowcov_reads_dropped : 0;
    if (seeds_removed) *seeds_removed = m->masked ? m->lowcov_seeds_removed : 0;
    if (reads_left) *reads_left = m->n_reads;
    return PMX_OK;
}

int64_t pmx_meta_mask_num_counts(const pmx_meta* m) { return m && m->masked ? (int64_t)m->lowcov_hash.size() : 0; }

int pmx_meta_mask_counts(const pmx_meta* m, uint64_t* hash, int64_t* count, int64_t cap) {
    if (!m) return PMX_ERR_ARG;
    if (!m->masked) return fail(PMX_ERR_ARG, "pmx_meta_mask_counts: the last pmx_meta_set_reads ran without a mask");
    if (cap < (int64_t)m->lowcov_hash.size()) return PMX_ERR_ARG;
    if (hash) std::copy(m->lowcov_hash.begin(), m->lowcov_hash.end(), hash);
    if (count) std::copy(m->lowcov_count.begin(), m->lowcov_count.end(), count);
    return PMX_OK;
}

}  // extern "C"
