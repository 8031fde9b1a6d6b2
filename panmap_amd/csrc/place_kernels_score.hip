// PLACE stage, scoring pass for gfx950 (wave64): the probe table of the kept seeds, the weighted-containment
// denominator, the per-change terms, per-node delta scoring down the tree in its three forms, and the score getters.
// Nothing here is shared with the seeding side (place_kernels.hip).  FP64 accumulation in the reference's order on
// latency-bound access patterns: no MFMA.  Reference behaviour: src/placement.cpp:242-345 (computeChildMetrics),
// :1863-1876 (weighted-containment denominator), src/placement.hpp:120-149 (score getters).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device/pmx_math.h"
#include "place_kernels.h"

namespace pmx {

__global__ void k_kept_table_build(const uint64_t* __restrict__ kept_hash, const double* __restrict__ kept_log, int64_t n,
                                   uint64_t* tkeys, double* tvals, uint64_t mask) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = kept_hash[i];
        uint64_t slot = mix64(key) & mask;
        while (true) {
            unsigned long long prev = atomicCAS((unsigned long long*)&tkeys[slot], (unsigned long long)PMX_EMPTY_KEY, (unsigned long long)key);
            if (prev == PMX_EMPTY_KEY) { tvals[slot] = kept_log[i]; break; }
            slot = (slot + 1) & mask;
        }
    }
}

__device__ __forceinline__ bool kept_lookup(const uint64_t* __restrict__ tkeys, const double* __restrict__ tvals, uint64_t mask,
                                            uint64_t key, double* L) {
    uint64_t slot = mix64(key) & mask;
    while (true) {
        const uint64_t k = tkeys[slot];
        if (k == key) { *L = tvals[slot]; return true; }
        if (k == PMX_EMPTY_KEY) return false;
        slot = (slot + 1) & mask;
    }
}

// weighted-containment denominator: root changes in stored order (src/placement.cpp:1863-1876).  One wave:
// lanes probe 64 changes at a time, then the additions run in stored order.
__global__ void __launch_bounds__(1024)
k_wc_denominator(const uint64_t* __restrict__ ch_hash, const int16_t* __restrict__ ch_child, uint64_t beg, uint64_t end,
                 const uint64_t* __restrict__ tkeys, const double* __restrict__ tvals, uint64_t mask, int has_kept, double* out) {
    // one block: every thread probes its changes in parallel into an LDS tile, then thread 0 adds the tile in
    // stored order (a no-hit change contributes +0.0, which is exact; see add_changes)
    __shared__ double tile[1024];
    if (blockIdx.x != 0) return;
    double acc = 0.0;
    for (uint64_t base = beg; base < end; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        double inv = 0.0;
        if (i < end) {
            const int16_t cc = ch_child[i];
            double L;
            if (cc > 0 && has_kept && kept_lookup(tkeys, tvals, mask, ch_hash[i], &L)) inv = 1.0 / (double)cc;
        }
        tile[threadIdx.x] = inv;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = (int)((end - base) < blockDim.x ? (end - base) : blockDim.x);
            int j = 0;
            for (; j + 8 <= cnt; j += 8) {
                const double v0 = tile[j], v1 = tile[j + 1], v2 = tile[j + 2], v3 = tile[j + 3], v4 = tile[j + 4], v5 = tile[j + 5],
                             v6 = tile[j + 6], v7 = tile[j + 7];
                acc += v0; acc += v1; acc += v2; acc += v3; acc += v4; acc += v5; acc += v6; acc += v7;
            }
            for (; j < cnt; ++j) acc += tile[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = acc;
}

// --------------------------------------------------------------------------- node scoring
// Child state = parent state + own deltas applied in stored order (src/placement.cpp:242-345, :772-774).
// The floating-point additions are replayed strictly in stored order so every accumulator sees the
// reference's operation sequence (the integer counters are order-free and are wave-reduced).  A BFS level
// lasts as long as its largest node, so the per-change critical path is what matters: everything that does
// not depend on the order (log1p, table probe, the terms) is computed for all changes at once in pass 1;
// pass 2 streams the terms (two 64-change chunks in flight), stages each chunk in LDS and lets five lanes add
// it up, one accumulator each (add_changes).  A change that misses the kept-seed table carries +0.0 for the
// four hit-only accumulators: the reference's control flow skips it, and adding +0.0 changes nothing.

// Pass 1 (one launch, every seed change of the index in parallel): the order-independent part -- log1p,
// kept-seed table probe, the five per-change terms -- written as SoA so pass 2 streams them coalesced.
// meta: bit 0 = hit, bits 1-2 = d_pres + 1, bits 3-4 = d_uniq + 1.
__global__ void __launch_bounds__(256)
k_score_terms(const uint64_t* __restrict__ ch_hash, const int16_t* __restrict__ ch_par, const int16_t* __restrict__ ch_child,
              int64_t n_changes, const uint64_t* __restrict__ tkeys, const double* __restrict__ tvals, uint64_t mask, int has_kept,
              double* __restrict__ t_mag, double* __restrict__ t_raw, double* __restrict__ t_cos, double* __restrict__ t_wc,
              double* __restrict__ t_lc, uint8_t* __restrict__ t_meta) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_changes; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pc = ch_par[i], cc = ch_child[i];
        const double logC = cc > 0 ? log1p_count(cc) : 0.0;
        const double logP = pc > 0 ? log1p_count(pc) : 0.0;
        t_mag[i] = logC * logC - logP * logP;
        const int d_uniq = (cc > 0) - (pc > 0);
        int d_pres = 0, hit = 0;
        double L, d_raw = 0.0, d_cos = 0.0, d_wc = 0.0, d_lc = 0.0;
        if (cc != pc && has_kept && kept_lookup(tkeys, tvals, mask, ch_hash[i], &L)) {
            hit = 1;
            d_pres = (int)((pc == 0) & (cc != 0)) - (int)((cc == 0) & (pc != 0));
            const double o1 = pc > 0 ? L / (double)pc : 0.0, n1 = cc > 0 ? L / (double)cc : 0.0;
            d_raw = n1 - o1;
            d_cos = L * (logC - logP);
            const double o2 = pc > 0 ? 1.0 / (double)pc : 0.0, n2 = cc > 0 ? 1.0 / (double)cc : 0.0;
            d_wc = n2 - o2;
            d_lc = (double)d_pres * L;
        }
        t_raw[i] = d_raw; t_cos[i] = d_cos; t_wc[i] = d_wc; t_lc[i] = d_lc;
        t_meta[i] = (uint8_t)(hit | (d_pres + 1) << 1 | (d_uniq + 1) << 3);
    }
}

struct ScoreTerms {
    double d_raw, d_cos, d_wc, d_lc, d_mag;
    int d_pres, d_uniq, hit;
};

__device__ __forceinline__ ScoreTerms load_terms(uint64_t i, uint64_t end, const TermArrays& ta) {
    ScoreTerms t;
    t.d_raw = t.d_cos = t.d_wc = t.d_lc = t.d_mag = 0.0;
    t.d_pres = t.d_uniq = t.hit = 0;
    if (i < end) {   // all six loads are independent: nothing waits until the terms are used two chunks later
        const int m = ta.meta[i];
        t.d_mag = ta.mag[i];
        t.d_raw = ta.raw[i]; t.d_cos = ta.cos[i]; t.d_wc = ta.wc[i]; t.d_lc = ta.lc[i];
        t.hit = m & 1;
        t.d_pres = (m & 1) ? ((m >> 1) & 3) - 1 : 0;
        t.d_uniq = ((m >> 3) & 3) - 1;
    }
    return t;
}

// wave-wide integer sum through DPP (quad swaps, then the two row mirrors: every lane of a 16-lane row holds the row's
// total; four scalar reads add the rows): ~10 instructions instead of six ds_bpermute round trips through the LDS
// crossbar, each followed by a wait -- the sums sit in front of every chunk of the scoring kernels' serial add chains
__device__ __forceinline__ int wave_sum_int(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);   // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// What a wave carries from a node to its children: the five FP64 accumulators and the two integer counters.
struct NodeState {
    double acc = 0.0;              // lane k < 5: accumulator k (raw, cos, wc, lc, mag)
    int64_t c0 = 0, c1 = 0;        // present kept seeds, unique seeds (every lane)

    __device__ __forceinline__ void load(const double* metrics5, const int64_t* counts2, uint32_t nd, int lane) {
        if (lane < 5) acc = metrics5[5 * (size_t)nd + lane];
        c0 = counts2[2 * (size_t)nd + 0]; c1 = counts2[2 * (size_t)nd + 1];
    }
    __device__ __forceinline__ void store(double* metrics5, int64_t* counts2, uint32_t nd, int lane) const {
        if (lane < 5) metrics5[5 * (size_t)nd + lane] = acc;
        if (lane == 0) { counts2[2 * (size_t)nd + 0] = c0; counts2[2 * (size_t)nd + 1] = c1; }
    }
};

// The per-node arithmetic of all three scoring kernels: the terms of the changes [beg, end) are added to the state in
// stored order.  cur and nx1 are the node's first two 64-change chunks, requested by the caller (before it waits for
// anything); sh is the wave's own 64 * 5 doubles of LDS.
// The five accumulators are five independent serial chains, so they run in five LANES: each 64-change chunk
// is staged in LDS as [change][accumulator] and lanes 0..4 walk it with one ds_read + one v_add_f64 per
// change (a no-hit change carries +0.0 for the four hit-only terms: adding +0.0 is exact, and no accumulator
// can be -0.0).  The critical path per change is one FP64 add instead of a dozen broadcast instructions.
__device__ __forceinline__ void add_changes(NodeState& s, uint64_t beg, uint64_t end, ScoreTerms cur, ScoreTerms nx1, const TermArrays& ta,
                                            double* sh, int lane) {
    double acc = s.acc;   // a local, written back once: added to through the reference, every kernel takes 14-16 more VGPRs
    for (uint64_t base = beg; base < end; base += 64) {
        // two chunks of terms are in flight while this one is added up
        const ScoreTerms nx2 = load_terms(base + 128 + lane, end, ta);
        const int cnt = (int)((end - base) < 64 ? (end - base) : 64);
        s.c1 += wave_sum_int(cur.d_uniq);
        s.c0 += wave_sum_int(cur.d_pres);          // d_pres is 0 unless hit
        sh[lane * 5 + 0] = cur.d_raw; sh[lane * 5 + 1] = cur.d_cos; sh[lane * 5 + 2] = cur.d_wc; sh[lane * 5 + 3] = cur.d_lc;
        sh[lane * 5 + 4] = cur.d_mag;
        __builtin_amdgcn_wave_barrier();          // same-wave LDS traffic is ordered; this only pins the compiler
        if (lane < 5) {
            // eight terms per step, the next eight requested from LDS before these are added: the chain of FP64
            // adds is the kernels' critical path and does not wait for an LDS round trip per step
            int j = 0;
            if (cnt >= 8) {
                const double* q = sh + lane;
                double a0 = q[0], a1 = q[5], a2 = q[10], a3 = q[15], a4 = q[20], a5 = q[25], a6 = q[30], a7 = q[35];
                for (; j + 16 <= cnt; j += 8) {
                    q += 40;
                    const double b0 = q[0], b1 = q[5], b2 = q[10], b3 = q[15], b4 = q[20], b5 = q[25], b6 = q[30], b7 = q[35];
                    acc += a0; acc += a1; acc += a2; acc += a3; acc += a4; acc += a5; acc += a6; acc += a7;
                    a0 = b0; a1 = b1; a2 = b2; a3 = b3; a4 = b4; a5 = b5; a6 = b6; a7 = b7;
                }
                acc += a0; acc += a1; acc += a2; acc += a3; acc += a4; acc += a5; acc += a6; acc += a7;
                j += 8;
            }
            for (; j < cnt; ++j) acc += sh[j * 5 + lane];
        }
        __builtin_amdgcn_wave_barrier();
        cur = nx1;
        nx1 = nx2;
    }
    s.acc = acc;
}

// A wave of a persistent kernel waits until node pa is finished: done[] holds the epoch of the call that last finished
// the node (no clearing between calls).  A wave that polls longer than any sane run sets *status and every wave
// leaves: false, and the caller returns (uniform: every lane polls the same flag).  On success the acquire fence has
// been passed and pa's state may be loaded.  SLEEP is s_sleep's argument, which has to be a constant.
template <int SLEEP>
__device__ __forceinline__ bool wait_for_parent(const uint32_t* done, uint32_t pa, uint32_t epoch, uint32_t* status, int lane) {
    uint32_t polls = 0;
    while (__hip_atomic_load(&done[pa], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
        __builtin_amdgcn_s_sleep(SLEEP);
        // (the shared status word is looked at every 1024 polls only: one word read by every waiting wave is a hot spot)
        if (++polls > (1u << 24) || ((polls & 1023u) == 0u && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            if (lane == 0) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}

// Pass 2, one launch per BFS level, one wave per node: parent state + the node's terms added in stored order.
__global__ void __launch_bounds__(256)
k_score_level(const uint32_t* __restrict__ level_nodes, int64_t n_level, const uint32_t* __restrict__ parent,
              const uint64_t* __restrict__ offsets, const TermArrays ta, double* metrics5, int64_t* counts2) {
    __shared__ double stage[4][64 * 5];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + wib;
    if (wv >= n_level) return;
    const uint32_t nd = level_nodes[wv];
    const uint64_t beg = offsets[nd], end = offsets[nd + 1];
    const ScoreTerms cur = load_terms(beg + lane, end, ta);
    const ScoreTerms nx1 = load_terms(beg + 64 + lane, end, ta);
    NodeState s;
    if (nd != 0) s.load(metrics5, counts2, parent[nd], lane);
    add_changes(s, beg, end, cur, nx1, ta, stage[wib], lane);
    s.store(metrics5, counts2, nd, lane);
}

// Pass 2 as ONE persistent launch: wave w takes the BFS positions w, w + W, w + 2W, ... (W = resident waves) and
// waits for its node's parent through a per-node flag instead of a kernel boundary per level.  A parent always
// sits at an earlier BFS position, and every wave works through its positions in ascending order, so the wave that
// owns the earliest unfinished position never waits on anything unfinished: no deadlock as long as all W waves are
// resident (the host launches at most one workgroup per CU).  The arithmetic per node is add_changes, as in
// k_score_level.
__global__ void __launch_bounds__(256)
k_score_tree(const uint32_t* __restrict__ order, int64_t n_nodes, const uint32_t* __restrict__ parent, const uint64_t* __restrict__ offsets,
             const TermArrays ta, double* metrics5, int64_t* counts2, uint32_t* done, uint32_t epoch, uint32_t* status) {
    __shared__ double stage[4][64 * 5];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + wib; p < n_nodes; p += n_waves) {
        const uint32_t nd = order[p];
        const uint64_t beg = offsets[nd], end = offsets[nd + 1];
        // the node's own terms do not depend on the parent: in flight while the wave waits for it
        const ScoreTerms cur = load_terms(beg + lane, end, ta);
        const ScoreTerms nx1 = load_terms(beg + 64 + lane, end, ta);
        NodeState s;
        if (nd != 0) {
            const uint32_t pa = parent[nd];
            if (!wait_for_parent<2>(done, pa, epoch, status, lane)) return;
            s.load(metrics5, counts2, pa, lane);
        }
        add_changes(s, beg, end, cur, nx1, ta, stage[wib], lane);
        s.store(metrics5, counts2, nd, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // the wave's stores are visible before the flag
        if (lane == 0) __hip_atomic_store(&done[nd], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Pass 2, heavy-path form: the host cuts the tree into chains (a node followed by its heaviest child, and so on
// down to a leaf) and one wave walks one chain with the five accumulators staying in registers from node to node.
// Only the HEAD of a chain waits on a flag (its parent lies in a chain that started earlier), and only nodes with
// two or more children publish one: a root-to-leaf path crosses O(log n) chain boundaries instead of one kernel
// boundary (or flag) per level.  chain_nodes[k] = node id | publish << 31; chain_beg/end[k] = the node's change
// range, gathered in chain order so that the next node's terms are requested while this one is being added up.
// Chains are sorted by the BFS position of their head and wave w takes chains w, w + W, ...: the chain that holds
// a head's parent starts earlier, so the earliest unfinished chain never waits on an unfinished one (all W waves
// are resident: at most one workgroup per CU).  Per node the arithmetic is add_changes, as in k_score_level.
#define PMX_CHAIN_FLUSH 8u
#define PMX_CHAIN_AHEAD 3
__global__ void __launch_bounds__(256)
k_score_chains(const uint32_t* __restrict__ chain_off, int64_t n_chains, const uint32_t* __restrict__ chain_nodes,
               const uint64_t* __restrict__ chain_beg, const uint64_t* __restrict__ chain_end, const uint32_t* __restrict__ parent,
               const TermArrays ta, double* metrics5, int64_t* counts2, uint32_t* done, uint32_t epoch, uint32_t* status) {
    __shared__ double stage[4][64 * 5];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wib; c < n_chains; c += n_waves) {
        const uint32_t cb = chain_off[c], ce = chain_off[c + 1];
        // Software pipeline over the chain: the first two 64-change chunks of the nodes k+1 .. k+PMX_CHAIN_AHEAD are
        // in flight while node k is added up (a node's own arithmetic is a fraction of a microsecond, a load from
        // HBM two), and the (node, range) records run one node further ahead still.
        constexpr int AH = PMX_CHAIN_AHEAD;
        uint32_t m_ent[AH + 2];
        uint64_t m_beg[AH + 2], m_end[AH + 2];
#pragma unroll
        for (int a_ = 0; a_ < AH + 2; ++a_) {
            const bool in = cb + (uint32_t)a_ < ce;
            m_ent[a_] = in ? chain_nodes[cb + a_] : 0u;
            m_beg[a_] = in ? chain_beg[cb + a_] : 0;
            m_end[a_] = in ? chain_end[cb + a_] : 0;
        }
        ScoreTerms q_cur[AH + 1], q_nx1[AH + 1];
#pragma unroll
        for (int a_ = 0; a_ < AH + 1; ++a_) {
            q_cur[a_] = load_terms(m_beg[a_] + lane, m_end[a_], ta);
            q_nx1[a_] = load_terms(m_beg[a_] + 64 + lane, m_end[a_], ta);
        }
        NodeState s;
        const uint32_t head = m_ent[0] & 0x7fffffffu;
        if (head != 0) {
            const uint32_t pa = parent[head];
            if (!wait_for_parent<1>(done, pa, epoch, status, lane)) return;
            s.load(metrics5, counts2, pa, lane);
        }
        // Flags are published in batches: the release fence (an L2 write-back plus a wait, ~2-6 us) would otherwise sit
        // on the chain's critical path at every node that has a second child -- on a caterpillar-shaped tree that is
        // every node of the spine.  One fence per PMX_CHAIN_FLUSH publishing nodes (and one at the chain's end)
        // covers all their stores; the lanes then set the flags of chain positions [k_from, k] in one instruction.
        uint32_t k_from = cb, n_pend = 0;
        for (uint32_t k = cb; k < ce; ++k) {
            const uint32_t ent = m_ent[0];
            const uint32_t nd = ent & 0x7fffffffu;
            const bool publish = (ent >> 31) != 0;
            // request the chunks of node k + AH + 1 (its record arrived an iteration ago) and the record after that
            const ScoreTerms f_cur = load_terms(m_beg[AH + 1] + lane, m_end[AH + 1], ta);
            const ScoreTerms f_nx1 = load_terms(m_beg[AH + 1] + 64 + lane, m_end[AH + 1], ta);
            const bool in_f = k + (uint32_t)(AH + 2) < ce;
            const uint32_t f_ent = in_f ? chain_nodes[k + AH + 2] : 0u;
            const uint64_t f_beg = in_f ? chain_beg[k + AH + 2] : 0, f_end = in_f ? chain_end[k + AH + 2] : 0;
            add_changes(s, m_beg[0], m_end[0], q_cur[0], q_nx1[0], ta, stage[wib], lane);
            s.store(metrics5, counts2, nd, lane);
            n_pend += publish ? 1u : 0u;   // children in other chains wait for this node
            if (n_pend >= PMX_CHAIN_FLUSH || (k + 1 == ce && n_pend > 0)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                for (uint32_t q = k_from + (uint32_t)lane; q <= k; q += 64u) {
                    const uint32_t e = chain_nodes[q];
                    if (e >> 31) __hip_atomic_store(&done[e & 0x7fffffffu], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                k_from = k + 1;
                n_pend = 0;
            }
#pragma unroll
            for (int a_ = 0; a_ < AH; ++a_) { q_cur[a_] = q_cur[a_ + 1]; q_nx1[a_] = q_nx1[a_ + 1]; }
            q_cur[AH] = f_cur; q_nx1[AH] = f_nx1;
#pragma unroll
            for (int a_ = 0; a_ < AH + 1; ++a_) { m_ent[a_] = m_ent[a_ + 1]; m_beg[a_] = m_beg[a_ + 1]; m_end[a_] = m_end[a_ + 1]; }
            m_ent[AH + 1] = f_ent; m_beg[AH + 1] = f_beg; m_end[AH + 1] = f_end;
        }
    }
}

// score getters (src/placement.hpp:120-149); TSV order log_raw, log_cosine, containment,
// weighted_containment, log_containment
// scores5[node][metric] for the node outputs, and scores_bfs[metric][visit position] for the host's sequential
// best/tie rule (one contiguous array per metric, in the order the rule visits the nodes)
// (the three denominators are read from the device scalars [sum L^2, sum L, wc_den]: no host round trip before this launch)
__global__ void k_score_getters(const double* __restrict__ metrics5, const int64_t* __restrict__ counts2, int64_t n_nodes,
                                const double* __restrict__ scalars, int64_t n_kept, double* scores5,
                                const uint32_t* __restrict__ order, double* scores_bfs) {
    const double log_mag = sqrt(scalars[0]), log_cont_den = scalars[1], wc_den = scalars[2];
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_nodes; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t nd = (int64_t)order[j];
        const double* m = metrics5 + 5 * nd;
        double* sc = scores5 + 5 * nd;
        sc[0] = log_mag <= 0.0 ? 0.0 : m[0] / log_mag;
        const double gm = sqrt(m[4]);
        if (log_mag <= 0.0 || gm <= 0.0) sc[1] = 0.0;
        else {
            const double v = m[1] / (log_mag * gm);
            sc[1] = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        }
        sc[2] = n_kept > 0 ? (double)(uint64_t)counts2[2 * nd] / (double)(uint64_t)n_kept : 0.0;
        sc[3] = wc_den > 0.0 ? m[2] / wc_den : 0.0;
        sc[4] = log_cont_den > 0.0 ? m[3] / log_cont_den : 0.0;
        for (int q = 0; q < 5; ++q) scores_bfs[(size_t)q * (size_t)n_nodes + (size_t)j] = sc[q];
    }
}

}  // namespace pmx
