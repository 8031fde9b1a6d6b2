// C ABI, device part 4b: --meta --filter-and-assign (filterAndAssignBatch, src/main.cpp:720-1016; scoreReadsBatch /
// assignReadsBatch, src/mgsr.cpp:7477-7575, 6415-6516).
//
// What the reference does: every read (mates are independent reads) is scored against EVERY node of the tree by one DFS that
// applies and reverts per-node seed deltas (scoreReadsBatchHelper, :7477-7570), score(read, node) = max(f, r) as in the
// abundance mode (api_meta.hip).  A read's maximum over the nodes decides its fate (src/main.cpp:856-863 with the threshold of
// mgsr.cpp:1693, static_cast<int32_t>(discard * n), n = the read's seedmers, :1640, 1667): max == 0 -> unmapped, max below
// the threshold -> discarded, else assigned; the assigned nodes of a read are the nodes whose score equals its maximum, and
// its LCA node is their lowest common ancestor (assignReadsBatchHelper, :6415-6461).
//
// keepForFilterAndAssign changes nothing about that set.  scoreReadsBatchHelper records a read's score at a node only once the
// flag is set, and sets it at the first node (in DFS order) where the score reaches the threshold (:7508-7513, :7549-7551);
// from there on every change of the score is recorded.  assignReadsBatchHelper keeps a read in the running set from a recorded
// score equal to its maximum to the next recorded score that is not, within the subtree (:6432-6443, backtracked :6454-6460).
// For an assigned read max >= threshold, so the node where the score first equals max is recorded (the flag is set there at
// the latest); every later node in DFS order is recorded too, the whole subtree of that node included.  The unrecorded changes
// lie before the flag was set, at scores below the threshold <= max, where the read is not in the running set anyway.  So the
// read is reported exactly at the nodes with score == max, and the LCA accumulated at :6437 is the LCA of that set.
// (--ambiguous-score-threshold(-ratio), --maximum-taxon-number and --taxonomic-metadata act through taxonomy only,
//  checkTaxonIndicesBatch :6463-6496: not built.)
//
// Here every node is a column.  Nodes are in DFS pre-order, so a seedmer that becomes present / absent at node v toggles the
// columns [v, subtree_end[v]]:
//   * k_assign_mark_ends writes only the two END bits of every transition (bit v and bit subtree_end[v] + 1) into the seedmer's
//     row of a (distinct read seedmer x node) bit matrix, one per orientation: two atomics per transition whatever the subtree;
//   * k_assign_prefix_xor turns every row into presence: bit c = XOR of the end bits <= c.  A wave per row, a lane per word: six
//     shift-XOR steps inside the word, the carry into a word is the parity of the lower words' top bits (one ballot);
//   * k_meta_assign_max<PLANES>: a wave per merged read, a lane per pair of words (16-byte loads; rows are padded to an even
//     word count).  The read's seedmers are added into the same / other bit planes as k_meta_scores does; everything after
//     stays bit-sliced: a plane-wise compare gives the columns where same > other and the score planes by select, one
//     top-down pass over the planes gives the word's maximum and the columns that reach it.  A wave max-reduction gives the
//     read's maximum; the same lanes then clear the words that fell short and count what is left;
//   * k_meta_assign_emit: after an exclusive scan of the node counts, a wave per read expands its set bits into the CSR list
//     read -> DFS indices, ascending.
// The merged reads are processed in chunks, each with the rows of ITS distinct seedmers, so that the two bit matrices stay
// under kAssignMatrixBytes and the per-read word masks under kAssignReadRowBytes; no result depends on the chunking.
// The host derives the LCA from (first, last) assigned node: in pre-order it is the lowest ancestor a of `first` with
// subtree_end[a] >= last.  Folding of identical nodes (src/mgsr.cpp:505-532) happens at output time: pmx_index_node_heads.
// parity: unpinned against the reference itself, as for --meta (api_meta.hip); tests/assign_checks.py restates the mode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <vector>

#include "api_internal.hpp"
#include "device/dev_util.hpp"
#include "host/index_build.hpp"
#include "meta_state.hpp"

using namespace pmx;

namespace {
// the two (distinct seedmer x node) bit matrices of a chunk together; 2 GiB holds the SARS 20k tree (626 words a row) with
// 100,000 distinct seedmers: 2 x 100,000 x 626 x 8 B = 1.0 GB
constexpr size_t kAssignMatrixBytes = (size_t)2 << 30;
// the per-read word masks and word maxima of a chunk (10 B per read and word)
constexpr size_t kAssignReadRowBytes = (size_t)1 << 30;

// Every count change of the oriented index whose seedmer becomes present (parent count 0) or absent (child count 0) and whose
// hash the chunk's reads carry: the two end bits of its column range [v, subtree_end[v]] in the seedmer's row.
__global__ void k_assign_mark_ends(const uint64_t* __restrict__ ch_key, const int16_t* __restrict__ ch_pc, const int16_t* __restrict__ ch_cc,
                                   const uint32_t* __restrict__ ch_node, int64_t n_changes, const uint32_t* __restrict__ subtree_end, int64_t n_nodes,
                                   const uint64_t* __restrict__ uniq, int64_t n_uniq, int words, unsigned long long* mask_fwd, unsigned long long* mask_rev) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_changes; c += (int64_t)gridDim.x * blockDim.x) {
        const bool was = ch_pc[c] > 0, is = ch_cc[c] > 0;
        if (was == is) continue;
        const uint64_t key = ch_key[c];
        int64_t uid = find_sorted(uniq, n_uniq, key);
        unsigned long long* row = mask_fwd;
        if (uid < 0) { uid = find_sorted(uniq, n_uniq, key ^ PMX_ORIENT_XOR); row = mask_rev; }
        if (uid < 0) continue;
        row += (size_t)uid * (size_t)words;
        const uint32_t v = ch_node[c];
        const int64_t e = (int64_t)subtree_end[v] + 1;
        atomicXor(&row[v >> 6], 1ULL << (v & 63));
        if (e < n_nodes) atomicXor(&row[e >> 6], 1ULL << (e & 63));   // (a range that ends with the last node has no closing bit)
    }
}

// rows of end bits -> rows of presence: an inclusive prefix XOR along each row.  A wave per row (rows [0, n_rows) of mask_fwd,
// then of mask_rev), a lane per word, 64 words a step.
__global__ void __launch_bounds__(256) k_assign_prefix_xor(unsigned long long* mask_fwd, unsigned long long* mask_rev, int64_t n_rows, int words) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < 2 * n_rows; r += n_waves) {
        unsigned long long* row = (r < n_rows ? mask_fwd + (size_t)r * (size_t)words : mask_rev + (size_t)(r - n_rows) * (size_t)words);
        unsigned carry = 0;   // parity of all bits below this step's words
        for (int base = 0; base < words; base += 64) {
            const int w = base + lane;
            unsigned long long x = w < words ? row[w] : 0ULL;
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
            const unsigned long long tops = __ballot((x >> 63) != 0);   // bit l: the parity of lane l's whole word
            const unsigned below = (unsigned)__popcll(tops & ((1ULL << lane) - 1ULL)) & 1u;
            if ((below ^ carry) != 0) x = ~x;
            if (w < words) row[w] = x;
            carry ^= (unsigned)__popcll(tops) & 1u;
        }
    }
}

// the columns of one word that reach the word's maximum of max(same, other), and that maximum; `valid` masks the columns < N
template <int PLANES>
__device__ __forceinline__ void word_max(const unsigned long long (&same)[PLANES], const unsigned long long (&other)[PLANES], unsigned long long valid,
                                         unsigned long long* cols, uint32_t* mx) {
    unsigned long long gt = 0, eq = ~0ULL;   // same > other, decided from the top plane down
#pragma unroll
    for (int p = PLANES - 1; p >= 0; --p) {
        gt |= eq & same[p] & ~other[p];
        eq &= ~(same[p] ^ other[p]);
    }
    unsigned long long cand = valid;
    uint32_t m = 0;
#pragma unroll
    for (int p = PLANES - 1; p >= 0; --p) {
        const unsigned long long plane = (gt & same[p]) | (~gt & other[p]);
        const unsigned long long t = cand & plane;
        if (t) { cand = t; m |= 1u << p; }
    }
    *cols = cand;
    *mx = m;
}

// A wave per merged read of the chunk (reads [0, n_reads) of read_off, which points at the chunk's first read; seed_uid holds
// the chunk's seedmers from seed_base on as rows of the chunk's matrices, seed_rev is indexed like the whole sample's).
// wmask / wmax: [n_reads][words] scratch; the outputs are per read.  state: 0 unmapped, 1 discarded, 2 assigned; count,
// first and last describe the assigned nodes (count 0 unless assigned).
template <int PLANES>
__global__ void __launch_bounds__(256) k_meta_assign_max(const int64_t* __restrict__ read_off, int64_t seed_base, const uint32_t* __restrict__ seed_uid,
                                                        const uint8_t* __restrict__ seed_rev, int64_t n_reads, const unsigned long long* __restrict__ mask_fwd,
                                                        const unsigned long long* __restrict__ mask_rev, int words, int64_t n_nodes, double discard,
                                                        unsigned long long* wmask, uint16_t* wmax, uint16_t* out_max, uint32_t* out_count,
                                                        uint32_t* out_first, uint32_t* out_last, uint8_t* out_state) {
    const int lane = threadIdx.x & 63;
    const int pairs = words >> 1;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t i0 = read_off[r], i1 = read_off[r + 1];
        unsigned long long* rmask = wmask + (size_t)r * (size_t)words;
        uint16_t* rmaxw = wmax + (size_t)r * (size_t)words;
        uint32_t best = 0;
        for (int q = lane; q < pairs; q += 64) {
            unsigned long long same0[PLANES], other0[PLANES], same1[PLANES], other1[PLANES];
#pragma unroll
            for (int p = 0; p < PLANES; ++p) { same0[p] = 0; other0[p] = 0; same1[p] = 0; other1[p] = 0; }
            for (int64_t i = i0; i < i1; ++i) {
                const size_t at = (size_t)seed_uid[i - seed_base] * (size_t)words + (size_t)(2 * q);
                const ulonglong2 f = *reinterpret_cast<const ulonglong2*>(mask_fwd + at), b = *reinterpret_cast<const ulonglong2*>(mask_rev + at);
                const bool rev = seed_rev[i] != 0;
                planes_add<PLANES>(same0, rev ? b.x : f.x);    // the genome holds it the way the read does
                planes_add<PLANES>(other0, rev ? f.x : b.x);
                planes_add<PLANES>(same1, rev ? b.y : f.y);
                planes_add<PLANES>(other1, rev ? f.y : b.y);
            }
            const int64_t c0 = (int64_t)q * 128, left0 = n_nodes - c0, left1 = left0 - 64;
            const unsigned long long v0 = left0 >= 64 ? ~0ULL : left0 <= 0 ? 0ULL : (1ULL << left0) - 1ULL;
            const unsigned long long v1 = left1 >= 64 ? ~0ULL : left1 <= 0 ? 0ULL : (1ULL << left1) - 1ULL;
            unsigned long long m0, m1;
            uint32_t x0, x1;
            word_max<PLANES>(same0, other0, v0, &m0, &x0);
            word_max<PLANES>(same1, other1, v1, &m1, &x1);
            rmask[2 * q] = m0; rmask[2 * q + 1] = m1;
            rmaxw[2 * q] = (uint16_t)x0; rmaxw[2 * q + 1] = (uint16_t)x1;
            best = max(best, max(x0, x1));
        }
        for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o));
        // src/main.cpp:856-863, mgsr.cpp:1693: the threshold is truncated to an integer
        const int thr = (int)((double)(i1 - i0) * discard);
        const int state = best == 0 ? 0 : (int)best < thr ? 1 : 2;
        uint32_t count = 0, first = 0xffffffffu, last = 0;
        if (state == 2) {
            for (int q = lane; q < pairs; q += 64) {   // (each lane reads back what it wrote)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int w = 2 * q + h;
                    unsigned long long mk = rmask[w];
                    if ((uint32_t)rmaxw[w] < best) { mk = 0; rmask[w] = 0; }
                    if (mk) {
                        count += (uint32_t)__popcll(mk);
                        first = min(first, (uint32_t)(w * 64 + __ffsll((long long)mk) - 1));
                        last = max(last, (uint32_t)(w * 64 + 63 - __clzll((long long)mk)));
                    }
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                count += (uint32_t)__shfl_xor((int)count, o);
                first = min(first, (uint32_t)__shfl_xor((int)first, o));
                last = max(last, (uint32_t)__shfl_xor((int)last, o));
            }
        }
        if (lane == 0) { out_max[r] = (uint16_t)best; out_count[r] = count; out_first[r] = first; out_last[r] = last; out_state[r] = (uint8_t)state; }
    }
}

// A wave per read: the set bits of its word masks as DFS indices, ascending, at off[r] of `nodes` (off: the exclusive scan of
// the counts).  64 words a step, a lane per word; the lanes' positions are the running sum of their popcounts.
__global__ void __launch_bounds__(256) k_meta_assign_emit(const uint32_t* __restrict__ count, const int64_t* __restrict__ off, int64_t n_reads,
                                                         const unsigned long long* __restrict__ wmask, int words, uint32_t* __restrict__ nodes) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        if (count[r] == 0) continue;
        int64_t at = off[r];
        for (int base = 0; base < words; base += 64) {
            const int w = base + lane;
            unsigned long long mk = w < words ? wmask[(size_t)r * (size_t)words + (size_t)w] : 0ULL;
            const int c = __popcll(mk);
            int incl = c;
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            int64_t p = at + (incl - c);
            while (mk) {
                nodes[p++] = (uint32_t)(w * 64 + __ffsll((long long)mk) - 1);
                mk &= mk - 1;
            }
            at += __shfl(incl, 63);
        }
    }
}

// One call of pmx_meta_assign: the plan of the chunks, then one function per chunk step.
struct AssignStage {
    pmx_ctx* const ctx;
    pmx_meta* const m;
    const hipStream_t st;
    const double discard;
    const int64_t n_reads;
    const int words;   // 64-bit words of a row: one bit per node, padded to an even count
    std::vector<int64_t> chunk_first;                  // first merged read of every chunk, then n_reads
    // per merged read, on the device
    DevBuf<uint16_t> d_max;
    DevBuf<uint32_t> d_count, d_first, d_last;
    DevBuf<uint8_t> d_state;
    // per chunk
    DevBuf<uint64_t> d_uniq;
    DevBuf<uint32_t> d_uid, d_nodes;
    DevBuf<unsigned long long> d_fwd, d_rev, d_wmask;
    DevBuf<uint16_t> d_wmax;
    DevBuf<int64_t> d_off;
    DevBuf<char> tmp;
    std::vector<int64_t> h_off;

    AssignStage(pmx_ctx* c, pmx_meta* mm, double d)
        : ctx(c), m(mm), st(c->stream), discard(d), n_reads(mm->n_reads), words((int)(((mm->n_nodes + 63) / 64 + 1) & ~(int64_t)1)) {}
    void plan_chunks();
    void run_chunk(int64_t r0, int64_t r1);
    void finish();
};

// Chunks of consecutive merged reads whose distinct seedmers fit kAssignMatrixBytes and whose word masks fit
// kAssignReadRowBytes (a read that alone exceeds them is a chunk of its own); PMX_META_ASSIGN_CHUNK forces a size in reads.
void AssignStage::plan_chunks() {
    const int64_t cap_rows = std::max<int64_t>(1, (int64_t)(kAssignMatrixBytes / (16 * (size_t)words)));
    int64_t cap_reads = std::max<int64_t>(1, (int64_t)(kAssignReadRowBytes / (10 * (size_t)words)));
    if (const char* f = opt_str(O_META_ASSIGN_CHUNK)) cap_reads = std::max<int64_t>(1, atoll(f));
    std::vector<int64_t> seen(m->h_uniq.size(), -1);   // the chunk (by its first read) that last counted the seedmer
    chunk_first.assign(1, 0);
    int64_t r0 = 0, rows = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        int64_t fresh = 0;
        for (int64_t i = m->h_read_off[(size_t)r]; i < m->h_read_off[(size_t)r + 1]; ++i) fresh += seen[m->h_seed_uid[(size_t)i]] != r0;
        if (r > r0 && (r - r0 >= cap_reads || rows + fresh > cap_rows)) {
            chunk_first.push_back(r);
            r0 = r;
            rows = 0;
        }
        for (int64_t i = m->h_read_off[(size_t)r]; i < m->h_read_off[(size_t)r + 1]; ++i) {
            int64_t& s = seen[m->h_seed_uid[(size_t)i]];
            if (s != r0) { s = r0; ++rows; }
        }
    }
    chunk_first.push_back(n_reads);
}

// Merged reads [r0, r1): their distinct seedmers' rows, the reads' maxima and assigned nodes.
// Leaves: d_max .. d_state of the reads, m->as_off (r0, r1] and m->as_nodes grown by the chunk's lists.
void AssignStage::run_chunk(int64_t r0, int64_t r1) {
    const int64_t n = r1 - r0, s0 = m->h_read_off[(size_t)r0], s1 = m->h_read_off[(size_t)r1];
    // the chunk's distinct seedmers (ascending, as h_uniq is) and every seedmer as its row
    std::vector<uint32_t> ids(m->h_seed_uid.begin() + s0, m->h_seed_uid.begin() + s1);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int64_t n_rows = (int64_t)ids.size();
    std::vector<uint64_t> uniq((size_t)n_rows);
    for (int64_t i = 0; i < n_rows; ++i) uniq[(size_t)i] = m->h_uniq[ids[(size_t)i]];
    std::vector<uint32_t> uid((size_t)(s1 - s0));
    for (int64_t i = s0; i < s1; ++i) uid[(size_t)(i - s0)] = (uint32_t)(std::lower_bound(ids.begin(), ids.end(), m->h_seed_uid[(size_t)i]) - ids.begin());
    const size_t mat = (size_t)n_rows * (size_t)words;
    d_uniq.ensure((size_t)n_rows); d_uid.ensure(uid.size()); d_fwd.ensure(mat); d_rev.ensure(mat);
    d_wmask.ensure((size_t)n * (size_t)words); d_wmax.ensure((size_t)n * (size_t)words); d_off.ensure((size_t)n + 1);
    PMX_HIP(hipMemcpyAsync(d_uniq.p, uniq.data(), sizeof(uint64_t) * (size_t)n_rows, hipMemcpyHostToDevice, st));
    PMX_HIP(hipMemcpyAsync(d_uid.p, uid.data(), sizeof(uint32_t) * uid.size(), hipMemcpyHostToDevice, st));
    timer_begin(ctx, "meta_assign");
    PMX_HIP(hipMemsetAsync(d_fwd.p, 0, sizeof(unsigned long long) * mat, st));
    PMX_HIP(hipMemsetAsync(d_rev.p, 0, sizeof(unsigned long long) * mat, st));
    if (m->n_changes > 0)
        hipLaunchKernelGGL(k_assign_mark_ends, dim3(grid_for(m->n_changes, 256, ctx->n_cu * 8)), dim3(256), 0, st, m->ch_key.p, m->ch_pc.p, m->ch_cc.p,
                           m->ch_node.p, m->n_changes, m->subtree_end.p, m->n_nodes, d_uniq.p, n_rows, words, d_fwd.p, d_rev.p);
    hipLaunchKernelGGL(k_assign_prefix_xor, dim3(grid_for(2 * n_rows * 64, 256, ctx->n_cu * 16)), dim3(256), 0, st, d_fwd.p, d_rev.p, n_rows, words);
    const dim3 grid(grid_for(n * 64, 256, ctx->n_cu * 16)), block(256);
    if (m->longest < 128)
        hipLaunchKernelGGL(k_meta_assign_max<7>, grid, block, 0, st, m->d_read_off.p + r0, s0, d_uid.p, m->d_seed_rev.p, n, d_fwd.p, d_rev.p, words, m->n_nodes,
                           discard, d_wmask.p, d_wmax.p, d_max.p + r0, d_count.p + r0, d_first.p + r0, d_last.p + r0, d_state.p + r0);
    else
        hipLaunchKernelGGL(k_meta_assign_max<16>, grid, block, 0, st, m->d_read_off.p + r0, s0, d_uid.p, m->d_seed_rev.p, n, d_fwd.p, d_rev.p, words, m->n_nodes,
                           discard, d_wmask.p, d_wmax.p, d_max.p + r0, d_count.p + r0, d_first.p + r0, d_last.p + r0, d_state.p + r0);
    PMX_HIP(hipGetLastError());
    // (d_count has one entry past the last read, zero: the scan's entry n is the chunk's total; the entry it reads past the
    //  chunk's own counts plays no part in any output)
    PMX_ROCPRIM(tmp, exclusive_scan, d_count.p + r0, d_off.p, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st);
    timer_end(ctx, "meta_assign", 1);
    h_off.resize((size_t)n + 1);
    PMX_HIP(hipMemcpyAsync(h_off.data(), d_off.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, st));
    PMX_HIP(hipStreamSynchronize(st));   // (uniq / uid go out of scope; the total sizes the list)
    timer_sum_add(ctx, "meta_assign");
    const int64_t total = h_off[(size_t)n], base = (int64_t)m->as_nodes.size();
    for (int64_t i = 1; i <= n; ++i) m->as_off[(size_t)(r0 + i)] = base + h_off[(size_t)i];
    if (total == 0) return;
    d_nodes.ensure((size_t)total);
    timer_begin(ctx, "meta_assign_emit");
    hipLaunchKernelGGL(k_meta_assign_emit, grid, block, 0, st, d_count.p + r0, d_off.p, n, d_wmask.p, words, d_nodes.p);
    PMX_HIP(hipGetLastError());
    timer_end(ctx, "meta_assign_emit", 1);
    m->as_nodes.resize((size_t)(base + total));
    PMX_HIP(hipMemcpyAsync(m->as_nodes.data() + base, d_nodes.p, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipStreamSynchronize(st));
    timer_sum_add(ctx, "meta_assign_emit");
}

// The per-read results to the host; the LCA of every assigned read from its first and last node: in pre-order the LCA of a
// set is the lowest ancestor a of its first node with subtree_end[a] >= its last node.
void AssignStage::finish() {
    std::vector<uint32_t> first((size_t)n_reads), last((size_t)n_reads);
    PMX_HIP(hipMemcpyAsync(m->as_max.data(), d_max.p, sizeof(uint16_t) * (size_t)n_reads, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipMemcpyAsync(m->as_count.data(), d_count.p, sizeof(uint32_t) * (size_t)n_reads, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipMemcpyAsync(m->as_state.data(), d_state.p, (size_t)n_reads, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipMemcpyAsync(first.data(), d_first.p, sizeof(uint32_t) * (size_t)n_reads, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipMemcpyAsync(last.data(), d_last.p, sizeof(uint32_t) * (size_t)n_reads, hipMemcpyDeviceToHost, st));
    PMX_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < n_reads; ++r) {
        if (m->as_state[(size_t)r] != PMX_META_ASSIGNED) continue;
        uint32_t a = first[(size_t)r];
        while (m->h_subtree_end[a] < last[(size_t)r]) a = m->h_parent[a];
        m->as_lca[(size_t)r] = a;
    }
}
}  // namespace

extern "C" {

int pmx_meta_assign(pmx_ctx* ctx, pmx_meta* m, double discard) {
    if (!ctx || !m || !(discard >= 0.0 && discard <= 1.0)) return PMX_ERR_ARG;   // src/main.cpp:1358-1361
    if (m->dist) return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign runs on one GPU: not with an attached dist");
    if (!m->reads_set) return fail(PMX_ERR_ARG, "pmx_meta_assign: call pmx_meta_set_reads first");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    m->assigned = false;
    const int64_t n = m->n_reads;
    int64_t longest = 0;
    for (int64_t r = 0; r < n; ++r) longest = std::max(longest, m->h_read_off[(size_t)r + 1] - m->h_read_off[(size_t)r]);
    if (longest >= 65535) return fail(PMX_ERR_UNSUPPORTED, "a read with 65,535 seedmers or more (16-bit scores)");
    m->longest = longest;
    m->as_state.assign((size_t)n, PMX_META_UNMAPPED);
    m->as_max.assign((size_t)n, 0);
    m->as_count.assign((size_t)n, 0);
    m->as_lca.assign((size_t)n, UINT32_MAX);
    m->as_off.assign((size_t)n + 1, 0);
    m->as_nodes.clear();
    if (n > 0) {
        AssignStage S(ctx, m, discard);
        S.plan_chunks();
        S.d_max.alloc((size_t)n); S.d_count.alloc((size_t)n + 1); S.d_first.alloc((size_t)n); S.d_last.alloc((size_t)n); S.d_state.alloc((size_t)n);
        timer_sum_reset(ctx, "meta_assign");
        timer_sum_reset(ctx, "meta_assign_emit");
        PMX_HIP(hipMemsetAsync(S.d_count.p, 0, sizeof(uint32_t) * ((size_t)n + 1), ctx->stream));
        for (size_t c = 0; c + 1 < S.chunk_first.size(); ++c) S.run_chunk(S.chunk_first[c], S.chunk_first[c + 1]);
        S.finish();
    }
    m->assigned = true;
    return PMX_OK;
    PMX_CATCH
}

int pmx_meta_assign_reads(const pmx_meta* m, uint8_t* state, uint16_t* max_score, uint32_t* lca, uint32_t* n_nodes, int64_t cap) {
    if (!m || !m->assigned || cap < m->n_reads) return PMX_ERR_ARG;
    if (state) std::copy(m->as_state.begin(), m->as_state.end(), state);
    if (max_score) std::copy(m->as_max.begin(), m->as_max.end(), max_score);
    if (lca) std::copy(m->as_lca.begin(), m->as_lca.end(), lca);
    if (n_nodes) std::copy(m->as_count.begin(), m->as_count.end(), n_nodes);
    return PMX_OK;
}

int64_t pmx_meta_assign_num_nodes(const pmx_meta* m) { return m && m->assigned ? (int64_t)m->as_nodes.size() : 0; }

int pmx_meta_assign_nodes(const pmx_meta* m, int64_t* offsets, uint32_t* nodes, int64_t cap_nodes) {
    if (!m || !m->assigned || !offsets || cap_nodes < (int64_t)m->as_nodes.size()) return PMX_ERR_ARG;
    std::copy(m->as_off.begin(), m->as_off.end(), offsets);
    if (nodes) std::copy(m->as_nodes.begin(), m->as_nodes.end(), nodes);
    return PMX_OK;
}

int64_t pmx_meta_num_raw_reads(const pmx_meta* m) { return m ? m->n_raw_reads : 0; }

int pmx_meta_raw_to_merged(const pmx_meta* m, int64_t* map, int64_t cap) {
    if (!m || !map || !m->reads_set) return PMX_ERR_ARG;
    if (m->dist) return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_raw_to_merged: the merged reads of an attached dist are the whole sample's");
    if (cap < (int64_t)m->h_raw_to_merged.size()) return PMX_ERR_ARG;
    std::copy(m->h_raw_to_merged.begin(), m->h_raw_to_merged.end(), map);
    return PMX_OK;
}

}  // extern "C"
