// C ABI, device part 4b: --meta --filter-and-assign (filterAndAssignBatch, src/main.cpp:720-1016; scoreReadsBatch /
// assignReadsBatch, src/mgsr.cpp:7477-7575, 6415-6516).
//
// What the reference does: every read (mates are independent reads) is scored against EVERY node of the tree by one DFS that
// applies and reverts per-node seed deltas (scoreReadsBatchHelper, :7477-7570), score(read, node) = max(f, r) as in the
// abundance mode (api_meta.hip).  A read's maximum over the nodes decides its fate (src/main.cpp:856-863 with the threshold of
// mgsr.cpp:1693, static_cast<int32_t>(discard * n), n = the read's seedmers, :1640, 1667): max == 0 -> unmapped, max below
// the threshold -> discarded, else assigned; the assigned nodes of a read are the nodes whose score equals its maximum, and
// its LCA node is their lowest common ancestor (assignReadsBatchHelper, :6415-6461).
// --breadth-ratio (calculateBreadthRatio, :6518-6584): see "Breadth" below.
//
// keepForFilterAndAssign changes nothing about that set.  scoreReadsBatchHelper records a read's score at a node only once the
// flag is set, and sets it at the first node (in DFS order) where the score reaches the threshold (:7508-7513, :7549-7551);
// from there on every change of the score is recorded.  assignReadsBatchHelper keeps a read in the running set from a recorded
// score equal to its maximum to the next recorded score that is not, within the subtree (:6432-6443, backtracked :6454-6460).
// For an assigned read max >= threshold, so the node where the score first equals max is recorded (the flag is set there at
// the latest); every later node in DFS order is recorded too, the whole subtree of that node included.  The unrecorded changes
// lie before the flag was set, at scores below the threshold <= max, where the read is not in the running set anyway.  So the
// read is reported exactly at the nodes with score == max, and the LCA accumulated at :6437 is the LCA of that set.
//
// Taxonomy (--taxonomic-metadata, --maximum-taxon-number M, --ambiguous-score-threshold A, -ratio; fillTaxonIndices :156-196,
// checkTaxonIndicesBatch :6463-6496).  Every node has S(v), the taxa of its subtree, "over" when |S(v)| > M.  A read with max != 0
// after the discard step has amb = max(A, (int)(max * ratio)), lo = max(0, max - amb); at every node where it has a RECORD (one of
// its seedmers changes presence there, 0 <-> positive, in either orientation; :7488-7552) and scores >= lo, S(v) joins the
// read's set; the read is over, and dropped from both assignments, when it meets an over node or its set exceeds M.
// In closed form (DESIGN.md section 4.3 has the argument): for lo >= 1 the records need not be told apart, the union over ALL
// nodes with score >= lo is the same set, because an unrecorded qualifying node has a recorded ancestor with its score, whose
// S contains its own; with amb == 0 those nodes are the best columns that k_meta_assign_max leaves in its word masks.  Only lo
// == 0 needs the recorded nodes themselves: the touch matrix of k_assign_mark_ends.  A discard threshold with amb > 0 is refused:
// the reference then starts recording in the middle of a node's updates, in an order this index does not keep.
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
//   * with a taxonomy, k_meta_assign_near<PLANES> (only with an ambiguity option) and k_meta_assign_taxa: see there;
//   * k_meta_assign_emit: after an exclusive scan of the node counts, a wave per read expands its set bits into the CSR list
//     read -> DFS indices, ascending.
//   * for the read-score reports of the abundance mode (pmx_meta_read_best), instead of all that follows the prefix XOR:
//     k_meta_active_nodes once per read set and k_meta_read_best<PLANES>, which keeps a read's maximum and the number of
//     active columns that reach it and stores nothing per word: see there.
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
#include <string>
#include <unordered_map>
#include <vector>

#include "api_internal.hpp"
#include "device/dev_util.hpp"
#include "host/index_build.hpp"
#include "meta_state.hpp"

using namespace pmx;

namespace {
// the (distinct seedmer x node) bit matrices of a chunk together (two; three with the touch matrix); 2 GiB holds the SARS 20k
// tree (626 words a row) with 100,000 distinct seedmers: 2 x 100,000 x 626 x 8 B = 1.0 GB
constexpr size_t kAssignMatrixBytes = (size_t)2 << 30;
// the per-read word masks and word maxima of a chunk (10 B per read and word; 18 B with k_meta_assign_near's rows)
constexpr size_t kAssignReadRowBytes = (size_t)1 << 30;
// the most taxa a read or a node may span (--maximum-taxon-number): k_meta_assign_taxa keeps a read's set in registers
constexpr int kAssignMaxTaxa = 16;

// Every count change of the oriented index whose seedmer becomes present (parent count 0) or absent (child count 0) and whose
// hash the chunk's reads carry: the two end bits of its column range [v, subtree_end[v]] in the seedmer's row.  With `touch`
// (one matrix for both orientations, or null) also bit v itself: the seedmer changes presence AT v.  The end bits cannot
// serve for that: the closing bit of one transition cancels the opening bit of the next.
__global__ void k_assign_mark_ends(const uint64_t* __restrict__ ch_key, const int16_t* __restrict__ ch_pc, const int16_t* __restrict__ ch_cc,
                                   const uint32_t* __restrict__ ch_node, int64_t n_changes, const uint32_t* __restrict__ subtree_end, int64_t n_nodes,
                                   const uint64_t* __restrict__ uniq, int64_t n_uniq, int words, unsigned long long* mask_fwd, unsigned long long* mask_rev,
                                   unsigned long long* touch) {
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
        if (touch) atomicOr(&touch[(size_t)uid * (size_t)words + (v >> 6)], 1ULL << (v & 63));   // (either orientation; never cancels)
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

// the same / other planes of one read (seedmers [i0, i1)) over the pair of words q of its seedmers' rows
template <int PLANES>
__device__ __forceinline__ void read_planes(const unsigned long long* __restrict__ mask_fwd, const unsigned long long* __restrict__ mask_rev,
                                            const uint32_t* __restrict__ seed_uid, const uint8_t* __restrict__ seed_rev, int64_t i0, int64_t i1,
                                            int64_t seed_base, int words, int q, unsigned long long (&same0)[PLANES], unsigned long long (&other0)[PLANES],
                                            unsigned long long (&same1)[PLANES], unsigned long long (&other1)[PLANES]) {
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
}

// the columns < N of the word at column c0
__device__ __forceinline__ unsigned long long valid_columns(int64_t n_nodes, int64_t c0) {
    const int64_t left = n_nodes - c0;
    return left >= 64 ? ~0ULL : left <= 0 ? 0ULL : (1ULL << left) - 1ULL;
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
            read_planes<PLANES>(mask_fwd, mask_rev, seed_uid, seed_rev, i0, i1, seed_base, words, q, same0, other0, same1, other1);
            const unsigned long long v0 = valid_columns(n_nodes, (int64_t)q * 128), v1 = valid_columns(n_nodes, (int64_t)q * 128 + 64);
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

// ---- The read-score reports of the abundance mode (--write-meta-read-scores-*; scoreReads, src/mgsr.cpp:7325-7420: maxScore and
// epp of every read over the whole collapsed tree; collapseIdenticalScoringNodes, :794-847).
// The active nodes of a read set as one row of `words` words: the root, and every node with a change whose hash, in either
// orientation, is among the distinct seedmers of the whole sample (uniq, ascending).  A thread per change of the oriented
// index; `active` comes in zeroed.  An inactive node holds none of the reads' seedmers differently from its parent, scores
// as its nearest active ancestor for every read, and is what the reference folds away before it counts.
__global__ void k_meta_active_nodes(const uint64_t* __restrict__ ch_key, const uint32_t* __restrict__ ch_node, int64_t n_changes,
                                    const uint64_t* __restrict__ uniq, int64_t n_uniq, unsigned long long* active) {
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) atomicOr(&active[0], 1ULL);   // the root
    for (int64_t c = t0; c < n_changes; c += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = ch_key[c];
        if (find_sorted(uniq, n_uniq, key) < 0 && find_sorted(uniq, n_uniq, key ^ PMX_ORIENT_XOR) < 0) continue;
        const uint32_t v = ch_node[c];
        atomicOr(&active[v >> 6], 1ULL << (v & 63));
    }
}

// a word's maximum x and its active best columns taken into a lane's running (best, cnt)
__device__ __forceinline__ void best_take(uint32_t x, unsigned long long cols, uint32_t& best, uint32_t& cnt) {
    const uint32_t c = (uint32_t)__popcll(cols);
    if (x > best) { best = x; cnt = c; }
    else if (x == best) cnt += c;
}

// A wave per merged read of the chunk, a lane per pair of words, the loads and the word maxima of k_meta_assign_max; nothing
// is stored per word.  out_max: the read's maximum over all columns < N; out_nbest: the ACTIVE columns that reach it (0 when
// the maximum is 0).  active: one row of `words` words.
template <int PLANES>
__global__ void __launch_bounds__(256) k_meta_read_best(const int64_t* __restrict__ read_off, int64_t seed_base, const uint32_t* __restrict__ seed_uid,
                                                       const uint8_t* __restrict__ seed_rev, int64_t n_reads, const unsigned long long* __restrict__ mask_fwd,
                                                       const unsigned long long* __restrict__ mask_rev, int words, int64_t n_nodes,
                                                       const unsigned long long* __restrict__ active, uint16_t* out_max, uint32_t* out_nbest) {
    const int lane = threadIdx.x & 63;
    const int pairs = words >> 1;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        const int64_t i0 = read_off[r], i1 = read_off[r + 1];
        uint32_t best = 0, cnt = 0;
        for (int q = lane; q < pairs; q += 64) {
            unsigned long long same0[PLANES], other0[PLANES], same1[PLANES], other1[PLANES];
            read_planes<PLANES>(mask_fwd, mask_rev, seed_uid, seed_rev, i0, i1, seed_base, words, q, same0, other0, same1, other1);
            const unsigned long long v0 = valid_columns(n_nodes, (int64_t)q * 128), v1 = valid_columns(n_nodes, (int64_t)q * 128 + 64);
            const ulonglong2 act = *reinterpret_cast<const ulonglong2*>(active + 2 * q);
            unsigned long long m0, m1;
            uint32_t x0, x1;
            word_max<PLANES>(same0, other0, v0, &m0, &x0);
            word_max<PLANES>(same1, other1, v1, &m1, &x1);
            best_take(x0, m0 & act.x, best, cnt);
            best_take(x1, m1 & act.y, best, cnt);
        }
        uint32_t top = best;
        for (int o = 32; o > 0; o >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, o));
        if (best != top || top == 0) cnt = 0;
        for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
        if (lane == 0) { out_max[r] = (uint16_t)top; out_nbest[r] = cnt; }
    }
}

// the columns of one word where max(same, other) >= lo (1 <= lo < 2^PLANES), bit-sliced against the scalar lo
template <int PLANES>
__device__ __forceinline__ unsigned long long word_ge(const unsigned long long (&same)[PLANES], const unsigned long long (&other)[PLANES], uint32_t lo) {
    unsigned long long gt = 0, eq = ~0ULL;   // same > other, as in word_max
#pragma unroll
    for (int p = PLANES - 1; p >= 0; --p) {
        gt |= eq & same[p] & ~other[p];
        eq &= ~(same[p] ^ other[p]);
    }
    unsigned long long above = 0, tie = ~0ULL;   // score > lo / score == lo on the planes seen so far
#pragma unroll
    for (int p = PLANES - 1; p >= 0; --p) {
        const unsigned long long plane = (gt & same[p]) | (~gt & other[p]);
        if ((lo >> p) & 1u) tie &= plane;
        else { above |= tie & plane; tie &= ~plane; }
    }
    return above | tie;
}

// Taxonomy with a non-zero ambiguity option (checkTaxonIndicesBatch, src/mgsr.cpp:6463-6496): a wave per ASSIGNED read of the
// chunk, a lane per pair of words, the loads of k_meta_assign_max.  amb = max(amb_abs, (int)(max * amb_ratio)), lo = max(0, max -
// amb).  lo >= 1: the read's row of `near` gets the columns < N with score >= lo (the records of the
// reference need not be told apart there).  lo == 0: the nodes where one of the read's seedmers changes presence, the OR of its
// seedmers' rows of `touch` (the host allocates `touch` whenever some maximum can give lo == 0).
template <int PLANES>
__global__ void __launch_bounds__(256) k_meta_assign_near(const int64_t* __restrict__ read_off, int64_t seed_base, const uint32_t* __restrict__ seed_uid,
                                                         const uint8_t* __restrict__ seed_rev, int64_t n_reads, const unsigned long long* __restrict__ mask_fwd,
                                                         const unsigned long long* __restrict__ mask_rev, const unsigned long long* __restrict__ touch, int words,
                                                         int64_t n_nodes, int amb_abs, double amb_ratio, const uint16_t* __restrict__ in_max,
                                                         const uint8_t* __restrict__ in_state, unsigned long long* near) {
    const int lane = threadIdx.x & 63;
    const int pairs = words >> 1;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        if (in_state[r] != PMX_META_ASSIGNED) continue;
        const int64_t i0 = read_off[r], i1 = read_off[r + 1];
        const int mx = (int)in_max[r];
        const int lo = max(0, mx - max(amb_abs, (int)((double)mx * amb_ratio)));
        unsigned long long* rnear = near + (size_t)r * (size_t)words;
        if (lo == 0) {
            for (int w = lane; w < words; w += 64) {
                unsigned long long acc = 0;
                for (int64_t i = i0; i < i1; ++i) acc |= touch[(size_t)seed_uid[i - seed_base] * (size_t)words + (size_t)w];
                rnear[w] = acc;
            }
            continue;
        }
        for (int q = lane; q < pairs; q += 64) {
            unsigned long long same0[PLANES], other0[PLANES], same1[PLANES], other1[PLANES];
            read_planes<PLANES>(mask_fwd, mask_rev, seed_uid, seed_rev, i0, i1, seed_base, words, q, same0, other0, same1, other1);
            rnear[2 * q] = word_ge<PLANES>(same0, other0, (uint32_t)lo) & valid_columns(n_nodes, (int64_t)q * 128);
            rnear[2 * q + 1] = word_ge<PLANES>(same1, other1, (uint32_t)lo) & valid_columns(n_nodes, (int64_t)q * 128 + 64);
        }
    }
}

// The taxa of every ASSIGNED read of the chunk: U = the union of S(v) over its qualifying nodes (rows of `qual`: the best
// columns, or k_meta_assign_near's), S(v) from the node table of pmx_meta_set_taxonomy: tx_over = the nodes with |S(v)| >
// max_taxa as a row of `words` words, tx_count[v] <= max_taxa ids at tx_ids[v * max_taxa].  A wave per read, a lane per word, 64
// words a step.  A qualifying node in tx_over ends the read at once (one ballot a step).  Otherwise every lane walks its set
// bits and offers the next taxon of its node that the set does not hold; the lowest offering lane's id goes into the set
// (`set`, `nset`: the same in every lane), which drops that id from every lane's offers.  |U| > max_taxa: the read's state
// becomes PMX_META_OVER_TAXA and its node count 0, so that the scan and k_meta_assign_emit pass it by.  Else its taxa, ascending,
// at rd_tax[r * max_taxa].  max_taxa <= kAssignMaxTaxa.
__global__ void __launch_bounds__(256) k_meta_assign_taxa(const unsigned long long* __restrict__ qual, int words, int64_t n_reads,
                                                         const unsigned long long* __restrict__ tx_over, const uint8_t* __restrict__ tx_count,
                                                         const uint32_t* __restrict__ tx_ids, int max_taxa, uint8_t* state, uint32_t* count, uint8_t* rd_ntax,
                                                         uint32_t* rd_tax) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n_reads; r += n_waves) {
        if (state[r] != PMX_META_ASSIGNED) {
            if (lane == 0) rd_ntax[r] = 0;
            continue;
        }
        uint32_t set[kAssignMaxTaxa];
#pragma unroll
        for (int k = 0; k < kAssignMaxTaxa; ++k) set[k] = 0;
        int nset = 0;
        bool over = false;
        for (int base = 0; base < words && !over; base += 64) {
            const int w = base + lane;
            unsigned long long q = w < words ? qual[(size_t)r * (size_t)words + (size_t)w] : 0ULL;
            if (__ballot(w < words && (q & tx_over[w]) != 0)) { over = true; break; }
            int j = 0;   // the next taxon of the node of q's lowest bit
            for (;;) {
                bool have = false;
                uint32_t cand = 0;
                while (q) {
                    const size_t v = (size_t)w * 64 + (size_t)(__ffsll((long long)q) - 1);
                    if (j >= (int)tx_count[v]) { q &= q - 1; j = 0; continue; }
                    cand = tx_ids[v * (size_t)max_taxa + (size_t)j];
                    bool held = false;
#pragma unroll
                    for (int k = 0; k < kAssignMaxTaxa; ++k) held |= k < nset && set[k] == cand;
                    if (!held) { have = true; break; }
                    ++j;
                }
                const unsigned long long offers = __ballot(have);
                if (!offers) break;
                if (nset == max_taxa) { over = true; break; }
                const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)cand, __ffsll((long long)offers) - 1));
#pragma unroll
                for (int k = 0; k < kAssignMaxTaxa; ++k)
                    if (k == nset) set[k] = id;
                ++nset;
            }
        }
        if (over) {
            if (lane == 0) { state[r] = PMX_META_OVER_TAXA; count[r] = 0; rd_ntax[r] = 0; }
            continue;
        }
        // ascending: lane k < nset holds set[k] and writes it at its rank
        uint32_t mine = 0;
        int rank = 0;
#pragma unroll
        for (int k = 0; k < kAssignMaxTaxa; ++k)
            if (k == lane) mine = set[k];
#pragma unroll
        for (int k = 0; k < kAssignMaxTaxa; ++k) rank += k < nset && set[k] < mine;
        if (lane < nset) rd_tax[(size_t)r * (size_t)max_taxa + (size_t)rank] = mine;
        if (lane == 0) rd_ntax[r] = (uint8_t)nset;
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

// ---- Breadth (--breadth-ratio; calculateBreadthRatio, src/mgsr.cpp:6518-6584; src/main.cpp:957-1015).
// The reference reads the assigned FASTQ back, scores and assigns those reads again (the same assignment: a read's fate depends
// on its own list only) and walks the collapsed tree: at node v, for every merged read r assigned to v and every DISTINCT hash
// s of r that v's genome holds in either orientation, seedHitCounts[s] += dup(r), totalDepth += dup(r).  In closed form, with
// P[s][v] = fwd row | rev row of seedmer s and mask[r][v] = the best columns of an ASSIGNED read:
//   observed(v) = |{ s : some r carries s, mask[r][v] and P[s][v] }|,   depth(v) = sum_r mult(r) |{ s in distinct(r) : P[s][v] }| mask[r][v].
// Both come from bit matrices the chunk already holds:
//   * k_meta_breadth_rows, once per chunk after the states are final: a wave per (block of rows, span of 64 words), a lane
//     per word.  For a row, p = fwd | rev once; for each of the row's carriers (the chunk's inverted list row -> reads, a read
//     once per row however often it repeats the hash) that is ASSIGNED, its mask word mk: a |= mk, and mk & p is added with
//     weight mult(r) into bit-sliced per-column counters (planes_add from every set bit of the weight).  a & p is ORed into the
//     row of `hit`, the (distinct seedmer of the READ SET x node) matrix that lives across the chunks, so that a seedmer whose
//     carriers fall into different chunks is counted once.  One wave owns a (row, word) within a launch and launches are
//     stream-ordered: a plain read-modify-write.
//   * k_meta_breadth_count, once at the end: the same layout over `hit`, every row's word added into the counters.
// The counters hold kBreadthPlanes bits a column.  `sum`, the weight added since the last flush, bounds every column and is the
// same in all lanes; a weight is added in pieces of at most cap - sum and the counters are flushed when sum reaches cap
// (<= 2^kBreadthPlanes - 1; PMX_META_BREADTH_FLUSH lowers it for the tests), so no column can wrap whatever the multiplicities.
// A flush transposes: for every word j of the span the 64 lanes take the 64 columns of that word (lane c assembles bit c of
// lane j's planes, read across the wave) and add them to out[] with ONE wave instruction over 64 consecutive 64-bit counters.
// Integer sums only: no result depends on the order or on the chunking.
constexpr size_t kBreadthHitBytes = (size_t)8 << 30;
constexpr int kBreadthPlanes = 20;
// k_meta_breadth_rows adds into kBreadthLowPlanes planes first and carries them into the full counters once their own weight
// sum would pass 2^kBreadthLowPlanes - 1: an add then costs 4 plane steps, not 20, and the carry 20 steps per 15 unit weights
constexpr int kBreadthLowPlanes = 4;

// `inc` added `weight` times (weight < 2^PLANES, the same in all lanes)
template <int PLANES>
__device__ __forceinline__ void planes_add_weighted(unsigned long long (&plane)[PLANES], unsigned long long inc, uint32_t weight) {
    if (weight == 1u) { planes_add<PLANES>(plane, inc); return; }
#pragma unroll
    for (int b = 0; b < PLANES; ++b) {
        if (((weight >> b) & 1u) == 0u) continue;
        unsigned long long carry = inc;
#pragma unroll
        for (int p = b; p < PLANES; ++p) {
            const unsigned long long t = plane[p] & carry;
            plane[p] ^= carry;
            carry = t;
        }
    }
}

// plane += low, a LOW-plane number per column; low is cleared
template <int LOW, int PLANES>
__device__ __forceinline__ void planes_spill(unsigned long long (&low)[LOW], unsigned long long (&plane)[PLANES]) {
    unsigned long long carry = 0;
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
        const unsigned long long x = p < LOW ? low[p] : 0ULL, h = plane[p];
        plane[p] = h ^ x ^ carry;
        carry = (h & x) | (carry & (h ^ x));
    }
#pragma unroll
    for (int p = 0; p < LOW; ++p) low[p] = 0;
}

// lane j's value in every lane (j the same in all lanes)
__device__ __forceinline__ unsigned long long lane_value(unsigned long long x, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}

// The counters of a wave (lane l: the 64 columns of word w0 + l) added to out[column], then cleared: for every word j of the
// span that has a count, lane c assembles the count of column c of that word from bit c of lane j's planes, and the wave adds
// 64 consecutive counters with one instruction.  All lanes of the wave call it together.
template <int PLANES>
__device__ __forceinline__ void planes_flush(unsigned long long (&plane)[PLANES], int lane, int w0, int words, unsigned long long* __restrict__ out) {
    unsigned long long any = 0;
#pragma unroll
    for (int p = 0; p < PLANES; ++p) any |= plane[p];
    unsigned long long todo = __ballot(any != 0 && w0 + lane < words);
    while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        unsigned long long c = 0;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) c |= ((lane_value(plane[p], j) >> lane) & 1ULL) << p;
        if (c) atomicAdd(&out[(size_t)(w0 + j) * 64 + (size_t)lane], c);
    }
#pragma unroll
    for (int p = 0; p < PLANES; ++p) plane[p] = 0;
}

// One chunk's part of hit[] and depth[] (see "Breadth").  Rows [0, n_rows) of the chunk's fwd / rev matrices; row_id: the row
// of `hit` (the seedmer's index among the read set's distinct seedmers); car_off / car: the chunk's reads (indices into mult /
// wmask, which point at the chunk's first read, read0; state_words: the states of ALL reads of the call, four to a word, padded to whole
// words) that carry the row's seedmer.  The carriers are taken four at a time,
// their states, multiplicities and mask words loaded before any is used (a read that is not ASSIGNED is loaded too and masked
// out): one load after the other left the kernel waiting on latency.
__global__ void __launch_bounds__(256) k_meta_breadth_rows(const unsigned long long* __restrict__ mask_fwd, const unsigned long long* __restrict__ mask_rev,
                                                           int64_t n_rows, int words, const uint32_t* __restrict__ row_id, const int64_t* __restrict__ car_off,
                                                           const uint32_t* __restrict__ car, const uint32_t* __restrict__ state_words, int64_t read0,
                                                           const int64_t* __restrict__ mult,
                                                           const unsigned long long* __restrict__ wmask, int rows_per_block, uint32_t cap,
                                                           unsigned long long* hit, unsigned long long* depth) {
    const int lane = threadIdx.x & 63;
    // (said to the compiler: the wave's index is the same in all lanes, so rows, carriers and their loads are scalar)
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int spans = (words + 63) >> 6;
    const int64_t n_items = ((n_rows + rows_per_block - 1) / rows_per_block) * spans;
    for (int64_t item = wave; item < n_items; item += n_waves) {
        const int64_t row0 = (item / spans) * rows_per_block, row1 = min(n_rows, row0 + rows_per_block);
        const int w0 = (int)(item % spans) * 64, w = min(w0 + lane, words - 1);   // (a lane past the row reads its last word, and drops it)
        const bool live = w0 + lane < words;
        constexpr uint32_t low_cap = (1u << kBreadthLowPlanes) - 1u;
        unsigned long long plane[kBreadthPlanes], low[kBreadthLowPlanes];
#pragma unroll
        for (int p = 0; p < kBreadthPlanes; ++p) plane[p] = 0;
#pragma unroll
        for (int p = 0; p < kBreadthLowPlanes; ++p) low[p] = 0;
        uint32_t sum = 0, low_sum = 0;   // the weight in plane + low / in low since the last flush / spill
        for (int64_t row = row0; row < row1; ++row) {
            const size_t at = (size_t)row * (size_t)words + (size_t)w;
            const unsigned long long p = live ? (mask_fwd[at] | mask_rev[at]) : 0ULL;
            unsigned long long a = 0;
            const int64_t c1 = car_off[row + 1];
            for (int64_t c = car_off[row]; c < c1; c += 4) {
                uint32_t r[4];
                bool ok[4];
                uint64_t weight[4];
                unsigned long long mk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = car[min(c + u, c1 - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t at_state = read0 + r[u];   // (a byte of its word: a scalar load, no wait on the vector loads in flight)
                    ok[u] = (c + u < c1) & (((state_words[at_state >> 2] >> ((at_state & 3) * 8)) & 0xffu) == (uint32_t)PMX_META_ASSIGNED);
                    weight[u] = (uint64_t)mult[r[u]];
                    mk[u] = wmask[(size_t)r[u] * (size_t)words + (size_t)w];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!ok[u]) continue;
                    a |= mk[u];
                    const unsigned long long inc = mk[u] & p;   // (p is 0 in a lane past the row)
                    if (__ballot(inc != 0) == 0) continue;
                    uint64_t rem = weight[u];
                    while (rem) {
                        if (sum == cap) {
                            planes_spill(low, plane);
                            planes_flush<kBreadthPlanes>(plane, lane, w0, words, depth);
                            sum = low_sum = 0;
                        }
                        const uint32_t piece = (uint32_t)min(rem, (uint64_t)(cap - sum));
                        if (piece > low_cap - low_sum) { planes_spill(low, plane); low_sum = 0; }
                        if (piece <= low_cap) { planes_add_weighted<kBreadthLowPlanes>(low, inc, piece); low_sum += piece; }
                        else planes_add_weighted<kBreadthPlanes>(plane, inc, piece);
                        sum += piece;
                        rem -= piece;
                    }
                }
            }
            const unsigned long long x = a & p;
            if (x) hit[(size_t)row_id[row] * (size_t)words + (size_t)w] |= x;
        }
        if (sum) {
            planes_spill(low, plane);
            planes_flush<kBreadthPlanes>(plane, lane, w0, words, depth);
        }
    }
}

// observed[column] += the set bits of hit's rows, once per call: the layout of k_meta_breadth_rows.
__global__ void __launch_bounds__(256) k_meta_breadth_count(const unsigned long long* __restrict__ hit, int64_t n_rows, int words, int rows_per_block,
                                                            uint32_t cap, unsigned long long* observed) {
    const int lane = threadIdx.x & 63;
    // (said to the compiler: the wave's index is the same in all lanes, so rows, carriers and their loads are scalar)
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int spans = (words + 63) >> 6;
    const int64_t n_items = ((n_rows + rows_per_block - 1) / rows_per_block) * spans;
    for (int64_t item = wave; item < n_items; item += n_waves) {
        const int64_t row0 = (item / spans) * rows_per_block, row1 = min(n_rows, row0 + rows_per_block);
        const int w0 = (int)(item % spans) * 64, w = w0 + lane;
        unsigned long long plane[kBreadthPlanes];
#pragma unroll
        for (int p = 0; p < kBreadthPlanes; ++p) plane[p] = 0;
        uint32_t sum = 0;
        for (int64_t row = row0; row < row1; ++row) {
            planes_add<kBreadthPlanes>(plane, w < words ? hit[(size_t)row * (size_t)words + (size_t)w] : 0ULL);
            if (++sum == cap) { planes_flush<kBreadthPlanes>(plane, lane, w0, words, observed); sum = 0; }
        }
        if (sum) planes_flush<kBreadthPlanes>(plane, lane, w0, words, observed);
    }
}

// --gpus N: the ranks' copies of one slab of `hit` (world x slab), the buffer of AssignStage::breadth_merge; it counts against
// nothing else: the chunks' matrices are released only with the stage, `hit` itself is under kBreadthHitBytes
constexpr size_t kBreadthSlabBytes = (size_t)1 << 30;

// dst[i] |= all[r * stride + i] for every rank r < world and word i < n: the ranks' copies of a slab of `hit` folded into the
// local rows.  Pure streaming: (world + 1) reads and one write of the slab.  Two words a lane and step (16-byte loads and stores)
// in a grid-stride loop while dst, all and the copies' stride are 16-byte aligned, the words left over (n odd, or no alignment)
// one at a time.  One thread owns a word: no atomics.
__global__ void __launch_bounds__(256) k_meta_breadth_or(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ all, int64_t n,
                                                         int64_t stride, int world) {
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_thr = (int64_t)gridDim.x * blockDim.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(all)) & 15) == 0 && (stride & 1) == 0;
    const int64_t n_vec = aligned ? n >> 1 : 0;
    for (int64_t i = t0; i < n_vec; i += n_thr) {
        ulonglong2 a = reinterpret_cast<const ulonglong2*>(dst)[i];
        for (int r = 0; r < world; ++r) {
            const ulonglong2 b = reinterpret_cast<const ulonglong2*>(all + (size_t)r * (size_t)stride)[i];
            a.x |= b.x;
            a.y |= b.y;
        }
        reinterpret_cast<ulonglong2*>(dst)[i] = a;
    }
    for (int64_t i = 2 * n_vec + t0; i < n; i += n_thr) {
        unsigned long long a = dst[i];
        for (int r = 0; r < world; ++r) a |= all[(size_t)r * (size_t)stride + (size_t)i];
        dst[i] = a;
    }
}

// One call of pmx_meta_assign: the plan of the chunks, then one function per chunk step.
int assign_words(int64_t n_nodes) { return (int)(((n_nodes + 63) / 64 + 1) & ~(int64_t)1); }

struct AssignStage {
    pmx_ctx* const ctx;
    pmx_meta* const m;
    const hipStream_t st;
    const double discard;
    const int64_t row0, n_reads;   // this rank's rows of the merged reads (all of them without a dist): the per-read buffers hold these
    const int words;   // 64-bit words of a row: one bit per node, padded to an even count
    // taxonomy (pmx_meta_set_taxonomy / pmx_meta_set_ambiguous): none, the best columns, or k_meta_assign_near's rows
    const int max_taxa;
    const bool near;    // an ambiguity option is non-zero
    bool touch = false; // ... and some maximum gives lo == 0: the touch matrix is needed
    std::vector<int64_t> chunk_first;                  // first merged read of every chunk, then n_reads
    // per merged read, on the device
    DevBuf<uint16_t> d_max;
    DevBuf<uint32_t> d_count, d_first, d_last;
    DevBuf<uint8_t> d_state, d_ntax;
    DevBuf<uint32_t> d_tax;
    // per chunk
    DevBuf<uint64_t> d_uniq;
    DevBuf<uint32_t> d_uid, d_nodes;
    DevBuf<unsigned long long> d_fwd, d_rev, d_touch, d_wmask, d_near;
    DevBuf<uint16_t> d_wmax;
    DevBuf<int64_t> d_off;
    DevBuf<char> tmp;
    std::vector<int64_t> h_off;
    // breadth (pmx_meta_set_breadth): hit, depth, observed and the multiplicities live across the chunks; the inverted list
    // (row -> the chunk's reads that carry it) and the rows' places in `hit` are per chunk
    const bool breadth;
    uint32_t breadth_cap = (1u << kBreadthPlanes) - 1u;
    DevBuf<unsigned long long> d_hit, d_depth, d_observed, d_slabs;   // (d_slabs: --gpus N, the ranks' copies of a slab of d_hit)
    DevBuf<int64_t> d_mult, d_car_off;
    DevBuf<uint32_t> d_car, d_row_id;

    AssignStage(pmx_ctx* c, pmx_meta* mm, double d)
        : ctx(c), m(mm), st(c->stream), discard(d), row0(mm->row_first), n_reads(mm->row_count), words(assign_words(mm->n_nodes)), max_taxa(mm->max_taxa),
          near(mm->max_taxa > 0 && (mm->amb_abs > 0 || mm->amb_ratio > 0.0)), breadth(mm->breadth_on) {
        // lo = max(0, max - max(abs, (int)(max * ratio))) == 0 for some maximum a read of this set can have
        for (int64_t mx = 1; near && !touch && mx <= mm->longest; ++mx)
            touch = mx <= std::max<int64_t>(mm->amb_abs, (int64_t)((double)mx * mm->amb_ratio));
    }
    void plan_chunks();
    void begin();
    void run_chunk(int64_t r0, int64_t r1);
    void finish();
    void breadth_begin();
    void breadth_merge();
    int breadth_rows_per_block(int64_t n_rows) const;
};

// Chunks of consecutive merged reads of this rank's rows [row_first, row_first + row_count) whose distinct seedmers number at
// most cap_rows, at most cap_reads reads each (a read that alone exceeds them is a chunk of its own): the first merged read of
// every chunk, then the end of the rows (a rank without rows: the first row alone, no chunk).
std::vector<int64_t> plan_read_chunks(const pmx_meta* m, int64_t cap_rows, int64_t cap_reads) {
    std::vector<int64_t> seen(m->h_uniq.size(), -1);   // the chunk (by its first read) that last counted the seedmer
    const int64_t row_end = m->row_first + m->row_count;
    std::vector<int64_t> chunk_first(1, m->row_first);
    int64_t r0 = m->row_first, rows = 0;
    for (int64_t r = m->row_first; r < row_end; ++r) {
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
    if (m->row_count > 0) chunk_first.push_back(row_end);   // (a rank without rows: no chunk)
    return chunk_first;
}

// Chunks whose distinct seedmers fit kAssignMatrixBytes and whose word masks fit kAssignReadRowBytes; PMX_META_ASSIGN_CHUNK
// forces a size in reads.
void AssignStage::plan_chunks() {
    const int64_t cap_rows = std::max<int64_t>(1, (int64_t)(kAssignMatrixBytes / ((touch ? 24 : 16) * (size_t)words)));
    int64_t cap_reads = std::max<int64_t>(1, (int64_t)(kAssignReadRowBytes / ((near ? 18 : 10) * (size_t)words)));
    if (const char* f = opt_str(O_META_ASSIGN_CHUNK)) cap_reads = std::max<int64_t>(1, atoll(f));
    chunk_first = plan_read_chunks(m, cap_rows, cap_reads);
}

// The rows of a chunk, merged reads [r0, r1): its distinct seedmers as indices into h_uniq (ids, ascending, as h_uniq is) and
// as hashes (uniq), and every seedmer of those reads as its row (uid).
struct ChunkRows {
    std::vector<uint32_t> ids, uid;
    std::vector<uint64_t> uniq;
};
ChunkRows chunk_rows(const pmx_meta* m, int64_t r0, int64_t r1) {
    const int64_t s0 = m->h_read_off[(size_t)r0], s1 = m->h_read_off[(size_t)r1];
    ChunkRows C;
    C.ids.assign(m->h_seed_uid.begin() + s0, m->h_seed_uid.begin() + s1);
    std::sort(C.ids.begin(), C.ids.end());
    C.ids.erase(std::unique(C.ids.begin(), C.ids.end()), C.ids.end());
    C.uniq.resize(C.ids.size());
    for (size_t i = 0; i < C.ids.size(); ++i) C.uniq[i] = m->h_uniq[C.ids[i]];
    C.uid.resize((size_t)(s1 - s0));
    for (int64_t i = s0; i < s1; ++i)
        C.uid[(size_t)(i - s0)] = (uint32_t)(std::lower_bound(C.ids.begin(), C.ids.end(), m->h_seed_uid[(size_t)i]) - C.ids.begin());
    return C;
}

// Leaves: the per-read device buffers of the call (d_tax and d_count zeroed: a read fills its first ids only, the scans read
// one count past the last read), the summed spans of the call reset (no "meta_assign_taxa" span without a taxonomy) and,
// with breadth, what breadth_begin leaves.
void AssignStage::begin() {
    const size_t n = (size_t)n_reads;
    d_max.alloc(n); d_count.alloc(n + 1); d_first.alloc(n); d_last.alloc(n);
    d_state.alloc(n + (breadth ? 3 : 0));   // (k_meta_breadth_rows reads the states by whole words)
    if (max_taxa > 0) {
        d_ntax.alloc(n); d_tax.alloc(n * (size_t)max_taxa);
        PMX_ZERO(d_tax, n * (size_t)max_taxa, st);
        timer_sum_reset(ctx, "meta_assign_taxa");
    }
    timer_sum_reset(ctx, "meta_assign");
    timer_cancel(ctx, "meta_assign_taxa");
    timer_sum_reset(ctx, "meta_assign_emit");
    if (breadth) {
        timer_sum_reset(ctx, "meta_breadth");
        breadth_begin();
    }
    PMX_ZERO(d_count, n + 1, st);
}

// Merged reads [r0, r1): their distinct seedmers' rows, the reads' maxima and assigned nodes.
// With a taxonomy the reads spanning too many taxa become PMX_META_OVER_TAXA before the scan (d_ntax, d_tax: the others' taxa).
// Leaves: d_max .. d_state of the reads, m->as_off (r0, r1] and m->as_nodes grown by the chunk's lists.
void AssignStage::run_chunk(int64_t r0, int64_t r1) {
    const int64_t n = r1 - r0, s0 = m->h_read_off[(size_t)r0], l0 = r0 - row0;   // l0: the chunk's first read among this rank's rows
    const ChunkRows C = chunk_rows(m, r0, r1);
    const std::vector<uint32_t>& ids = C.ids;
    const std::vector<uint32_t>& uid = C.uid;
    const std::vector<uint64_t>& uniq = C.uniq;
    const int64_t n_rows = (int64_t)ids.size();
    const size_t mat = (size_t)n_rows * (size_t)words;
    d_uniq.ensure((size_t)n_rows); d_uid.ensure(uid.size()); d_fwd.ensure(mat); d_rev.ensure(mat);
    d_wmask.ensure((size_t)n * (size_t)words); d_wmax.ensure((size_t)n * (size_t)words); d_off.ensure((size_t)n + 1);
    if (touch) d_touch.ensure(mat);
    if (near) d_near.ensure((size_t)n * (size_t)words);
    PMX_H2D(d_uniq, uniq, n_rows, st);
    PMX_H2D(d_uid, uid, st);
    std::vector<int64_t> car_off;   // breadth: the chunk's inverted list, alive until the synchronize below
    std::vector<uint32_t> car;
    if (breadth) {
        car_off.assign((size_t)n_rows + 1, 0);
        std::vector<uint32_t> mine;
        for (int pass = 0; pass < 2; ++pass) {   // count, then fill: a read once per row
            for (int64_t r = r0; r < r1; ++r) {
                mine.assign(uid.begin() + (m->h_read_off[(size_t)r] - s0), uid.begin() + (m->h_read_off[(size_t)r + 1] - s0));
                std::sort(mine.begin(), mine.end());
                mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
                for (uint32_t row : mine) {
                    if (pass == 0) ++car_off[(size_t)row + 1];
                    else car[(size_t)car_off[(size_t)row]++] = (uint32_t)(r - r0);
                }
            }
            if (pass == 0) {
                for (int64_t i = 0; i < n_rows; ++i) car_off[(size_t)i + 1] += car_off[(size_t)i];
                car.resize((size_t)car_off[(size_t)n_rows]);
            } else {   // (the fill moved every offset to its row's end: shift them back)
                for (int64_t i = n_rows; i > 0; --i) car_off[(size_t)i] = car_off[(size_t)i - 1];
                car_off[0] = 0;
            }
        }
        d_car_off.ensure(car_off.size()); d_car.ensure(car.size()); d_row_id.ensure((size_t)n_rows);
        PMX_H2D(d_car_off, car_off, st);
        if (!car.empty()) PMX_H2D(d_car, car, st);
        PMX_H2D(d_row_id, ids, n_rows, st);
    }
    timer_begin(ctx, "meta_assign");
    PMX_ZERO(d_fwd, mat, st);
    PMX_ZERO(d_rev, mat, st);
    if (touch) PMX_ZERO(d_touch, mat, st);
    if (m->n_changes > 0)
        PMX_LAUNCH(k_assign_mark_ends, dim3(grid_for(m->n_changes, 256, ctx->n_cu * 8)), dim3(256), 0, st, m->ch_key.p, m->ch_pc.p, m->ch_cc.p,
                   m->ch_node.p, m->n_changes, m->subtree_end.p, m->n_nodes, d_uniq.p, n_rows, words, d_fwd.p, d_rev.p,
                   touch ? d_touch.p : nullptr);
    PMX_LAUNCH(k_assign_prefix_xor, dim3(grid_for(2 * n_rows * 64, 256, ctx->n_cu * 16)), dim3(256), 0, st, d_fwd.p, d_rev.p, n_rows, words);
    const dim3 grid(grid_for(n * 64, 256, ctx->n_cu * 16)), block(256);
    meta_with_planes(m->longest, [&](auto planes) {
        PMX_LAUNCH(k_meta_assign_max<decltype(planes)::value>, grid, block, 0, st, m->d_read_off.p + r0, s0, d_uid.p, m->d_seed_rev.p, n, d_fwd.p, d_rev.p,
                   words, m->n_nodes, discard, d_wmask.p, d_wmax.p, d_max.p + l0, d_count.p + l0, d_first.p + l0, d_last.p + l0, d_state.p + l0);
    });
    if (max_taxa > 0) {   // its own span: "meta_assign" then ends here, the scan below belongs to "meta_assign_taxa"
        timer_end(ctx, "meta_assign", 1);
        timer_begin(ctx, "meta_assign_taxa");
        if (near)
            meta_with_planes(m->longest, [&](auto planes) {
                PMX_LAUNCH(k_meta_assign_near<decltype(planes)::value>, grid, block, 0, st, m->d_read_off.p + r0, s0, d_uid.p, m->d_seed_rev.p, n, d_fwd.p,
                           d_rev.p, touch ? d_touch.p : nullptr, words, m->n_nodes, (int)m->amb_abs, m->amb_ratio, d_max.p + l0, d_state.p + l0, d_near.p);
            });
        PMX_LAUNCH(k_meta_assign_taxa, grid, block, 0, st, near ? d_near.p : d_wmask.p, words, n, m->tx_over.p, m->tx_count.p, m->tx_ids.p, max_taxa,
                   d_state.p + l0, d_count.p + l0, d_ntax.p + l0, d_tax.p + (size_t)l0 * (size_t)max_taxa);
    }
    // (d_count has one entry past the last read, zero: the scan's entry n is the chunk's total; the entry it reads past the
    //  chunk's own counts plays no part in any output)
    PMX_ROCPRIM(tmp, exclusive_scan, d_count.p + l0, d_off.p, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st);
    timer_end(ctx, max_taxa > 0 ? "meta_assign_taxa" : "meta_assign", 1);
    if (breadth) {   // the states are final
        timer_begin(ctx, "meta_breadth");
        const int rpb = breadth_rows_per_block(n_rows);
        const int64_t items = ((n_rows + rpb - 1) / rpb) * (int64_t)((words + 63) / 64);
        PMX_LAUNCH(k_meta_breadth_rows, dim3(grid_for(items * 64, 256, ctx->n_cu * 8)), dim3(256), 0, st, d_fwd.p, d_rev.p, n_rows, words, d_row_id.p,
                   d_car_off.p, d_car.p, reinterpret_cast<const uint32_t*>(d_state.p), l0, d_mult.p + l0, d_wmask.p, rpb, breadth_cap, d_hit.p, d_depth.p);
        timer_end(ctx, "meta_breadth", 1);
    }
    h_off.resize((size_t)n + 1);
    PMX_D2H_SYNC(h_off, d_off, (size_t)n + 1, st);   // (uniq / uid go out of scope; the total sizes the list)
    timer_sum_add(ctx, "meta_assign");
    if (max_taxa > 0) timer_sum_add(ctx, "meta_assign_taxa");
    if (breadth) timer_sum_add(ctx, "meta_breadth");
    const int64_t total = h_off[(size_t)n], base = (int64_t)m->as_nodes.size();
    for (int64_t i = 1; i <= n; ++i) m->as_off[(size_t)(l0 + i)] = base + h_off[(size_t)i];
    if (total == 0) return;
    d_nodes.ensure((size_t)total);
    timer_begin(ctx, "meta_assign_emit");
    PMX_LAUNCH(k_meta_assign_emit, grid, block, 0, st, d_count.p + l0, d_off.p, n, d_wmask.p, words, d_nodes.p);
    timer_end(ctx, "meta_assign_emit", 1);
    m->as_nodes.resize((size_t)(base + total));
    PMX_D2H_SYNC(m->as_nodes.data() + base, d_nodes, total, st);
    timer_sum_add(ctx, "meta_assign_emit");
}

// The per-read results to the host; the LCA of every assigned read from its first and last node: in pre-order the LCA of a
// set is the lowest ancestor a of its first node with subtree_end[a] >= its last node.
void AssignStage::finish() {
    std::vector<uint32_t> first((size_t)n_reads), last((size_t)n_reads);
    PMX_D2H(m->as_max, d_max, n_reads, st);
    PMX_D2H(m->as_count, d_count, n_reads, st);
    PMX_D2H(m->as_state, d_state, n_reads, st);
    PMX_D2H(first, d_first, n_reads, st);
    PMX_D2H(last, d_last, n_reads, st);
    if (max_taxa > 0) {
        PMX_D2H(m->as_ntax, d_ntax, n_reads, st);
        PMX_D2H(m->as_tax, d_tax, (size_t)n_reads * (size_t)max_taxa, st);
    }
    PMX_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < n_reads; ++r) {
        if (m->as_state[(size_t)r] != PMX_META_ASSIGNED) continue;
        uint32_t a = first[(size_t)r];
        while (m->h_subtree_end[a] < last[(size_t)r]) a = m->h_parent[a];
        m->as_lca[(size_t)r] = a;
    }
    if (!breadth) return;
    // observed: the column counts of `hit`, once
    const int64_t n_uniq = (int64_t)m->h_uniq.size();
    const int rpb = breadth_rows_per_block(n_uniq);
    const int64_t items = ((n_uniq + rpb - 1) / rpb) * (int64_t)((words + 63) / 64);
    if (m->dist) breadth_merge();   // the whole sample's hit matrix on every rank
    timer_begin(ctx, "meta_breadth");
    timer_begin(ctx, "meta_breadth_count");   // (the count kernel alone; "meta_breadth" holds it too)
    PMX_LAUNCH(k_meta_breadth_count, dim3(grid_for(items * 64, 256, ctx->n_cu * 8)), dim3(256), 0, st, d_hit.p, n_uniq, words, rpb, breadth_cap, d_observed.p);
    timer_end(ctx, "meta_breadth_count", 1);
    timer_end(ctx, "meta_breadth", 1);
    PMX_D2H(m->br_observed, d_observed, m->n_nodes, st);
    PMX_D2H_SYNC(m->br_depth, d_depth, m->n_nodes, st);
    timer_sum_add(ctx, "meta_breadth");
    // (the depths are 64-bit sums over the reads of a node: the ranks' sums add up)
    if (m->dist && pmx_dist_sum_i64(m->dist, reinterpret_cast<int64_t*>(m->br_depth.data()), m->n_nodes) != PMX_OK) throw HipError{pmx_last_error()};
}

// --gpus N, after the last chunk: every rank's `hit` holds the (seedmer, node) pairs its own rows hit; the whole sample's
// matrix is their bitwise OR (a pair hit on two ranks counts once).  The matrices have one shape (rows: h_uniq, the same on every
// rank), so whole rows are exchanged in slabs through the dist's device all-gather -- world x slab words in d_slabs, at most
// kBreadthSlabBytes, pmx_meta_set_breadth_slab forces the rows of a slab -- and k_meta_breadth_or folds the copies into the local rows.
// The number of exchanges is a function of h_uniq, the words of a row and the world: the same on every rank, a rank without rows
// included.  "meta_breadth_merge": the OR kernels, summed over the slabs.
void AssignStage::breadth_merge() {
    const int world = pmx_dist_world(m->dist);
    const int64_t n_uniq = (int64_t)m->h_uniq.size();
    int64_t slab_rows = std::max<int64_t>(1, (int64_t)(kBreadthSlabBytes / ((size_t)world * (size_t)words * sizeof(unsigned long long))));
    if (m->breadth_slab_rows > 0) slab_rows = m->breadth_slab_rows;
    slab_rows = std::min(slab_rows, std::max<int64_t>(n_uniq, 1));
    d_slabs.alloc((size_t)world * (size_t)slab_rows * (size_t)words);
    timer_sum_reset(ctx, "meta_breadth_merge");
    for (int64_t row0 = 0; row0 < n_uniq; row0 += slab_rows) {
        const int64_t n = std::min(slab_rows, n_uniq - row0) * (int64_t)words;   // words of this slab, and from one copy to the next
        unsigned long long* mine = d_hit.p + (size_t)row0 * (size_t)words;
        dist_all_gather(m->dist, mine, (size_t)n * sizeof(unsigned long long), d_slabs.p);
        timer_begin(ctx, "meta_breadth_merge");
        PMX_LAUNCH(k_meta_breadth_or, dim3(grid_for((n + 1) / 2, 256, ctx->n_cu * 8)), dim3(256), 0, st, mine, d_slabs.p, n, n, world);
        timer_end(ctx, "meta_breadth_merge", 1);
        PMX_HIP(hipStreamSynchronize(st));   // (the next exchange writes d_slabs)
        timer_sum_add(ctx, "meta_breadth_merge");
    }
}

// Rows a wave walks before it expands its counters: enough (block, span) items for 32 waves a CU, 16 to 512 rows.
int AssignStage::breadth_rows_per_block(int64_t n_rows) const {
    const int64_t spans = (words + 63) / 64;
    return (int)std::min<int64_t>(512, std::max<int64_t>(16, n_rows * spans / ((int64_t)ctx->n_cu * 32)));
}

// The buffers that live across the chunks, zeroed; the flush bound.
void AssignStage::breadth_begin() {
    const size_t mat = m->h_uniq.size() * (size_t)words, cols = (size_t)words * 64;
    d_hit.alloc(mat); d_depth.alloc(cols); d_observed.alloc(cols); d_mult.alloc((size_t)n_reads);
    PMX_ZERO(d_hit, mat, st);
    PMX_ZERO(d_depth, cols, st);
    PMX_ZERO(d_observed, cols, st);
    PMX_H2D(d_mult, m->h_mult.data() + row0, (size_t)n_reads, st);
    if (const char* f = opt_str(O_META_BREADTH_FLUSH)) breadth_cap = (uint32_t)std::min<long long>(breadth_cap, std::max<long long>(1, atoll(f)));
}

// TotalRefSeeds of every node (node->totalRefSeeds, src/mgsr.cpp:590-610): the distinct hashes of its genome, a hash being the
// pair {key, key ^ PMX_ORIENT_XOR} of the oriented index, present when either count is positive.  One DFS over the changes
// (nodes are in pre-order: the open ancestors are a stack), applied on the way in and reverted on the way out.
std::vector<uint64_t> total_ref_seeds(const pmx_meta* m) {
    const LiteIndex* O = pmx_index_internal(m->idx_oriented);
    std::vector<uint64_t> total((size_t)m->n_nodes);
    std::unordered_map<uint64_t, int16_t> count;
    count.reserve(O->hash.size());
    int64_t present = 0;
    auto set = [&](uint64_t key, int16_t to) {
        const auto o = count.find(key ^ PMX_ORIENT_XOR);
        const bool other = o != count.end() && o->second > 0;
        int16_t& c = count[key];
        present += (int64_t)(to > 0 || other) - (int64_t)(c > 0 || other);
        c = to;
    };
    std::vector<uint32_t> open;
    for (int64_t v = 0; v < m->n_nodes; ++v) {
        while (!open.empty() && (int64_t)m->h_subtree_end[open.back()] < v) {
            const uint32_t u = open.back();
            open.pop_back();
            for (uint64_t q = O->offsets[(size_t)u + 1]; q > O->offsets[u]; --q) set(O->hash[q - 1], O->parent_count[q - 1]);
        }
        for (uint64_t q = O->offsets[(size_t)v]; q < O->offsets[(size_t)v + 1]; ++q) set(O->hash[q], O->child_count[q]);
        total[(size_t)v] = (uint64_t)present;
        open.push_back((uint32_t)v);
    }
    return total;
}

// The results of a call that assigns nothing, sized for the merged reads: every read unmapped, no nodes, no taxa; with breadth
// zero counts per node and TotalRefSeeds, computed on the first such call.  No "meta_breadth" spans are left from an earlier call.
void reset_assign_results(pmx_ctx* ctx, pmx_meta* m) {
    const size_t n = (size_t)m->row_count;   // (--gpus N: this rank's rows)
    m->as_rows = m->row_count;
    m->as_gathered = false;
    m->as_state.assign(n, PMX_META_UNMAPPED);
    m->as_max.assign(n, 0);
    m->as_count.assign(n, 0);
    m->as_lca.assign(n, UINT32_MAX);
    m->as_off.assign(n + 1, 0);
    m->as_nodes.clear();
    m->as_max_taxa = m->max_taxa;
    m->as_ntax.assign(n, 0);
    m->as_tax.assign(n * (size_t)m->max_taxa, 0);
    if (m->breadth_on) {
        if (m->total_ref_seeds.empty()) m->total_ref_seeds = total_ref_seeds(m);
        m->br_observed.assign((size_t)m->n_nodes, 0);
        m->br_depth.assign((size_t)m->n_nodes, 0);
    }
    timer_cancel(ctx, "meta_breadth");
    timer_cancel(ctx, "meta_breadth_count");
    timer_cancel(ctx, "meta_breadth_merge");
}

// One call of pmx_meta_read_best: the chunks of AssignStage without its word masks (nothing is kept per read and word, so
// kAssignReadRowBytes does not bound a chunk), per chunk the two matrices and k_meta_read_best.
struct BestStage {
    pmx_ctx* const ctx;
    pmx_meta* const m;
    const hipStream_t st;
    const int words;
    DevBuf<uint16_t> d_max;
    DevBuf<uint32_t> d_nbest, d_uid;
    DevBuf<uint64_t> d_uniq;
    DevBuf<unsigned long long> d_fwd, d_rev;

    BestStage(pmx_ctx* c, pmx_meta* mm) : ctx(c), m(mm), st(c->stream), words(assign_words(mm->n_nodes)) {}   // (d_max / d_nbest: this rank's rows)
    void active_nodes();
    void run_chunk(int64_t r0, int64_t r1);
};

// Leaves: m->d_active and m->h_active for the reads of the last set_reads (built by the first call after it).
void BestStage::active_nodes() {
    if (m->active_built) return;
    m->d_active.ensure((size_t)words);
    std::vector<unsigned long long> row((size_t)words);
    timer_begin(ctx, "meta_read_best");
    PMX_ZERO(m->d_active, (size_t)words, st);
    PMX_LAUNCH(k_meta_active_nodes, dim3(grid_for(m->n_changes, 256, ctx->n_cu * 8)), dim3(256), 0, st, m->ch_key.p, m->ch_node.p, m->n_changes, m->d_uniq.p,
               (int64_t)m->h_uniq.size(), m->d_active.p);
    timer_end(ctx, "meta_read_best", 1);
    PMX_D2H_SYNC(row, m->d_active, (size_t)words, st);
    timer_sum_add(ctx, "meta_read_best");
    m->h_active.resize((size_t)m->n_nodes);
    for (int64_t v = 0; v < m->n_nodes; ++v) m->h_active[(size_t)v] = (uint8_t)((row[(size_t)v >> 6] >> (v & 63)) & 1ULL);
    m->active_built = true;
}

// Merged reads [r0, r1): their distinct seedmers' rows, then d_max / d_nbest of the reads.
void BestStage::run_chunk(int64_t r0, int64_t r1) {
    const int64_t n = r1 - r0, s0 = m->h_read_off[(size_t)r0];
    const ChunkRows C = chunk_rows(m, r0, r1);
    const int64_t n_rows = (int64_t)C.ids.size();
    const size_t mat = (size_t)n_rows * (size_t)words;
    d_uniq.ensure((size_t)n_rows); d_uid.ensure(C.uid.size()); d_fwd.ensure(mat); d_rev.ensure(mat);
    PMX_H2D(d_uniq, C.uniq, n_rows, st);
    PMX_H2D(d_uid, C.uid, st);
    timer_begin(ctx, "meta_read_best");
    PMX_ZERO(d_fwd, mat, st);
    PMX_ZERO(d_rev, mat, st);
    if (m->n_changes > 0)
        PMX_LAUNCH(k_assign_mark_ends, dim3(grid_for(m->n_changes, 256, ctx->n_cu * 8)), dim3(256), 0, st, m->ch_key.p, m->ch_pc.p, m->ch_cc.p,
                   m->ch_node.p, m->n_changes, m->subtree_end.p, m->n_nodes, d_uniq.p, n_rows, words, d_fwd.p, d_rev.p, nullptr);
    PMX_LAUNCH(k_assign_prefix_xor, dim3(grid_for(2 * n_rows * 64, 256, ctx->n_cu * 16)), dim3(256), 0, st, d_fwd.p, d_rev.p, n_rows, words);
    meta_with_planes(m->longest, [&](auto planes) {
        PMX_LAUNCH(k_meta_read_best<decltype(planes)::value>, dim3(grid_for(n * 64, 256, ctx->n_cu * 16)), dim3(256), 0, st, m->d_read_off.p + r0, s0, d_uid.p,
                   m->d_seed_rev.p, n, d_fwd.p, d_rev.p, words, m->n_nodes, m->d_active.p, d_max.p + (r0 - m->row_first), d_nbest.p + (r0 - m->row_first));
    });
    timer_end(ctx, "meta_read_best", 1);
    PMX_HIP(hipStreamSynchronize(st));   // (the chunk's host lists go out of scope)
    timer_sum_add(ctx, "meta_read_best");
}

// ---- --gpus N (pmx_meta_attach_dist): pmx_meta_assign and pmx_meta_read_best as collectives.
// A merged read's results depend on its own list and the index only, and after a collective set_reads every rank holds the whole
// sample's merged reads, h_uniq and the index: a rank runs its chunk loop over ITS rows [row_first, row_first + row_count) (the
// rule of pmx_meta_score) and nothing in the per-read kernels changes.  Only breadth is not per read (AssignStage::breadth_merge
// and the sum of the depths).  What keeps a collective from hanging:
//   * every refusal is decided from settings, identically on every rank, and before any exchange but the digest's: the masks,
//     the amplicons and the masked ends of the last set_reads (itself collective) before it; after it, when the ranks are known
//     to be set alike, discard together with an ambiguity threshold and the kBreadthHitBytes bound, a function of h_uniq and the
//     node count;
//   * pmx_meta_assign starts by exchanging a digest of its settings -- the bits of discard, breadth on / off, max_taxa, the
//     ambiguity pair, a hash of the node table of pmx_meta_set_taxonomy -- and ranks that disagree ALL return PMX_ERR_ARG after that
//     exchange and before any other (the rule of MetaReads::merge_over_ranks for the amplicon groups);
//   * no exchange sits inside the per-chunk loop: ranks have different numbers of chunks.  Exchanges happen only at points
//     whose number depends on global quantities (h_uniq.size(), the words of a row, the world);
//   * a rank with an empty shard, or with zero rows, takes part in every exchange.
// A dist of ONE rank stays PMX_ERR_UNSUPPORTED for both calls, as every dist was before they became collective: one GPU has no
// use for the exchanges and runs the calls without a dist.
// pmx_meta_read_best exchanges nothing: the active nodes are a function of h_uniq.

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ULL;
    return h;
}

// the settings of a pmx_meta_assign call as six numbers: equal on ranks that were configured alike
void assign_digest(const pmx_meta* m, double discard, int64_t (&d)[6]) {
    uint64_t tx = 0xcbf29ce484222325ULL;
    if (m->max_taxa > 0) {
        tx = fnv1a(tx, m->h_tx_count.data(), m->h_tx_count.size());
        tx = fnv1a(tx, m->h_tx_ids.data(), m->h_tx_ids.size() * sizeof(uint32_t));
        tx = fnv1a(tx, m->h_tx_over.data(), m->h_tx_over.size() * sizeof(unsigned long long));
    }
    memcpy(&d[0], &discard, 8);
    d[1] = m->breadth_on ? 1 : 0;
    d[2] = m->max_taxa;
    d[3] = m->amb_abs;
    memcpy(&d[4], &m->amb_ratio, 8);
    memcpy(&d[5], &tx, 8);
}

// Every rank's part of a per-row array to `root`, in rank order: elems[r] elements of rank r.  The root returns the whole
// array, the others an empty one.  The dist's gather (send / receive, exact sizes); every rank calls it, whatever its part.
template <class T>
std::vector<T> gather_rows(pmx_meta* m, const T* mine, const std::vector<int64_t>& elems, int root) {
    pmx_ctx* ctx = m->ctx;
    const int world = pmx_dist_world(m->dist), rank = pmx_dist_rank(m->dist);
    std::vector<size_t> sizes((size_t)world), offs((size_t)world);
    size_t total = 0;
    for (int r = 0; r < world; ++r) { offs[(size_t)r] = total; sizes[(size_t)r] = (size_t)elems[(size_t)r] * sizeof(T); total += sizes[(size_t)r]; }
    DevBuf<char> d_mine, d_all;
    d_mine.alloc(sizes[(size_t)rank]);
    if (rank == root) d_all.alloc(total);
    PMX_H2D(d_mine, reinterpret_cast<const char*>(mine), sizes[(size_t)rank], ctx->stream);
    dist_gather_v(m->dist, d_mine.p, sizes, offs, d_all.p, root);
    std::vector<T> all;
    if (rank == root) {
        all.resize(total / sizeof(T));
        PMX_D2H(reinterpret_cast<char*>(all.data()), d_all, total, ctx->stream);
    }
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return all;
}
}  // namespace

extern "C" {

int pmx_meta_assign(pmx_ctx* ctx, pmx_meta* m, double discard) {
    if (!ctx || !m || !(discard >= 0.0 && discard <= 1.0)) return PMX_ERR_ARG;   // src/main.cpp:1358-1361
    if (m->dist && pmx_dist_world(m->dist) < 2)   // (as before the call was collective; the same on every rank)
        return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign with an attached dist of one rank: the collective needs two ranks or more, one GPU runs it without a dist");
    if (!m->reads_set) return fail(PMX_ERR_ARG, "pmx_meta_assign: call pmx_meta_set_reads first");
    if (m->masked)   // (the reference's reader for this mode, initializeQueryDataBatch, never masks: src/mgsr.cpp:1575)
        return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign: the reads were set with a low-coverage mask (pmx_meta_set_masks), which --filter-and-assign "
                                         "does not have: clear the masks and set the reads again");
    if (m->read_ends_masked > 0)   // (that reader takes the value and ignores it: `uint32_t /*maskReadsEnds*/`, src/mgsr.cpp:1575)
        return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign: the reads were set with masked read ends (pmx_meta_set_mask_read_ends), which --filter-and-assign "
                                         "does not have: set the masked ends to 0 and set the reads again");
    if (m->amp_on)   // (that reader takes no amplicon file either)
        return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign: the reads were set with amplicons (pmx_meta_set_amplicons), which --filter-and-assign does not "
                                         "have: clear the amplicons and set the reads again");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (m->dist) {   // the first exchange: the ranks' settings
        int64_t mine[6];
        assign_digest(m, discard, mine);
        const std::vector<int64_t> all = dist_exchange_counts(m->dist, mine, 6);
        for (size_t i = 0; i < all.size(); ++i)
            if (all[i] != all[i % 6])
                return fail(PMX_ERR_ARG, "pmx_meta_assign: the ranks disagree on the settings of the call (discard, breadth, max_taxa, the ambiguity "
                                         "thresholds or the taxonomy): rank " + std::to_string(i / 6) + " differs from rank 0");
    }
    // (the refusals that depend on the call's own settings: after the digest, so that ranks set differently have all left above)
    if (m->max_taxa > 0 && discard > 0.0 && (m->amb_abs > 0 || m->amb_ratio > 0.0))
        return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign: a discard threshold together with an ambiguity threshold (the reference's records then depend "
                                         "on the order of a node's seed changes)");
    if (m->breadth_on) {   // nothing is approximated: the hit matrix fits its budget or the call is refused
        const size_t bytes = m->h_uniq.size() * (size_t)assign_words(m->n_nodes) * sizeof(unsigned long long);
        if (bytes > kBreadthHitBytes)
            return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_assign with breadth: the hit matrix (distinct seedmers of the reads x nodes, one bit each) needs " +
                                                 std::to_string(bytes) + " bytes, the budget is " + std::to_string(kBreadthHitBytes));
    }
    m->assigned = false;
    m->as_breadth = false;
    const int rc = meta_longest_read(m);   // (of the whole sample's merged reads: the same on every rank)
    if (rc != PMX_OK) return rc;
    meta_own_row_slice(m);
    reset_assign_results(ctx, m);
    if (m->n_reads > 0) {   // (the whole sample's: a rank without rows runs no chunk and takes part in the breadth merge)
        AssignStage S(ctx, m, discard);
        S.plan_chunks();
        S.begin();
        for (size_t c = 0; c + 1 < S.chunk_first.size(); ++c) S.run_chunk(S.chunk_first[c], S.chunk_first[c + 1]);
        S.finish();
    }
    m->assigned = true;
    m->as_breadth = m->breadth_on;
    return PMX_OK;
    PMX_CATCH
}

int pmx_meta_read_best(pmx_ctx* ctx, pmx_meta* m) {
    if (!ctx || !m) return PMX_ERR_ARG;
    if (m->dist && pmx_dist_world(m->dist) < 2)   // (as before the call was collective)
        return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_read_best with an attached dist of one rank: the collective needs two ranks or more, one GPU runs it without a dist");
    if (!m->reads_set) return fail(PMX_ERR_ARG, "pmx_meta_read_best: call pmx_meta_set_reads first");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    m->best_done = false;
    const int rc = meta_longest_read(m);
    if (rc != PMX_OK) return rc;
    meta_own_row_slice(m);
    BestStage S(ctx, m);
    const size_t n = (size_t)m->row_count;   // (--gpus N: this rank's rows; nothing is exchanged)
    m->rb_rows = m->row_count;
    m->rb_gathered = false;
    timer_sum_reset(ctx, "meta_read_best");
    timer_cancel(ctx, "meta_read_best");   // (no span when nothing below runs: the active nodes are built, no reads)
    S.active_nodes();
    m->rb_max.assign(n, 0);
    m->rb_nbest.assign(n, 0);
    if (n > 0) {
        S.d_max.alloc(n); S.d_nbest.alloc(n);
        const int64_t cap_rows = std::max<int64_t>(1, (int64_t)(kAssignMatrixBytes / (16 * (size_t)S.words)));
        int64_t cap_reads = INT64_MAX;
        if (const char* f = opt_str(O_META_ASSIGN_CHUNK)) cap_reads = std::max<int64_t>(1, atoll(f));
        const std::vector<int64_t> chunk_first = plan_read_chunks(m, cap_rows, cap_reads);
        for (size_t c = 0; c + 1 < chunk_first.size(); ++c) S.run_chunk(chunk_first[c], chunk_first[c + 1]);
        PMX_D2H(m->rb_max, S.d_max, n, S.st);
        PMX_D2H_SYNC(m->rb_nbest, S.d_nbest, n, S.st);
    }
    m->best_done = true;
    return PMX_OK;
    PMX_CATCH
}

int pmx_meta_read_best_get(const pmx_meta* m, uint16_t* max_score, uint32_t* n_best, int64_t cap) {
    if (!m || !m->best_done || cap < m->rb_rows) return PMX_ERR_ARG;
    if (max_score) std::copy(m->rb_max.begin(), m->rb_max.end(), max_score);
    if (n_best) std::copy(m->rb_nbest.begin(), m->rb_nbest.end(), n_best);
    return PMX_OK;
}

int pmx_meta_active_nodes(const pmx_meta* m, uint8_t* active, int64_t cap_nodes) {
    if (!m || !m->active_built || !active || cap_nodes < m->n_nodes) return PMX_ERR_ARG;
    std::copy(m->h_active.begin(), m->h_active.end(), active);
    return PMX_OK;
}

int pmx_meta_set_breadth(pmx_meta* m, int on) {
    if (!m) return PMX_ERR_ARG;
    m->breadth_on = on != 0;
    return PMX_OK;
}

int pmx_meta_set_breadth_slab(pmx_meta* m, int64_t rows) {
    if (!m || rows < 0) return PMX_ERR_ARG;
    m->breadth_slab_rows = rows;
    return PMX_OK;
}

int pmx_meta_breadth(const pmx_meta* m, uint64_t* total_ref_seeds, uint64_t* observed, uint64_t* depth, int64_t cap_nodes) {
    if (!m || !m->assigned || !m->as_breadth || cap_nodes < m->n_nodes) return PMX_ERR_ARG;
    if (total_ref_seeds) std::copy(m->total_ref_seeds.begin(), m->total_ref_seeds.end(), total_ref_seeds);
    if (observed) std::copy(m->br_observed.begin(), m->br_observed.end(), observed);
    if (depth) std::copy(m->br_depth.begin(), m->br_depth.end(), depth);
    return PMX_OK;
}

int pmx_meta_assign_reads(const pmx_meta* m, uint8_t* state, uint16_t* max_score, uint32_t* lca, uint32_t* n_nodes, int64_t cap) {
    if (!m || !m->assigned || cap < m->as_rows) return PMX_ERR_ARG;
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

// S(v) of every node, bottom-up in the unfolded tree (nodes are in pre-order: children after their parents), each capped at
// max_taxa + 1 ids; then the node table of k_meta_assign_taxa.
int pmx_meta_set_taxonomy(pmx_meta* m, const int32_t* node_taxon, int64_t n_nodes, int64_t n_taxa, int32_t max_taxa) {
    if (!m || max_taxa < 0) return PMX_ERR_ARG;
    if (max_taxa == 0) {
        m->max_taxa = 0;
        m->n_taxa = 0;
        m->h_tx_count.clear(); m->h_tx_ids.clear(); m->h_tx_over.clear();
        return PMX_OK;
    }
    if (!node_taxon || n_nodes != m->n_nodes || n_taxa < 0) return PMX_ERR_ARG;
    if (max_taxa > kAssignMaxTaxa) return fail(PMX_ERR_UNSUPPORTED, "pmx_meta_set_taxonomy: at most 16 taxa a read (max_taxa)");
    for (int64_t v = 0; v < n_nodes; ++v)
        if (node_taxon[v] < -1 || node_taxon[v] >= n_taxa) return fail(PMX_ERR_ARG, "pmx_meta_set_taxonomy: a taxon outside [0, n_taxa)");
    PMX_TRY
    PMX_HIP(hipSetDevice(m->ctx->device));
    const size_t M = (size_t)max_taxa, n = (size_t)n_nodes;
    std::vector<std::vector<uint32_t>> S(n);   // ascending; max_taxa + 1 ids = over
    auto add = [&](std::vector<uint32_t>& s, uint32_t t) {
        const auto at = std::lower_bound(s.begin(), s.end(), t);
        if ((at == s.end() || *at != t) && s.size() <= M) s.insert(at, t);
    };
    for (size_t v = n; v-- > 0;) {
        if (node_taxon[v] >= 0) add(S[v], (uint32_t)node_taxon[v]);
        if (v > 0) {
            std::vector<uint32_t>& up = S[m->h_parent[v]];
            for (uint32_t t : S[v]) add(up, t);
        }
    }
    const size_t words = (size_t)assign_words(n_nodes);
    m->h_tx_count.assign(n, 0);
    m->h_tx_ids.assign(n * M, 0);
    m->h_tx_over.assign(words, 0ULL);
    for (size_t v = 0; v < n; ++v) {
        if (S[v].size() > M) { m->h_tx_over[v >> 6] |= 1ULL << (v & 63); continue; }
        m->h_tx_count[v] = (uint8_t)S[v].size();
        std::copy(S[v].begin(), S[v].end(), m->h_tx_ids.begin() + v * M);
    }
    const hipStream_t st = m->ctx->stream;
    m->tx_count.ensure(n); m->tx_ids.ensure(n * M); m->tx_over.ensure(words);
    PMX_H2D(m->tx_count, m->h_tx_count, n, st);
    PMX_H2D(m->tx_ids, m->h_tx_ids, n * M, st);
    PMX_H2D(m->tx_over, m->h_tx_over, words, st);
    PMX_HIP(hipStreamSynchronize(st));
    m->max_taxa = max_taxa;
    m->n_taxa = n_taxa;
    return PMX_OK;
    PMX_CATCH
}

int pmx_meta_set_ambiguous(pmx_meta* m, int32_t abs, double ratio) {
    if (!m || abs < 0 || !(ratio >= 0.0)) return PMX_ERR_ARG;
    m->amb_abs = abs;
    m->amb_ratio = std::min(ratio, 1.0);   // (from 1 on amb >= max, lo = 0: all the same)
    return PMX_OK;
}

int pmx_meta_assign_taxa(const pmx_meta* m, uint32_t* n_taxa, uint32_t* taxa, int64_t cap) {
    if (!m || !m->assigned || cap < m->as_rows) return PMX_ERR_ARG;
    if (n_taxa) std::copy(m->as_ntax.begin(), m->as_ntax.end(), n_taxa);
    if (taxa) std::copy(m->as_tax.begin(), m->as_tax.end(), taxa);
    return PMX_OK;
}

int32_t pmx_meta_assign_max_taxa(const pmx_meta* m) { return m && m->assigned ? m->as_max_taxa : 0; }

int64_t pmx_meta_node_taxa(const pmx_meta* m, int64_t v, uint32_t* ids, int64_t cap) {
    if (!m || m->max_taxa == 0 || v < 0 || v >= m->n_nodes) return -2;
    if ((m->h_tx_over[(size_t)v >> 6] >> (v & 63)) & 1ULL) return -1;
    const int64_t c = m->h_tx_count[(size_t)v];
    if (ids) {
        if (cap < c) return -2;
        std::copy_n(m->h_tx_ids.begin() + (size_t)v * (size_t)m->max_taxa, (size_t)c, ids);
    }
    return c;
}

// (--gpus N: n_raw_reads counts the whole sample's reads, the map covers the shard's)
// The rows of every rank to `root`: afterwards its getters cover all merged reads, as one rank's would -- the per-read arrays in
// row order (the ranks' rows tile the merged reads in rank order), the node lists back to back, the offsets rebased (a read's
// stretch of the list is its node count, on one rank as here).  The other ranks keep their rows.
int pmx_meta_assign_gather(pmx_ctx* ctx, pmx_meta* m, int root) {
    if (!ctx || !m || !m->dist || root < 0 || root >= pmx_dist_world(m->dist)) return PMX_ERR_ARG;
    if (!m->assigned || m->as_gathered) return fail(PMX_ERR_ARG, "pmx_meta_assign_gather: call pmx_meta_assign first, and gather its results once");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const int world = pmx_dist_world(m->dist);
    const int64_t mine[2] = {m->as_rows, (int64_t)m->as_nodes.size()};
    const std::vector<int64_t> counts = dist_exchange_counts(m->dist, mine, 2);
    std::vector<int64_t> rows((size_t)world), lists((size_t)world), taxa((size_t)world);
    for (int r = 0; r < world; ++r) {
        rows[(size_t)r] = counts[2 * (size_t)r];
        lists[(size_t)r] = counts[2 * (size_t)r + 1];
        taxa[(size_t)r] = rows[(size_t)r] * m->as_max_taxa;
    }
    std::vector<uint8_t> state = gather_rows(m, m->as_state.data(), rows, root), ntax = gather_rows(m, m->as_ntax.data(), rows, root);
    std::vector<uint16_t> mx = gather_rows(m, m->as_max.data(), rows, root);
    std::vector<uint32_t> lca = gather_rows(m, m->as_lca.data(), rows, root), count = gather_rows(m, m->as_count.data(), rows, root);
    std::vector<uint32_t> tax = gather_rows(m, m->as_tax.data(), taxa, root), nodes = gather_rows(m, m->as_nodes.data(), lists, root);
    m->as_gathered = true;
    if (pmx_dist_rank(m->dist) != root) return PMX_OK;
    m->as_state.swap(state); m->as_ntax.swap(ntax); m->as_max.swap(mx); m->as_lca.swap(lca); m->as_count.swap(count); m->as_tax.swap(tax);
    m->as_nodes.swap(nodes);
    m->as_rows = (int64_t)m->as_state.size();
    m->as_off.assign((size_t)m->as_rows + 1, 0);
    for (int64_t r = 0; r < m->as_rows; ++r) m->as_off[(size_t)r + 1] = m->as_off[(size_t)r] + (int64_t)m->as_count[(size_t)r];
    return PMX_OK;
    PMX_CATCH
}

int pmx_meta_read_best_gather(pmx_ctx* ctx, pmx_meta* m, int root) {
    if (!ctx || !m || !m->dist || root < 0 || root >= pmx_dist_world(m->dist)) return PMX_ERR_ARG;
    if (!m->best_done || m->rb_gathered) return fail(PMX_ERR_ARG, "pmx_meta_read_best_gather: call pmx_meta_read_best first, and gather its results once");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const std::vector<int64_t> rows = dist_exchange_counts(m->dist, &m->rb_rows, 1);
    std::vector<uint16_t> mx = gather_rows(m, m->rb_max.data(), rows, root);
    std::vector<uint32_t> nbest = gather_rows(m, m->rb_nbest.data(), rows, root);
    m->rb_gathered = true;
    if (pmx_dist_rank(m->dist) != root) return PMX_OK;
    m->rb_max.swap(mx); m->rb_nbest.swap(nbest);
    m->rb_rows = (int64_t)m->rb_max.size();
    return PMX_OK;
    PMX_CATCH
}

int64_t pmx_meta_num_raw_reads(const pmx_meta* m) { return !m ? 0 : m->dist ? (int64_t)m->h_raw_to_merged.size() : m->n_raw_reads; }

int pmx_meta_raw_to_merged(const pmx_meta* m, int64_t* map, int64_t cap) {
    if (!m || !map || !m->reads_set) return PMX_ERR_ARG;
    if (cap < (int64_t)m->h_raw_to_merged.size()) return PMX_ERR_ARG;
    std::copy(m->h_raw_to_merged.begin(), m->h_raw_to_merged.end(), map);
    return PMX_OK;
}

}  // extern "C"
