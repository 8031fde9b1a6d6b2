// What the translation units of --meta share: the state behind a pmx_meta handle (api_meta.hip makes and fills it,
// meta_assign.hip reads the merged reads and the oriented index from it, meta_mask.hip rewrites the merged reads under a
// low-coverage mask), the two device helpers both scoring kernels use, and the few host helpers more than one of them needs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <vector>

#include "api_internal.hpp"
#include "device/dev_util.hpp"
#include "host/seed_host.hpp"

// index of `key` in the ascending array keys[0..n), or -1
__device__ __forceinline__ int64_t find_sorted(const uint64_t* __restrict__ keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && keys[lo] == key ? lo : -1;
}

// bit-sliced counters: plane[p] holds bit p of 64 independent counts; add one 64-bit row of 0/1 increments
template <int PLANES>
__device__ __forceinline__ void planes_add(unsigned long long (&plane)[PLANES], unsigned long long inc) {
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
        const unsigned long long carry = plane[p] & inc;
        plane[p] ^= inc;
        inc = carry;
    }
}

struct pmx_meta_group {
    uint32_t node;                   // representative (lowest DFS index of the group)
    std::vector<uint32_t> members;   // the other candidates with the same score column
    double prop = 0.0;
};

struct pmx_meta {
    pmx_ctx* ctx = nullptr;
    const pmx_index* idx_std = nullptr;
    const pmx_index* idx_oriented = nullptr;   // (read again by pmx_meta_assign with breadth: TotalRefSeeds)
    int64_t n_nodes = 0, n_changes = 0;
    pmx::SyncmerParams params;
    // oriented index on the device
    pmx::DevBuf<uint64_t> ch_key;
    pmx::DevBuf<int16_t> ch_pc, ch_cc;
    pmx::DevBuf<uint32_t> ch_node, subtree_end;
    std::vector<uint32_t> h_parent, h_subtree_end;   // the tree on the host (pmx_meta_assign: LCA)
    pmx_place* placer = nullptr;
    // reads (merged by seedmer list)
    int64_t n_raw_reads = 0, n_reads = 0, n_seedmers = 0;
    std::vector<int64_t> h_read_off;
    std::vector<uint64_t> h_seed_hash;
    std::vector<uint8_t> h_seed_rev;
    std::vector<int64_t> h_mult;
    std::vector<uint64_t> h_uniq;
    std::vector<uint32_t> h_seed_uid;       // every seedmer as its index into h_uniq
    std::vector<int64_t> h_raw_to_merged;   // per raw read of the last set_reads: its merged read, -1 = dropped (DUST, no seedmers, a mask); --gpus N: this rank's shard -> the whole sample's merged reads
    pmx::DevBuf<int64_t> d_read_off;
    pmx::DevBuf<uint32_t> d_seed_uid;
    pmx::DevBuf<uint8_t> d_seed_rev;
    pmx::DevBuf<uint64_t> d_uniq;
    std::vector<double> oc;                 // per node
    // candidates
    std::vector<uint32_t> cand;             // DFS indices, ascending
    pmx::DevBuf<uint32_t> d_cand;
    pmx::DevBuf<unsigned long long> mask_fwd, mask_rev;
    pmx::DevBuf<uint16_t> score;            // [n_reads][n_cand]
    // result
    std::vector<pmx_meta_group> groups;     // sorted by proportion, descending
    int em_rounds = 0, em_iterations = 0;
    double llh = 0.0;
    double dust_threshold = 100.0;          // --dust: 100 = no filter
    int64_t n_dust_dropped = 0;
    // --mask-read-ends (pmx_meta_set_mask_read_ends; extractReadSequences, src/mgsr.cpp:1274-1280): bases the next set_reads
    // cuts from both ends of every read, and what the last one cut
    int64_t mask_read_ends = 0, read_ends_masked = 0;
    bool em_leaves_only = false;            // --em-leaves-only (pmx_meta_set_em_leaves_only): pmx_meta_score's candidates
    int64_t longest = 0;                    // seedmers of the longest merged read
    // --gpus N (pmx_meta_attach_dist): `score` holds merged reads [row_first, row_first + row_count) only (pass A), score_em
    // the EM rows this rank owns (pass B)
    pmx_dist* dist = nullptr;
    bool reads_set = false;
    int64_t row_first = 0, row_count = 0;
    pmx::DevBuf<uint16_t> score_em;
    // pmx_meta_assign (meta_assign.hip), per merged read of the last call; emptied by set_reads.  --gpus N: per merged read of
    // this rank's rows, as_rows of them from row_first on; after pmx_meta_assign_gather (as_gathered) the root holds all n_reads
    bool assigned = false, as_gathered = false;
    int64_t as_rows = 0;
    std::vector<uint8_t> as_state;
    std::vector<uint16_t> as_max;
    std::vector<uint32_t> as_lca, as_count;
    std::vector<int64_t> as_off;            // n_reads + 1 offsets into as_nodes
    std::vector<uint32_t> as_nodes;         // the assigned nodes of every read, ascending DFS indices
    int32_t as_max_taxa = 0;                // max_taxa of that call: as_tax holds as_max_taxa ids a read, as_ntax of them set
    std::vector<uint8_t> as_ntax;
    std::vector<uint32_t> as_tax;
    // breadth (pmx_meta_set_breadth; calculateBreadthRatio, src/mgsr.cpp:6518-6584), per node: total_ref_seeds once per pmx_meta,
    // br_observed / br_depth of the last pmx_meta_assign when as_breadth
    bool breadth_on = false, as_breadth = false;
    int64_t breadth_slab_rows = 0;   // pmx_meta_set_breadth_slab: rows of the hit matrix per exchange of its merge over the ranks, 0 = what the slab buffer holds
    std::vector<uint64_t> total_ref_seeds, br_observed, br_depth;
    // pmx_meta_read_best (meta_assign.hip): per merged read its best score over ALL nodes and the number of ACTIVE nodes that
    // reach it; the active nodes of the read set as a row of assign_words(n_nodes) words, on the device and one byte a node on
    // the host (built by the first call after a set_reads).  All emptied by set_reads
    bool best_done = false, active_built = false, rb_gathered = false;   // (rb_rows / rb_gathered: as as_rows / as_gathered)
    int64_t rb_rows = 0;
    std::vector<uint16_t> rb_max;
    std::vector<uint32_t> rb_nbest;
    pmx::DevBuf<unsigned long long> d_active;
    std::vector<uint8_t> h_active;
    // low-coverage masks (pmx_meta_set_masks; meta_mask.hip; src/mgsr.cpp:2049-2139): the thresholds the next set_reads applies
    // (at most one above 0), and of the last set_reads: whether it masked, the reference's three numbers, the distinct hashes
    // of the merged reads BEFORE masking (ascending) with their occurrence counts, and on the device the counts of the
    // surviving distinct hashes (one per entry of d_uniq)
    int64_t lowcov_reads = 0, lowcov_seeds = 0;
    bool masked = false;
    int64_t lowcov_reads_dropped = 0, lowcov_seeds_removed = 0, lowcov_reads_left = 0;
    std::vector<uint64_t> lowcov_hash;
    std::vector<int64_t> lowcov_count;
    pmx::DevBuf<int64_t> d_uniq_count;
    // amplicons (pmx_meta_set_amplicons / pmx_meta_set_relative_masks; src/mgsr.cpp:1216-1342, :2062-2075).  What the next
    // set_reads applies: amp_of_raw (the amplicon of every raw read, in [0, amp_n_groups], amp_n_groups = unlisted) and the
    // relative parameters.  Of the last set_reads when amp_on: n_amp = its groups + 1, the amplicon of every merged read
    // (survivors after a mask), per group its raw reads, threshold, merged reads before masking and left, and under a mask
    // the (group, hash, count) triples before masking, ascending
    bool amp_set = false;
    int32_t amp_n_groups = 0;
    std::vector<int32_t> amp_of_raw;
    double lowcov_reads_rf = 0.0, lowcov_seeds_rf = 0.0;
    bool amp_on = false;
    int32_t n_amp = 0;
    std::vector<int32_t> h_read_amp;
    std::vector<int64_t> amp_raw, amp_thr, amp_before, amp_left;
    std::vector<int32_t> ampc_group;
    std::vector<uint64_t> ampc_hash;
    std::vector<int64_t> ampc_count;
    // taxonomy (pmx_meta_set_taxonomy; max_taxa 0 = none) and the ambiguity thresholds (pmx_meta_set_ambiguous).  The node table:
    // the taxa S(v) of every node's subtree, ascending, max_taxa slots a node; h_tx_over: bit v = |S(v)| > max_taxa (then no ids)
    int32_t max_taxa = 0, amb_abs = 0;
    int64_t n_taxa = 0;
    double amb_ratio = 0.0;
    std::vector<uint8_t> h_tx_count;
    std::vector<uint32_t> h_tx_ids;
    std::vector<unsigned long long> h_tx_over;
    pmx::DevBuf<uint8_t> tx_count;
    pmx::DevBuf<uint32_t> tx_ids;
    pmx::DevBuf<unsigned long long> tx_over;
};

// how many of the four masking parameters are above 0: at most one may be ("Only one masking parameter ...", src/mgsr.cpp:2049-2053)
inline int meta_masks_above_zero(int64_t reads, int64_t seeds, double reads_rf, double seeds_rf) {
    return (reads > 0) + (seeds > 0) + (reads_rf > 0) + (seeds_rf > 0);
}

// The per-end trim the seeding kernels get for --mask-read-ends: a k-mer counts when it lies inside read[n : len - n], which
// is seeding the trimmed string.  The kernels' positions are 32-bit, so a read has fewer than 2^31 bases: a cut of 2^30 bases
// or more leaves nothing of any read, as 2^30 itself does, and len - trim - k stays inside an int.
inline int meta_read_end_trim(const pmx_meta* m) { return (int)std::min<int64_t>(m->mask_read_ends, (int64_t)1 << 30); }

// The plane count of the bit-sliced scoring kernels for a sample whose longest merged read has `longest` seedmers: launch is
// called with it as a compile-time constant, std::integral_constant<int, 7> (counts below 128) or <int, 16>.
template <class F>
inline void meta_with_planes(int64_t longest, F&& launch) {
    if (longest < 128) launch(std::integral_constant<int, 7>());
    else launch(std::integral_constant<int, 16>());
}

// This rank's rows of the merged reads: all of them, or (--gpus N) a balanced contiguous slice.  The rule of pmx_meta_score,
// which pmx_meta_assign and pmx_meta_read_best follow.  Leaves: m->row_first / row_count.
inline void meta_own_row_slice(pmx_meta* m) {
    m->row_first = 0;
    m->row_count = m->n_reads;
    if (m->dist) {
        const int64_t rank = pmx_dist_rank(m->dist), world = pmx_dist_world(m->dist);
        m->row_first = m->n_reads * rank / world;
        m->row_count = m->n_reads * (rank + 1) / world - m->row_first;
    }
}

// m->longest = the seedmers of the longest merged read; refused from 65,535 on (the scores are 16-bit)
inline int meta_longest_read(pmx_meta* m) {
    int64_t longest = 0;
    for (int64_t r = 0; r < m->n_reads; ++r) longest = std::max(longest, m->h_read_off[(size_t)r + 1] - m->h_read_off[(size_t)r]);
    if (longest >= 65535) return pmx::fail(PMX_ERR_UNSUPPORTED, "a read with 65,535 seedmers or more (16-bit scores)");
    m->longest = longest;
    return PMX_OK;
}

// meta_mask.hip, a step of pmx_meta_set_reads after the lists were uploaded.  False when no mask is set: m->masked cleared, no
// "meta_mask" span, nothing launched or allocated.  Else it counts every distinct hash of the merged reads, drops reads
// (lowcov_reads) or list entries (lowcov_seeds) whose count is at most the threshold and leaves m->h_* / d_* / n_reads /
// n_seedmers / h_raw_to_merged describing the survivors.  With amplicons (m->amp_on) the counts and the thresholds are per
// amplicon, and it also leaves h_read_amp, amp_thr, amp_left and the ampc_* triples.  Throws pmx::HipError.
bool meta_apply_masks(pmx_ctx* ctx, pmx_meta* m);
// ... and then the overlap coefficients of the survivors (m->oc), from the device arrays that step left; a place-API code
int meta_masked_overlap_coefficients(pmx_ctx* ctx, pmx_meta* m);
// api_meta.hip, the tail both overlap-coefficient paths share once the placer's histogram is loaded (`rc`: how loading it
// went; not PMX_OK: returned as it is): the tree scored with every read seed kept and n_kept reads, the per-node counts,
// m->oc = intersection / genome seeds.  `seeded`, when given, is the read set the histogram was seeded from: released as soon
// as the tree is scored, however that went.
int meta_overlap_from_histogram(pmx_ctx* ctx, pmx_meta* m, int rc, int64_t n_kept, std::unique_ptr<pmx_readset>* seeded);
