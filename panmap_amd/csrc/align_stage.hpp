// ALIGN stage, private to its translation units: the aligner's state and what align_stage.hip (the tiers of one call),
// align_pairs.hip (what depends on the reads alone, and the fan-out) and api_align.hip (the C ABI) share.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "align_kernel.h"
#include "align_kernel_dpg.h"
#include "device/dev_util.hpp"
#include "readset.hpp"
#include "ref_index_device.h"

struct pmx_aligner {
    pmx::aln::Opt opt;
    pmx::aln::HostRefIndex host;
    pmx::DevBuf<uint8_t> d_seq;
    pmx::DevBuf<uint64_t> d_pos;
    pmx::DevBuf<pmx::aln::HtEnt> d_ht;
    pmx::DevBuf<float> d_logf_ratio, d_logf_int;
    pmx::DevBuf<uint64_t> d_pk, d_pk_amb;
    pmx::DevBuf<uint32_t> d_ht_pv;
    pmx::aln::RefIndexDevice dev_index;   // the index when it was built on the device (set_reference)
    bool logf_uploaded = false;
    pmx::aln::RefIndex ri;
    int mean_len = 150;
    // last result
    pmx::DevBuf<pmx::aln::AlnRecord> records;
    pmx::DevBuf<uint32_t> cigars;
    pmx::DevBuf<unsigned long long> cigar_used;
    pmx::DevBuf<uint8_t> slow, slow2, slab0, slab_raw;
    pmx::DevBuf<pmx::aln::A128> mv_handover;
    uint32_t mv_epoch = 0;
    pmx::DevBuf<uint32_t> retry_list2, bail_list;
    pmx::DevBuf<uint32_t> cseeds;            // compact tier, two-kernel form: seed hand-over (AlignArgs::cseeds / cseed_n)
    pmx::DevBuf<uint16_t> cseed_n;
    pmx::DevBuf<uint32_t> multi_list;        // compact tier, second form (several regions per mate): launch positions + counters
    pmx::DevBuf<unsigned long long> multi_count;
    pmx::DevBuf<uint32_t> multi_ws;
    pmx::DevBuf<uint32_t> simple_list;       // compact tier: the two class lists of launch positions (AlignArgs::simple_list)
    pmx::DevBuf<uint8_t> dp_req;
    pmx::DevBuf<pmx::aln::DpRes> dp_res;
    pmx::DevBuf<uint32_t> dp_ncached, dp_slot_pairs, dp_list_a, dp_list_b;
    pmx::DevBuf<uint32_t> dpg_keys, dpg_keys2, dpg_ids, dpg_ids2, dpg_counts;   // grouped DP service (align_kernel_dpg.hip)
    pmx::DevBuf<char> dpg_tmp;
    pmx::DevBuf<uint8_t> dpg_tb;
    pmx::DevBuf<unsigned long long> dpg_prof;
    int64_t last_dp_requests = 0;
    int last_dp_rounds = 0;
    pmx::DevBuf<uint32_t> retry_list;
    pmx::DevBuf<unsigned long long> retry_count;
    int64_t last_retry = 0, last_tpp_retry = 0, last_huge = 0;
    pmx::DevBuf<unsigned long long> prof;
    pmx::DevBuf<unsigned long long> stats;   // AlignArgs::stats
    pmx::DevBuf<unsigned long long> dd_count;   // distinct-pair map counters (align_readset_once)
    pmx::DevBuf<uint32_t> dd_list;           // representatives in launch order
    pmx::DevBuf<char> dd_tmp;
    pmx::DevBuf<int32_t> edits;              // AlignArgs::edits while pmx_align_score_reads runs
    bool want_edits = false;
    pmx_align_stats last_stats;
    int64_t last_dp_slots = 0, last_compact = 0, last_simple = 0, last_near = 0;
    int64_t n_records = 0;
    uint64_t cigar_cap = 0;
    size_t dev_total_mem = 0;            // hipMemGetInfo total, asked once
    double cigar_words_per_kbase = 0.0;   // CIGAR words per 1,000 read bases the last calls needed (sizes the next arena)
    unsigned long long last_cigar_used = 0;   // read back at the end of pmx_align_readset
    double last_occupancy = 0;
    hipEvent_t ev_results = nullptr, ev_fetched = nullptr;   // pmx_align_fetch_async: results ready / download finished
    bool fetch_pending = false;
};

namespace pmx {

// align_stage.hip: one attempt of pmx_align_readset with a CIGAR arena of `cigar_cap` words (the caller redoes an overflow)
int align_readset_once(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, int paired, int revcomp_mate2, uint64_t cigar_cap, bool allow_dedup);
// align_stage.hip: the grouped DP service (align_kernel_dpg.hip), shared with pmx_align_dp_batch
constexpr int kDpgWavesDefault = 8;   // its waves per CU unless PMX_ALIGN_DPG_WAVES says otherwise
bool dpg_setup(const aln::Opt& o, aln::DpgArgs& DG);
void dpg_launch(pmx_ctx* ctx, pmx_aligner* al, aln::DpgArgs& DG, int64_t n_slots, const uint32_t* worklist, int waves_per_cu, bool serve);

// align_stage.hip: the wave DP service (k_align_dp_serve), its two classes: everything else (dp) / register DP (dps).  One
// planner and one launch function for AlignStage::dp_round and pmx_align_dp_probe.
struct DpServePlan {
    static constexpr int kSmallQlen = 192, kSmallTlen = 192;   // the small class (ksw_extd2_reg<3>: up to three target columns per lane)
    aln::Layout dp_layout, dps_layout;
    size_t dp_lds = 0, dp_stride = 0, dps_lds = 0, dps_stride = 0;
    int64_t dp_max_grid = 0, dps_max_grid = 0;
};
DpServePlan plan_dp_serve(const pmx_ctx* ctx, int max_read_len, int n_segs, const aln::Opt& o);
// A: the base arguments with dp_req_base / dp_res_base / n_items / worklist set; slow / slow2: the two classes' slabs
// (dp_stride x grid, dps_stride x grid bytes).  two_class false: one launch with dp_class = 0.
void launch_dp_serve(aln::AlignArgs A, const DpServePlan& P, bool two_class, uint8_t* slow, uint8_t* slow2, hipStream_t stream);
// the layouts of the wave-per-read launches: AlignStage::setup's `general`, AlignStage::long_reads' first launch
aln::Layout plan_general_layout(int max_read_len, int n_segs, const aln::Opt& o);
aln::Layout plan_long_reads_layout(int max_read_len, int n_segs, const aln::Opt& o, bool no_dp_fast);
// align_stage.hip: pmx_align_dp_probe behind its argument checks (include/panmap_amd.h)
int align_dp_probe(pmx_ctx* ctx, pmx_aligner* al, int path, int max_read_len, int n_segs, int no_rows_dp, int no_dp_fast, const uint8_t* seqs,
                   const int64_t* q_off, const int64_t* t_off, int64_t n, const int32_t* w, const int32_t* zdrop, const int32_t* end_bonus,
                   const int32_t* flag, pmx_dp_probe_result* out, uint32_t* cigar_arena, int64_t arena_cap, pmx_dp_probe_caps* caps);

// align_stage.hip: pmx_align_chain_probe behind its argument checks (include/panmap_amd.h)
int align_chain_probe(pmx_ctx* ctx, pmx_aligner* al, int path, int op, int max_read_len, int n_segs, pmx_chain_probe_params* par, const uint64_t* anchors,
                      const int64_t* a_off, const int32_t* qlen, int64_t n, pmx_chain_probe_result* out, uint64_t* out_anchors, uint64_t* out_u,
                      pmx_chain_probe_caps* caps);

// align_pairs.hip (readset_pair_order / readset_pair_map: readset.hpp)
// the representatives of the distinct-pair map in launch order (`order`, nullptr = input order) -> al->dd_list; their number
int64_t pair_select_reps(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, const uint32_t* order, int64_t n_pairs);
// al->dd_count[2] += the copies the representatives list[0 .. *n_list) stand for (n_launch bounds the list: sizes the grid)
void pair_count_copies(pmx_ctx* ctx, pmx_aligner* al, const uint32_t* list, const unsigned long long* n_list, const uint32_t* mult, int64_t n_launch);
// every tier is through: the copies take their representatives' records, edit counts (edits may be NULL) and CIGAR words
void pair_fanout(pmx_ctx* ctx, pmx_aligner* al, const uint32_t* rep, int64_t n_pairs, int32_t* edits);

}  // namespace pmx
