// ALIGN stage: the host code of one call -- which tier runs which pairs, in which order, with which launch arguments.
// The kernels are in align_kernel*.hip; what depends on the reads alone (pair order, distinct-pair map) in align_pairs.hip.
#include <hip/hip_runtime.h>

#include <string.h>

#include <rocprim/rocprim.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>

#include "align/aln_compact_defs.hpp"
#include "align_stage.hpp"

using namespace pmx;
using namespace pmx::aln;

namespace pmx {
// Grouped DP service (align_kernel_dpg.hip): scoring parameters for the kernel; false = the parameters leave the range in which
// plain 32-bit arithmetic stands for the reference's int8 lanes (no preset does): the wave service then takes everything
bool dpg_setup(const Opt& o, DpgArgs& DG) {
    memset(&DG, 0, sizeof(DG));
    bool ok = true;
    int q = o.q, e = o.e, q2 = o.q2, e2 = o.e2;
    if (q2 + e2 < q + e) { std::swap(q, q2); std::swap(e, e2); }
    int min_sc = o.mat[1], max_abs = 0;
    for (int t = 0; t < 25; ++t) { if (t >= 1) min_sc = std::min<int>(min_sc, o.mat[t]); max_abs = std::max(max_abs, std::abs((int)o.mat[t])); }
    if (-min_sc > 2 * (q + e)) ok = false;   // (ksw2_extd2_sse.c:100: the reference returns without aligning)
    if (2 * (q2 + e2) + 2 * max_abs > 100 || q < 0 || e < 0 || q2 < 0 || e2 < 0) ok = false;
    DG.q = q; DG.e = e; DG.q2 = q2; DG.e2 = e2;
    DG.sc_mch = o.mat[0]; DG.sc_mis = o.mat[1]; DG.sc_N = o.mat[24] == 0 ? -e2 : o.mat[24];
    int long_thres = e != e2 ? (q2 - q) / (e - e2) - 1 : 0;
    if (q2 + e2 + long_thres * e2 > q + e + long_thres * e) ++long_thres;
    DG.long_thres = long_thres;
    DG.long_diff = long_thres * (e - e2) - (q2 - q) - e2;
    return ok;
}

// collect the requests of `n_slots` slots, order them by (columns per lane, kind, query length), serve them eight per wave
void dpg_launch(pmx_ctx* ctx, pmx_aligner* al, DpgArgs& DG, int64_t n_slots, const uint32_t* worklist, int waves_per_cu, bool serve) {
    const int64_t n_ent = n_slots * PMX_DP_REQ_PER_PASS;
    al->dpg_keys.ensure((size_t)n_ent); al->dpg_keys2.ensure((size_t)n_ent); al->dpg_ids.ensure((size_t)n_ent); al->dpg_ids2.ensure((size_t)n_ent);
    al->dpg_counts.ensure(16);
    const int64_t grid = std::min<int64_t>((int64_t)ctx->n_cu * waves_per_cu, (n_ent + 7) / 8 + PMX_DPG_BUCKETS);
    al->dpg_tb.ensure((size_t)grid * PMX_DPG_TB_BYTES);   // a traceback window per launched wave (not per wave the chip could hold: --refine keeps an aligner per worker)
    DG.worklist = worklist; DG.n_slots = n_slots;
    DG.keys = al->dpg_keys.p; DG.ids = al->dpg_ids.p; DG.sorted_ids = al->dpg_ids2.p; DG.counts = al->dpg_counts.p;
    DG.tb = al->dpg_tb.p;
    if (!DG.dp_req_base || !DG.dp_res_base) throw std::runtime_error("grouped DP service: a buffer is missing");
    PMX_ZERO(al->dpg_counts, 16, ctx->stream);
    PMX_LAUNCH(k_dpg_collect, dim3((unsigned)std::min<int64_t>((n_ent + 255) / 256, (int64_t)ctx->n_cu * 8)), dim3(256), 0, ctx->stream, DG);
    PMX_ROCPRIM(al->dpg_tmp, radix_sort_pairs, al->dpg_keys.p, al->dpg_keys2.p, al->dpg_ids.p, al->dpg_ids2.p, (size_t)n_ent, 0, 12, ctx->stream);
    if (serve) PMX_LAUNCH(k_align_dp_group, dim3((unsigned)grid), dim3(64), PMX_DPG_LDS_BYTES, ctx->stream, DG);
}

// The wave DP service's layouts, LDS bytes, slab strides and resident grids
DpServePlan plan_dp_serve(const pmx_ctx* ctx, int max_read_len, int n_segs, const Opt& o) {
    DpServePlan P;
    P.dp_layout = plan_layout_dp(max_read_len, n_segs, o);
    P.dp_lds = PMX_ALIGN_WORK_BYTES + P.dp_layout.fast_bytes + 16;
    P.dp_stride = (P.dp_layout.slow_bytes + 255) & ~(size_t)255;
    P.dp_max_grid = (int64_t)ctx->n_cu * (int64_t)std::min<size_t>(16, (size_t)(160 * 1024) / P.dp_lds);
    P.dps_layout = plan_layout_dp(max_read_len, n_segs, o, DpServePlan::kSmallQlen, DpServePlan::kSmallTlen);
    P.dps_lds = PMX_ALIGN_WORK_BYTES + P.dps_layout.fast_bytes + 16;
    P.dps_max_grid = (int64_t)ctx->n_cu * (int64_t)std::min<size_t>(16, (size_t)(160 * 1024) / P.dps_lds);
    P.dps_stride = (P.dps_layout.slow_bytes + 255) & ~(size_t)255;
    return P;
}

// k_align_dp_serve reads, beyond the base: dp_req_base / dp_res_base, layout, slow_base / slow_stride, n_items, worklist,
// dp_class, dp_small_qlen / dp_small_tlen / dp_small_tb, and dp_left (null: it always looks at every entry).
void launch_dp_serve(AlignArgs A, const DpServePlan& P, bool two_class, uint8_t* slow, uint8_t* slow2, hipStream_t stream) {
    const int64_t n_dp = A.n_items;
    A.dp_small_qlen = DpServePlan::kSmallQlen; A.dp_small_tlen = DpServePlan::kSmallTlen;
    A.dp_small_tb = (uint32_t)P.dps_layout.tb_cap;
    A.layout = P.dp_layout;
    A.slow_stride = P.dp_stride;
    A.slow_base = slow;
    A.dp_class = two_class ? 2 : 0;
    // (tier 0 runs for the short-read preset only; with max_gap of a long-read preset the arrays of this class exceed the LDS of a
    //  CU and pmx_align_dp_probe is left with the small class)
    if (P.dp_max_grid > 0)
        PMX_LAUNCH(k_align_dp_serve, dim3((unsigned)std::min<int64_t>(P.dp_max_grid, n_dp * PMX_DP_REQ_PER_PASS)), dim3(64), P.dp_lds, stream, A);
    if (two_class) {
        A.layout = P.dps_layout;
        A.slow_stride = P.dps_stride;
        A.slow_base = slow2;
        A.dp_class = 1;
        PMX_LAUNCH(k_align_dp_serve, dim3((unsigned)std::min<int64_t>(P.dps_max_grid, n_dp * PMX_DP_REQ_PER_PASS)), dim3(64), P.dps_lds, stream, A);
    }
}
}  // namespace pmx

namespace {

// Every switch the stage reads (device/pmx_options.hpp), parsed here and nowhere below.
struct AlignSwitches {
    static bool on(OptId id) { return pmx::opt_str(id) != nullptr; }
    const bool no_tpp = on(O_ALIGN_NO_TPP), no_compact = on(O_ALIGN_NO_COMPACT), no_dedup = on(O_ALIGN_NO_DEDUP);
    const bool compact_pos32 = on(O_ALIGN_COMPACT_POS32), compact_fused = on(O_ALIGN_COMPACT_FUSED), no_multi = on(O_ALIGN_NO_MULTI), no_simple = on(O_ALIGN_NO_SIMPLE), no_near = on(O_ALIGN_NO_NEAR);
    const bool prof = on(O_ALIGN_PROF), verbose = on(O_ALIGN_VERBOSE);                                                    // diagnostics
    const bool dp_hist = on(O_DP_HIST), dpg_prof = on(O_DPG_PROF);
    int waves_per_simd = 4;
    int tpp_waves = 16;                 // 4 per SIMD: what k_align_reads_tpp's register allocation targets (PMX_TPP_OCC)
    int dpg_waves = kDpgWavesDefault;
    int compact_waves = 0, cseed_waves = 0;   // waves per CU of a resident grid; 0 = one workgroup per 64 pairs
    int test_max_cigar = 0;             // test hook: cap the CIGAR operations per region in EVERY tier, so that gapped alignments overflow and
                                        // the boundary's handling of invalid records can be exercised (tests/test_align_gpu.py)
    size_t lds_budget = 24 * 1024, lr_lds_budget = 8900;   // wave tiers: short reads / long reads (one switch sets both)
    size_t slab_budget = 0;             // tests: force a small grid; 0 = a third of the device memory
    const size_t tpp_tb = 0;            // in-lane DPs measured slower than request + replay (divergence): off, and no switch for it any more
    size_t tb_small = (size_t)8 << 20;  // long reads: traceback per wave of the first launch
    int64_t small_rounds = 8192, bail_tpp_min = 4096, dpg_left_few = 256;
    double dedup_depth = 64.0;
    AlignSwitches() {
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_LDS_KB)) lds_budget = lr_lds_budget = (size_t)atoi(e) * 1024;
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_WAVES)) waves_per_simd = atoi(e);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_SLAB_MB)) slab_budget = (size_t)std::max<long long>(atoll(e), 1) << 20;
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_TEST_MAX_CIGAR)) test_max_cigar = atoi(e);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_TPP_WAVES)) tpp_waves = atoi(e);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_TPP_MIN)) small_rounds = atoll(e);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_DPG_WAVES)) dpg_waves = std::max(1, atoi(e));
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_BAIL_TPP_MIN)) bail_tpp_min = atoll(e);
        if (const char* e = pmx::opt_str(pmx::O_DPG_LEFT_TO_WAVE_TIER)) dpg_left_few = atoll(e);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_DEDUP_DEPTH)) dedup_depth = atof(e);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_COMPACT_WAVES)) compact_waves = std::max(atoi(e), 1);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_CSEED_WAVES)) cseed_waves = std::max(atoi(e), 1);
        if (const char* e = pmx::opt_str(pmx::O_ALIGN_TB_KB)) tb_small = std::max<size_t>((size_t)atoll(e), 1) << 10;
    }
};

}  // namespace

namespace pmx {
// general capacities (AlignStage::setup) / the first launch of the long reads (AlignStage::long_reads: small LDS budget, 8 MB of
// traceback per wave, the dp_fast LDS copy of the DP arrays)
Layout plan_general_layout(int max_read_len, int n_segs, const Opt& o) {
    const AlignSwitches sw;
    return plan_layout(max_read_len, n_segs, o, sw.lds_budget);
}
Layout plan_long_reads_layout(int max_read_len, int n_segs, const Opt& o, bool no_dp_fast) {
    const AlignSwitches sw;
    return plan_layout(max_read_len, n_segs, o, sw.lr_lds_budget, sw.tb_small, 1, no_dp_fast ? 0 : PMX_DP_FAST_TLEN);
}
}  // namespace pmx

namespace {

typedef void (*AlignKernel)(AlignArgs);

// One call of the stage.  `base` holds what every launch of the call shares; a launch function copies it, sets the fields its
// kernel reads (listed above each function) and launches: no launch depends on what another one left in the arguments.
struct AlignStage {
    pmx_ctx* const ctx;
    pmx_aligner* const al;
    const pmx_readset* const rs;
    const hipStream_t stream;   // everything is enqueued here
    const AlignSwitches sw;
    const bool paired, allow_dedup;
    const int64_t n_items;      // an odd trailing read is ignored (src/mm_align.c:372)
    const int n_segs;
    const AlignKernel kern, kern_t1;
    AlignArgs base{};           // reads, reference, options, outputs, stats / edits / prof, paired, revcomp_mate2, the first mv_epoch
                                // of the call, and (plan_tier0) the thread-per-pair arena; every other field zero
    Layout general, compact;    // wave tiers: general capacities; all-LDS layout (typical short-read pairs)
    // thread-per-pair tier and its DP service (plan_tier0)
    Layout tpp_layout;
    DpServePlan dpp;            // the wave service's two classes
    size_t tpp_raw_stride = 0, tpp_lds_bytes = 0;
    int64_t tpp_max_grid = 0;
    bool use_compact = false, dpg_ok = false;
    DpgArgs dpg_base;           // scoring parameters of the grouped service (dpg_setup)
    // launch order (launch_order)
    bool dedup = false;         // distinct-pair map in use: the compact tier and the tail run representatives only
    int64_t n_launch = 0;

    AlignStage(pmx_ctx* c, pmx_aligner* a, const pmx_readset* r, int paired_, bool allow_dedup_)
        : ctx(c), al(a), rs(r), stream(c->stream), paired(paired_ != 0), allow_dedup(allow_dedup_), n_items(paired_ ? r->n / 2 : r->n),
          n_segs(paired_ ? 2 : 1), kern(sw.waves_per_simd >= 4 ? k_align_reads_w4 : k_align_reads),
          kern_t1(sw.waves_per_simd >= 4 ? k_align_reads_t1_w4 : k_align_reads_t1) {}

    Layout hooked(Layout L) const { if (sw.test_max_cigar > 0 && L.caps.max_cigar > sw.test_max_cigar) L.caps.max_cigar = sw.test_max_cigar; return L; }
    bool setup(int revcomp_mate2, uint64_t cigar_cap);
    void launch_wave(AlignArgs A, AlignKernel kfn, const Layout& L, int64_t n_work, const uint32_t* worklist, uint32_t* retry_list, DevBuf<uint8_t>& slab, int64_t max_grid = 0);
    void read_counts(int64_t& n_next_tier, int64_t& n_dp, bool reset_next_tier);
    void wave_tiers(int64_t n_t1, const uint32_t* t1_list);
    void long_reads();
    void plan_tier0();
    const uint32_t* launch_order();
    int64_t compact_tier(const uint32_t* order);
    AlignArgs tail_args();
    void launch_tpp(const AlignArgs& T, int round, int64_t n_work, const uint32_t* worklist, uint32_t* next_list, const uint32_t* pair_perm);
    void dp_round(const AlignArgs& T, int round, int64_t n_dp, const uint32_t* cur, uint32_t* next);
    void tail(const uint32_t* order, int64_t n_t0);
    // diagnostics (each behind its switch: they download and print)
    void print_dp_requests(int round, int64_t n_dp);
    void print_dpg_prof();
    void print_compact_prof();
    void print_phase_prof(bool tier1_fits);
};

// The resets of a call, each once: result buffers, device counters, the aligner's last_* counters; then the base arguments
// and the wave tiers' layouts.  false = the read set is empty (the counters are read back after such a call too: a rank
// whose shard holds no read).
bool AlignStage::setup(int revcomp_mate2, uint64_t cigar_cap) {
    if (al->fetch_pending) {   // a download of the previous results on another stream (pmx_align_fetch_async) reads the buffers this call overwrites
        PMX_HIP(hipStreamWaitEvent(stream, al->ev_fetched, 0));
        al->fetch_pending = false;
    }
    al->n_records = rs->n;
    al->records.ensure((size_t)std::max<int64_t>(rs->n, 1));
    PMX_ZERO(al->records, (size_t)std::max<int64_t>(rs->n, 1), stream);
    al->cigar_cap = cigar_cap;
    al->cigars.ensure(al->cigar_cap);
    PMX_ZERO(al->cigar_used, 1, stream);
    al->stats.ensure(4);
    PMX_ZERO(al->stats, 4, stream);
    al->dd_count.ensure(4);   // distinct-pair map: [0] representatives, [1] copies of an arena-overflowed representative, [2] copies of bails
    PMX_ZERO(al->dd_count, 4, stream);
    al->last_dp_slots = 0; al->last_compact = 0; al->last_simple = 0; al->last_near = 0; al->last_tpp_retry = 0; al->last_retry = 0; al->last_huge = 0; al->last_dp_rounds = 0; al->last_dp_requests = 0;
    memset(&al->last_stats, 0, sizeof(al->last_stats));
    if (n_items <= 0) return false;
    al->last_stats.n_items = n_items;
    if (sw.prof) {
        al->prof.ensure(32);
        PMX_ZERO(al->prof, 32, stream);
    }
    al->retry_count.ensure(4);   // [0] pairs for the next (wave) tier, [1] DP requests of the current tier-0 round, [2] compact-tier bails, [3] long reads: work queue
    PMX_ZERO(al->retry_count, 4, stream);
    if (al->want_edits) al->edits.ensure((size_t)std::max<int64_t>(rs->n, 1));

    base.words = rs->words.p; base.amb = rs->amb.p; base.woff = rs->woff.p; base.off = rs->off.p;
    base.recs = rs->has_recs && rs->packed ? rs->recs.p : nullptr;
    base.paired = paired ? 1 : 0;
    base.revcomp_mate2 = revcomp_mate2 ? 1 : 0;
    base.opt = al->opt;
    base.ri = al->ri;
    base.records = al->records.p;
    base.cigars = al->cigars.p;
    base.cigar_cap = al->cigar_cap;
    base.cigar_used = al->cigar_used.p;
    base.stats = al->stats.p;
    base.edits = al->want_edits ? al->edits.p : nullptr;
    base.prof = sw.prof ? al->prof.p : nullptr;
    base.mv_epoch = ++al->mv_epoch;
    general = hooked(plan_general_layout((int)rs->max_len, n_segs, al->opt));
    compact = hooked(plan_layout_compact((int)rs->max_len, n_segs, al->opt));
    return true;
}

// Wave-per-item kernels (k_align_reads*: align_kernel_body.hpp).  They read, beyond the base: layout, slow_base / slow_stride,
// n_items, worklist, retry_list / retry_count (set here); work_queue, dp_slot_pairs, mv_handover / mv_stride / mv_slots /
// mv_epoch (the caller's A: null in `base`); dp_req_base, which only keys which profile slots are added and is null in
// every launch of these kernels.
void AlignStage::launch_wave(AlignArgs A, AlignKernel kfn, const Layout& L, int64_t n_work, const uint32_t* worklist, uint32_t* retry_list,
                             DevBuf<uint8_t>& slab, int64_t max_grid) {
    const size_t lds_bytes = PMX_ALIGN_WORK_BYTES + L.fast_bytes + 16;
    if (sw.verbose) fprintf(stderr, "[pmx align] wave-tier launch: %lld items, %zu LDS bytes per wave, %zu HBM slab bytes per wave\n", (long long)n_work, lds_bytes, (size_t)L.slow_bytes);
    if (lds_bytes > 160 * 1024) throw std::runtime_error("reads too long for the LDS work arena");
    if (lds_bytes > 64 * 1024) PMX_HIP(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int waves_per_cu = (int)std::min<size_t>((size_t)(sw.waves_per_simd >= 4 ? 16 : 8), (size_t)(160 * 1024) / lds_bytes);
    if (waves_per_cu < 1) waves_per_cu = 1;
    int64_t grid = (int64_t)ctx->n_cu * waves_per_cu;
    // a few thousand pairs: one workgroup each, so that the hardware hands a free slot the next pair (with a resident
    // grid and a strided loop a wave that drew two slow pairs decides the launch)
    if (n_work <= 16384) grid = n_work;
    if (grid > n_work) grid = n_work;
    if (max_grid > 0 && grid > max_grid) grid = max_grid;
    A.layout = L;
    A.slow_stride = (L.slow_bytes + 255) & ~(size_t)255;
    // every workgroup owns a slab (long reads: ~20 MB each, 8 MB of it traceback): the grid is what a third of the
    // device memory -- at most 96 GB -- pays for (10 kb reads: 4,096 waves = 82 GB, the resident set of the chip);
    // the kernel strides over the items with whatever grid it gets
    if (al->dev_total_mem == 0) {
        size_t free_b = 0, total_b = 0;
        PMX_HIP(hipMemGetInfo(&free_b, &total_b));
        al->dev_total_mem = total_b;
    }
    size_t budget = std::max<size_t>(std::min<size_t>((size_t)96 << 30, al->dev_total_mem / 3), slab.n * sizeof(uint8_t));
    if (sw.slab_budget) budget = sw.slab_budget;
    const int64_t fit = (int64_t)(budget / std::max<size_t>(A.slow_stride, 1));
    if (grid > fit) grid = std::max<int64_t>(fit, 1);
    slab.ensure(A.slow_stride * (size_t)grid);
    A.slow_base = slab.p;
    A.n_items = n_work;
    A.worklist = worklist;
    A.retry_list = retry_list;
    A.retry_count = al->retry_count.p;
    PMX_LAUNCH(kfn, dim3((unsigned)grid), dim3(64), lds_bytes, stream, A);
}

// reads both counters; [1] is reset for the next round, [0] only when asked
void AlignStage::read_counts(int64_t& n_next_tier, int64_t& n_dp, bool reset_next_tier) {
    unsigned long long h[2] = {0, 0};
    PMX_D2H_SYNC(h, al->retry_count, stream);
    PMX_ZERO(pmx::at(al->retry_count, reset_next_tier ? 0 : 1), reset_next_tier ? 2 : 1, stream);
    n_next_tier = (int64_t)h[0];
    n_dp = (int64_t)h[1];
}

// The wave-per-pair tiers over a list of pairs (nullptr: every item): compact layout, then general capacities for what
// overflowed it; what overflows even those (a mate whose every minimizer hits a long repeat: hundreds of anchors per
// minimizer) runs once more with 16x the anchors (the chain cells index anchors with 16 bits), a few waves with their
// arrays in HBM.
void AlignStage::wave_tiers(int64_t n_t1, const uint32_t* t1_list) {
    int64_t n_retry = 0, unused = 0;
    if (n_t1 > 0) {
        launch_wave(base, kern_t1, compact, n_t1, t1_list, al->retry_list.p, al->slow);
        read_counts(n_retry, unused, true);
    }
    al->last_retry += n_retry;
    if (n_retry > 0) {
        launch_wave(base, kern, general, n_retry, al->retry_list.p, al->retry_list2.p, al->slow2);
        int64_t n_huge = 0;
        read_counts(n_huge, unused, true);
        al->last_huge += n_huge;
        if (n_huge > 0) {
            const Layout huge = hooked(plan_layout((int)rs->max_len, n_segs, al->opt, sw.lds_budget, 0, 16));
            launch_wave(base, kern, huge, n_huge, al->retry_list2.p, nullptr, al->slow2, 64);
        }
    }
}

// Long reads (map-ont / map-hifi branch): wave per read with the general capacities.  The band of those presets
// allows traceback matrices up to max_sw_mat bytes (100 MB) although nearly every DP between two anchors is a few
// hundred bases wide: the first launch gives every wave 8 MB of traceback in HBM, the reads that need more come
// back on the retry list and run in a second launch of few waves with the full capacity.
void AlignStage::long_reads() {
    // The arrays of a 10 kb read (anchors, chain cells, the DP arrays sized for the longest allowed target) live in the
    // wave's HBM slab whatever the LDS budget, and the kernel is bound by the latency of those accesses: what counts is
    // resident waves (16 per CU: 32.4 k reads/s, 8 per CU: 21.1 k) and that the DPs -- nearly all a few hundred bases
    // wide -- run on a small LDS copy of their arrays (plan_layout dp_fast_tlen)
    const Layout g1 = hooked(plan_long_reads_layout((int)rs->max_len, n_segs, al->opt, false));
    al->retry_list.ensure((size_t)n_items);
    timer_begin(ctx, "align_dom");
    AlignArgs A = base;
    PMX_ZERO(pmx::at(al->retry_count, 3), 1, stream);   // the waves draw their reads from a counter
    A.work_queue = al->retry_count.p + 3;
    launch_wave(A, kern, g1, n_items, nullptr, general.tb_cap > g1.tb_cap ? al->retry_list.p : nullptr, al->slow2);
    timer_end(ctx, "align_dom", 1);
    int64_t n_retry = 0, unused = 0;
    read_counts(n_retry, unused, true);
    al->last_retry = n_retry;
    if (n_retry > 0) {
        const size_t stride = (general.slow_bytes + 255) & ~(size_t)255;
        const int64_t big_grid = std::max<int64_t>(1, std::min<int64_t>(64, (int64_t)(((size_t)24 << 30) / std::max<size_t>(stride, 1))));
        launch_wave(base, kern, general, n_retry, al->retry_list.p, nullptr, al->slow, big_grid);
    }
}

// Tier 0 (thread per pair + DP service rounds): layouts, grids and buffers.  The thread-per-pair arena (AlignArgs::tpp) goes
// into the base arguments: the compact tier's and the thread-per-pair kernels are compiled to address through it.
void AlignStage::plan_tier0() {
    tpp_max_grid = std::min<int64_t>((int64_t)ctx->n_cu * sw.tpp_waves, (n_items + 63) / 64);
    // thread-per-pair layout: interleaved arena per wave + a small contiguous struct region per thread
    tpp_layout = hooked(plan_layout_tpp((int)rs->max_len, n_segs, al->opt, sw.tpp_tb));
    const size_t tpp_wave_stride = tpp_arena_bytes(tpp_layout) * 64;
    tpp_raw_stride = (tpp_layout.raw_bytes + 255) & ~(size_t)255;
    al->slab0.ensure(tpp_wave_stride * (size_t)tpp_max_grid);
    al->slab_raw.ensure(tpp_raw_stride * (size_t)tpp_max_grid);   // per wave
    if (tpp_wave_stride > UINT32_MAX) throw std::runtime_error("thread-per-pair arena stride exceeds 32 bits");
    base.tpp.base = al->slab0.p;
    base.tpp.wave_stride = (uint32_t)tpp_wave_stride;
    dpp = plan_dp_serve(ctx, (int)rs->max_len, n_segs, al->opt);
    dpg_ok = dpg_setup(al->opt, dpg_base);
    al->dp_req.ensure((size_t)n_items * PMX_DP_REQ_PER_PASS * sizeof(DpReq));
    al->dp_res.ensure((size_t)n_items * PMX_DP_MAX_CALLS);
    al->dp_ncached.ensure((size_t)n_items);
    al->dp_slot_pairs.ensure((size_t)n_items);
    al->dp_list_a.ensure((size_t)n_items);
    al->dp_list_b.ensure((size_t)n_items);
    al->slow.ensure(dpp.dp_stride * (size_t)dpp.dp_max_grid);
    al->slow2.ensure(dpp.dps_stride * (size_t)dpp.dps_max_grid);
    al->mv_handover.ensure((size_t)std::min<int64_t>(std::min<int64_t>(n_items, UINT32_MAX - 1), 131072) * ((size_t)tpp_layout.caps.max_mini + 1u));
    // minimizer window ring in LDS when 16 waves per CU still fit (12 B x w x 64 lanes per wave)
    tpp_lds_bytes = (size_t)al->opt.w * 64 * 12;
    if (tpp_lds_bytes * (size_t)sw.tpp_waves > (size_t)150 * 1024) tpp_lds_bytes = 0;
}

// Launch order of the first pass: pairs sorted by a locality key; with the compact tier and enough depth, the
// representatives of the distinct pairs in that order (sets n_launch and dedup).  nullptr = input order.
const uint32_t* AlignStage::launch_order() {
    // the read set's locality order (shared with the seeding stage)
    const uint32_t* read_order = readset_locality_order(ctx, rs);
    const uint32_t* order = nullptr;
    if (read_order && !paired) order = read_order;
    // pairs by (key of mate 1, key of mate 2): the 64 pairs of a wave then start AND end within a few bases
    // of each other -- same anchors, same overlap of the mates, same trip counts in every per-lane loop
    // (round 3, 10M reads: k_align_compact16 28.2 -> 25.0 ms against the order by mate 1 alone; the extra
    // 64-bit sort of the pairs is ~1 ms of that)
    // (made ahead of time by pmx_readset_order_pairs when the host asked for it: then only an event to wait for)
    else if (read_order) order = readset_pair_order(ctx, rs, nullptr);
    // Distinct pairs (readset_pair_map): the compact tier and the tail run one representative of every set of equal
    // pairs, in launch order, and k_pair_fanout hands the copies their results at the end (10M bench reads: 18 % of
    // the pairs are copies).  PMX_ALIGN_NO_DEDUP: every pair.
    // Copies are many only at depth: the bench workload at 10M reads (167 pairs per reference base) has 18 %, at
    // 1.25M reads (21 per base) a few percent, which do not repay the map's launches and its host round trip --
    // measured 6.6 -> 6.9 ms per step there.  Below PMX_ALIGN_DEDUP_DEPTH pairs per reference base (default 64)
    // every pair runs itself.
    n_launch = n_items;
    dedup = use_compact && allow_dedup && base.recs && !sw.no_dedup && (double)n_items >= sw.dedup_depth * (double)al->ri.len;
    if (dedup) {
        n_launch = pair_select_reps(ctx, al, rs, order, n_items);
        order = al->dd_list.p;
    }
    return order;
}

// Compact tier (align_kernel_compact.hip): every pair of the launch order first, work state in LDS; what it cannot finish
// comes back as the bail list (al->bail_list), which is the launch order of the tail.  -> the length of that list.
// Its kernels read, beyond the base: n_items, pair_perm, retry_list / retry_count (the bail list), cseeds / cseed_n,
// multi_list / multi_count (chain kernel and second form), multi_ws (second form), simple_list (seeds and chain kernels).
int64_t AlignStage::compact_tier(const uint32_t* order) {
    al->bail_list.ensure((size_t)n_items);
    const bool pos16 = al->ri.len <= 32767 && !sw.compact_pos32;
    const bool c_fused = sw.compact_fused;
    auto c_kern = c_fused ? (pos16 ? k_align_compact16_fused : k_align_compact32_fused) : (pos16 ? k_align_compact16 : k_align_compact32);
    // (the first form of the two-kernel chain kernel keeps 48 anchors per pair: eight waves per CU; the fused kernels
    //  and the second form all 56)
    const size_t c_lds_full = (size_t)(pos16 ? PMX_C_LANE_WORDS16 : PMX_C_LANE_WORDS32) * 64 * sizeof(uint32_t) + PMX_C_PEN_BYTES;
    const size_t c_lds = c_fused ? c_lds_full : (size_t)(pos16 ? PMX_C_LANE_WORDS16_1 : PMX_C_LANE_WORDS32_1) * 64 * sizeof(uint32_t) + PMX_C_PEN_BYTES;
    // One workgroup (wave) per 64 pairs, handed out by the dispatcher as CUs free up: the pairs of a wave cost what
    // their worst lane costs, and with a resident grid striding over the positions (PMX_ALIGN_COMPACT_WAVES = waves
    // per CU brings it back) the slowest stride set the kernel's end -- 10M reads: 17.05 -> 15.5 ms, and the seeds
    // kernel below 4.77 -> 4.10 ms.  (The hardware keeps 160 KB / c_lds = seven waves per CU resident either way.)
    int64_t c_grid = (n_launch + 63) / 64;
    if (sw.compact_waves) c_grid = std::min<int64_t>((int64_t)ctx->n_cu * sw.compact_waves, c_grid);
    AlignArgs A = base;
    A.n_items = n_launch;
    A.pair_perm = order;
    A.retry_list = al->bail_list.p;
    A.retry_count = al->retry_count.p + 2;
    // Two-kernel form (default): sketch + index probes in k_compact_seeds, whose only LDS is the minimizer queue
    // -- 7 KB per wave against the 21 KB of the pairs' work state, so that part runs at the occupancy its
    // registers allow instead of seven waves per CU; the seeds cross in HBM (224 bytes per pair with 16-bit
    // position words).  PMX_ALIGN_COMPACT_FUSED keeps everything in k_align_compact.
    // PMX_ALIGN_NO_SIMPLE: no class lists, the chain kernel runs every launch position.
    // PMX_ALIGN_NO_NEAR: only the pairs the seeding marked (extents apart) on the simple list, not the near class.
    const bool c_simple = !c_fused && !sw.no_simple;
    if (!c_fused) {
        const size_t blocks = (size_t)((n_launch + 63) / 64);
        // [0] length of multi_list, [1] pairs the second form finished, [2] / [3] lengths of the two class lists,
        // [4] / [5] pairs k_align_simple finished: marked by the seeding / of the near class
        al->multi_count.ensure(8);
        PMX_ZERO(al->multi_count, 8, stream);
        if (c_simple) {
            al->simple_list.ensure(blocks * 64 * 2);   // the simple list, behind it (from n_launch rounded up to 64) the other
            A.simple_list = al->simple_list.p;
            A.multi_count = al->multi_count.p;
        }
        al->cseeds.ensure(blocks * (size_t)PMX_C_CAP * (pos16 ? 1 : 2) * 64);
        al->cseed_n.ensure(blocks * 64);
        A.cseeds = al->cseeds.p;
        A.cseed_n = al->cseed_n.p;
        // (four waves per SIMD by the kernel's 113 VGPRs; a resident grid of 8 / 12 / 16 waves per CU -- PMX_ALIGN_CSEED_WAVES --
        // takes 7.5 / 6.0 / 4.8 ms per 5M pairs, one workgroup per 64 pairs 4.1; the register budget of five waves per
        // SIMD spills and gains 1 %, of six loses)
        auto s_kern = pos16 ? k_compact_seeds16 : k_compact_seeds32;
        int64_t s_grid = (n_launch + 63) / 64;
        if (sw.cseed_waves) s_grid = std::min<int64_t>((int64_t)ctx->n_cu * sw.cseed_waves, s_grid);
        timer_begin(ctx, "align_cseeds");
        PMX_LAUNCH(s_kern, dim3((unsigned)s_grid), dim3(64), ((size_t)PMX_C_SEEDQ * 2 + 8) * 64 * sizeof(uint32_t),   // queues + eight staging words per lane
                   stream, A);
        if (c_simple) {
            PMX_LAUNCH(sw.no_near ? k_compact_classes : pos16 ? k_compact_classes_near16 : k_compact_classes_near32, dim3((unsigned)((n_launch + 2047) / 2048)), dim3(256), 0, stream, A);   // PMX_C_CLASS_BLOCK positions each
        }
        timer_end(ctx, "align_cseeds", 1);
    }
    // Second form (k_align_compact*_multi): the pairs that leave the first one after their seeds -- a third chain, two
    // regions on one mate (mates that overlap on the reference: 55 % of the real example pairs), ... -- are run again
    // from their hand-over words with up to four chains and several regions per mate; what is still left goes to the
    // thread-per-pair tier.  PMX_ALIGN_NO_MULTI: every bail goes there at once.
    const bool c_multi = !c_fused && !sw.no_multi;
    if (c_multi) {
        al->multi_list.ensure((size_t)n_items);
        A.multi_list = al->multi_list.p;
        A.multi_count = al->multi_count.p;
    }
    timer_begin(ctx, "align_dom");   // the dominant kernels on their own (bench.py roofline): the chain work of every pair
    // Pairs whose mates do not overlap on the reference (half of a 300 +- 30 bp library of 150-base reads) are chained
    // from their hand-over words in registers, k_align_simple*: no per-pair LDS, so the kernel runs at the waves its
    // registers allow; the chain kernel below then runs the other list.  Both lists' lengths stay on the device: one
    // workgroup per 64 positions of the launch, those beyond a list's end leave at once (a resident grid striding over
    // the lists -- PMX_ALIGN_COMPACT_WAVES -- is the slower form here as it is for the chain kernel alone).
    // The near class (mates that overlap by less than a seed, another 29 % of that library) is on the same list.
    if (c_simple) {
        PMX_LAUNCH(pos16 ? k_align_simple16 : k_align_simple32, dim3((unsigned)c_grid), dim3(64), (size_t)PMX_C_SIMPLE_LDS_PAD + PMX_C_PEN_BYTES, stream, A);
    }
    PMX_LAUNCH(c_kern, dim3((unsigned)c_grid), dim3(64), c_lds, stream, A);
    timer_end(ctx, "align_dom", 1);
    if (c_multi) {
        // (the list's length stays on the device: a resident grid -- seven waves per CU by the LDS -- strides over it)
        const int64_t m_grid = std::min<int64_t>((n_launch + 63) / 64, (int64_t)ctx->n_cu * 7);
        al->multi_ws.ensure((size_t)m_grid * PMX_CM_WS_WORDS * 64);
        A.multi_ws = al->multi_ws.p;
        timer_begin(ctx, "align_cmulti");
        PMX_LAUNCH(pos16 ? k_align_compact16_multi : k_align_compact32_multi, dim3((unsigned)m_grid), dim3(64), c_lds_full, stream, A);
        timer_end(ctx, "align_cmulti", 1);
    }
    if (sw.prof) print_compact_prof();
    unsigned long long h_dups = 0, h_bail = 0;
    if (dedup) {   // the copies of the pairs handed to the general tiers (compact_tier_items counts pairs, copies too)
        pair_count_copies(ctx, al, al->bail_list.p, al->retry_count.p + 2, rs->pd_mult.p, n_launch);
        PMX_D2H(&h_dups, pmx::at(al->dd_count, 2), 1, stream);
    }
    unsigned long long h_cnt[6] = {0, 0, 0, 0, 0, 0};   // multi_count[0 .. 5]
    PMX_D2H(&h_bail, pmx::at(al->retry_count, 2), 1, stream);
    if (!c_fused) PMX_D2H(h_cnt, al->multi_count, stream);
    PMX_HIP(hipStreamSynchronize(stream));
    if (sw.verbose && !c_fused)
        fprintf(stderr, "align: compact tier, %lld launch positions: simple list %llu (k_align_simple finished %llu marked by the seeding, %llu of the near class), other list %llu; second form: %llu listed, %llu finished; %llu bails\n",
                (long long)n_launch, h_cnt[2], h_cnt[4], h_cnt[5], h_cnt[3], h_cnt[0], h_cnt[1], h_bail);
    al->last_simple = (int64_t)h_cnt[4];
    al->last_near = (int64_t)h_cnt[5];
    al->last_compact = n_items - (int64_t)h_bail - (int64_t)h_dups;
    return (int64_t)h_bail;
}

// What the thread-per-pair passes of a tail and the launches over its DP slots share: the DP service's buffers, the
// minimizer hand-over with an epoch of its own (a slot may hold an entry of an earlier run), the list and the counters
// the pairs for the wave tiers and the DP requests are counted in, the thread-per-pair layout.
AlignArgs AlignStage::tail_args() {
    AlignArgs T = base;
    PMX_ZERO(al->dp_ncached, n_items, stream);
    T.dp_req_base = al->dp_req.p; T.dp_res_base = al->dp_res.p; T.dp_ncached = al->dp_ncached.p;
    T.dp_slot_pairs = al->dp_slot_pairs.p;
    T.dp_slot_cap = (uint32_t)std::min<int64_t>(n_items, UINT32_MAX - 1);
    T.mv_stride = (uint32_t)tpp_layout.caps.max_mini + 1u;
    T.mv_slots = (uint32_t)std::min<int64_t>(T.dp_slot_cap, 131072);
    T.mv_handover = al->mv_handover.p;
    T.mv_epoch = ++al->mv_epoch;
    T.tpp_ring_w = tpp_lds_bytes ? al->opt.w : 0;
    T.dp_count = al->retry_count.p + 1;
    T.retry_list = al->retry_list2.p;
    T.retry_count = al->retry_count.p;
    T.layout = tpp_layout;
    return T;
}

// k_align_reads_tpp reads, beyond the base: everything tail_args sets, and slow_base / slow_stride (the lanes' Reg region),
// n_items, dp_round, pair_perm (round 0), worklist and dp_next_list (rounds >= 1), set here.
void AlignStage::launch_tpp(const AlignArgs& T, int round, int64_t n_work, const uint32_t* worklist, uint32_t* next_list, const uint32_t* pair_perm) {
    const int64_t grid = std::min<int64_t>(tpp_max_grid, (n_work + 63) / 64);
    AlignArgs A = T;
    A.slow_stride = tpp_raw_stride;
    A.slow_base = al->slab_raw.p;
    A.n_items = n_work;
    A.worklist = worklist;
    A.dp_round = round;
    A.dp_next_list = next_list;
    A.pair_perm = pair_perm;
    PMX_LAUNCH(k_align_reads_tpp, dim3((unsigned)grid), dim3(64), tpp_lds_bytes, stream, A);
}

// One DP service round over the slots `cur` (nullptr: 0 .. n_dp-1): the grouped service, what it left, the wave service
// for that (or nothing, or the left-overs refused), then the replay of the pairs, which lists the slots that post again
// in `next`.
void AlignStage::dp_round(const AlignArgs& T, int round, int64_t n_dp, const uint32_t* cur, uint32_t* next) {
    if (sw.dp_hist) print_dp_requests(round, n_dp);
    bool wave_service = true;
    if (dpg_ok) {
        // the grouped service first (eight lanes per request: align_kernel_dpg.hip): it takes every request whose band
        // never cuts its matrix and whose sides are <= 128 bases -- on 150 bp reads all of them -- and marks them served;
        // the wave-per-request launches below see what is left
        DpgArgs DG = dpg_base;
        DG.dp_req_base = al->dp_req.p; DG.dp_res_base = al->dp_res.p; DG.stats = base.stats;
        DG.n_entries = (uint32_t)std::min<size_t>(al->dp_req.n / sizeof(DpReq), UINT32_MAX);
        if (sw.dpg_prof) { al->dpg_prof.ensure(8); PMX_ZERO(al->dpg_prof, 8, stream); DG.prof = al->dpg_prof.p; }
        dpg_launch(ctx, al, DG, n_dp, cur, sw.dpg_waves, true);
        if (sw.dpg_prof) print_dpg_prof();
        // what did the grouped service leave?  Nothing: no launch of the wave service.  A handful (a side beyond 128
        // bases on 150 bp reads: ~8 requests per 400k pairs): those pairs go to the wave-per-pair tier instead
        uint32_t left[2] = {0, 0};
        PMX_D2H_SYNC(left, pmx::at(al->dpg_counts, PMX_DPG_NO_BUCKET - 1), stream);
        if (left[0] + left[1] == 0) wave_service = false;
        else if ((int64_t)left[0] + left[1] <= sw.dpg_left_few) {
            PMX_LAUNCH(k_dpg_refuse_left, dim3((unsigned)std::min<int64_t>((n_dp * PMX_DP_REQ_PER_PASS + 255) / 256, (int64_t)ctx->n_cu * 8)), dim3(256), 0, stream, DG);
            wave_service = false;
        }
    }
    if (wave_service) {
        AlignArgs A = base;
        A.dp_req_base = al->dp_req.p; A.dp_res_base = al->dp_res.p;
        A.n_items = n_dp;
        A.worklist = cur;
        launch_dp_serve(A, dpp, true, al->slow.p, al->slow2.p, stream);
    }
    launch_tpp(T, round, n_dp, cur, next, nullptr);
}

// THE TAIL: the general tiers over a list of pairs in launch order (`order`, n_t0 of them; nullptr = every item):
// thread-per-pair pass, DP service rounds with replays, the small remainder of the requests through the wave-per-pair
// kernel, then the wave-per-pair tiers for what is left.
void AlignStage::tail(const uint32_t* order, int64_t n_t0) {
    const AlignArgs T = tail_args();
    int64_t n_t1 = n_t0;
    // Few bails: a thread-per-pair launch that small cannot fill the chip and lasts as long as a full one (a wave takes
    // ~2 ms whatever the grid) before the wave-per-pair tier gets the pairs that need a DP; below 4096 bails the wave
    // tier takes all of them at once (measured with 2.8k bails of 500k pairs: 5.8 ms for the stage instead of 7.0).
    const bool skip_t0 = use_compact && n_t0 < sw.bail_tpp_min;
    if (n_t0 > 0 && !skip_t0) launch_tpp(T, 0, n_t0, nullptr, nullptr, order);
    if (!use_compact) timer_end(ctx, "align_dom", 1);
    int64_t n_dp = 0;
    if (!skip_t0) read_counts(n_t1, n_dp, false);
    n_dp = std::min<int64_t>(n_dp, (int64_t)T.dp_slot_cap);
    al->last_dp_slots += n_dp;
    // A replay round costs a fixed ~4-5 ms (one pair's pass through the thread-per-pair kernel) plus the DPs, the
    // wave tier ~0.2 us per easy pair and ~0.9 us per hard one.  First round (pairs asking for their first DP: mostly
    // easy ones): the wave tier below 16,384 pairs.  Later rounds hold the pairs that needed a DP before, i.e.
    // hard ones: another service round pays down to a quarter of that (real 150 bp reads: 53.8 -> 50.3 ms).
    // (round 3, 10M reads: 13.9k first-round requests through the service + one replay: 34.4 ms for the stage, through
    // the wave tier 35.9)
    const uint32_t* cur = nullptr;   // round 1 serves slots 0..n_dp-1
    uint32_t* lists[2] = {al->dp_list_a.p, al->dp_list_b.p};
    int round = 1;
    int64_t n_small = 0;
    while (n_dp > 0) {   // ends by itself: a pair posts at most PMX_DP_MAX_CALLS requests, then goes to the wave tier
        if (n_dp < (round == 1 ? sw.small_rounds : sw.small_rounds / 4)) {   // remainder: wave-per-pair kernel over the slots
            n_small = n_dp;
            break;
        }
        al->last_dp_requests += n_dp;
        uint32_t* next = lists[round & 1];
        dp_round(T, round, n_dp, cur, next);
        read_counts(n_t1, n_dp, false);
        cur = next;
        ++round;
    }
    al->last_dp_rounds = std::max(al->last_dp_rounds, round - 1);
    if (n_small > 0) {   // their capacity overflows (rare) join the tier-1 retry list through counter [0]
        if (!cur) {      // round-1 remainder: slots are 0..n-1
            std::vector<uint32_t> iota((size_t)n_small);
            for (int64_t i = 0; i < n_small; ++i) iota[(size_t)i] = (uint32_t)i;
            PMX_H2D(lists[0], iota, n_small, stream);
            PMX_HIP(hipStreamSynchronize(stream));
            cur = lists[0];
        }
        // the work list holds DP slots: dp_slot_pairs maps them to pairs, and a pair takes the minimizers it left at its slot
        AlignArgs A = base;
        A.dp_slot_pairs = T.dp_slot_pairs;
        A.mv_handover = T.mv_handover; A.mv_stride = T.mv_stride; A.mv_slots = T.mv_slots; A.mv_epoch = T.mv_epoch;
        launch_wave(A, kern_t1, compact, n_small, cur, al->retry_list2.p, al->slow);
        int64_t unused = 0;
        read_counts(n_t1, unused, false);
    }
    PMX_ZERO(al->retry_count, 2, stream);
    const uint32_t* t1_list = al->retry_list2.p;
    if (skip_t0) { t1_list = order; n_t1 = n_t0; }
    al->last_tpp_retry += n_t1;
    wave_tiers(n_t1, t1_list);
}

// diagnostic (PMX_DP_HIST): the shapes of the posted requests
void AlignStage::print_dp_requests(int round, int64_t n_dp) {
    std::vector<DpReq> h((size_t)n_dp * PMX_DP_REQ_PER_PASS);
    PMX_D2H_SYNC(h, pmx::as<DpReq>(al->dp_req), stream);
    std::map<std::tuple<int, int, int, int>, std::pair<long, long>> hist;   // (flag, q bucket, t bucket, band-free) -> (n, cells)
    long n_req = 0;
    for (const DpReq& r : h) {
        if (r.call == 0xffffffffu) continue;
        ++n_req;
        const int w = r.w < 0 ? std::max(r.qlen, r.tlen) : r.w;
        const int free_band = w >= std::max(r.qlen, r.tlen) - 1;
        auto& e = hist[std::make_tuple(r.flag, (r.qlen + 15) / 16 * 16, (r.tlen + 31) / 32 * 32, free_band)];
        ++e.first;
        e.second += (long)r.qlen * r.tlen;
    }
    fprintf(stderr, "[pmx dp requests, round %d] %ld\n  flag  qlen<= tlen<= bandfree        n      cells\n", round, n_req);
    for (auto& kv : hist)
        fprintf(stderr, "  0x%02x %6d %6d %8d %8ld %10ld\n", std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), std::get<3>(kv.first), kv.second.first, kv.second.second);
}

// diagnostic (PMX_DPG_PROF): the grouped service's phase cycles
void AlignStage::print_dpg_prof() {
    unsigned long long h[8];
    PMX_D2H_SYNC(h, al->dpg_prof, stream);
    const double t = (double)std::max<unsigned long long>(h[4], 1);
    fprintf(stderr, "[dpg prof] %llu tasks; cycles per task (lane 0 of the wave): set-up %.0f fill %.0f replay %.0f traceback %.0f; fill steps %.1f\n", h[4], h[0] / t, h[1] / t, h[2] / t, h[3] / t, h[5] / t);
}

// diagnostic (PMX_ALIGN_PROF): the compact tier's own phase profile, then the accumulators start over for the general tiers
void AlignStage::print_compact_prof() {
    unsigned long long h[8];
    PMX_D2H_SYNC(h, al->prof, stream);
    PMX_ZERO(al->prof, 32, stream);
    static const char* cn[8] = {"sketch", "probes", "merge", "chain fill", "backtrack", "regions", "align+mapq", "pairing"};
    const double waves = (double)((n_items + 63) / 64);
    fprintf(stderr, "[pmx compact tier: cycles per wave (lane 0)]");
    for (int k = 0; k < 8; ++k) fprintf(stderr, " %s=%.0f", cn[k], (double)h[k] / waves);
    fprintf(stderr, "\n");
}

// diagnostic (PMX_ALIGN_PROF): the per-phase profile of the general tiers, at the end of the call
void AlignStage::print_phase_prof(bool tier1_fits) {
    unsigned long long h[32];
    PMX_D2H_SYNC(h, al->prof, stream);
    static const char* names[16] = {"decode", "sketch", "seed+heap", "chain", "gen_regs+post", "seg_gen", "squeeze", "align1(all regs)", "filter/sort/parent", "mapq", "pair", "output", "", "", "", ""};
    fprintf(stderr, "[pmx align phase cycles per item]");
    for (int k = 0; k < 12; ++k) fprintf(stderr, " %s=%.0f", names[k], (double)h[k] / (double)n_items);
    // sub-phases (thread-per-pair kernel): "seed+heap" then holds only the heap merge, "chain" only the compaction
    fprintf(stderr, " [of which index lookups=%.0f stage+heapify=%.0f chain fill=%.0f backtrack=%.0f]", (double)h[16] / (double)n_items,
            (double)h[17] / (double)n_items, (double)h[18] / (double)n_items, (double)h[19] / (double)n_items);
    // align1 (thread-per-pair kernel): "align1(all regs)" then holds only what follows the right extension
    fprintf(stderr, " [align1: prologue+filters=%.0f left ext=%.0f gap fills=%.0f right ext=%.0f]", (double)h[20] / (double)n_items,
            (double)h[21] / (double)n_items, (double)h[22] / (double)n_items, (double)h[23] / (double)n_items);
    fprintf(stderr, " [dp serve: cycles traceback=%.0f ksw=%.0f store=%.0f, anti-diagonals filled=%.1f per pair that posted requests]", (double)h[12] / std::max<double>(1, (double)al->last_dp_requests),
            (double)h[13] / std::max<double>(1, (double)al->last_dp_requests), (double)h[14] / std::max<double>(1, (double)al->last_dp_requests),
            (double)h[15] / std::max<double>(1, (double)al->last_dp_requests));
    fprintf(stderr, " dp_requests=%lld dp_rounds=%d tpp_retry=%lld retry=%lld\n", (long long)al->last_dp_requests, al->last_dp_rounds,
            (long long)al->last_tpp_retry, (long long)al->last_retry);
    if (!tier1_fits)   // wave-per-read kernels: slots 23..31 count the DPs by the kernel that ran them
        fprintf(stderr, "[pmx long-read DPs] row by row: %llu calls, %.1f Mcells, %.0f cycles each; anti-diagonals in LDS: %llu calls, %.1f Mcells, %.0f cycles each; anti-diagonals, general arrays: %llu calls, %.1f Mcells, %.0f cycles each\n",
                h[23], h[24] / 1e6, (double)h[25] / std::max<double>(1, (double)h[23]), h[26], h[27] / 1e6, (double)h[28] / std::max<double>(1, (double)h[26]),
                h[29], h[30] / 1e6, (double)h[31] / std::max<double>(1, (double)h[29]));
}

}  // namespace

// Tier 1: compact all-LDS layout (typical short-read pairs); tier 2: general capacities for the pairs that overflowed
// tier 1 (and for everything when the compact layout does not fit LDS).  Tier 0, in front of them for short reads: the
// compact tier and the thread-per-pair kernel with its DP service.
int pmx::align_readset_once(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, int paired, int revcomp_mate2, uint64_t cigar_cap, bool allow_dedup) {
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    AlignStage S(ctx, al, rs, paired, allow_dedup);
    if (!S.setup(revcomp_mate2, cigar_cap)) return PMX_OK;
    const bool tier1_fits = al->opt.is_sr_like && PMX_ALIGN_WORK_BYTES + S.compact.fast_bytes + 16 <= 40 * 1024;
    const bool use_tier0 = tier1_fits && !S.sw.no_tpp;
    timer_begin(ctx, "align");
    if (!tier1_fits) S.long_reads();
    else {
        al->retry_list.ensure((size_t)S.n_items);
        al->retry_list2.ensure((size_t)S.n_items);
        if (!use_tier0) S.wave_tiers(S.n_items, nullptr);
        else {
            S.plan_tier0();
            S.use_compact = paired && al->opt.is_sr_like && al->opt.w == PMX_C_W && (al->opt.k & 1) && rs->max_len <= PMX_C_MAXLEN && S.n_items < (int64_t)UINT32_MAX && !S.sw.no_compact;
            const uint32_t* order = S.launch_order();
            if (!S.use_compact) {
                timer_begin(ctx, "align_dom");   // the dominant kernel on its own (bench.py roofline): the tail closes it
                S.tail(order, S.n_items);
            } else {
                const int64_t n_bail = S.compact_tier(order);
                S.tail(al->bail_list.p, n_bail);
                if (S.dedup) pair_fanout(ctx, al, rs->pd_rep.p, S.n_items, S.base.edits);
            }
        }
    }
    timer_end(ctx, "align", 1);
    if (S.sw.prof) S.print_phase_prof(tier1_fits);
    return PMX_OK;
    PMX_CATCH
}

// pmx_align_dp_probe (include/panmap_amd.h): a chosen DP path on the caller's requests
namespace pmx {
int align_dp_probe(pmx_ctx* ctx, pmx_aligner* al, int path, int max_read_len, int n_segs, int no_rows_dp, int no_dp_fast, const uint8_t* seqs,
                   const int64_t* q_off, const int64_t* t_off, int64_t n, const int32_t* w, const int32_t* zdrop, const int32_t* end_bonus,
                   const int32_t* flag, pmx_dp_probe_result* out, uint32_t* cigar_arena, int64_t arena_cap, pmx_dp_probe_caps* caps) {
    const hipStream_t stream = ctx->stream;
    const bool serve = path == PMX_DP_PROBE_SERVE || path == PMX_DP_PROBE_SERVE_ONE_CLASS;
    memset(caps, 0, 2 * sizeof(*caps));
    auto set_caps = [](pmx_dp_probe_caps& c, const Layout& L, int max_cigar) {
        c.max_qlen = L.caps.max_qlen; c.max_tlen = L.caps.max_tlen; c.max_cigar = max_cigar;
        c.tb_cap = (int64_t)L.tb_cap; c.tb_fast_cap = (int64_t)L.tb_fast_cap;
    };
    for (int64_t i = 0; i < n; ++i) {
        memset(&out[i], 0, sizeof(out[i]));
        if (q_off[i + 1] < q_off[i] || t_off[i + 1] < t_off[i]) return fail(PMX_ERR_ARG, "pmx_align_dp_probe: descending offsets");
    }
    int64_t used = 0;
    if (serve) {
        const DpServePlan P = plan_dp_serve(ctx, max_read_len, n_segs, al->opt);
        const bool class2_fits = P.dp_max_grid > 0;   // (else: its arrays exceed the LDS of a CU, nothing of that class can run: capacities 0)
        if (class2_fits) set_caps(caps[0], P.dp_layout, std::min<int>(P.dp_layout.caps.max_cigar, PMX_DP_MAX_CIGAR));
        else caps[0].max_cigar = PMX_DP_MAX_CIGAR;
        set_caps(caps[1], P.dps_layout, std::min<int>(P.dps_layout.caps.max_cigar, PMX_DP_MAX_CIGAR));
        if (n == 0) return PMX_OK;
        if (n > (int64_t)(UINT32_MAX / PMX_DP_REQ_PER_PASS) - 1) return fail(PMX_ERR_CAPACITY, "pmx_align_dp_probe: too many requests");
        if (P.dps_lds > 160 * 1024) return fail(PMX_ERR_CAPACITY, "pmx_align_dp_probe: reads too long for the LDS work arena");
        const bool two_class = path == PMX_DP_PROBE_SERVE;
        std::vector<DpReq> req((size_t)n * PMX_DP_REQ_PER_PASS);
        for (int64_t i = 0; i < n; ++i) {
            for (int j = 0; j < PMX_DP_REQ_PER_PASS; ++j) req[(size_t)i * PMX_DP_REQ_PER_PASS + j].call = 0xffffffffu;
            DpReq& r = req[(size_t)i * PMX_DP_REQ_PER_PASS];
            const int64_t ql = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i];
            if (ql < 1 || tl < 1 || ((ql + 15) & ~(int64_t)15) + tl > PMX_DP_SEQ_BYTES) continue;   // cannot be posted
            // the pairs that post requests hold reads of at most max_read_len bases: a query beyond the class's capacity (the
            // off[] arrays are sized by it) is refused here
            const bool small = two_class && ql <= DpServePlan::kSmallQlen && tl <= DpServePlan::kSmallTlen &&
                               dp_request_tb_bytes((int)ql, (int)tl, w[i]) <= P.dps_layout.tb_cap;
            if (!small && (!class2_fits || ql > P.dp_layout.caps.max_qlen)) continue;
            r.qlen = (int32_t)ql; r.tlen = (int32_t)tl;
            r.w = w[i]; r.zdrop = zdrop[i]; r.end_bonus = end_bonus[i]; r.flag = flag[i];
            r.key = (uint32_t)i;
            r.call = 0;
            memset(r.seq, 0, sizeof(r.seq));
            memcpy(r.seq, seqs + q_off[i], (size_t)ql);
            memcpy(r.seq + ((ql + 15) & ~(int64_t)15), seqs + t_off[i], (size_t)tl);
        }
        DevBuf<uint8_t> d_req, slow, slow2;
        DevBuf<DpRes> d_res;
        d_req.alloc(req.size() * sizeof(DpReq));
        d_res.alloc((size_t)n * PMX_DP_MAX_CALLS);
        const int64_t g0 = std::min<int64_t>(P.dp_max_grid, n * PMX_DP_REQ_PER_PASS), g1 = std::min<int64_t>(P.dps_max_grid, n * PMX_DP_REQ_PER_PASS);
        slow.alloc(P.dp_stride * (size_t)std::max<int64_t>(g0, 1));
        slow2.alloc(P.dps_stride * (size_t)g1);
        PMX_H2D(pmx::as<DpReq>(d_req), req, stream);
        PMX_FILL(d_res, 0xff, (size_t)n * PMX_DP_MAX_CALLS, stream);
        const size_t lds_max = std::max(class2_fits ? P.dp_lds : 0, P.dps_lds);
        if (lds_max > 64 * 1024) PMX_HIP(hipFuncSetAttribute((const void*)k_align_dp_serve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        AlignArgs A{};
        A.opt = al->opt;
        A.no_rows_dp = no_rows_dp ? 1 : 0;
        A.dp_req_base = d_req.p; A.dp_res_base = d_res.p;
        A.n_items = n;
        launch_dp_serve(A, P, two_class, slow.p, slow2.p, stream);
        std::vector<DpRes> res((size_t)n * PMX_DP_MAX_CALLS);
        PMX_D2H(res, d_res, stream);
        PMX_D2H(req, pmx::as<DpReq>(d_req), stream);   // (a served entry holds its PMX_DPP_* code)
        PMX_HIP(hipStreamSynchronize(stream));
        for (int64_t i = 0; i < n; ++i) {
            const DpRes& R = res[(size_t)i * PMX_DP_MAX_CALLS];
            const DpReq& r = req[(size_t)i * PMX_DP_REQ_PER_PASS];
            pmx_dp_probe_result& o = out[i];
            if (r.key == (uint32_t)i && r.call == 0xffffffffu && r.qlen > 0) o.path_taken = r.flag;   // ran (even when the result overflowed)
            if (R.key != (uint32_t)i) continue;
            if (R.ez.n_cigar < 0 || R.ez.n_cigar > PMX_DP_MAX_CIGAR) continue;
            if (used + R.ez.n_cigar > arena_cap) return fail(PMX_ERR_CAPACITY, "pmx_align_dp_probe: CIGAR arena too small");
            o.served = 1;
            o.max = R.ez.max; o.zdropped = R.ez.zdropped; o.max_q = R.ez.max_q; o.max_t = R.ez.max_t; o.mqe = R.ez.mqe; o.mqe_t = R.ez.mqe_t;
            o.mte = R.ez.mte; o.mte_q = R.ez.mte_q; o.score = R.ez.score; o.n_cigar = R.ez.n_cigar; o.reach_end = R.ez.reach_end;
            o.cigar_off = used;
            for (int k = 0; k < R.ez.n_cigar; ++k) cigar_arena[used + k] = R.cigar[k];
            used += R.ez.n_cigar;
        }
        return PMX_OK;
    }
    const Layout L = path == PMX_DP_PROBE_WAVE_GENERAL ? plan_general_layout(max_read_len, n_segs, al->opt)
                                                       : plan_long_reads_layout(max_read_len, n_segs, al->opt, no_dp_fast != 0);
    set_caps(caps[0], L, L.caps.max_cigar);
    if (n == 0) return PMX_OK;
    const size_t lds_bytes = PMX_ALIGN_WORK_BYTES + L.fast_bytes + 16;
    if (lds_bytes > 160 * 1024) return fail(PMX_ERR_CAPACITY, "pmx_align_dp_probe: reads too long for the LDS work arena");
    if (lds_bytes > 64 * 1024) PMX_HIP(hipFuncSetAttribute((const void*)k_align_dp_probe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const int64_t total = std::max<int64_t>(q_off[n], t_off[n]);
    DpProbeArgs A{};
    DevBuf<uint8_t> d_seqs, slab;
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_par;
    DevBuf<DpProbeOut> d_out;
    DevBuf<uint32_t> d_cig;
    const int64_t grid = std::min<int64_t>(n, 128);   // (a long-read slab is ~8 MB per wave and more with the full traceback)
    A.slow_stride = (L.slow_bytes + 255) & ~(size_t)255;
    d_seqs.alloc((size_t)total);
    d_off.alloc((size_t)(2 * (n + 1)));
    d_par.alloc((size_t)(4 * n));
    d_out.alloc((size_t)n);
    d_cig.alloc((size_t)n * (size_t)L.caps.max_cigar);
    slab.alloc(A.slow_stride * (size_t)grid);
    PMX_H2D(d_seqs, seqs, total, stream);
    PMX_H2D(d_off, q_off, n + 1, stream);
    PMX_H2D(pmx::at(d_off, n + 1), t_off, n + 1, stream);
    const int32_t* par[4] = {w, zdrop, end_bonus, flag};
    for (int k = 0; k < 4; ++k) PMX_H2D(pmx::at(d_par, (size_t)k * n), par[k], n, stream);
    PMX_ZERO(d_out, n, stream);
    A.seqs = d_seqs.p; A.q_off = d_off.p; A.t_off = d_off.p + (n + 1);
    A.w = d_par.p; A.zdrop = d_par.p + n; A.end_bonus = d_par.p + 2 * n; A.flag = d_par.p + 3 * n;
    A.n = n;
    A.out = d_out.p; A.cigars = d_cig.p;
    A.sw_ll = path == PMX_DP_PROBE_SW_LL ? 1 : 0;
    A.no_rows_dp = no_rows_dp ? 1 : 0;
    A.opt = al->opt;
    A.layout = L;
    A.slow_base = slab.p;
    PMX_LAUNCH(k_align_dp_probe, dim3((unsigned)grid), dim3(64), lds_bytes, stream, A);
    std::vector<DpProbeOut> res((size_t)n);
    std::vector<uint32_t> cig((size_t)n * (size_t)L.caps.max_cigar);
    PMX_D2H(res, d_out, n, stream);
    PMX_D2H_SYNC(cig, d_cig, stream);
    for (int64_t i = 0; i < n; ++i) {
        const DpProbeOut& R = res[(size_t)i];
        pmx_dp_probe_result& o = out[i];
        o.path_taken = R.path;
        o.ok = R.ok; o.qe = R.qe; o.te = R.te;
        if (!R.served) continue;
        if (used + R.ez.n_cigar > arena_cap) return fail(PMX_ERR_CAPACITY, "pmx_align_dp_probe: CIGAR arena too small");
        o.served = 1;
        o.max = R.ez.max; o.zdropped = R.ez.zdropped; o.max_q = R.ez.max_q; o.max_t = R.ez.max_t; o.mqe = R.ez.mqe; o.mqe_t = R.ez.mqe_t;
        o.mte = R.ez.mte; o.mte_q = R.ez.mte_q; o.score = R.ez.score; o.n_cigar = R.ez.n_cigar; o.reach_end = R.ez.reach_end;
        o.cigar_off = used;
        for (int k = 0; k < R.ez.n_cigar; ++k) cigar_arena[used + k] = cig[(size_t)i * (size_t)L.caps.max_cigar + k];
        used += R.ez.n_cigar;
    }
    return PMX_OK;
}

// pmx_align_chain_probe (include/panmap_amd.h): one operation of the sort / chaining code on the caller's anchor lists
static_assert(sizeof(pmx_chain_probe_params) == sizeof(ChainProbeParams) && sizeof(pmx_chain_probe_result) == sizeof(ChainProbeOut) &&
                  offsetof(pmx_chain_probe_params, n_seg) == offsetof(ChainProbeParams, n_seg) && sizeof(A128) == 16 &&
                  PMX_CHAIN_PROBE_SORT128 == PMX_CP_SORT128 && PMX_CHAIN_PROBE_SORT64 == PMX_CP_SORT64 && PMX_CHAIN_PROBE_CHAIN_DP == PMX_CP_CHAIN_DP &&
                  PMX_CHAIN_PROBE_CHAIN_RMQ == PMX_CP_CHAIN_RMQ && PMX_CHAIN_PROBE_DEFAULT == PMX_CP_DEFAULT,
              "the chain probe's records of the public header");
int align_chain_probe(pmx_ctx* ctx, pmx_aligner* al, int path, int op, int max_read_len, int n_segs, pmx_chain_probe_params* par, const uint64_t* anchors,
                      const int64_t* a_off, const int32_t* qlen, int64_t n, pmx_chain_probe_result* out, uint64_t* out_anchors, uint64_t* out_u,
                      pmx_chain_probe_caps* caps) {
    const hipStream_t stream = ctx->stream;
    ChainProbeParams P;
    memcpy(&P, par, sizeof(P));
    const Opt o = chain_probe_resolve(P, al->opt);
    memcpy(par, &P, sizeof(P));
    const bool lane = path == PMX_CHAIN_PROBE_LANE;
    const AlignSwitches sw;
    const Layout L = lane ? plan_layout_tpp(max_read_len, n_segs, o, sw.tpp_tb)
                          : path == PMX_CHAIN_PROBE_WAVE_GENERAL ? plan_general_layout(max_read_len, n_segs, o) : plan_long_reads_layout(max_read_len, n_segs, o, false);
    memset(caps, 0, sizeof(*caps));
    caps->max_anchor = L.caps.max_anchor; caps->max_reg = L.caps.max_reg; caps->max_qlen = L.caps.max_qlen;
    if (n == 0) return PMX_OK;
    for (int64_t i = 0; i < n; ++i) {
        memset(&out[i], 0, sizeof(out[i]));
        if (a_off[i + 1] < a_off[i] || a_off[i] < 0) return fail(PMX_ERR_ARG, "pmx_align_chain_probe: descending offsets");
    }
    const int64_t total = a_off[n];
    ChainProbeArgs A{};
    DevBuf<A128> d_in, d_out_a;
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_qlen;
    DevBuf<ChainProbeOut> d_out;
    DevBuf<uint64_t> d_u;
    DevBuf<uint8_t> slab, arena;
    d_in.alloc((size_t)std::max<int64_t>(total, 1));
    d_out_a.alloc((size_t)std::max<int64_t>(total, 1));
    d_u.alloc((size_t)std::max<int64_t>(total, 1));
    d_off.alloc((size_t)(n + 1));
    d_out.alloc((size_t)n);
    if (total > 0) PMX_H2D(pmx::as<uint64_t>(d_in), anchors, 2 * total, stream);
    PMX_H2D(d_off, a_off, n + 1, stream);
    if (qlen) {
        d_qlen.alloc((size_t)(2 * n));
        PMX_H2D(d_qlen, qlen, 2 * n, stream);
    }
    PMX_ZERO(d_out, n, stream);
    PMX_ZERO(d_out_a, std::max<int64_t>(total, 1), stream);
    PMX_ZERO(d_u, std::max<int64_t>(total, 1), stream);
    A.anchors = d_in.p; A.a_off = d_off.p; A.qlen = qlen ? d_qlen.p : nullptr;
    A.n = n;
    A.out = d_out.p; A.out_anchors = d_out_a.p; A.out_u = d_u.p;
    A.op = op; A.n_segs = n_segs; A.max_dist_x = P.max_dist_x; A.max_dist_y = P.max_dist_y; A.n_seg = P.n_seg;
    A.opt = o;
    A.layout = L;
    if (lane) {
        const int64_t grid = std::min<int64_t>((n + 63) / 64, 256);
        const size_t wave_stride = tpp_arena_bytes(L) * 64;
        if (wave_stride > UINT32_MAX) return fail(PMX_ERR_CAPACITY, "pmx_align_chain_probe: thread-per-pair arena stride exceeds 32 bits");
        A.slow_stride = (L.raw_bytes + 255) & ~(size_t)255;
        arena.alloc(wave_stride * (size_t)grid);
        slab.alloc(A.slow_stride * (size_t)grid);
        A.tpp.base = arena.p;
        A.tpp.wave_stride = (uint32_t)wave_stride;
        A.slow_base = slab.p;
        PMX_LAUNCH(k_align_chain_probe_lane, dim3((unsigned)grid), dim3(64), 0, stream, A);
    } else {
        const size_t lds_bytes = PMX_ALIGN_WORK_BYTES + L.fast_bytes + 16;
        if (lds_bytes > 160 * 1024) return fail(PMX_ERR_CAPACITY, "pmx_align_chain_probe: reads too long for the LDS work arena");
        if (lds_bytes > 64 * 1024) PMX_HIP(hipFuncSetAttribute((const void*)k_align_chain_probe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        const int64_t grid = std::min<int64_t>(n, 128);   // (as the DP probe: a long-read slab is ~8 MB per wave)
        A.slow_stride = (L.slow_bytes + 255) & ~(size_t)255;
        slab.alloc(A.slow_stride * (size_t)grid);
        A.slow_base = slab.p;
        PMX_LAUNCH(k_align_chain_probe, dim3((unsigned)grid), dim3(64), lds_bytes, stream, A);
    }
    std::vector<ChainProbeOut> res((size_t)n);
    PMX_D2H(res, d_out, n, stream);
    if (total > 0) {
        PMX_D2H(out_anchors, pmx::as<uint64_t>(d_out_a), 2 * total, stream);
        PMX_D2H(out_u, d_u, total, stream);
    }
    PMX_HIP(hipStreamSynchronize(stream));
    for (int64_t i = 0; i < n; ++i) {
        out[i].served = res[(size_t)i].served; out[i].status = res[(size_t)i].status; out[i].n_a = res[(size_t)i].n_a; out[i].n_u = res[(size_t)i].n_u;
    }
    return PMX_OK;
}
}  // namespace pmx
