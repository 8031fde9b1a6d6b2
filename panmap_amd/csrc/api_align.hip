// C ABI, device part 2: ALIGN stage (see include/panmap_amd.h).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "align/aln_compact_defs.hpp"
#include "align_stage.hpp"

using namespace pmx;
using namespace pmx::aln;

static_assert(sizeof(Work) <= PMX_ALIGN_WORK_BYTES, "Work descriptor exceeds its LDS reservation");
static_assert(sizeof(AlnRecord) == sizeof(pmx_aln_record), "record layout mismatch");

// [0] += edit counts, [1] += records flagged invalid (pmx_align_score_reads)
// (off != NULL: a flagged record counts as an unmapped read -- its length -- the way the drop-in boundary reports it)
__global__ void k_sum_edits(const AlnRecord* __restrict__ recs, const int32_t* __restrict__ edits, int64_t n, unsigned long long* out,
                            const int64_t* __restrict__ off) {
    unsigned long long sum = 0, bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool flagged = (recs[i].flags & 3u) != 0;
        sum += flagged && off ? (unsigned long long)(off[i + 1] - off[i]) : (unsigned long long)(uint32_t)edits[i];
        bad += flagged ? 1ULL : 0ULL;
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); bad += __shfl_xor(bad, o); }
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&out[0], sum);
        if (bad) atomicAdd(&out[1], bad);
    }
}

extern "C" {

int pmx_aligner_set_reference(pmx_ctx* ctx, pmx_aligner* al, const char* reference, int64_t ref_len, int mean_read_len) {
    if (!ctx || !al || !reference || ref_len <= 0) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    al->mean_len = mean_read_len;
    al->opt = make_opt(mean_read_len);
    const int max_score = std::max(8192, (mean_read_len * 4 + 1024) * (al->opt.a + 1));
    RefIndex& r = al->ri;
    // Device build (ref_index_kernels.hip): stream-ordered behind whatever still reads the old index, one short host round
    // trip.  PMX_ALIGN_HOST_INDEX=1, an even k, a reference of 2 Mb or more, or a repeat-rich reference whose mid_occ the
    // counters cannot decide: the host build.
    bool on_device = false;
    if (!pmx::opt_str(pmx::O_ALIGN_HOST_INDEX) && ref_index_device_supported(al->opt, ref_len))
        on_device = build_ref_index_device(ctx->stream, reference, ref_len, al->opt, al->dev_index);
    if (on_device) {
        const bool new_tables = finish_ref_opt(al->opt, max_score, al->host) || !al->logf_uploaded;
        if (new_tables) {
            upload(al->d_logf_ratio, al->host.logf_ratio, ctx->stream);
            upload(al->d_logf_int, al->host.logf_int, ctx->stream);
            PMX_HIP(hipStreamSynchronize(ctx->stream));   // (pageable source)
            al->logf_uploaded = true;
        }
        const RefIndexDevice& d = al->dev_index;
        r.seq = d.seq.p;
        r.ht_mask = d.ht_mask;
        r.ht = d.ht.p;
        r.pos = d.pos.p;
        r.pk = d.pk.p;
        r.pk_amb = d.pk_amb.p;
        r.ht_pv = d.ht_pv.p;
    } else {
        PMX_HIP(hipStreamSynchronize(ctx->stream));   // nothing may still read the old index
        al->opt = make_opt(mean_read_len);
        build_ref_index(reference, ref_len, al->opt, max_score, al->host);
        upload(al->d_seq, al->host.seq, ctx->stream);
        upload(al->d_ht, al->host.ht, ctx->stream);
        upload(al->d_pos, al->host.pos, ctx->stream);
        upload(al->d_logf_ratio, al->host.logf_ratio, ctx->stream);
        upload(al->d_logf_int, al->host.logf_int, ctx->stream);
        upload(al->d_pk, al->host.pk, ctx->stream);
        upload(al->d_pk_amb, al->host.pk_amb, ctx->stream);
        upload(al->d_ht_pv, al->host.ht_pv, ctx->stream);
        al->logf_uploaded = true;
        r.seq = al->d_seq.p;
        r.ht_mask = (uint32_t)al->host.ht.size() - 1;
        r.ht = al->d_ht.p;
        r.pos = al->d_pos.p;
        r.pk = al->d_pk.p;
        r.pk_amb = al->d_pk_amb.p;
        r.ht_pv = al->d_ht_pv.p;
        PMX_HIP(hipStreamSynchronize(ctx->stream));
    }
    r.len = (int32_t)ref_len;
    r.logf_ratio = al->d_logf_ratio.p;
    r.logf_int = al->d_logf_int.p;
    r.n_logf = (int32_t)al->host.logf_int.size();
    return PMX_OK;
    PMX_CATCH
}

int pmx_aligner_index_digest(pmx_ctx* ctx, pmx_aligner* al, uint64_t out[5]) {
    if (!ctx || !al || !out) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const RefIndex& r = al->ri;
    const size_t cap = (size_t)r.ht_mask + 1;
    std::vector<HtEnt> ht(cap);
    std::vector<uint32_t> pv(cap);
    PMX_D2H(ht, r.ht, cap, ctx->stream);
    PMX_D2H_SYNC(pv, r.ht_pv, cap, ctx->stream);
    uint64_t n_pos = 0, n_keys = 0;
    for (const HtEnt& e : ht)
        if (e.key != UINT64_MAX) { ++n_keys; n_pos = std::max<uint64_t>(n_pos, (uint64_t)e.off + e.cnt); }
    std::vector<uint64_t> pos((size_t)n_pos);
    PMX_D2H_BLOCKING(pos.data(), r.pos, n_pos);
    uint64_t digest = 0, covered = 0;
    for (size_t s = 0; s < cap; ++s) {
        const HtEnt& e = ht[s];
        if (e.key == UINT64_MAX) continue;
        if (((uint32_t)mix64(e.key) & r.ht_mask) != s) {   // every slot between the home slot and this one must be taken
            for (uint32_t q = (uint32_t)mix64(e.key) & r.ht_mask; q != s; q = (q + 1) & r.ht_mask)
                if (ht[q].key == UINT64_MAX) return fail(PMX_ERR_DEVICE, "reference index: a key is not reachable by linear probing");
        }
        uint64_t h = mix64(e.key) ^ mix64((uint64_t)e.cnt + 0x9e3779b97f4a7c15ULL);
        for (uint32_t q = 0; q < e.cnt; ++q) h = mix64(h ^ (pos[(size_t)e.off + q] + q));
        if (e.cnt == 1 && (pos[e.off] >> 32) == 0 && pv[s] != (uint32_t)pos[e.off]) return fail(PMX_ERR_DEVICE, "reference index: ht_pv does not match pos");
        if (e.cnt != 1 && pv[s] != 0xffffffffu) return fail(PMX_ERR_DEVICE, "reference index: ht_pv set for a repeated minimizer");
        digest += h;
        covered += e.cnt;
    }
    out[0] = covered;
    out[1] = n_keys;
    out[2] = (uint64_t)(int64_t)al->opt.mid_occ;
    out[3] = digest;
    out[4] = r.ht == al->dev_index.ht.p ? 1 : 0;
    return PMX_OK;
    PMX_CATCH
}

int pmx_aligner_create(pmx_ctx* ctx, const char* reference, int64_t ref_len, int mean_read_len, pmx_aligner** out) {
    if (!ctx || !reference || ref_len <= 0 || !out) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<pmx_aligner> al(new pmx_aligner());
    al->cigar_used.alloc(1);
    const int rc = pmx_aligner_set_reference(ctx, al.get(), reference, ref_len, mean_read_len);
    if (rc != PMX_OK) return rc;
    *out = al.release();
    return PMX_OK;
    PMX_CATCH
}

void pmx_aligner_free(pmx_ctx* ctx, pmx_aligner* al) {
    if (ctx) (void)hipSetDevice(ctx->device);
    if (al && al->ev_results) (void)hipEventDestroy(al->ev_results);
    if (al && al->ev_fetched) (void)hipEventDestroy(al->ev_fetched);
    delete al;
}

// The CIGAR arena is sized optimistically (16 words per read); the kernels count what they WOULD have written
// exactly (cigar_used runs past the capacity), so a call that overflowed is redone once with the counted size:
// no record ever leaves this function with PMX_REC_OVERFLOW set because of the arena.
int pmx_align_readset(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, int paired, int revcomp_mate2) {
    if (!ctx || !al || !rs) return PMX_ERR_ARG;
    if (rs->hpc) return fail(PMX_ERR_ARG, "the read set is homopolymer-compressed: the align stage works on the uncompressed reads, pass the read set it was compressed from");
    if (!rs->packed) return fail(PMX_ERR_ARG, "read set is not packed (call pmx_readset_pack first)");
    uint64_t cap = (uint64_t)std::max<int64_t>(rs->n * 16, 4096);
    // long reads: an operation every ~20 bases at 5 % errors; and whatever the previous call on this aligner needed per base
    // (a redo costs the whole stage again: 4.5 s per 100k reads of 10 kb)
    if (!al->opt.is_sr_like) cap = std::max<uint64_t>(cap, (uint64_t)rs->total / 8 + (uint64_t)rs->n * 16);
    if (al->cigar_words_per_kbase > 0.0) cap = std::max<uint64_t>(cap, (uint64_t)(al->cigar_words_per_kbase * 1.25 * (double)rs->total / 1000.0) + 4096);
    if (const char* e = pmx::opt_str(pmx::O_ALIGN_CIGAR_CAP)) cap = (uint64_t)std::max<long long>(atoll(e), 16);   // tests: force the redo
    bool dedup = true;
    for (int attempt = 0;; ++attempt) {
        const int rc = align_readset_once(ctx, al, rs, paired, revcomp_mate2, cap, dedup);
        if (rc != PMX_OK) return rc;
        unsigned long long used = 0, st[4] = {0, 0, 0, 0}, dd[2] = {0, 0};
        PMX_TRY
        PMX_D2H(&used, al->cigar_used, 1, ctx->stream);
        PMX_D2H(st, al->stats, ctx->stream);
        PMX_D2H_SYNC(dd, al->dd_count, ctx->stream);
        PMX_CATCH
        al->last_cigar_used = used;
        al->last_stats.dp_calls = (int64_t)st[0];
        al->last_stats.dp_cells = (int64_t)st[1];
        al->last_stats.dp_pairs = al->last_dp_slots + (int64_t)st[2];
        al->last_stats.dp_rounds = al->last_dp_rounds;
        al->last_stats.wave_tier_items = al->last_tpp_retry;
        al->last_stats.general_tier_items = al->last_retry;
        al->last_stats.compact_tier_items = al->last_compact;
        al->last_stats.simple_chain_items = al->last_simple;
        al->last_stats.near_chain_items = al->last_near;
        al->last_stats.huge_tier_items = al->last_huge;
        if (rs->total > 0) al->cigar_words_per_kbase = std::max(al->cigar_words_per_kbase * 0.5, (double)used * 1000.0 / (double)rs->total);
        if (used <= cap) return PMX_OK;
        if (attempt >= 2) return fail(PMX_ERR_CAPACITY, "CIGAR arena overflow persists after resizing");
        cap = used + 64;
        // copies of a representative that overflowed the arena could not count their words (k_pair_fanout): `used` falls short
        // by those, and the redo aligns every pair itself (its count is then exact for the last attempt)
        if (dd[1] > 0) dedup = false;
    }
}

// score_reads_vs_reference (src/mm_align.c:144-199): minus the summed count_read_errors of every read against the
// aligner's reference -- the alignment-based score of one --refine candidate (src/placement.cpp:489-514)
static int score_reads_impl(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, int paired, int revcomp_mate2, int64_t* score, int64_t* n_flagged) {
    al->want_edits = true;
    const int rc = pmx_align_readset(ctx, al, rs, paired, revcomp_mate2);
    al->want_edits = false;
    if (rc != PMX_OK) return rc;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    al->stats.ensure(4);
    PMX_ZERO(al->stats, 2, ctx->stream);
    const int64_t n = al->n_records;
    if (n > 0)
        PMX_LAUNCH(k_sum_edits, dim3((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->n_cu * 8)), dim3(256), 0, ctx->stream, al->records.p,
                   al->edits.p, n, al->stats.p, n_flagged ? rs->off.p : (const int64_t*)nullptr);
    unsigned long long h[2] = {0, 0};
    PMX_D2H_SYNC(h, al->stats, ctx->stream);
    if (n_flagged) *n_flagged = (int64_t)h[1];
    else if (h[1]) return fail(PMX_ERR_UNSUPPORTED, "reads with flagged (overflow / unsupported) records: their edit counts are not the reference's");
    *score = -(int64_t)h[0];
    return PMX_OK;
    PMX_CATCH
}

int pmx_align_score_reads(pmx_ctx* ctx, pmx_aligner* al, const pmx_readset* rs, int paired, int revcomp_mate2, int64_t* score) {
    if (!ctx || !al || !rs || !score) return PMX_ERR_ARG;
    if (paired && (rs->n & 1)) return fail(PMX_ERR_UNSUPPORTED, "paired scoring of an odd number of reads (the reference maps the last one alone: pmx_score_reads_vs_reference does)");
    return score_reads_impl(ctx, al, rs, paired, revcomp_mate2, score, nullptr);
}

// Drop-in for score_reads_vs_reference (src/mm_align.h:13-17, src/mm_align.c:144-199), the reference's own signature: host
}  // extern "C"

// Contexts of the two drop-in boundaries below.  The reference calls them from several TBB workers at a time, call after
// call; a context per call would create and destroy its hardware queues (CU-masked streams) over and over, beside the
// running queues of the other workers -- the pattern behind the hang of round 4 (a destroyed stream's queue recycled under
// the next one's kernels) and one hung run of tests/test_align_gpu.py::test_direct_boundary_is_reentrant.  The contexts are
// kept: a call borrows one (or makes one: there are never more than the workers that were inside at the same time) and
// hands it back; they live as long as the process.
namespace {
std::mutex g_ctx_pool_mu;
std::vector<pmx_ctx*> g_ctx_pool;
pmx_ctx* borrow_ctx(int dev) {
    {
        std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
        for (size_t i = 0; i < g_ctx_pool.size(); ++i)
            if (g_ctx_pool[i]->device == dev) {
                pmx_ctx* c = g_ctx_pool[i];
                g_ctx_pool.erase(g_ctx_pool.begin() + (long)i);
                if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); g_ctx_pool.push_back(c); return nullptr; }
                return c;
            }
    }
    pmx_ctx* c = nullptr;
    return pmx_ctx_create(dev, &c) == PMX_OK ? c : nullptr;
}
void return_ctx(pmx_ctx* c) {
    if (!c) return;
    if (hipStreamSynchronize(c->stream) != hipSuccess) {   // a context whose stream failed is not handed to the next caller
        (void)hipGetLastError();
        pmx_ctx_destroy(c);
        return;
    }
    std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
    g_ctx_pool.push_back(c);
}
}  // namespace

extern "C" {

// strings in, minus the total edit distance out; 0 on failure, as the reference returns 0 when its index cannot be built.
// An odd read of a paired set is mapped alone (:178-185).  A pair whose record a kernel flagged invalid counts as unmapped
// reads (their lengths), the way pmx_align_reads_direct reports such pairs; pmx_last_error() says how many there were.
int64_t pmx_score_reads_vs_reference(const char* reference, int n_reads, const char** reads, const int* r_lens, int kmer_size, bool paired_end) {
    (void)kmer_size;
    if (!reference || !reads || !r_lens || n_reads <= 0) return 0;
    pmx_ctx* ctx = nullptr;
    int dev = 0;
    if (const char* e = pmx::opt_str(pmx::O_DEVICE)) dev = atoi(e);
    if (!(ctx = borrow_ctx(dev))) return 0;
    pmx_aligner* al = nullptr;
    int64_t total = 0, withheld = 0;
    bool ok = false;
    do {
        std::vector<int64_t> off((size_t)n_reads + 1, 0);
        for (int i = 0; i < n_reads; ++i) off[(size_t)i + 1] = off[(size_t)i] + r_lens[i];
        std::string concat;
        concat.reserve((size_t)off[(size_t)n_reads]);
        for (int i = 0; i < n_reads; ++i) concat.append(reads[i], (size_t)r_lens[i]);
        for (char& ch : concat)
            if ((unsigned char)ch < 4) ch = "ACGT"[(unsigned char)ch];   // (pre-encoded bases, as in pmx_align_reads_direct)
        const int avg_len = (int)(off[(size_t)n_reads] / n_reads);        // setup_minimap2 looks at every read (src/mm_align.c:124-130)
        if (pmx_aligner_create(ctx, reference, (int64_t)strlen(reference), avg_len, &al) != PMX_OK) break;
        const bool paired = paired_end && n_reads >= 2;
        const int n_main = paired ? n_reads & ~1 : n_reads;
        auto run = [&](int first, int count, int as_pairs) {
            pmx_readset* rs = nullptr;
            if (pmx_readset_upload(ctx, concat.data(), off.data() + first, count, &rs) != PMX_OK) return false;
            int64_t sc = 0, flagged = 0;
            const bool good = pmx_readset_pack(ctx, rs) == PMX_OK && score_reads_impl(ctx, al, rs, as_pairs, 0, &sc, &flagged) == PMX_OK;
            pmx_readset_free(ctx, rs);
            total += sc;
            withheld += flagged;
            return good;
        };
        if (!run(0, n_main, paired ? 1 : 0)) break;
        if (n_main < n_reads && !run(n_main, 1, 0)) break;   // the odd read, alone
        ok = true;
    } while (0);
    if (al) pmx_aligner_free(ctx, al);
    return_ctx(ctx);
    if (ok && withheld) set_error("pmx_score_reads_vs_reference: " + std::to_string(withheld) + " read(s) of flagged records counted as unmapped");
    return ok ? total : 0;
}

int64_t pmx_align_num_records(const pmx_aligner* al) { return al ? al->n_records : 0; }

int64_t pmx_align_cigar_words(pmx_ctx* ctx, pmx_aligner* al) {
    if (!ctx || !al) return PMX_ERR_ARG;
    return (int64_t)std::min<unsigned long long>(al->last_cigar_used, al->cigar_cap);
}

int pmx_align_fetch(pmx_ctx* ctx, pmx_aligner* al, pmx_aln_record* records, int64_t n_records, uint32_t* cigar_arena, int64_t arena_cap) {
    if (!ctx || !al || !records || n_records < al->n_records) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const int64_t used = pmx_align_cigar_words(ctx, al);
    if (used < 0) return (int)used;
    if (used > arena_cap || (used > 0 && !cigar_arena)) return fail(PMX_ERR_CAPACITY, "CIGAR arena buffer too small");
    if (al->n_records > 0)
        PMX_D2H(records, al->records, al->n_records, ctx->stream);
    PMX_D2H_SYNC(cigar_arena, al->cigars, used, ctx->stream);
    return PMX_OK;
    PMX_CATCH
}

int pmx_align_scoring(const pmx_aligner* al, int32_t out[9]) {
    if (!al || !out) return PMX_ERR_ARG;
    const Opt& o = al->opt;
    const int32_t v[9] = {o.a, o.b, o.q, o.e, o.q2, o.e2, o.sc_ambi, o.zdrop, o.end_bonus};
    memcpy(out, v, sizeof(v));
    return PMX_OK;
}

// ksw_extd2 on a batch of sequence pairs through the grouped DP service (include/panmap_amd.h): one request slot per pair
int pmx_align_dp_batch(pmx_ctx* ctx, pmx_aligner* al, const uint8_t* seqs, const int64_t* q_off, const int64_t* t_off, int64_t n, const int32_t* w,
                       const int32_t* zdrop, const int32_t* end_bonus, const int32_t* flag, pmx_dp_result* out, int reps, double* kernel_ms) {
    if (!ctx || !al || n < 0 || (n > 0 && (!seqs || !q_off || !t_off || !w || !zdrop || !end_bonus || !flag || !out))) return PMX_ERR_ARG;
    if (n > (int64_t)(UINT32_MAX / PMX_DP_REQ_PER_PASS) - 1) return PMX_ERR_CAPACITY;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (kernel_ms) *kernel_ms = 0;
    if (n == 0) return PMX_OK;
    DpgArgs DG;
    const bool ok = dpg_setup(al->opt, DG);
    std::vector<DpReq> req((size_t)n * PMX_DP_REQ_PER_PASS);
    for (int64_t i = 0; i < n; ++i) {
        for (int j = 0; j < PMX_DP_REQ_PER_PASS; ++j) req[(size_t)i * PMX_DP_REQ_PER_PASS + j].call = 0xffffffffu;
        DpReq& r = req[(size_t)i * PMX_DP_REQ_PER_PASS];
        const int64_t ql = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i];
        if (ql < 0 || tl < 0) return fail(PMX_ERR_ARG, "pmx_align_dp_batch: descending offsets");
        r.qlen = (int32_t)std::min<int64_t>(ql, INT32_MAX); r.tlen = (int32_t)std::min<int64_t>(tl, INT32_MAX);
        r.w = w[i]; r.zdrop = zdrop[i]; r.end_bonus = end_bonus[i]; r.flag = flag[i];
        r.key = (uint32_t)i;
        if (ql >= 1 && tl >= 1 && ((ql + 15) & ~(int64_t)15) + tl <= PMX_DP_SEQ_BYTES) {   // (longer ones cannot be posted: left unserved)
            r.call = 0;
            memset(r.seq, 0, sizeof(r.seq));
            memcpy(r.seq, seqs + q_off[i], (size_t)ql);
            memcpy(r.seq + ((ql + 15) & ~(int64_t)15), seqs + t_off[i], (size_t)tl);
        }
    }
    DevBuf<uint8_t> d_req;
    DevBuf<DpRes> d_res;
    d_req.alloc(req.size() * sizeof(DpReq));
    d_res.alloc((size_t)n * PMX_DP_MAX_CALLS);
    PMX_H2D(pmx::as<DpReq>(d_req), req, ctx->stream);
    PMX_FILL(d_res, 0xff, (size_t)n * PMX_DP_MAX_CALLS, ctx->stream);
    DG.dp_req_base = d_req.p; DG.dp_res_base = d_res.p;
    DG.n_entries = (uint32_t)req.size();
    DG.shadow = 1;   // the requests stay posted: the launch can be repeated
    int dpg_waves = pmx::kDpgWavesDefault;
    if (const char* e = pmx::opt_str(pmx::O_ALIGN_DPG_WAVES)) dpg_waves = std::max(1, atoi(e));
    if (ok) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        PMX_HIP(hipEventCreate(&e0)); PMX_HIP(hipEventCreate(&e1));
        float best = 0;
        for (int rep = 0; rep < std::max(reps, 1); ++rep) {
            dpg_launch(ctx, al, DG, n, nullptr, dpg_waves, false);   // collect + order
            PMX_HIP(hipEventRecord(e0, ctx->stream));
            const int64_t grid = std::min<int64_t>((int64_t)ctx->n_cu * dpg_waves, (n * PMX_DP_REQ_PER_PASS + 7) / 8 + PMX_DPG_BUCKETS);
            PMX_LAUNCH(k_align_dp_group, dim3((unsigned)grid), dim3(64), PMX_DPG_LDS_BYTES, ctx->stream, DG);
            PMX_HIP(hipEventRecord(e1, ctx->stream));
            PMX_HIP(hipEventSynchronize(e1));
            float ms = 0;
            PMX_HIP(hipEventElapsedTime(&ms, e0, e1));
            if (rep == 0 || ms < best) best = ms;
        }
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (kernel_ms) *kernel_ms = best;
    }
    std::vector<DpRes> res((size_t)n * PMX_DP_MAX_CALLS);
    PMX_D2H_SYNC(res, d_res, ctx->stream);
    for (int64_t i = 0; i < n; ++i) {
        const DpRes& R = res[(size_t)i * PMX_DP_MAX_CALLS];
        pmx_dp_result& o = out[i];
        memset(&o, 0, sizeof(o));
        if (R.key != (uint32_t)i) continue;   // not taken (0xffffffff: never written, or more CIGAR operations than a result holds)
        o.served = 1;
        o.max = R.ez.max; o.zdropped = R.ez.zdropped; o.max_q = R.ez.max_q; o.max_t = R.ez.max_t; o.mqe = R.ez.mqe; o.mqe_t = R.ez.mqe_t;
        o.mte = R.ez.mte; o.mte_q = R.ez.mte_q; o.score = R.ez.score; o.n_cigar = R.ez.n_cigar; o.reach_end = R.ez.reach_end;
        for (int k = 0; k < R.ez.n_cigar && k < PMX_DP_MAX_CIGAR; ++k) o.cigar[k] = R.cigar[k];
    }
    return PMX_OK;
    PMX_CATCH
}

static_assert(PMX_DP_PATH_REG == PMX_DPP_REG && PMX_DP_PATH_ROWS == PMX_DPP_ROWS && PMX_DP_PATH_DIAG == PMX_DPP_DIAG && PMX_DP_PATH_KIND == PMX_DPP_KIND &&
                  PMX_DP_PATH_EXACT == PMX_DPP_EXACT && PMX_DP_PATH_FAST == PMX_DPP_FAST && PMX_DP_PATH_TB_LDS == PMX_DPP_TB_LDS &&
                  PMX_DP_PATH_ALL_LDS == PMX_DPP_ALL_LDS, "path codes of the public header");

int pmx_align_dp_probe(pmx_ctx* ctx, pmx_aligner* al, int path, int max_read_len, int n_segs, int no_rows_dp, int no_dp_fast, const uint8_t* seqs,
                       const int64_t* q_off, const int64_t* t_off, int64_t n, const int32_t* w, const int32_t* zdrop, const int32_t* end_bonus,
                       const int32_t* flag, pmx_dp_probe_result* out, uint32_t* cigar_arena, int64_t arena_cap, pmx_dp_probe_caps caps[2]) {
    if (!ctx || !al || !caps || n < 0 || path < PMX_DP_PROBE_SERVE || path > PMX_DP_PROBE_SW_LL || max_read_len < 1 || max_read_len > (1 << 20) ||
        n_segs < 1 || n_segs > 2 || arena_cap < 0)
        return PMX_ERR_ARG;
    if (n > 0 && (!seqs || !q_off || !t_off || !w || !zdrop || !end_bonus || !flag || !out || (arena_cap > 0 && !cigar_arena))) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    return align_dp_probe(ctx, al, path, max_read_len, n_segs, no_rows_dp, no_dp_fast, seqs, q_off, t_off, n, w, zdrop, end_bonus, flag, out, cigar_arena,
                          arena_cap, caps);
    PMX_CATCH
}

int pmx_align_chain_probe(pmx_ctx* ctx, pmx_aligner* al, int path, int op, int max_read_len, int n_segs, pmx_chain_probe_params* par, const uint64_t* anchors,
                          const int64_t* a_off, const int32_t* qlen, int64_t n, pmx_chain_probe_result* out, uint64_t* out_anchors, uint64_t* out_u,
                          pmx_chain_probe_caps* caps) {
    if (!ctx || !al || !par || !caps || n < 0 || path < PMX_CHAIN_PROBE_WAVE_LONG || path > PMX_CHAIN_PROBE_LANE || op < PMX_CHAIN_PROBE_SORT128 ||
        op > PMX_CHAIN_PROBE_CHAIN_RMQ || max_read_len < 1 || max_read_len > (1 << 20) || n_segs < 1 || n_segs > 2)
        return PMX_ERR_ARG;
    if (n > 0 && (!anchors || !a_off || !out || !out_anchors || !out_u)) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    return align_chain_probe(ctx, al, path, op, max_read_len, n_segs, par, anchors, a_off, qlen, n, out, out_anchors, out_u, caps);
    PMX_CATCH
}

// The download of pmx_align_fetch on a stream of the caller's choice, without waiting for it: the copies start when the
// results are complete (event on the context's stream) and the next pmx_align_readset on this aligner waits for them
// before it overwrites the buffers.  The caller synchronises `stream` before it reads the host buffers (pinned memory, or
// the copies are staged).  stream NULL = the context's stream.
int pmx_align_fetch_async(pmx_ctx* ctx, pmx_aligner* al, pmx_aln_record* records, int64_t n_records, uint32_t* cigar_arena, int64_t arena_cap, void* stream) {
    if (!ctx || !al || !records || n_records < al->n_records) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const int64_t used = pmx_align_cigar_words(ctx, al);
    if (used < 0) return (int)used;
    if (used > arena_cap || (used > 0 && !cigar_arena)) return fail(PMX_ERR_CAPACITY, "CIGAR arena buffer too small");
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (!al->ev_results) {
        PMX_HIP(hipEventCreateWithFlags(&al->ev_results, hipEventDisableTiming));
        PMX_HIP(hipEventCreateWithFlags(&al->ev_fetched, hipEventDisableTiming));
    }
    if (st != ctx->stream) {
        PMX_HIP(hipEventRecord(al->ev_results, ctx->stream));
        PMX_HIP(hipStreamWaitEvent(st, al->ev_results, 0));
    }
    PMX_D2H(records, al->records, al->n_records, st);
    PMX_D2H(cigar_arena, al->cigars, used, st);
    if (st != ctx->stream) {
        PMX_HIP(hipEventRecord(al->ev_fetched, st));
        al->fetch_pending = true;
    }
    return PMX_OK;
    PMX_CATCH
}

int pmx_align_copy_records_device(pmx_ctx* ctx, pmx_aligner* al, void* d_records, int64_t n_records) {
    if (!ctx || !al || !d_records || n_records < al->n_records) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (al->n_records > 0)
        PMX_D2D(d_records, al->records, al->n_records, ctx->stream);
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
    PMX_CATCH
}

int pmx_align_copy_cigars_device(pmx_ctx* ctx, pmx_aligner* al, void* d_cigars, int64_t n_words) {
    if (!ctx || !al || (!d_cigars && n_words > 0)) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const int64_t used = pmx_align_cigar_words(ctx, al);
    if (n_words < used) return fail(PMX_ERR_CAPACITY, "CIGAR arena buffer too small");
    PMX_D2D(d_cigars, al->cigars, used, ctx->stream);
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
    PMX_CATCH
}

int pmx_align_get_stats(pmx_ctx* ctx, pmx_aligner* al, pmx_align_stats* out) {
    if (!ctx || !al || !out) return PMX_ERR_ARG;
    *out = al->last_stats;
    return PMX_OK;
}

const void* pmx_align_device_records(const pmx_aligner* al) { return al ? al->records.p : nullptr; }
const void* pmx_align_device_cigars(const pmx_aligner* al) { return al ? al->cigars.p : nullptr; }

// Drop-in for align_reads_direct (src/mm_align.h:44-53): host strings in, read_align_t out.
void pmx_align_reads_direct(const char* reference, const char* refName, int n_reads, const char** reads, const char** quality,
                            const char** read_names, const int* r_lens, align_pair_result_t* results, bool pairedEndReads, int n_threads) {
    (void)refName; (void)quality; (void)read_names; (void)n_threads;
    if (!reference || !reads || !r_lens || !results || n_reads <= 0) return;
    pmx_ctx* ctx = nullptr;
    pmx_readset* rs = nullptr;
    pmx_aligner* al = nullptr;
    int dev = 0;
    if (const char* e = pmx::opt_str(pmx::O_DEVICE)) dev = atoi(e);
    if (!(ctx = borrow_ctx(dev))) return;   // like the reference: results stay untouched on failure
    do {
        int64_t total = 0;
        std::vector<int64_t> off((size_t)n_reads + 1, 0);
        for (int i = 0; i < n_reads; ++i) { off[i] = total; total += r_lens[i]; }
        off[n_reads] = total;
        std::string concat;
        concat.reserve((size_t)total);
        for (int i = 0; i < n_reads; ++i) concat.append(reads[i], (size_t)r_lens[i]);
        // seq_nt4_table (sketch.c:9-26) passes the bytes 0..3 through as pre-encoded bases; the packed read set knows letters
        // only (those bytes would be ambiguous), so they become letters here
        for (char& ch : concat)
            if ((unsigned char)ch < 4) ch = "ACGT"[(unsigned char)ch];
        const int avg_len = (int)(total / n_reads);   // src/mm_align.c:124-130
        if (pmx_readset_upload(ctx, concat.data(), off.data(), n_reads, &rs) != PMX_OK) break;
        if (pmx_readset_pack(ctx, rs) != PMX_OK) break;
        if (pmx_aligner_create(ctx, reference, (int64_t)strlen(reference), avg_len, &al) != PMX_OK) break;
        if (pmx_align_readset(ctx, al, rs, pairedEndReads ? 1 : 0, 0) != PMX_OK) break;
        std::vector<pmx_aln_record> recs((size_t)n_reads);
        const int64_t words = pmx_align_cigar_words(ctx, al);
        if (words < 0) break;
        std::vector<uint32_t> arena((size_t)std::max<int64_t>(words, 1));
        if (pmx_align_fetch(ctx, al, recs.data(), n_reads, arena.data(), (int64_t)arena.size()) != PMX_OK) break;
        auto fill = [&](const pmx_aln_record& r, read_align_t* o) {
            memset(o, 0, sizeof(*o));
            if (r.mapped && (r.flags & PMX_REC_HAS_ALN)) {
                o->pos = r.rs + 1; o->rs = r.rs; o->re = r.re; o->qs = r.qs; o->qe = r.qe;
                o->mapq = r.mapq; o->rev = r.rev; o->proper_frag = r.proper_frag;
                o->n_cigar = r.n_cigar;
                o->cigar = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)std::max<int>(r.n_cigar, 1));
                memcpy(o->cigar, arena.data() + r.cigar_off, sizeof(uint32_t) * r.n_cigar);
            } else o->pos = INT_MAX;
        };
        const int n_items = pairedEndReads ? n_reads / 2 : n_reads;
        // A record flagged PMX_REC_OVERFLOW / PMX_REC_UNSUPPORTED is INVALID (a work capacity or an unrestated
        // branch of the reference was hit): it never leaves the boundary as an alignment.  The pair is reported
        // unmapped and pmx_last_error() says how many were withheld.
        int64_t n_withheld = 0;
        for (int k = 0; k < n_items; ++k) {
            align_pair_result_t* res = &results[k];
            memset(res, 0, sizeof(*res));
            const bool invalid = pairedEndReads ? ((recs[2 * k].flags | recs[2 * k + 1].flags) & 3) != 0 : (recs[k].flags & 3) != 0;
            if (invalid) {
                ++n_withheld;
                res->mapped = 0; res->r1.pos = INT_MAX; res->r2.pos = INT_MAX;
            } else if (pairedEndReads) {
                const pmx_aln_record &a = recs[2 * k], &b = recs[2 * k + 1];
                if (a.mapped) { res->mapped = 1; fill(a, &res->r1); fill(b, &res->r2); }
                else { res->mapped = 0; res->r1.pos = INT_MAX; res->r2.pos = INT_MAX; }
            } else {
                const pmx_aln_record& a = recs[k];
                if (a.mapped) { res->mapped = 1; fill(a, &res->r1); }
                else res->r1.pos = INT_MAX;
            }
        }
        if (n_withheld) set_error("pmx_align_reads_direct: " + std::to_string(n_withheld) + " invalid record(s) withheld (reported unmapped)");
    } while (0);
    if (al) pmx_aligner_free(ctx, al);
    if (rs) pmx_readset_free(ctx, rs);
    return_ctx(ctx);
}

}  // extern "C"