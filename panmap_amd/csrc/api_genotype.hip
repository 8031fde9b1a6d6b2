// C ABI of the device pileup (pmx_pileup_*, include/panmap_amd.h): the host sweep that decides which reads are in the
// pileup, then the two kernels of pileup_kernels.hip.
//
// The sweep restates, over the records in BAM order (host/bam_writer.cpp: bam_record_order), what decides a read's fate
// before bcftools looks at a single base:
//   * mplp_func (bcftools/mpileup.c:196-299) with the defaults of :1363-1384: unmapped / secondary / QC-fail / duplicate
//     reads are skipped (the align stage writes none), a read starting outside the reference is skipped, min_mq is 0, and
//     without -A a paired read that is not in a proper pair is skipped (MPLP_NO_ORPHAN, :294);
//   * bam_plp_push (htslib-1.20/sam.c:6097-6151): a read is dropped when the pileup already stands at its start position
//     (an earlier read with that start was pushed) and more than maxcnt nodes are live -- the live reads are the pushed
//     ones that end behind the last position taken (bam_plp64_next removes a read once its end <= that position), plus the
//     list's tail sentinel, so it is dropped when max_depth or more pushed reads end at or behind its start;
//   * overlap_push (sam.c:5969-6003): mates are reconciled when both were pushed and both are proper.
// O(records + genome length), one pass; its product is one byte and one rank per read.
//
// pmx_pileup_bias runs k_pileup_bias over the device state the last run left (kept in the handle until the next run).
#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "device/dev_util.hpp"
#include "host/bam_writer.hpp"
#include "pileup_kernels.h"
#include "readset.hpp"

using namespace pmx;

struct pmx_pileup {
    int64_t ref_len = 0, n_reads = 0, bytes = 0;
    DevBuf<uint32_t> hist, aux, rank, first_ge, s_idx;
    DevBuf<int32_t> s_rs, late_idx;
    DevBuf<uint8_t> rinfo, effq, late_q;
    // pmx_pileup_run_records: the uploaded inputs
    DevBuf<pmx_aln_record> recs;
    DevBuf<uint32_t> cigars;
    DevBuf<uint8_t> ascii, qual;
    DevBuf<int64_t> off;
    std::vector<uint8_t> h_rinfo;
    std::vector<uint32_t> h_rank;
    // pmx_pileup_bias: the arguments of the last run (its sorted starts, admit flags, reconciled qualities and late_* stay
    // in the buffers above until the next run) and the pass's own buffers
    PileupArgs last;
    bool have_run = false;
    DevBuf<int32_t> b_sites;
    DevBuf<uint8_t> b_ref;
    DevBuf<uint32_t> b_out;
};

namespace {

// the name hash of tweak_overlap_quality (sam.c:5853): __ac_Wang_hash(__ac_X31_hash_string(qname)) & 1 (htslib/khash.h:399-449)
bool first_mate_keeps(const std::string& qname) {
    uint32_t h = qname.empty() ? 0u : (uint32_t)(int)(signed char)qname[0];
    for (size_t i = 1; i < qname.size(); ++i) h = (h << 5) - h + (uint32_t)(int)(signed char)qname[i];
    h += ~(h << 15); h ^= h >> 10; h += h << 3; h ^= h >> 6; h += ~(h << 11); h ^= h >> 16;
    return (h & 1u) != 0;
}

struct Sweep {
    std::vector<uint8_t> rinfo;
    std::vector<uint32_t> rank, first_ge, s_idx;
    std::vector<int32_t> s_rs;
    int32_t max_span = 0;
};

void sweep(const pmx_aln_record* recs, int64_t n, int64_t n_words, const int64_t* off, int64_t ref_len, bool paired, int max_depth,
           const char* names, const int64_t* name_off, Sweep& sw) {
    sw.rinfo.assign((size_t)n, 0);
    sw.rank.assign((size_t)n, UINT32_MAX);
    sw.first_ge.assign((size_t)ref_len + 2, UINT32_MAX);
    // the records write_bam writes, in its input order: both mates of every valid pair whose first record is mapped
    // (cli/panmap_main.cpp and api.records_to_results build the results that way)
    const int64_t unit = paired ? 2 : 1;
    std::vector<int64_t> written;
    std::vector<int32_t> sort_pos;
    written.reserve((size_t)n);
    for (int64_t u = 0; u + unit <= n; u += unit) {
        const uint16_t fl = paired ? (uint16_t)(recs[u].flags | recs[u + 1].flags) : recs[u].flags;
        if ((fl & (PMX_ALN_OVERFLOW | PMX_ALN_UNSUPPORTED)) || !recs[u].mapped) continue;
        for (int64_t r = u; r < u + unit; ++r) {
            written.push_back(r);
            sort_pos.push_back(recs[r].mapped && (recs[r].flags & PMX_ALN_HAS_ALN) ? recs[r].rs + 1 : INT_MAX);
        }
    }
    const std::vector<std::pair<int32_t, size_t>> order = bam_record_order(sort_pos);
    std::vector<uint32_t> cnt_end((size_t)ref_len + 2, 0);
    int64_t admitted = 0, expired = 0, swept = 0;   // expired = admitted reads with end < swept
    int32_t last_start = -1;
    for (size_t k = 0; k < order.size(); ++k) {
        const int64_t r = written[order[k].second];
        const pmx_aln_record& rec = recs[r];
        sw.rank[(size_t)r] = (uint32_t)k;
        if (!rec.mapped || !(rec.flags & PMX_ALN_HAS_ALN)) continue;
        if (paired && !rec.proper_frag) continue;                    // MPLP_NO_ORPHAN
        if (rec.rs < 0 || rec.rs >= ref_len) continue;               // mpileup.c:239-243
        const int64_t len = off[r + 1] - off[r];
        if (rec.re <= rec.rs || rec.re > ref_len || rec.qs < 0 || rec.qe > len || rec.qe < rec.qs ||
            (int64_t)rec.cigar_off + rec.n_cigar > n_words)
            throw std::runtime_error("pileup: alignment record " + std::to_string(r) + " is inconsistent with its read or the reference");
        if (max_depth > 0 && rec.rs == last_start) {
            for (; swept < rec.rs; ++swept) expired += cnt_end[(size_t)swept];
            if (admitted - expired >= max_depth) continue;           // sam.c:6104
        }
        last_start = rec.rs;
        ++admitted;
        ++cnt_end[(size_t)rec.re];
        sw.rinfo[(size_t)r] |= PLP_ADMIT;
        sw.s_rs.push_back(rec.rs);
        sw.s_idx.push_back((uint32_t)r);
        sw.max_span = std::max(sw.max_span, rec.re - rec.rs);
    }
    {   // first_ge[pos] = rank of the first admitted read with start >= pos
        int64_t pos = 0;
        for (size_t j = 0; j < sw.s_rs.size(); ++j)
            for (; pos <= sw.s_rs[j]; ++pos) sw.first_ge[(size_t)pos] = sw.rank[sw.s_idx[j]];
    }
    if (!paired) return;
    for (int64_t u = 0; u + 2 <= n; u += 2) {
        if (!(sw.rinfo[(size_t)u] & sw.rinfo[(size_t)u + 1] & PLP_ADMIT)) continue;
        const int64_t ra = sw.rank[(size_t)u] < sw.rank[(size_t)u + 1] ? u : u + 1, rb = ra == u ? u + 1 : u;
        std::string qname;
        if (names && name_off) {
            qname.assign(names + name_off[ra], (size_t)(name_off[ra + 1] - name_off[ra]));
            const size_t z = qname.find('\0');
            if (z != std::string::npos) qname.resize(z);
            if (qname.size() >= 2 && qname[qname.size() - 2] == '/' && (qname.back() == '1' || qname.back() == '2')) qname.resize(qname.size() - 2);
        } else qname = "r" + std::to_string(ra);
        const bool a_keeps = first_mate_keeps(qname);
        sw.rinfo[(size_t)ra] |= PLP_TWEAK | (a_keeps ? PLP_KEEP : 0);
        sw.rinfo[(size_t)rb] |= PLP_TWEAK | PLP_SECOND | (a_keeps ? 0 : PLP_KEEP);
    }
}

int run_core(pmx_ctx* ctx, pmx_pileup* pu, const pmx_aln_record* h_recs, int64_t n, int64_t n_words, const int64_t* h_off, const pmx_aln_record* d_recs,
             const uint32_t* d_cigars, const uint8_t* d_ascii, const uint8_t* d_qual, const int64_t* d_off, int64_t ref_len, int paired,
             int revcomp_mate2, const char* names, const int64_t* name_off, const pmx_pileup_params* pp_in) {
    pmx_pileup_params pp;
    pmx_pileup_default_params(&pp);
    if (pp_in) pp = *pp_in;
    if (ref_len <= 0 || ref_len > INT32_MAX - 2) return fail(PMX_ERR_ARG, "pileup: reference length out of range");
    if (paired && (n & 1)) return fail(PMX_ERR_ARG, "pileup: a paired read set has an even number of reads");
    if (pp.max_depth < 0 || pp.min_baseq < 0 || pp.delta_baseq < 0 || pp.cap_mapq < 0 || pp.cap_mapq > 63)
        return fail(PMX_ERR_ARG, "pileup: parameters out of range");
    pu->have_run = false;
    Sweep sw;
    sweep(h_recs, n, n_words, h_off, ref_len, paired != 0, pp.max_depth, names, name_off, sw);
    const int64_t total = h_off[n] - h_off[0];
    pu->ref_len = ref_len;
    pu->n_reads = n;
    pu->hist.ensure((size_t)ref_len * PLP_HIST);
    pu->aux.ensure((size_t)ref_len * PLP_AUX);
    pu->rinfo.ensure((size_t)n);
    pu->rank.ensure((size_t)n);
    pu->first_ge.ensure(sw.first_ge.size());
    pu->late_idx.ensure((size_t)n);
    pu->late_q.ensure((size_t)n);
    pu->effq.ensure((size_t)h_off[n] + 1);
    pu->s_rs.ensure(sw.s_rs.size());
    pu->s_idx.ensure(sw.s_idx.size());
    hipStream_t st = ctx->stream;
    if (n > 0) {
        PMX_H2D(pu->rinfo, sw.rinfo, n, st);
        PMX_H2D(pu->rank, sw.rank, n, st);
    }
    PMX_H2D(pu->first_ge, sw.first_ge, st);
    if (!sw.s_rs.empty()) {
        PMX_H2D(pu->s_rs, sw.s_rs, st);
        PMX_H2D(pu->s_idx, sw.s_idx, st);
    }
    PileupArgs a;
    memset(&a, 0, sizeof(a));
    a.recs = d_recs; a.cigars = d_cigars; a.ascii = d_ascii; a.qual = d_qual; a.off = d_off;
    a.rinfo = pu->rinfo.p; a.rank = pu->rank.p; a.first_ge = pu->first_ge.p;
    a.effq = pu->effq.p; a.late_idx = pu->late_idx.p; a.late_q = pu->late_q.p;
    a.n_reads = n; a.ref_len = (int32_t)ref_len; a.paired = paired ? 1 : 0; a.revcomp_mate2 = revcomp_mate2 ? 1 : 0;
    a.s_rs = pu->s_rs.p; a.s_idx = pu->s_idx.p; a.n_sorted = (int64_t)sw.s_rs.size(); a.max_span = sw.max_span;
    a.hist = pu->hist.p; a.aux = pu->aux.p;
    a.min_baseq = pp.min_baseq; a.max_baseq = pp.max_baseq; a.delta_baseq = pp.delta_baseq; a.cap_mapq = pp.cap_mapq;
    const int64_t n_units = paired ? n / 2 : n;
    timer_begin(ctx, "pileup_quals");
    if (n_units > 0) PMX_LAUNCH(k_pileup_quals, dim3(grid_for(n_units, 256, ctx->n_cu * 16)), dim3(256), 0, st, a);
    timer_end(ctx, "pileup_quals", 1);
    const int64_t n_windows = (ref_len + PLP_WINDOW - 1) / PLP_WINDOW;
    timer_begin(ctx, "pileup");
    PMX_LAUNCH(k_pileup_window, dim3((unsigned)std::min<int64_t>(n_windows, (int64_t)ctx->n_cu * 64)), dim3(256), 0, st, a);
    timer_end(ctx, "pileup", 1);
    PMX_HIP(hipStreamSynchronize(st));
    pu->h_rinfo.swap(sw.rinfo);
    pu->h_rank.swap(sw.rank);
    pu->last = a;
    pu->have_run = true;
    // bases + qualities read, reconciled qualities written and read back, records + CIGARs, the sweep's arrays, the tables
    pu->bytes = 4 * total + n * (int64_t)(sizeof(pmx_aln_record) + 8 + 1 + 4 + 5) + 4 * n_words + 8 * (int64_t)sw.s_rs.size() +
                ref_len * (int64_t)(4 * PLP_CELLS + 4);
    return PMX_OK;
}

}  // namespace

extern "C" {

void pmx_pileup_default_params(pmx_pileup_params* pp) {
    if (!pp) return;
    memset(pp, 0, sizeof(*pp));
    pp->max_depth = 250; pp->min_baseq = 1; pp->max_baseq = 60; pp->delta_baseq = 30; pp->cap_mapq = 60;
}

int pmx_pileup_create(pmx_ctx* ctx, pmx_pileup** out) {
    if (!ctx || !out) return PMX_ERR_ARG;
    *out = new pmx_pileup();
    return PMX_OK;
}

void pmx_pileup_free(pmx_ctx* ctx, pmx_pileup* pu) {
    if (ctx) (void)hipSetDevice(ctx->device);
    delete pu;
}

int pmx_pileup_run(pmx_ctx* ctx, pmx_pileup* pu, pmx_aligner* al, const pmx_readset* rs, int64_t ref_len, int paired, int revcomp_mate2,
                   const char* names_concat, const int64_t* name_offsets, const pmx_pileup_params* pp) {
    if (!ctx || !pu || !al || !rs) return PMX_ERR_ARG;
    if (rs->hpc) return fail(PMX_ERR_ARG, "the read set is homopolymer-compressed: the pileup reads the bases the aligner saw, pass the uncompressed read set");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    const int64_t n = pmx_align_num_records(al);
    if (n != rs->n) return fail(PMX_ERR_ARG, "pileup: the aligner's last results are not those of this read set");
    const int64_t words = pmx_align_cigar_words(ctx, al);
    if (words < 0) return (int)words;
    std::vector<pmx_aln_record> recs((size_t)std::max<int64_t>(n, 1));
    std::vector<int64_t> off((size_t)n + 1);
    PMX_D2H(recs, pmx_align_device_records(al), n, ctx->stream);
    PMX_D2H_SYNC(off, rs->off, (size_t)n + 1, ctx->stream);
    if (rs->has_qual && rs->off0 != 0) return fail(PMX_ERR_ARG, "pileup: qualities need a read set whose offsets start at 0");
    return run_core(ctx, pu, recs.data(), n, words, off.data(), (const pmx_aln_record*)pmx_align_device_records(al),
                    (const uint32_t*)pmx_align_device_cigars(al), rs->ascii.p, rs->has_qual ? rs->qual.p : nullptr, rs->off.p, ref_len, paired,
                    revcomp_mate2, names_concat, name_offsets, pp);
    PMX_CATCH
}

int pmx_pileup_run_records(pmx_ctx* ctx, pmx_pileup* pu, const pmx_aln_record* records, int64_t n, const uint32_t* cigar_arena, int64_t n_words,
                           const char* concat, const char* qual_concat, const int64_t* offsets, int64_t ref_len, int paired, int revcomp_mate2,
                           const char* names_concat, const int64_t* name_offsets, const pmx_pileup_params* pp) {
    if (!ctx || !pu || n < 0 || n_words < 0 || !offsets || (n > 0 && (!records || !concat)) || (n_words > 0 && !cigar_arena)) return PMX_ERR_ARG;
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (offsets[0] != 0) return fail(PMX_ERR_ARG, "pileup: offsets start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(PMX_ERR_ARG, "pileup: read offsets are not monotone");
    const int64_t total = offsets[n];
    pu->recs.ensure((size_t)n);
    pu->cigars.ensure((size_t)n_words);
    pu->ascii.ensure((size_t)total + 1);
    pu->off.ensure((size_t)n + 1);
    hipStream_t st = ctx->stream;
    PMX_H2D(pu->recs, records, n, st);
    PMX_H2D(pu->cigars, cigar_arena, n_words, st);
    PMX_H2D(pu->ascii, concat, total, st);
    PMX_H2D(pu->off, offsets, (size_t)n + 1, st);
    if (qual_concat) {
        pu->qual.ensure((size_t)total + 1);
        PMX_H2D(pu->qual, qual_concat, total, st);
    }
    return run_core(ctx, pu, records, n, n_words, offsets, pu->recs.p, pu->cigars.p, pu->ascii.p, qual_concat ? pu->qual.p : nullptr, pu->off.p, ref_len,
                    paired, revcomp_mate2, names_concat, name_offsets, pp);
    PMX_CATCH
}

int pmx_pileup_fetch(pmx_ctx* ctx, pmx_pileup* pu, uint32_t* hist, uint32_t* aux) {
    if (!ctx || !pu) return PMX_ERR_ARG;
    if (pu->ref_len <= 0) return fail(PMX_ERR_ARG, "pileup: nothing has been run");
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    if (hist) PMX_D2H(hist, pu->hist, (size_t)pu->ref_len * PLP_HIST, ctx->stream);
    if (aux) PMX_D2H(aux, pu->aux, (size_t)pu->ref_len * PLP_AUX, ctx->stream);
    PMX_HIP(hipStreamSynchronize(ctx->stream));
    return PMX_OK;
    PMX_CATCH
}

int pmx_pileup_bias(pmx_ctx* ctx, pmx_pileup* pu, const int32_t* positions, const char* ref_bases, int64_t n_sites, uint32_t* out) {
    if (!ctx || !pu || n_sites < 0) return PMX_ERR_ARG;
    if (n_sites == 0) return PMX_OK;
    if (!positions || !ref_bases || !out) return PMX_ERR_ARG;
    if (!pu->have_run) return fail(PMX_ERR_ARG, "pileup bias: nothing has been run");
    for (int64_t i = 0; i < n_sites; ++i) {
        if (positions[i] < 0 || positions[i] >= pu->ref_len)
            return fail(PMX_ERR_ARG, "pileup bias: position " + std::to_string(positions[i]) + " is outside the reference (length " + std::to_string(pu->ref_len) + ")");
        if (i > 0 && positions[i] <= positions[i - 1])
            return fail(PMX_ERR_ARG, "pileup bias: positions must be strictly ascending (entry " + std::to_string(i) + ")");
    }
    PMX_TRY
    PMX_HIP(hipSetDevice(ctx->device));
    pu->b_sites.ensure((size_t)n_sites);
    pu->b_ref.ensure((size_t)n_sites);
    pu->b_out.ensure((size_t)n_sites * PLB_CELLS);
    hipStream_t st = ctx->stream;
    PMX_H2D(pu->b_sites, positions, n_sites, st);
    PMX_H2D(pu->b_ref, ref_bases, n_sites, st);
    PileupBiasArgs b;
    b.run = pu->last;
    b.sites = pu->b_sites.p; b.ref_bases = pu->b_ref.p; b.n_sites = n_sites; b.out = pu->b_out.p;
    timer_begin(ctx, "pileup_bias");
    PMX_LAUNCH(k_pileup_bias, dim3((unsigned)std::min<int64_t>(n_sites, (int64_t)ctx->n_cu * 16)), dim3(256), 0, st, b);
    timer_end(ctx, "pileup_bias", 1);
    PMX_D2H_SYNC(out, pu->b_out, (size_t)n_sites * PLB_CELLS, st);
    return PMX_OK;
    PMX_CATCH
}

int pmx_pileup_read_info(const pmx_pileup* pu, uint8_t* flags, uint32_t* bam_rank, int64_t cap) {
    if (!pu || cap < pu->n_reads) return PMX_ERR_ARG;
    if (flags && pu->n_reads > 0) memcpy(flags, pu->h_rinfo.data(), (size_t)pu->n_reads);
    if (bam_rank && pu->n_reads > 0) memcpy(bam_rank, pu->h_rank.data(), sizeof(uint32_t) * (size_t)pu->n_reads);
    return PMX_OK;
}

int64_t pmx_pileup_bytes(const pmx_pileup* pu) { return pu ? pu->bytes : 0; }

}  // extern "C"
