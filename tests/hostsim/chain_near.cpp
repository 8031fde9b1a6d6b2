// CPU unit-test build of the compact tier's near class (compact_near_class, panmap_amd/csrc/align/aln_compact_simple.hpp)
// beside the two forms its pairs must agree with.  TEST INFRASTRUCTURE, like chain_simple.cpp: never linked into
// libpanmap_amd.so.  Every pair goes through compact_seed_pair into hand-over words, as k_compact_seeds leaves them; from
// those words
//   * the class, as k_compact_classes_near16/32 decide it: marked by the seeding, or compact_near_class,
//   * compact_chain_simple, when the pair is of either class (what k_align_simple runs),
//   * compact_chain_pair with the first form's 48 anchors (k_align_compact),
//   * compact_chain_pair<true> (k_align_compact*_multi: where a pair goes that the path bails on).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align/aln_host.hpp"
#include "align/aln_compact.hpp"
#include "align/aln_compact_simple.hpp"

using namespace pmx::aln;

static void put_records(const CResult& res, bool done, AlnRecord* recs, uint32_t* cigars, int32_t* edits, int it) {
    for (int s = 0; s < 2; ++s) {
        AlnRecord& rec = recs[2 * it + s];
        memset(&rec, 0, sizeof(rec));
        cigars[2 * it + s] = 0;
        edits[2 * it + s] = done ? res.edit[s] : -1;
        if (!done || !res.mapped) continue;
        const CMate& t = res.m[s];
        rec.mapped = 1;
        rec.flags = PMX_REC_HAS_ALN;
        rec.rs = t.rs; rec.re = t.re; rec.qs = t.qs; rec.qe = t.qe;
        rec.mapq = t.mapq; rec.rev = t.rev; rec.proper_frag = t.proper_frag;
        rec.n_cigar = 1;
        rec.score = t.dp_max;
        rec.cigar_off = (uint32_t)(2 * it + s);
        cigars[2 * it + s] = t.cigar;
    }
}

// cls[pair]: 0 the seeding bailed, 1 of neither class, 2 marked by the seeding and finished by compact_chain_simple, 3 marked
// and bailed, 4 of the near class and finished, 5 of the near class and bailed.
// bound[pair]: 1 when the pair is not marked, both mates have a seed, the first form's memory holds the seeds and the mates'
// extents (each projected from its first seed, as compact_seed_pair does) overlap by at most k - 1 bases: the class a rule
// without the junction read would give (tools/chain_fill_divergence.py compares the two).
// recs / cigars / edits: [0] the register-only path, [1] the first form, [2] the second form (2 * pairs entries each; edits -1
// where the form did not finish the pair); done: [1], [2].
extern "C" int hs_chain_near(const char* ref, int64_t ref_len, int n_reads, const char** reads, const int* lens, int rc2, int pos32, int want_edits,
                             int8_t* cls, int8_t* bound, AlnRecord* const* recs, uint32_t* const* cigars, int32_t* const* edits, int8_t* const* done) {
    int64_t total = 0;
    int max_len = 0;
    for (int i = 0; i < n_reads; ++i) { total += lens[i]; max_len = std::max(max_len, lens[i]); }
    const int avg_len = n_reads > 0 ? (int)(total / n_reads) : 150;
    Opt o = make_opt(avg_len);
    HostRefIndex hri;
    build_ref_index(ref, ref_len, o, std::max(4096, max_len * (o.a + 1) * 2 + 64), hri);
    const RefIndex ri = hri.view();
    std::vector<uint32_t> lds(CMemT<uint32_t>::kWords + 8);
    std::vector<uint8_t> pen(PMX_C_PEN_BYTES);
    for (int dd = 0; dd < PMX_C_PEN_DIFF; ++dd) {
        int ps, pd;
        c_pen_values(o.chn_pen_gap, dd, &ps, &pd);
        if (dd < PMX_C_PEN_SAME) pen[(size_t)dd] = (uint8_t)(ps < 255 ? ps : 255);
        pen[(size_t)PMX_C_PEN_SAME + dd] = (uint8_t)(pd < 255 ? pd : 255);
    }
    const CPenTab tab{pen.data(), pen.data() + PMX_C_PEN_SAME};
    const bool pos16 = ref_len <= 32767 && !pos32;
    for (int it = 0; it < n_reads / 2; ++it) {
        std::vector<uint64_t> w[2];
        std::vector<uint32_t> am[2];
        CRead rd[2];
        const uint32_t* amb[2];
        for (int s = 0; s < 2; ++s) {
            const int idx = 2 * it + s, len = lens[idx];
            w[s].assign((size_t)(len + 31) / 32 + 1, 0);
            am[s].assign((size_t)(len + 31) / 32 + 1, 0);
            for (int i = 0; i < len; ++i) {   // k_pack_reads (place_kernels.hip)
                const unsigned char ch = (unsigned char)reads[idx][i] & 0xDF;
                const bool acgt = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
                const uint64_t code = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : (ch == 'T' || ch == 'U') ? 3 : 0;
                w[s][(size_t)(i >> 5)] |= code << (2 * (i & 31));
                if (!acgt) am[s][(size_t)(i >> 5)] |= 1u << (i & 31);
            }
            rd[s].w = w[s].data();
            rd[s].len = len;
            rd[s].flip = rc2 && s == 1;
            amb[s] = am[s].data();
        }
        std::vector<uint32_t> q(2 * PMX_C_SEEDQ, 0xdeadbeefu), ho((size_t)PMX_C_CAP * 2, 0xdeadbeefu);
        SReg mregs[PMX_CM_SREGS];
        uint32_t mints[PMX_CM_INTS];
        const SWork mw{mregs, mints};
        auto run = [&](auto pt) {
            typedef decltype(pt) PT;
            uint32_t stage[8];
            CSeedOutT<PT> so{q.data(), ho.data(), stage};
            int n_s = 0, n_s0 = 0;
            bool simple = false;
            CResult res;
            res.mapped = 0;
            cls[it] = 0;
            bound[it] = 0;
            done[1][it] = done[2][it] = 0;
            for (int f = 0; f < 3; ++f) put_records(res, false, recs[f], cigars[f], edits[f], it);
            if (compact_seed_pair(so, o, ri, rd, amb, &n_s, &n_s0, nullptr, false, &simple) != PMX_C_DONE) return;
            cls[it] = 1;
            // k_compact_classes_near*: the near class only where the seeding left no mark
            const bool near = !simple && compact_near_class<PT>(so.out, n_s, n_s0, o);
            if (!simple && n_s0 >= 1 && n_s - n_s0 >= 1 && n_s <= PMX_C_CAP1) {
                int32_t ext[2];
                for (int s = 0; s < 2; ++s) {
                    uint32_t x, y;
                    so.get(s ? n_s0 : 0, &x, &y);
                    const int32_t rpos = (int32_t)(x >> 1), qm = (int32_t)((y & 0x3ffu) >> 1) - (s ? rd[0].len : 0);
                    ext[s] = ((x ^ y) & 1u) ? rpos + qm - (o.k - 1) - (rd[s].len - 1) : rpos - qm;
                }
                bound[it] = ext[1] >= ext[0] + rd[0].len - (o.k - 1) || ext[0] >= ext[1] + rd[1].len - (o.k - 1);
            }
            if (simple || near) {
                const int rc = compact_chain_simple(so, o, ri, rd, n_s, n_s0, res, tab, want_edits != 0);
                cls[it] = (int8_t)((simple ? 2 : 4) + (rc == PMX_C_DONE ? 0 : 1));
                put_records(res, rc == PMX_C_DONE, recs[0], cigars[0], edits[0], it);
            }
            if (n_s <= PMX_C_CAP1) {
                std::fill(lds.begin(), lds.end(), 0xdeadbeefu);
                CMemT<PT, PMX_C_CAP1> m1{lds.data()};
                for (int i0 = 0; i0 < n_s; i0 += 4) {
                    uint32_t x[4], y[4];
                    so.get4(i0, x, y);
                    for (int b = 0; b < 4 && i0 + b < n_s; ++b) m1.setSeed(i0 + b, x[b], y[b]);
                }
                const int rc = compact_chain_pair(m1, o, ri, rd, n_s, n_s0, res, tab, nullptr, want_edits != 0);
                done[1][it] = rc == PMX_C_DONE;
                put_records(res, rc == PMX_C_DONE, recs[1], cigars[1], edits[1], it);
            }
            {
                std::fill(lds.begin(), lds.end(), 0xdeadbeefu);
                CMemT<PT> m{lds.data()};
                for (int i0 = 0; i0 < n_s; i0 += 4) {
                    uint32_t x[4], y[4];
                    so.get4(i0, x, y);
                    for (int b = 0; b < 4 && i0 + b < n_s; ++b) m.setSeed(i0 + b, x[b], y[b]);
                }
                const int rc = compact_chain_pair<true>(m, o, ri, rd, n_s, n_s0, res, tab, nullptr, want_edits != 0, false, &mw);
                done[2][it] = rc == PMX_C_DONE;
                put_records(res, rc == PMX_C_DONE, recs[2], cigars[2], edits[2], it);
            }
        };
        if (pos16) run((uint16_t)0);
        else run((uint32_t)0);
    }
    return 0;
}
