// Calls, filter and writers of the genotype / consensus stages (host; C ABI pmx_genotype_*, include/panmap_amd.h).
//
// The reference forks `bcftools call --ploidy 1 -m -A` on the output of `bcftools mpileup`, filters the lines with
// genotyping::applyMutationSpectrum / passesConsensusGate and forks `bcftools consensus`
// (src/conversion.cpp:130-255, src/genotyping.cpp:167-279).  Restated here as functions of the pileup tables:
//   * the htslib error model: errmod_cal with cal_coef's tables (src/3rdparty/samtools/htslib-1.20/errmod.c:51-208);
//   * allele order, PL and DP4 of a site: bcf_call_combine (src/3rdparty/bcftools/bam2bcf.c:955-1115); MQ as mcall.c:1659;
//   * the substitution spectrum of the tree (src/index_single_mode.cpp:1408-1558) as phred (src/main.cpp:290-311);
//   * the filter, line by line as the reference applies it.
//   * on request (pmx_genotype_annotate), the bias annotations of bcf_call_combine -- VDB, SGB, the five Mann-Whitney
//     Z scores, MQ0F -- from the histograms of the device's bias pass (bam2bcf.c:596-657, 813-927, 1152-1173).
// Not restated: INDEL records, BAQ and the QUAL of `call -m`.  A site is a
// candidate when an alternative base has a non-zero quality sum, and its record lists every such base, as `call -m -A`
// does (pinned to the reference's programs by tests/test_pileup_reference.py).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../api_internal.hpp"
#include "panman.hpp"

namespace pmx {
const Panman& panman_of(const pmx_panman* pm);   // api_host.cpp
}

namespace {

constexpr int NQ = 64, NB = 5, HIST = NQ * 2 * NB;

// ------------------------------------------------------------------------------------------------ error model
// cal_coef (errmod.c:66-112) with depcorr = 1 - CALL_DEFTHETA = 0.17 and eta = 0.03 (bam2bcf.c:47-54, errmod.c:123):
//   fk[n]         = 0.83^n * 0.97 + 0.03
//   beta[q][n][k] : phred of "k-th error among n bases of quality q" from the binomial tail, by the reference's recurrence
//   lhet[n][k]    = log C(n, k) - n log 2
// The reference fills 64 x 256 x 256 doubles up front; a site touches a few (q, n) rows, made here when first asked for.
double log_binom(int n, int k) { return k <= 0 || k > n ? 0.0 : lgamma(n + 1.0) - lgamma(k + 1.0) - lgamma(n - k + 1.0); }

double fk_of(int n) { return n == 0 ? 1.0 : pow(1.0 - 0.17, n) * (1.0 - 0.03) + 0.03; }

const std::vector<double>& beta_row(int q, int n) {
    static std::mutex mu;
    static std::map<int, std::vector<double>> rows;
    std::lock_guard<std::mutex> g(mu);
    std::vector<double>& row = rows[q << 8 | n];
    if (!row.empty()) return row;
    row.assign((size_t)n + 1, 0.0);
    const double e = pow(10.0, -q / 10.0), le = log(e), le1 = log(1.0 - e);
    double sum1 = log_binom(n, n) + n * le, sum = 0;
    row[(size_t)n] = HUGE_VAL;
    for (int k = n - 1; k >= 0; --k, sum1 = sum) {
        sum = sum1 + log1p(exp(log_binom(n, k) + k * le + (n - k) * le1 - sum1));
        row[(size_t)k] = -10.0 / M_LN10 * (sum1 - sum);
    }
    return row;
}

// More than 255 bases: errmod_cal shuffles them with a shared random generator and keeps 255 (errmod.c:156-159), which
// is no function of the site.  Here each (quality, strand, base) class keeps its share of 255, largest remainders first
// (ties: the higher class code) -- the expectation of that draw.
void thin_to_255(std::vector<std::pair<int, int64_t>>& classes, int64_t n) {
    std::vector<std::pair<int64_t, int>> rem;
    int64_t kept = 0;
    for (size_t i = 0; i < classes.size(); ++i) {
        const int64_t c = classes[i].second, share = c * 255 / n;
        rem.emplace_back(-(c * 255 % n), -(int)i);
        classes[i].second = share;
        kept += share;
    }
    std::sort(rem.begin(), rem.end());
    for (size_t j = 0; kept < 255 && j < rem.size(); ++j, ++kept) ++classes[(size_t)(-rem[j].second)].second;
}

// errmod_cal (errmod.c:143-208) for m = 5 over the classes of hist[pos]; q[25] as floats, like the reference's
int64_t error_model(const uint32_t* hist, float q[25]) {
    for (int i = 0; i < 25; ++i) q[i] = 0.f;
    // the sort key of bca->bases is quality << 5 | strand << 4 | base (bam2bcf.c:461): ascending class codes
    std::vector<std::pair<int, int64_t>> classes;
    int64_t n_all = 0;
    for (int ql = 0; ql < NQ; ++ql)
        for (int s = 0; s < 2; ++s)
            for (int b = 0; b < NB; ++b) {
                const uint32_t c = hist[(ql * 2 + s) * NB + b];
                if (c) { classes.emplace_back(ql << 5 | s << 4 | b, (int64_t)c); n_all += c; }
            }
    if (n_all == 0) return 0;
    int n = (int)std::min<int64_t>(n_all, 255);
    if (n_all > 255) thin_to_255(classes, n_all);
    double fsum[NB] = {0}, bsum[NB] = {0};
    int c[NB] = {0}, w[32] = {0};
    for (size_t ci = classes.size(); ci-- > 0;) {   // from the highest quality down, as the sorted array is read
        const int code = classes[ci].first, qual = std::min(std::max(code >> 5, 4), 63), bs = code & 0x1f, base = code & 0xf;
        const std::vector<double>& beta = beta_row(qual, n);
        for (int64_t t = 0; t < classes[ci].second; ++t) {
            const double f = fk_of(w[bs]);
            fsum[base] += f;
            bsum[base] += f * beta[(size_t)c[base]];
            ++c[base];
            ++w[bs];
        }
    }
    for (int j = 0; j < NB; ++j) {
        float tmp1 = 0.f;
        int tmp2 = 0;
        for (int k = 0; k < NB; ++k) {
            if (k == j) continue;
            tmp1 = (float)(tmp1 + bsum[k]);
            tmp2 += c[k];
        }
        if (tmp2) q[j * NB + j] = tmp1;
        for (int k = j + 1; k < NB; ++k) {
            const int cjk = c[j] + c[k];
            tmp1 = 0.f;
            tmp2 = 0;
            for (int i = 0; i < NB; ++i) {
                if (i == j || i == k) continue;
                tmp1 = (float)(tmp1 + bsum[i]);
                tmp2 += c[i];
            }
            const double lhet = log_binom(cjk, c[k]) - M_LN2 * cjk;
            q[j * NB + k] = q[k * NB + j] = tmp2 ? (float)(-4.343 * lhet + tmp1) : (float)(-4.343 * lhet);
        }
        for (int k = 0; k < NB; ++k)
            if (q[j * NB + k] < 0.0f) q[j * NB + k] = 0.0f;
    }
    return n_all;
}

int base_index(char c) {   // seq_nt16_int of the letter: A C G T -> 0..3, everything else 4
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}

// bcf_call_combine for one sample (bam2bcf.c:955-1115)
void site_call(const uint32_t* hist, char ref_base, pmx_site_call* out) {
    memset(out, 0, sizeof(*out));
    float p[25];
    out->n_bases = (int32_t)std::min<int64_t>(error_model(hist, p), INT32_MAX);
    const int ref4 = base_index(ref_base);
    // QS: sum of the capped qualities per base (bam2bcf.c:465-467); AD: bases per allele; DP4 from anno[0..3] (:476)
    int64_t qs[4] = {0, 0, 0, 0}, ad[NB] = {0}, dp4[4] = {0, 0, 0, 0};
    for (int ql = 0; ql < NQ; ++ql)
        for (int s = 0; s < 2; ++s)
            for (int b = 0; b < NB; ++b) {
                const int64_t c = hist[(ql * 2 + s) * NB + b];
                if (!c) continue;
                if (b < 4) qs[b] += c * ql;
                ad[b] += c;
                dp4[((ref4 < 4 && b == ref4) ? 0 : 2) + s] += c;
            }
    for (int i = 0; i < 4; ++i) out->dp4[i] = (int32_t)dp4[i];
    float qsum[5] = {0, 0, 0, 0, 0}, sum = 0;
    for (int j = 0; j < 4; ++j) sum += (float)qs[j];
    if (sum != 0)
        for (int j = 0; j < 4; ++j) qsum[j] += (float)qs[j] / sum;
    int ord[4] = {0, 1, 2, 3};   // ascending by qsum (insertion sort, strict <: equal sums keep their order)
    for (int i = 1; i < 4; ++i)
        for (int j = i; j > 0 && qsum[ord[j]] < qsum[ord[j - 1]]; --j) std::swap(ord[j], ord[j - 1]);
    int a[5] = {-1, -1, -1, -1, -1}, n_al = 1, i = 3, unseen = -1;
    a[0] = ref4;
    for (; i >= 0; --i) {
        if (ord[i] == ref4) continue;
        if (qsum[ord[i]] == 0) break;
        a[n_al++] = ord[i];
    }
    const int n_seen = n_al;
    if (((ref4 < 4 && n_al < 4) || (ref4 == 4 && n_al < 5)) && i >= 0) { unseen = n_al; a[n_al++] = ord[i]; }
    (void)unseen;
    // PL: the genotypes of a[] in VCF order, minimum subtracted, + .499 truncated, at most 255 (bam2bcf.c:1020-1046)
    float mn = 3.4e38f;
    for (int x = 0; x < n_al; ++x)
        for (int y = 0; y <= x; ++y) mn = std::min(mn, p[a[y] * NB + a[x]]);
    out->n_alleles = n_seen;
    for (int k = 0; k < n_seen; ++k) {
        int y = (int)(p[a[k] * NB + a[k]] - mn + .499);
        out->pl[k] = y > 255 ? 255 : y;
        out->alleles[k] = a[k];
        out->ad[k] = (int32_t)ad[a[k]];
    }
}

// ------------------------------------------------------------------------------------------------ filter
std::vector<std::string> split(const std::string& s, char sep) {   // std::getline semantics: no trailing empty field
    std::vector<std::string> out;
    std::istringstream ss(s);
    std::string f;
    while (std::getline(ss, f, sep)) out.push_back(f);
    return out;
}

int nuc_index(char c) {   // getIndexFromNucleotide (src/genotyping.cpp:112-125)
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; case '*': return 4; default: return 5; }
}

// passesConsensusGate (src/genotyping.cpp:167-174)
bool passes_gate(int called, const std::vector<int>& ad, int min_depth) {
    if (called <= 0) return false;
    if (ad.empty() || called >= (int)ad.size()) return true;
    long total = 0;
    for (int x : ad) total += x;
    if (total < min_depth) return false;
    return (long)ad[(size_t)called] * 2 > total;
}

// the sample-field form (src/genotyping.cpp:176-198)
bool passes_gate(const std::string& sample, int min_depth) {
    const std::vector<std::string> parts = split(sample, ':');
    if (parts.size() < 3) return true;
    int gt = 0;
    try { gt = std::stoi(parts[0]); } catch (...) { return true; }
    std::vector<int> ad;
    for (const std::string& x : split(parts[2], ','))
        try { ad.push_back(std::stoi(x)); } catch (...) {}
    return passes_gate(gt, ad, min_depth);
}

std::string fixed4(double v) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.4f", v);
    return buf;
}

// applyMutationSpectrum (src/genotyping.cpp:200-279); *called receives the allele index of a kept call
std::string apply_spectrum(const std::string& line, const double* sm, int min_depth, double min_qual, int* called) {
    const std::vector<std::string> f = split(line, '\t');
    if (f.size() < 10 || f[0] == "#CHROM") return line;
    if (f.size() != 10) throw std::runtime_error("Couldn't parse VCF. Unrecognized number of fields.");
    if (f[4] == ".") return "";
    if (f[7].substr(0, 2) != "DP" || f[3].empty() || nuc_index(f[3][0]) > 3) return (!f[9].empty() && f[9][0] == '0') ? "" : line;
    if (f[3].size() > 1) throw std::runtime_error("Error: reference allele parsing error.");
    const int ref = nuc_index(f[3][0]);
    std::vector<char> alts;
    for (const std::string& x : split(f[4], ',')) alts.push_back(x.empty() ? '.' : x[0]);
    const std::vector<std::string> sf = split(f[9], ':');
    if (sf.size() != 3) throw std::runtime_error("Couldn't parse VCF. Unrecognized sample format.");
    std::vector<double> pls;
    for (const std::string& x : split(sf[1], ',')) pls.push_back(std::stod(x));
    std::vector<int> ads;
    for (const std::string& x : split(sf[2], ',')) ads.push_back(std::stoi(x));
    std::vector<double> gls;
    if (alts.size() + 1 == pls.size()) gls = pls;
    else
        for (size_t i = 0; i < pls.size(); i += 2) {
            gls.push_back(pls[i]);
            if (gls.size() == alts.size() + 1) break;
        }
    if (gls.empty()) throw std::runtime_error("Couldn't parse VCF. No likelihoods.");
    gls[0] += sm[ref * 4 + ref];
    for (size_t i = 1; i < gls.size(); ++i) {
        const int alt = nuc_index(alts[i - 1]);
        if (alt <= 3) gls[i] += sm[ref * 4 + alt];   // a '*' ALT keeps its likelihood
    }
    const double mn = *std::min_element(gls.begin(), gls.end());
    int best = 0;
    for (size_t i = 0; i < gls.size(); ++i) {
        gls[i] -= mn;
        if (gls[i] == 0) best = (int)i;
    }
    if (best == 0) return "";
    if (!passes_gate(best, ads, min_depth)) return "";
    const double qual = gls[0];
    if (qual < min_qual) return "";
    if (called) *called = best;
    return f[0] + "\t" + f[1] + "\t" + f[2] + "\t" + f[3] + "\t" + f[4] + "\t" + fixed4(qual) + "\t" + f[6] + "\t" + f[7] + "\t" + f[8] + "\t" +
           std::to_string(best) + ":" + sf[1] + ":" + sf[2];
}

// the branch of createVcfWithMutationMatrices without a spectrum (src/conversion.cpp:163-178)
std::string plain_filter(const std::string& line, int min_depth, double min_qual) {
    if (line.empty()) return "";
    if (line[0] == '#') return line;
    const std::vector<std::string> f = split(line, '\t');
    const bool qual_ok = f.size() >= 6 && (f[5] == "." || std::stod(f[5]) >= min_qual);
    if (f.size() >= 10 && f[4] != "." && !f[9].empty() && f[9][0] != '0' && qual_ok && passes_gate(f[9], min_depth)) return line;
    return "";
}

// ------------------------------------------------------------------------------------------------ bias annotations
// kf_erfc (htslib-1.20/kfunc.c:58-84): the complementary error function by the rational approximation of Hart et al.,
// with a continued fraction in the tail.  Not libm's erfc: VDB values are printed to six digits down to 1e-37.
double kf_erfc(double x) {
    static const double p[7] = {220.2068679123761, 221.2135961699311, 112.0792914978709, 33.912866078383, 6.37396220353165, .7003830644436881,
                                .03526249659989109};
    static const double q[8] = {440.4137358247522, 793.8265125199484, 637.3336333788311, 296.5642487796737, 86.78073220294608, 16.06417757920695,
                                1.755667163182642, .08838834764831844};
    const double z = fabs(x) * M_SQRT2;
    if (z > 37.) return x > 0. ? 0. : 2.;
    const double expntl = exp(z * z * -.5);
    double r;
    if (z < 10. / M_SQRT2) {
        double num = p[6], den = q[7];
        for (int i = 5; i >= 0; --i) num = num * z + p[i];
        for (int i = 6; i >= 0; --i) den = den * z + q[i];
        r = expntl * num / den;
    } else r = expntl / 2.506628274631001 / (z + 1. / (z + 2. / (z + 3. / (z + 4. / (z + .65)))));
    return x > 0. ? 2. * r : 2. * (1. - r);
}

// calc_vdb (bam2bcf.c:596-657) over the alt bases' scaled positions: float accumulators, the truncation of the mean
// distance and the integer division of the depth-2 branch as the reference has them.  HUGE_VAL below two bases.
double calc_vdb(const uint32_t* pos, int npos) {
    static const float param[15][3] = {{3, 0.079, 18},   {4, 0.09, 19.8},  {5, 0.1, 20.5},   {6, 0.11, 21.5},  {7, 0.125, 21.6},
                                       {8, 0.135, 22},   {9, 0.14, 22.2},  {10, 0.153, 22.3}, {15, 0.19, 22.8}, {20, 0.22, 23.2},
                                       {30, 0.26, 23.4}, {40, 0.29, 23.5}, {50, 0.35, 23.65}, {100, 0.5, 23.7}, {200, 0.7, 23.7}};
    const int readlen = 100, nparam = 15;
    int dp = 0;
    float mean_pos = 0, mean_diff = 0;
    for (int i = 0; i < npos; ++i) {
        if (!pos[i]) continue;
        dp += (int)pos[i];
        mean_pos += (int)pos[i] * i;
    }
    if (dp < 2) return HUGE_VAL;
    mean_pos /= dp;
    for (int i = 0; i < npos; ++i) {
        if (!pos[i]) continue;
        mean_diff += (int)pos[i] * fabs((double)(i - mean_pos));   // float difference, double product, stored back into the float
    }
    mean_diff /= dp;
    const int ipos = (int)mean_diff;
    if (dp == 2) return (2 * readlen - 2 * (ipos + 1) - 1) * (ipos + 1) / (readlen - 1) / (readlen * 0.5);
    int i = nparam;
    if (dp < 200)
        for (i = 0; i < nparam; ++i)
            if (param[i][0] >= dp) break;
    float pshift, pscale;
    if (i == nparam) { pscale = param[nparam - 1][1]; pshift = param[nparam - 1][2]; }
    else if (i > 0 && param[i][0] != dp) {
        pscale = (param[i - 1][1] + param[i][1]) * 0.5;
        pshift = (param[i - 1][2] + param[i][2]) * 0.5;
    } else { pscale = param[i][1]; pshift = param[i][2]; }
    return 0.5 * kf_erfc(-(mean_diff - pshift) * pscale);
}

// calc_mwu_biasZ with do_Z = 1 (bam2bcf.c:813-864): the Mann-Whitney U of a against b as a Z score with the correction for
// ties; HUGE_VAL when either side is empty, 0 when the variance vanishes
double mwu_z(const uint32_t* a, const uint32_t* b, int n) {
    bool b_empty = true;
    for (int i = 0; i < n && b_empty; ++i) b_empty = b[i] == 0;
    int64_t t = 0, e = 0, l = 0, na = 0, nb = 0;
    for (int i = n - 1; i >= 0; --i) {
        const int64_t ai = a[i], bi = b_empty ? 0 : b[i];
        e += ai * bi;
        l += ai * nb;
        na += ai;
        nb += bi;
        const int64_t pi = ai + bi;
        t += (pi * pi - 1) * pi;
    }
    if (!na || !nb) return HUGE_VAL;
    const double U = l + e * 0.5, m = na * nb / 2.0;
    const double var2 = (na * nb) / 12.0 * ((na + nb + 1) - t / (double)((na + nb) * (na + nb - 1)));
    if (var2 <= 0) return 0;
    return (U - m) / sqrt(var2);
}

// calc_SegBias for one sample (bam2bcf.c:891-927): nref / nr = the reference / other bases of the site
double seg_bias(int nref, int nr) {
    if (!nr) return HUGE_VAL;
    const int n = 1, avg_dp = (nref + nr) / n;
    double M = floor((double)nr / avg_dp + 0.5);
    if (M > n) M = n;
    else if (M == 0) M = 1;
    const double f = M / 2. / n, p = (double)nr / n, q = (double)nr / M, log2 = log(2.0);
    const double x = log(2 * (1 - f)), y = log(f) + nr * log2 - q;
    double tmp = x > y ? log(1 + exp(y - x)) + x : log(1 + exp(x - y)) + y;
    tmp += log(f) + nr * log(q / p) - q + p;
    return tmp;
}

void site_tests(const uint32_t* hist, const uint32_t* aux, const uint32_t* bias, char ref_base, pmx_site_tests* out) {
    memset(out, 0, sizeof(*out));
    const int ref4 = base_index(ref_base);
    int64_t nref = 0, nr = 0;
    for (int c = 0; c < HIST; ++c) (ref4 < 4 && c % NB == ref4 ? nref : nr) += hist[c];
    const uint32_t *pos = bias + PMX_PLB_POS, *scl = bias + PMX_PLB_SCL, *mq = bias + PMX_PLB_MQ, *bq = bias + PMX_PLB_BQ, *mqs = bias + PMX_PLB_MQS;
    const int NP = PMX_PLB_NPOS, NQL = PMX_PLB_NQUAL;
    double v[PMX_N_TESTS];
    v[PMX_TEST_VDB] = calc_vdb(pos + NP, NP);
    v[PMX_TEST_SGB] = seg_bias((int)nref, (int)nr);
    v[PMX_TEST_RPBZ] = mwu_z(pos, pos + NP, NP);
    v[PMX_TEST_MQBZ] = mwu_z(mq, mq + NQL, NQL);
    v[PMX_TEST_MQSBZ] = mwu_z(mqs, mqs + NQL, NQL);
    v[PMX_TEST_BQBZ] = mwu_z(bq, bq + NQL, NQL);
    v[PMX_TEST_SCBZ] = mwu_z(scl, scl + NP, NP);
    for (int k = 0; k < PMX_TEST_MQ0F; ++k) {
        out->value[k] = (float)v[k];                       // the fields of bcf_call_t are floats (bam2bcf.h:178-180)
        if (v[k] != HUGE_VAL) out->present |= 1u << k;     // bam2bcf.c:1288-1309
    }
    out->value[PMX_TEST_MQ0F] = aux[0] ? (float)aux[2] / (float)aux[0] : 0.f;   // bam2bcf.c:1314
    out->present |= 1u << PMX_TEST_MQ0F;
}

const char* const TEST_NAMES[PMX_N_TESTS] = {"VDB", "SGB", "RPBZ", "MQBZ", "MQSBZ", "BQBZ", "SCBZ", "MQ0F"};

// htslib's kputd (kstring.c:38-140), the printer of every VCF float: outside [0.0001, 999999] printf's %g; inside, the
// value scaled to a six-digit integer by rint, the decimal point put back, trailing zeros (and a bare point) dropped
std::string format_float(double d) {
    if (d == 0) return std::signbit(d) ? "-0" : "0";
    std::string s;
    if (d < 0) { s = "-"; d = -d; }
    char buf[64];
    if (!(d >= 0.0001 && d <= 999999)) {
        snprintf(buf, sizeof(buf), "%g", d);
        return s + buf;
    }
    static const double bound[9] = {0.001, 0.01, 0.1, 1, 10, 100, 1000, 10000, 100000};
    static const double scale[10] = {1e9, 1e8, 1e7, 1e6, 1e5, 1e4, 1e3, 1e2, 1e1, 1};
    int k = 0;
    while (k < 9 && !(d < bound[k])) ++k;
    const int decimals = 9 - k;
    snprintf(buf, sizeof(buf), "%0*u", decimals + 1, (unsigned)(uint32_t)rint(d * scale[k]));
    std::string digits = buf;
    if (decimals) {
        digits.insert(digits.size() - (size_t)decimals, ".");
        digits.erase(digits.find_last_not_of('0') + 1);
        if (digits.back() == '.') digits.pop_back();
    }
    return s + digits;
}

std::string join_ints(const int32_t* v, int n) {
    std::string s;
    for (int i = 0; i < n; ++i) { if (i) s += ","; s += std::to_string(v[i]); }
    return s;
}

}  // namespace

struct pmx_genotyper {
    std::vector<std::string> records;
    // per record, for pmx_genotype_annotate: its 0-based position, reference letter and the site's hist / aux rows
    std::vector<int64_t> pos;
    std::vector<char> ref;
    std::vector<uint32_t> rows;   // HIST + 4 per record
    bool annotated = false;
};

extern "C" {

int pmx_genotype_spectrum_counts(const pmx_panman* pmh, int64_t counts[16], int64_t* n_branches, int64_t* genome_len) {
    if (!pmh || !counts) return PMX_ERR_ARG;
    try {
        const pmx::Panman& pm = pmx::panman_of(pmh);
        for (int i = 0; i < 16; ++i) counts[i] = 0;
        int64_t branches = 0;
        // the DFS of computeSubstitutionSpectrum (src/index_single_mode.cpp:1418-1477): block mutations switch blocks on and
        // off at every node; nucleotide mutations are applied (and counted) at every node but the root, so a child of the
        // root compares against the block consensus; a substitution counts when its block exists and both letters are A C G T
        std::string cols = pm.consensus_cols;
        std::vector<uint8_t> exists((size_t)pm.n_blocks, 0);
        struct Frame { int32_t node; size_t child; std::vector<std::pair<uint32_t, char>> col_undo; std::vector<std::pair<int32_t, uint8_t>> blk_undo; };
        std::vector<Frame> stack;
        auto enter = [&](int32_t ni) {
            stack.emplace_back();
            Frame& fr = stack.back();
            fr.node = ni;
            fr.child = 0;
            const pmx::PanmanNode& nd = pm.nodes[(size_t)ni];
            for (const pmx::BlockMut& bm : nd.block_muts) {
                if (bm.block < 0 || bm.block >= pm.n_blocks) continue;
                fr.blk_undo.emplace_back(bm.block, exists[(size_t)bm.block]);
                if (bm.insertion) exists[(size_t)bm.block] = 1;
                else if (!bm.inversion) exists[(size_t)bm.block] = 0;
            }
            if (ni == 0) return;
            ++branches;
            for (const pmx::NucMut& nm : nd.nuc_muts) {
                const int type = nm.type & 0x7;
                const bool is_sub = type == 0 || type == 3;   // NS, NSNPS
                if (nm.block < 0 || nm.block >= pm.n_blocks) continue;
                for (int i = 0; i < nm.len; ++i) {
                    const int32_t pos = nm.gap < 0 ? nm.pos + i : nm.pos, gap = nm.gap < 0 ? -1 : nm.gap + i;
                    if (pos < 0 || pos >= pm.block_len[(size_t)nm.block]) continue;
                    const int64_t c = pm.column(nm.block, pos, gap);
                    if (c < 0) continue;
                    const char old = cols[(size_t)c], nw = pmx::nuc_from_code((int)((nm.nucs >> (4 * (5 - i))) & 0xf));
                    fr.col_undo.emplace_back((uint32_t)c, old);
                    cols[(size_t)c] = nw;
                    if (is_sub && exists[(size_t)nm.block]) {
                        const int oi = base_index(old), ni2 = base_index(nw);
                        if (oi < 4 && ni2 < 4 && oi != ni2) ++counts[oi * 4 + ni2];
                    }
                }
            }
        };
        if (!pm.nodes.empty()) enter(0);
        while (!stack.empty()) {
            Frame& fr = stack.back();
            const pmx::PanmanNode& nd = pm.nodes[(size_t)fr.node];
            if (fr.child < nd.children.size()) { const int32_t ch = nd.children[fr.child++]; enter(ch); continue; }
            for (size_t i = fr.col_undo.size(); i-- > 0;) cols[fr.col_undo[i].first] = fr.col_undo[i].second;
            for (size_t i = fr.blk_undo.size(); i-- > 0;) exists[(size_t)fr.blk_undo[i].first] = fr.blk_undo[i].second;
            stack.pop_back();
        }
        if (n_branches) *n_branches = branches;
        if (genome_len) {
            // the median of ten leaf genomes (:1479-1502).  The reference takes its leaves from a hash map's iteration
            // order; here: the leaves in DFS order, every (leaves / 10)-th
            std::vector<int32_t> leaves;
            for (size_t i = 0; i < pm.nodes.size(); ++i)
                if (pm.nodes[i].children.empty()) leaves.push_back((int32_t)i);
            std::vector<int64_t> lengths;
            const size_t want = std::min<size_t>(10, leaves.size()), step = std::max<size_t>(1, want ? leaves.size() / want : 1);
            const pmx::PanmanState root = pmx::root_state_of(pm);
            for (size_t i = 0; i < leaves.size() && lengths.size() < want; i += step) lengths.push_back((int64_t)pmx::node_genome(pm, leaves[i], &root).size());
            std::sort(lengths.begin(), lengths.end());
            *genome_len = lengths.empty() ? 0 : lengths[lengths.size() / 2];
        }
        return PMX_OK;
    } catch (const std::exception& e) {
        pmx::set_error(e.what());
        return PMX_ERR_FORMAT;
    }
}

int pmx_genotype_spectrum_phred(const int64_t counts[16], int64_t n_branches, int64_t genome_len, double phred[16]) {
    if (!counts || !phred) return PMX_ERR_ARG;
    double rate[16];
    if (n_branches > 0 && genome_len > 0) {   // src/index_single_mode.cpp:1506-1538: every base is a quarter of the genome
        const int64_t base_count = genome_len / 4;
        for (int from = 0; from < 4; ++from)
            for (int to = 0; to < 4; ++to) {
                if (from == to) {
                    double off = 0;
                    for (int j = 0; j < 4; ++j)
                        if (j != from && base_count > 0) off += (double)counts[from * 4 + j] / (double)(n_branches * base_count);
                    rate[from * 4 + to] = 1.0 - off;
                } else rate[from * 4 + to] = base_count > 0 ? (double)counts[from * 4 + to] / (double)(n_branches * base_count) : 0.0;
            }
    } else
        for (int i = 0; i < 16; ++i) rate[i] = (i / 4 == i % 4) ? 1.0 : 0.0;
    bool any = false;   // loadSubstMatrixFromIndex (src/main.cpp:290-311)
    for (int i = 0; i < 16; ++i)
        if (i / 4 != i % 4 && rate[i] > 0) any = true;
    for (int i = 0; i < 16; ++i) phred[i] = rate[i] > 0 ? -10.0 * log10(rate[i]) : 100.0;
    return any ? 0 : 1;
}

int pmx_genotype_site(const uint32_t* hist, char ref_base, pmx_site_call* out) {
    if (!hist || !out) return PMX_ERR_ARG;
    try {
        site_call(hist, ref_base, out);
        return PMX_OK;
    } catch (const std::exception& e) {
        pmx::set_error(e.what());
        return PMX_ERR_ARG;
    }
}

int64_t pmx_genotype_filter_line(const char* line, const double* phred16, int min_depth, double min_qual, char* out, int64_t cap) {
    if (!line) return PMX_ERR_ARG;
    try {
        const std::string r = phred16 ? apply_spectrum(line, phred16, min_depth, min_qual, nullptr) : plain_filter(line, min_depth, min_qual);
        if (out && cap > 0) {
            const size_t n = std::min<size_t>(r.size(), (size_t)cap - 1);
            memcpy(out, r.data(), n);
            out[n] = '\0';
        }
        return (int64_t)r.size();
    } catch (const std::exception& e) {
        pmx::set_error(e.what());
        return PMX_ERR_FORMAT;
    }
}

int64_t pmx_genotype_call(const uint32_t* hist, const uint32_t* aux, const char* reference, int64_t ref_len, const char* chrom, const double* phred16,
                          int min_depth, double min_qual, pmx_genotyper** out) {
    if (!hist || !aux || !reference || !chrom || !out || ref_len < 0) return PMX_ERR_ARG;
    try {
        std::unique_ptr<pmx_genotyper> g(new pmx_genotyper());
        for (int64_t pos = 0; pos < ref_len; ++pos) {
            const uint32_t* h = hist + pos * HIST;
            // candidate: an alternative base with a non-zero quality sum (every counted base has quality >= 4)
            const int ref4 = base_index(reference[pos]);
            bool cand = false;
            for (int c = 0; c < HIST && !cand; ++c)
                if (h[c] && c % NB < 4 && c % NB != ref4) cand = true;
            if (!cand) continue;
            pmx_site_call sc;
            site_call(h, reference[pos], &sc);
            if (sc.n_alleles < 2) continue;
            const uint32_t* ax = aux + pos * 4;
            const int64_t depth = (int64_t)sc.dp4[0] + sc.dp4[1] + sc.dp4[2] + sc.dp4[3];
            const int mq = depth > 0 ? (int)((float)ax[1] / (float)depth) : 0;   // mcall.c:1659
            std::string alt;
            for (int k = 1; k < sc.n_alleles; ++k) { if (k > 1) alt += ","; alt += "ACGTN"[sc.alleles[k]]; }
            int raw_gt = 0;   // the most likely haploid genotype of the raw line (lowest index on ties)
            for (int k = 1; k < sc.n_alleles; ++k)
                if (sc.pl[k] < sc.pl[raw_gt]) raw_gt = k;
            const std::string ref_s(1, (char)toupper((unsigned char)reference[pos]));
            // AC: one count per alternative, 1 at the raw line's genotype (the haploid genotype of `call --ploidy 1`)
            auto info_of = [&](int gt) {
                std::string ac;
                for (int k = 1; k < sc.n_alleles; ++k) { if (k > 1) ac += ","; ac += k == gt ? "1" : "0"; }
                return "DP=" + std::to_string(ax[0]) + ";AC=" + ac + ";AN=1;DP4=" + join_ints(sc.dp4, 4) + ";MQ=" + std::to_string(mq);
            };
            const std::string head = std::string(chrom) + "\t" + std::to_string(pos + 1) + "\t.\t" + ref_s + "\t";
            const std::string raw = head + alt + "\t.\t.\t" + info_of(raw_gt) + "\tGT:PL:AD\t" + std::to_string(raw_gt) + ":" + join_ints(sc.pl, sc.n_alleles) +
                                    ":" + join_ints(sc.ad, sc.n_alleles);
            int called = raw_gt;
            const std::string kept = phred16 ? apply_spectrum(raw, phred16, min_depth, min_qual, &called) : plain_filter(raw, min_depth, min_qual);
            if (kept.empty()) continue;
            // the written record is the line the reference's filter leaves: every alternative `call -m -A` keeps, one PL and
            // one AD per allele, GT the filter's allele, INFO passed through as it stood (src/genotyping.cpp:274-277)
            g->records.push_back(kept);
            g->pos.push_back(pos);
            g->ref.push_back(reference[pos]);
            g->rows.insert(g->rows.end(), h, h + HIST);
            g->rows.insert(g->rows.end(), ax, ax + 4);
        }
        const int64_t n = (int64_t)g->records.size();
        *out = g.release();
        return n;
    } catch (const std::exception& e) {
        pmx::set_error(e.what());
        return PMX_ERR_FORMAT;
    }
}

int64_t pmx_genotype_num_records(const pmx_genotyper* g) { return g ? (int64_t)g->records.size() : 0; }
const char* pmx_genotype_record(const pmx_genotyper* g, int64_t i) {
    return g && i >= 0 && i < (int64_t)g->records.size() ? g->records[(size_t)i].c_str() : nullptr;
}
void pmx_genotype_free(pmx_genotyper* g) { delete g; }
int64_t pmx_genotype_record_pos(const pmx_genotyper* g, int64_t i) { return g && i >= 0 && i < (int64_t)g->pos.size() ? g->pos[(size_t)i] : -1; }

int pmx_genotype_site_tests(const uint32_t* hist_row, const uint32_t* aux_row, const uint32_t* bias_row, char ref_base, pmx_site_tests* out) {
    if (!hist_row || !aux_row || !bias_row || !out) return PMX_ERR_ARG;
    site_tests(hist_row, aux_row, bias_row, ref_base, out);
    return PMX_OK;
}

const char* pmx_genotype_test_name(int k) { return k >= 0 && k < PMX_N_TESTS ? TEST_NAMES[k] : nullptr; }

int64_t pmx_genotype_format_float(double v, char* out, int64_t cap) {
    const std::string r = format_float(v);
    if (out && cap > 0) {
        const size_t n = std::min<size_t>(r.size(), (size_t)cap - 1);
        memcpy(out, r.data(), n);
        out[n] = '\0';
    }
    return (int64_t)r.size();
}

int pmx_genotype_annotate(pmx_genotyper* g, const int32_t* positions, const uint32_t* bias, int64_t n_sites) {
    if (!g || n_sites < 0 || (n_sites > 0 && (!positions || !bias))) return PMX_ERR_ARG;
    try {
        size_t rec = 0;   // records and positions both ascend
        for (int64_t s = 0; s < n_sites; ++s) {
            if (s > 0 && positions[s] <= positions[s - 1]) throw std::runtime_error("annotate: positions must be strictly ascending");
            while (rec < g->pos.size() && g->pos[rec] < positions[s]) ++rec;
            if (rec == g->pos.size() || g->pos[rec] != positions[s]) throw std::runtime_error("annotate: no record at position " + std::to_string(positions[s]));
            const uint32_t* row = g->rows.data() + rec * (HIST + 4);
            pmx_site_tests t;
            site_tests(row, row + HIST, bias + s * PMX_PILEUP_BIAS, g->ref[rec], &t);
            std::vector<std::string> f = split(g->records[rec], '\t');
            if (f.size() != 10) throw std::runtime_error("annotate: unexpected record");
            // DP first, then the tests, then what the record held behind DP (AC;AN;DP4;MQ) -- the order of the reference's line
            const size_t semi = f[7].find(';');
            std::string info = f[7].substr(0, semi);
            if (info.rfind("DP=", 0) != 0) throw std::runtime_error("annotate: unexpected record");
            if (f[7].find(";MQ0F=") != std::string::npos)
                throw std::runtime_error("annotate: record at position " + std::to_string(positions[s]) + " is annotated already");
            for (int k = 0; k < PMX_N_TESTS; ++k)
                if (t.present >> k & 1u) info += std::string(";") + TEST_NAMES[k] + "=" + format_float(t.value[k]);
            if (semi != std::string::npos) info += f[7].substr(semi);
            f[7] = info;
            std::string line = f[0];
            for (size_t i = 1; i < f.size(); ++i) line += "\t" + f[i];
            g->records[rec] = line;
        }
        g->annotated = true;
        return PMX_OK;
    } catch (const std::exception& e) {
        pmx::set_error(e.what());
        return PMX_ERR_ARG;
    }
}

int pmx_genotype_write_vcf(const pmx_genotyper* g, const char* path, const char* chrom, int64_t ref_len, const char* sample_name) {
    if (!g || !path || !chrom || !sample_name) return PMX_ERR_ARG;
    FILE* f = fopen(path, "w");
    if (!f) { pmx::set_error(std::string("cannot write ") + path); return PMX_ERR_IO; }
    fprintf(f, "##fileformat=VCFv4.2\n##contig=<ID=%s,length=%lld>\n", chrom, (long long)ref_len);
    fputs("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Raw read depth\">\n", f);
    if (g->annotated)   // the lines of `bcftools mpileup`, in its order
        fputs("##INFO=<ID=VDB,Number=1,Type=Float,Description=\"Variant Distance Bias for filtering splice-site artefacts in RNA-seq data (bigger is better)\",Version=\"3\">\n"
              "##INFO=<ID=RPBZ,Number=1,Type=Float,Description=\"Mann-Whitney U-z test of Read Position Bias (closer to 0 is better)\">\n"
              "##INFO=<ID=MQBZ,Number=1,Type=Float,Description=\"Mann-Whitney U-z test of Mapping Quality Bias (closer to 0 is better)\">\n"
              "##INFO=<ID=BQBZ,Number=1,Type=Float,Description=\"Mann-Whitney U-z test of Base Quality Bias (closer to 0 is better)\">\n"
              "##INFO=<ID=MQSBZ,Number=1,Type=Float,Description=\"Mann-Whitney U-z test of Mapping Quality vs Strand Bias (closer to 0 is better)\">\n"
              "##INFO=<ID=SCBZ,Number=1,Type=Float,Description=\"Mann-Whitney U-z test of Soft-Clip Length Bias (closer to 0 is better)\">\n"
              "##INFO=<ID=SGB,Number=1,Type=Float,Description=\"Segregation based metric, http://samtools.github.io/bcftools/rd-SegBias.pdf\">\n"
              "##INFO=<ID=MQ0F,Number=1,Type=Float,Description=\"Fraction of MQ0 reads (smaller is better)\">\n", f);
    fputs("##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Allele count in genotypes for each ALT allele, in the same order as listed\">\n"
          "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Total number of alleles in called genotypes\">\n"
          "##INFO=<ID=DP4,Number=4,Type=Integer,Description=\"Number of high-quality ref-forward , ref-reverse, alt-forward and alt-reverse bases\">\n"
          "##INFO=<ID=MQ,Number=1,Type=Integer,Description=\"Average mapping quality\">\n"
          "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
          "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"List of Phred-scaled genotype likelihoods\">\n"
          "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Allelic depths (high-quality bases)\">\n", f);
    fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", sample_name);
    for (const std::string& r : g->records) fprintf(f, "%s\n", r.c_str());
    const bool ok = !ferror(f);
    if (fclose(f) != 0 || !ok) { pmx::set_error(std::string("write failed: ") + path); return PMX_ERR_IO; }
    return PMX_OK;
}

int pmx_genotype_write_consensus(const char* vcf_path, const char* ref_fa_path, const char* out_path, const char* header) {
    if (!vcf_path || !ref_fa_path || !out_path || !header) return PMX_ERR_ARG;
    try {
        std::ifstream fa(ref_fa_path);
        if (!fa) { pmx::set_error(std::string("cannot read ") + ref_fa_path); return PMX_ERR_IO; }
        std::string line, name, seq;
        bool first = false;
        while (std::getline(fa, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (!line.empty() && line[0] == '>') {
                if (first) break;   // the first sequence
                first = true;
                name = line.substr(1, line.find_first_of(" \t", 1) - 1);
            } else if (first) seq += line;
        }
        std::ifstream vcf(vcf_path);
        if (!vcf) { pmx::set_error(std::string("cannot read ") + vcf_path); return PMX_ERR_IO; }
        while (std::getline(vcf, line)) {
            if (line.empty() || line[0] == '#') continue;
            const std::vector<std::string> f = split(line, '\t');
            if (f.size() < 5 || f[0] != name || f[4] == ".") continue;
            const long long pos = std::stoll(f[1]);
            // `bcftools consensus -f ref -o out vcf` on a file with a sample column applies the allele the sample's GT names
            // (consensus.c:231-259: every sample is taken, iupac_GTs; :606-622: ialt = iupac_set_allele); a record whose
            // GT names the reference changes nothing, and a file without a sample column gets its first alternative
            size_t which = 1;
            if (f.size() >= 10) {
                const std::string gt = f[9].substr(0, f[9].find(':'));
                if (gt.empty() || gt.find_first_not_of("0123456789") != std::string::npos) continue;   // a missing genotype sets nothing
                which = (size_t)std::stoul(gt);
                if (which == 0) continue;
            }
            const std::vector<std::string> alts = split(f[4], ',');
            if (which > alts.size()) throw std::runtime_error("consensus: too few alternatives (" + f[0] + ":" + f[1] + ")");
            const std::string alt = alts[which - 1];
            if (f[3].size() != 1 || alt.size() != 1 || alt == "*") throw std::runtime_error("consensus: only substitution records are applied (" + f[0] + ":" + f[1] + ")");
            if (pos < 1 || pos > (long long)seq.size()) throw std::runtime_error("consensus: position outside the reference (" + f[0] + ":" + f[1] + ")");
            if (toupper((unsigned char)seq[(size_t)pos - 1]) != toupper((unsigned char)f[3][0]))
                throw std::runtime_error("consensus: REF of " + f[0] + ":" + f[1] + " is not the reference base");
            seq[(size_t)pos - 1] = alt[0];
        }
        FILE* o = fopen(out_path, "w");
        if (!o) { pmx::set_error(std::string("cannot write ") + out_path); return PMX_ERR_IO; }
        fprintf(o, ">%s\n", header);
        for (size_t i = 0; i < seq.size(); i += 60) {
            fwrite(seq.data() + i, 1, std::min<size_t>(60, seq.size() - i), o);
            fputc('\n', o);
        }
        const bool ok = !ferror(o);
        if (fclose(o) != 0 || !ok) { pmx::set_error(std::string("write failed: ") + out_path); return PMX_ERR_IO; }
        return PMX_OK;
    } catch (const std::exception& e) {
        pmx::set_error(e.what());
        return PMX_ERR_FORMAT;
    }
}

}  // extern "C"
