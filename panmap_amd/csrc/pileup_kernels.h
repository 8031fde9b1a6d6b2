// Device pileup of the genotype stage: what bcftools `mpileup -B` hands to its error model, as integer tables per
// reference position (pileup_kernels.hip; driven by api_genotype.hip).
#pragma once
#include <cstdint>

#include "../../include/panmap_amd.h"

namespace pmx {

// per-read byte the host sweep hands to the kernels
enum : uint8_t {
    PLP_ADMIT = 1,    // passes mplp_func's filters and the depth cap: the read is in the pileup
    PLP_TWEAK = 2,    // both mates are in the pileup and proper: htslib reconciles their overlap
    PLP_SECOND = 4,   // of a PLP_TWEAK pair: this mate comes second in BAM order (`b` of tweak_overlap_quality)
    PLP_KEEP = 8,     // of a PLP_TWEAK pair: this mate keeps the quality of agreeing bases (amul / bmul = 1)
};

constexpr int PLP_NQ = 64, PLP_NBASE = 5;                 // quality 0..63; A C G T N
constexpr int PLP_HIST = PLP_NQ * 2 * PLP_NBASE;          // counters of hist[pos]: [q][strand][base]
constexpr int PLP_AUX = 4;                                // aux[pos]: raw depth, sum of capped mapQ, mapQ-0 bases, deletions
constexpr int PLP_CELLS = PLP_HIST + PLP_AUX;
constexpr int PLP_WINDOW = 24;                            // positions per block: 24 * 644 * 4 B = 61.8 KB of LDS, two blocks per CU

struct PileupArgs {
    const pmx_aln_record* recs;
    const uint32_t* cigars;
    const uint8_t* ascii;     // reads as uploaded
    const uint8_t* qual;      // Phred+33 per base, same offsets; NULL = 'I' everywhere
    const int64_t* off;       // n_reads + 1
    const uint8_t* rinfo;     // PLP_* per read
    const uint32_t* rank;     // BAM rank per read (PLP_TWEAK pairs)
    const uint32_t* first_ge; // ref_len + 2: BAM rank of the first admitted read that starts at or after a position
    uint8_t* effq;            // out: quality per base in BAM orientation after the overlap rule, same offsets
    int32_t* late_idx;        // out, per read: query index whose right neighbour is read un-reconciled (-1: none)
    uint8_t* late_q;          // out, per read: that neighbour's original quality
    int64_t n_reads;
    int32_t ref_len;
    int32_t paired, revcomp_mate2;
    // the window kernel: admitted reads in BAM order
    const int32_t* s_rs;      // their starts, ascending
    const uint32_t* s_idx;    // their read indices
    int64_t n_sorted;
    int32_t max_span;         // longest reference span among them
    uint32_t* hist;           // out [ref_len][PLP_HIST]
    uint32_t* aux;            // out [ref_len][PLP_AUX]
    int32_t min_baseq, max_baseq, delta_baseq, cap_mapq;
};

// The bias pass (k_pileup_bias): the histograms the rank tests of bcf_call_combine read (bam2bcf.c:488-527), for a list of
// sites, over the state a run left behind.  One site = PLB_CELLS counters, layout published as PMX_PLB_* (panmap_amd.h).
constexpr int PLB_POS = PMX_PLB_POS, PLB_SCL = PMX_PLB_SCL, PLB_MQ = PMX_PLB_MQ, PLB_BQ = PMX_PLB_BQ, PLB_MQS = PMX_PLB_MQS;
constexpr int PLB_NPOS = PMX_PLB_NPOS, PLB_NQUAL = PMX_PLB_NQUAL, PLB_CELLS = PMX_PILEUP_BIAS;
static_assert(PLB_MQS + 2 * PLB_NQUAL == PLB_CELLS && PLB_SCL == 2 * PLB_NPOS && PLB_MQ == 4 * PLB_NPOS, "bias table layout");

struct PileupBiasArgs {
    PileupArgs run;           // the last run's arguments: its device state is read, nothing of it is written
    const int32_t* sites;     // 0-based positions, strictly ascending, inside [0, ref_len)
    const uint8_t* ref_bases; // the reference letter of every site
    int64_t n_sites;
    uint32_t* out;            // [n_sites][PLB_CELLS]
};

__global__ void k_pileup_quals(PileupArgs a);
__global__ void k_pileup_window(PileupArgs a);
__global__ void k_pileup_bias(PileupBiasArgs b);

}  // namespace pmx
