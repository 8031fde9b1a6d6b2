/*
 * panmap_amd.h -- C ABI of the MI355X-native panmap hot path (index -> place -> align).
 *
 * One shared library, libpanmap_amd.so: plain pointers and sizes, no C++/torch types.  Every
 * entry point cites the reference interface it stands in for (paths relative to amkram/panmap).
 * All functions returning int use 0 = success, negative = error (pmx_last_error() has the text);
 * there is NO CPU fallback: device entry points fail with PMX_ERR_NO_DEVICE when no gfx950 GPU is
 * usable.  Handles are thread-compatible, not thread-safe; one pmx_ctx per GPU.
 */
#ifndef PANMAP_AMD_H
#define PANMAP_AMD_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_OK 0
#define PMX_ERR_ARG (-1)
#define PMX_ERR_IO (-2)
#define PMX_ERR_FORMAT (-3)
#define PMX_ERR_NO_DEVICE (-4)
#define PMX_ERR_DEVICE (-5)
#define PMX_ERR_CAPACITY (-6)
#define PMX_ERR_UNSUPPORTED (-7)

const char *pmx_last_error(void);
const char *pmx_version(void);

/* ------------------------------------------------------------------------------------------
 * PanMAN + node genomes (host).  Replaces loadPanMAN (src/main.cpp:313-325, external panman
 * library) and panmapUtils::getStringFromReference (src/panmap_utils.cpp:182-190), which
 * runAlignment uses to materialise the placed node's genome (src/main.cpp:1757-1771).
 * ------------------------------------------------------------------------------------------ */
typedef struct pmx_panman pmx_panman;
int pmx_panman_open(const char *path, pmx_panman **out);
void pmx_panman_close(pmx_panman *pm);
int64_t pmx_panman_num_nodes(const pmx_panman *pm);
int64_t pmx_panman_num_blocks(const pmx_panman *pm);
int64_t pmx_panman_num_columns(const pmx_panman *pm);
const char *pmx_panman_node_id(const pmx_panman *pm, int64_t dfs_index);
int64_t pmx_panman_parent(const pmx_panman *pm, int64_t dfs_index);
int64_t pmx_panman_find_node(const pmx_panman *pm, const char *node_id); /* -1 if absent */
/* writes the ungapped genome (no NUL) into buf if cap suffices; always returns its length */
int64_t pmx_panman_node_genome(const pmx_panman *pm, int64_t dfs_index, char *buf, int64_t cap);
/* test hook (src/test/test_index.cpp:145-193 injects the same mutation into a loaded tree): appends a pure
 * inversion of the largest forward block with >= min_bases bases to the node's block mutations; returns the
 * block id, or -1 when the node has no such block */
int64_t pmx_panman_test_invert_block(pmx_panman *pm, int64_t dfs_index, int min_bases);

/* ------------------------------------------------------------------------------------------
 * Seed index (host).  Replaces IndexBuilder::buildIndexParallel (src/index_single_mode.hpp:207-214)
 * and the zero-copy SoA binding the place stage does on the loaded index
 * (src/placement.cpp:1054-1085; layout src/index_lite.capnp:36-70).
 * ------------------------------------------------------------------------------------------ */
typedef struct pmx_index pmx_index;
typedef struct {
    int32_t k, s, t, l;
    int32_t open_syncmer;
    int32_t hpc;
    int32_t flank_mask;
    int32_t reserved;
    int64_t n_nodes;
    int64_t n_changes;
} pmx_index_info;

int pmx_index_build(const pmx_panman *pm, int k, int s, int t, int l, int open_syncmer, int flank_mask,
                    pmx_index **out);
/* mode 0 = automatic (incremental DFS; from-scratch re-seeding of every node when the PanMAN has inverted
 * blocks), 1 = from scratch, 2 = incremental; max_nodes >= 0 stops after that many nodes in DFS order
 * (the remaining nodes carry no changes) -- both exist for the cross-check tests of the producer */
int pmx_index_build_ex(const pmx_panman *pm, int k, int s, int t, int l, int open_syncmer, int flank_mask,
                       int mode, int64_t max_nodes, pmx_index **out);
/* mode | PMX_INDEX_ORIENTED: the --meta form of the index.  A k-min-mer that reads right-to-left on the node's genome
 * (reverse rolled hash < forward rolled hash) is keyed hash ^ PMX_ORIENT_XOR: the per-node count changes then tell the
 * two orientations of one hash apart -- what the reference's MGSR index keeps as seedInfos[].isReverse
 * (src/mgsr.cpp:7225-7320 counts (forward, reverse) occurrences per hash).  Needs l >= 2. */
#define PMX_INDEX_ORIENTED 0x100
/* mode | PMX_INDEX_HPC: the index of the homopolymer-compressed genomes (--hpc).  Node n contributes the seeds of
 * hpcCompress(genome(n)) (src/seeding.cpp:286-306); the hard flank mask is judged at the UNCOMPRESSED coordinate of a k-mer's
 * first base (src/index_single_mode.cpp:878-883).  Always the from-scratch producer (mode 0 or 1; 2 and PMX_INDEX_ORIENTED
 * are PMX_ERR_UNSUPPORTED).  Not pinned to the reference's incremental HPC producer: DESIGN.md sections 1 and 7. */
#define PMX_INDEX_HPC 0x200
#define PMX_ORIENT_XOR 0x9e3779b97f4a7c15ULL
/* adopt caller-provided SoA arrays (copied): parent[n], offsets[n+1], hash/pc/cc[offsets[n]]; info->reserved & 1: the arrays
 * are an oriented index (keys as PMX_INDEX_ORIENTED makes them) */
int pmx_index_from_arrays(const pmx_index_info *info, const uint32_t *parent, const uint64_t *offsets,
                          const uint64_t *hash, const int16_t *parent_count, const int16_t *child_count,
                          pmx_index **out);
/* the node ids of an index adopted from arrays (copied; ids[v] for DFS index v, n = the index's nodes, else PMX_ERR_ARG):
 * what pmx_index_node_id returns from then on, and what --em-leaves-only reads */
int pmx_index_set_node_ids(pmx_index *idx, const char *const *ids, int64_t n);
/* The `.idx` container the reference's place stage loads and its index stage writes (32-byte PMI1 header + Cap'n Proto
 * LiteIndex message, raw or as concatenated zstd frames; src/index_single_mode.cpp:1561-1640, src/placement.cpp:1009-1092,
 * src/index_lite.capnp:36-70).  Load rejects a stale format version / missing struct-of-arrays fields / short offsets with
 * the reference's messages (pmx_last_error).  zstd_level as --zstd-level; uncompressed != 0 writes the mmap-able form. */
int pmx_index_save(const pmx_index *idx, const char *path, int zstd_level, int uncompressed);
int pmx_index_load(const char *path, pmx_index **out);
/* the seeding parameters from the header alone (cache validation, src/main.cpp:371-396); PMX_ERR_FORMAT if absent */
int pmx_index_read_header(const char *path, pmx_index_info *info, int *uncompressed);
const char *pmx_index_node_id(const pmx_index *idx, int64_t dfs_index); /* "" when the index was adopted from arrays */
void pmx_index_close(pmx_index *idx);
int pmx_index_get_info(const pmx_index *idx, pmx_index_info *info);
const uint32_t *pmx_index_parents(const pmx_index *idx);      /* n_nodes   */
const uint64_t *pmx_index_offsets(const pmx_index *idx);      /* n_nodes+1 */
const uint64_t *pmx_index_hashes(const pmx_index *idx);       /* n_changes */
const int16_t *pmx_index_parent_counts(const pmx_index *idx); /* n_changes */
const int16_t *pmx_index_child_counts(const pmx_index *idx);  /* n_changes */

/* ------------------------------------------------------------------------------------------
 * Device context (one per GPU / per process rank).
 * ------------------------------------------------------------------------------------------ */
typedef struct pmx_ctx pmx_ctx;
int pmx_ctx_create(int device_ordinal, pmx_ctx **out);
/* the HIP devices this process can open (0: none).  It initialises the runtime: a process that forks ranks asks in a child. */
int pmx_device_count(void);
void pmx_ctx_destroy(pmx_ctx *ctx);
int pmx_ctx_synchronize(pmx_ctx *ctx);
/* the HIP stream all kernels of this context are launched on (hipStream_t as void*).  Every context owns a hardware queue
   (a CU-masked stream with every CU enabled): contexts used from different host threads overlap their kernels. */
void *pmx_ctx_stream(pmx_ctx *ctx);

/* ------------------------------------------------------------------------------------------
 * Read sets.  The reference hands reads around as std::vector<std::string>
 * (extractReadSequences src/placement.cpp:164-197; readFastqPaired src/seeding.cpp:231-269).
 * Here: one concatenated ASCII buffer + n+1 offsets, uploaded once; pmx_readset_pack converts it
 * on the GPU to 2 bits/base + an ambiguity bitmask (every read starts on a 32-base word).
 * ------------------------------------------------------------------------------------------ */
typedef struct pmx_readset pmx_readset;
int pmx_readset_upload(pmx_ctx *ctx, const char *concat, const int64_t *offsets, int64_t n_reads,
                       pmx_readset **out);
/* wrap ASCII reads already resident in device memory (d_concat: total bytes, d_offsets: n+1 int64) */
int pmx_readset_wrap_device(pmx_ctx *ctx, const void *d_concat, const void *d_offsets, int64_t n_reads,
                            int64_t total_bytes, int64_t max_read_len, pmx_readset **out);
/* re-point an existing read set at another batch resident in device memory (streaming: the object's packed-read buffers
   are reused, the word offsets are computed and the offsets validated on the device; call pmx_readset_pack afterwards) */
int pmx_readset_rewrap_device(pmx_ctx *ctx, pmx_readset *rs, const void *d_concat, const void *d_offsets, int64_t n_reads,
                              int64_t total_bytes, int64_t max_read_len);
int pmx_readset_pack(pmx_ctx *ctx, pmx_readset *rs);
/* streaming form of the same: pack the reads [r0, r1) of a (re)wrapped read set as soon as THEIR bases have landed in the
   wrapped buffer (the offsets of the whole set are in place since the wrap); the set counts as packed once the ranges
   cover it.  Stream-ordered on the context's stream, no host round trip. */
int pmx_readset_pack_range(pmx_ctx *ctx, pmx_readset *rs, int64_t r0, int64_t r1);
/* FASTQ quality strings of the same reads (same offsets; one Phred+33 byte per base): only needed for
 * pmx_place_params.min_seed_quality > 0 (allReadQualities, src/placement.cpp:1386) */
int pmx_readset_set_qualities(pmx_ctx *ctx, pmx_readset *rs, const char *qual_concat);
/* Optional: enqueue the align stage's pair order (pairs by both mates' locality keys) of a packed, paired read set NOW, on a
 * side stream of the context.  It depends on the reads alone, so made here it runs beside the place stage instead of between
 * the placement and the first align kernel; an aligner that finds none makes it itself.  Same results either way. */
int pmx_readset_order_pairs(pmx_ctx *ctx, pmx_readset *rs);
/* the HPC form of a read set (seeding::hpcCompress, src/seeding.cpp:286-306, applied as src/placement.cpp:1143-1165
   applies it): *out == NULL makes a new read set, otherwise that object's buffers are reused (streaming).  The result owns
   its bases / offsets (/ qualities, when src has them: first base of each run), is marked HPC, is NOT packed.  Base 0 of a
   read is kept, base i > 0 iff toupper(seq[i]) != toupper(seq[i-1]); kept characters are copied as they are.  Only a placer
   over an HPC index takes such a set (it also takes the plain set and compresses it itself); the align stage, pmx_readset_order_pairs
   and pmx_pileup_run refuse it (PMX_ERR_ARG): they work on the uncompressed reads. */
int pmx_readset_hpc_compress(pmx_ctx *ctx, const pmx_readset *src, pmx_readset **out);
/* a read set made of the reads src[idx[0]], ..., src[idx[n-1]] of another, in that order: the nodeSeqs / nodeQuals copies of
   alignAssignedReads (src/main.cpp:691-699), as one gather on the device instead of a host copy per read.  idx is a HOST
   array; indices may repeat and come in any order, n == 0 gives a set of zero reads; an index outside [0, reads of src), a
   null argument or n < 0 is PMX_ERR_ARG with nothing launched.  *out == NULL makes a new read set, otherwise that object's
   buffers are reused and grown only when needed.  The result owns its bases, its n+1 offsets (starting at 0) and, when src
   has them, its qualities; it keeps src's HPC mark and is NOT packed: call pmx_readset_pack, as after
   pmx_readset_hpc_compress.  src may be packed or not, and may be a wrapped slice.  Stream-ordered on the context's
   stream, with one read-back (the size of the result). */
int pmx_readset_select(pmx_ctx *ctx, const pmx_readset *src, const int64_t *idx /* host */, int64_t n, pmx_readset **out);
int pmx_readset_is_hpc(const pmx_readset *rs);
int pmx_readset_has_qualities(const pmx_readset *rs);
/* download a read set's ASCII bases, offsets (n+1, starting at 0) and, if present and qual != NULL, qualities:
   returns the number of bases; copies only when cap suffices */
int64_t pmx_readset_export(pmx_ctx *ctx, const pmx_readset *rs, char *concat, int64_t cap, int64_t *offsets, char *qual);
/* TEST ACCESSOR: download the packed form of a packed read set as the pack kernels wrote it: words[n_words] (2 bits per base),
   amb[n_words] (1 bit per base), woff[n+1] (word offsets) and, when the set has read records (no read longer than 160 bases;
   *has_recs says so), the n x 64 record bytes.  Returns n_words and copies only when cap_words suffices and the pointers the
   set needs are there (recs may be NULL for a set without records), so a first call with cap_words = -1 asks for the sizes.
   An unpacked set is PMX_ERR_ARG.  Copies on the context's stream and a wait for it; no kernel. */
int64_t pmx_readset_export_packed(pmx_ctx *ctx, const pmx_readset *rs, uint64_t *words, uint32_t *amb, int64_t cap_words,
                                  int64_t *woff, uint8_t *recs, int *has_recs);
void pmx_readset_free(pmx_ctx *ctx, pmx_readset *rs);
int64_t pmx_readset_num_reads(const pmx_readset *rs);

/* ------------------------------------------------------------------------------------------
 * PLACE stage on the GPU.  Together these replace placement::placeLite
 * (src/placement.hpp:237-244, src/placement.cpp:986-2018).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    /* TraversalParams fields that change results (src/placement.hpp:28-54); k/s/t/l/open come
       from the index (src/placement.cpp:1094-1101) */
    double seed_mask_fraction; /* CLI default 0 (src/main.cpp:1967) */
    int32_t min_read_support;  /* -1 = auto */
    int32_t trim_start, trim_end;
    int32_t dedup_reads;       /* --dedup: each distinct sequence counted once */
    int32_t force_leaf;
    int32_t min_seed_quality;  /* --min-seed-quality: > 0 with qualities attached selects the quality-filtered
                                  seeding branch (src/placement.cpp:1386-1527; it ignores dedup_reads) */
    int32_t reserved[2];
} pmx_place_params;

typedef struct {
    double best_score[5];     /* log_raw, log_cosine, containment, weighted_containment, log_containment */
    uint32_t best_index[5];   /* lowest tied DFS index; UINT32_MAX if none */
    int64_t n_tied[5];
    int64_t n_reads;
    int64_t n_unique_seeds;   /* histogram size after homopolymer/mask erase */
    int64_t n_kept_seeds;     /* readUniqueSeedCount */
    int64_t total_seed_freq;  /* totalReadSeedFrequency */
    int64_t min_support;      /* resolved */
    double log_read_magnitude;
    double log_containment_den;
    double weighted_containment_den;
} pmx_place_result;

typedef struct pmx_place pmx_place; /* device-resident index + working buffers for one sample */

/* uploads the index SoA (replicated per GPU) and precomputes BFS levels.  Over an HPC index (pmx_index_info.hpc) the reads are
   seeded in their HPC form: pmx_place_add_reads* take a read set marked HPC as it is (packed, like any set), or a plain one,
   whose range they compress into a scratch set of the placer, pack and seed from (the caller's set is untouched).  A set marked
   HPC with another index, and a plain set in the pmx_place_dedup_* calls of an HPC placer, are PMX_ERR_ARG. */
int pmx_place_create(pmx_ctx *ctx, const pmx_index *idx, pmx_place **out);
void pmx_place_free(pmx_ctx *ctx, pmx_place *pl);

/* [hot] reads -> syncmers -> k-min-mers -> seed histogram (src/placement.cpp:1611-1686).
   Accumulates into the place object's device histogram; call once per read shard. */
int pmx_place_reset(pmx_ctx *ctx, pmx_place *pl);
int pmx_place_add_reads(pmx_ctx *ctx, pmx_place *pl, const pmx_readset *rs, const pmx_place_params *pp);
/* the reads [r0, r1) of the set alone (packed by pmx_readset_pack or pmx_readset_pack_range): a batch is seeded range by
   range while the H2D copy of the next range is in flight; the sum over the ranges is the histogram of the set.
   --dedup needs the whole set (PMX_ERR_UNSUPPORTED on a proper sub-range). */
int pmx_place_add_reads_range(pmx_ctx *ctx, pmx_place *pl, const pmx_readset *rs, int64_t r0, int64_t r1,
                              const pmx_place_params *pp);
/* export / import of the (hash,count) histogram, ascending hash: the multi-GPU exchange step
   (all-gather of per-rank histograms, then merge) */
int64_t pmx_place_histogram_size(pmx_ctx *ctx, pmx_place *pl);
int pmx_place_histogram_export(pmx_ctx *ctx, pmx_place *pl, uint64_t *hash, int64_t *count, int64_t cap);
int pmx_place_histogram_merge(pmx_ctx *ctx, pmx_place *pl, const uint64_t *hash, const int64_t *count, int64_t n);
/* same with caller-owned DEVICE buffers (e.g. torch tensors fed to an RCCL all-gather): no host bounce */
int pmx_place_histogram_export_device(pmx_ctx *ctx, pmx_place *pl, void *d_hash, void *d_count, int64_t cap);
/* for the multi-GPU exchange: the number of distinct seeds without sorting them, and the (hash, count) pairs in table
 * order written into DEVICE buffers (stream-ordered on the context's stream; synchronize the context before another
 * stream reads them).  The ranks' parts are merged with pmx_place_histogram_merge_device_parts; order plays no role. */
int64_t pmx_place_histogram_entries(pmx_ctx *ctx, pmx_place *pl);
int pmx_place_histogram_export_device_unsorted(pmx_ctx *ctx, pmx_place *pl, void *d_hash, void *d_count, int64_t cap);
/* n_parts (hash,count) runs laid out `part_stride` elements apart (the all-gather buffer of the multi-GPU
 * exchange: rank p's run at d_hash + p * part_stride, sizes[p] valid entries); skip_part = this rank's own run */
int pmx_place_histogram_merge_device_parts(pmx_ctx *ctx, pmx_place *pl, const void *d_hash, const void *d_count,
                                           int64_t part_stride, const int64_t *sizes, int n_parts, int skip_part);
int pmx_place_histogram_merge_device(pmx_ctx *ctx, pmx_place *pl, const void *d_hash, const void *d_count, int64_t n);

/* read-side filters + magnitudes (src/placement.cpp:1703-1856), then [hot] per-node delta scoring
   down the tree (src/placement.cpp:242-345, 701-918) and the sequential best/tie rule (:355-401) */
int pmx_place_score(pmx_ctx *ctx, pmx_place *pl, const pmx_place_params *pp, int64_t n_reads_total,
                    pmx_place_result *res);
/* which path the last pmx_place_score of this object took (diagnostic: it changes no result).  A call that finds the
   persistent launch starved (a wave gave up waiting for a flag: the grid was not resident, or a flag was withheld) is
   redone with the level kernels and gives the same bits; `redone` is the only place where that shows. */
enum {
    PMX_SCORE_FORM_CHAINS = 0,       /* heavy-path chains, one persistent launch (the default) */
    PMX_SCORE_FORM_TREE = 1,         /* flag per node, one persistent launch (PMX_PLACE_TREE_KERNEL) */
    PMX_SCORE_FORM_LEVELS_GRAPH = 2, /* one launch per BFS level, replayed from a captured graph (PMX_PLACE_LEVEL_KERNELS) */
    PMX_SCORE_FORM_LEVELS = 3        /* the same as plain launches (+ PMX_PLACE_NO_GRAPH) */
};
typedef struct {
    int32_t form;          /* PMX_SCORE_FORM_*; -1 before the first call */
    int32_t redone;        /* 1: the level kernels ran again after the persistent launch reported a starved grid */
    int64_t n_chains;      /* heavy-path decomposition of pmx_place_create */
    int64_t max_chain_len; /* nodes of its longest chain */
    int64_t n_levels;      /* BFS levels of the tree */
    int64_t grid_waves;    /* workgroups of the persistent launch x 4 waves; 0 for the level forms */
    int64_t reserved[4];
} pmx_score_info;
int pmx_place_score_info(const pmx_place *pl, pmx_score_info *out);
/* tied DFS indices of metric m (ascending), after pmx_place_score */
int pmx_place_tied(const pmx_place *pl, int metric, uint32_t *out, int64_t cap);
/* optional per-node outputs (host copies): scores [n_nodes][5] double, metrics [n_nodes][5] double,
   counts [n_nodes][2] int64; any pointer may be NULL */
int pmx_place_node_outputs(pmx_ctx *ctx, pmx_place *pl, double *scores5, double *metrics5, int64_t *counts2);
/* --refine (refineTopCandidates, src/placement.cpp:516-698): per metric the top refine_top_pct of the nodes (at most
 * max_top_n, always with the metric's winner) plus their neighbours within neighbor_radius branches (at most
 * max_neighbor_n each) are candidates; every candidate is scored once through `fn` (minus the total edit distance of the
 * reads against its genome: pmx_align_score_reads on pmx_panman_node_genome) and each metric keeps its best candidate
 * (ties: higher seed score, then lower DFS index).  Host logic; parent / scores5 / best_index as pmx_index_parents,
 * pmx_place_node_outputs and pmx_place_result give them.  fn returns 0 on success; anything else aborts with that code. */
typedef struct {
    double top_pct;          /* 0.01  (src/main.cpp:186-190) */
    int32_t max_top_n;       /* 150 */
    int32_t neighbor_radius; /* 2 */
    int32_t max_neighbor_n;  /* 150 */
    int32_t reserved;
} pmx_refine_params;
typedef struct {
    int32_t ran;             /* 0: no node had a positive score */
    int32_t n_candidates;
    int64_t score[5];        /* refined_<metric> score, metric order of the placement TSV */
    uint32_t node[5];        /* DFS index, 0xffffffff = none */
    uint32_t reserved;
} pmx_refine_result;
typedef int (*pmx_refine_score_fn)(void *user, uint32_t dfs_index, int64_t *score);
/* the candidate set alone (ascending DFS indices; returns its size): a caller may score the candidates concurrently and
 * hand pmx_refine_top_candidates a lookup */
int64_t pmx_refine_candidates(const uint32_t *parent, int64_t n_nodes, const double *scores5, const uint32_t best_index[5],
                              const pmx_refine_params *rp, uint32_t *cand_nodes, int64_t cand_cap);
int pmx_refine_top_candidates(const uint32_t *parent, int64_t n_nodes, const double *scores5, const uint32_t best_index[5],
                              const pmx_refine_params *rp, pmx_refine_score_fn fn, void *user, pmx_refine_result *out,
                              uint32_t *cand_nodes, int64_t *cand_scores, int64_t cand_cap);
/* kept read seeds after filtering: hash ascending + log1p(count) */
int64_t pmx_place_kept_seeds(pmx_ctx *ctx, pmx_place *pl, uint64_t *hash, double *logc, int64_t cap);

/* ------------------------------------------------------------------------------------------
 * ALIGN stage.  B-align boundary: identical to the reference's C ABI (src/mm_align.h:20-53).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t pos;    /* 1-based ref position (INT_MAX if unmapped) */
    int32_t rs, re; /* 0-based ref start/end */
    int32_t qs, qe; /* query start/end */
    uint8_t mapq;
    uint8_t rev;
    uint8_t proper_frag;
    int32_t n_cigar;
    uint32_t *cigar; /* BAM-encoded; malloc'd, caller frees */
    char *md;
} read_align_t;

typedef struct {
    read_align_t r1;
    read_align_t r2;
    int mapped;
} align_pair_result_t;

/* Drop-in for src/mm_align.h:44-53 (selected through the aligner function pointer at
   src/conversion.cpp:416-426).  Same argument meaning; n_threads is accepted and ignored (the GPU
   owns the parallelism).  On failure returns with `results` untouched, like the reference. */
void pmx_align_reads_direct(const char *reference, const char *refName, int n_reads, const char **reads,
                            const char **quality, const char **read_names, const int *r_lens,
                            align_pair_result_t *results, bool pairedEndReads, int n_threads);

/* ---- FASTA / FASTQ ingest (host): what seeding::readFastqPaired (src/seeding.cpp:231-269) and extractReadSequences
 * (src/placement.cpp:164-197) do with kseq.h, as flat arrays that upload to the device as they are.
 * kseq conventions: name = header up to the first white space; multi-line sequence / quality; CR stripped; a record
 * whose quality length differs from its sequence length ends the file.
 * pmx_fastx_read_paired: mate 2 reverse-complemented (upper-case ACGT only) with its qualities reversed, mates
 * interleaved (r1_0, r2_0, r1_1, ...), missing qualities 'I' x length; path2 NULL or "" = single-end; a mate-count
 * mismatch is PMX_ERR_ARG (the reference exits).  pmx_fastx_read: one file, records in file order, FASTA qualities
 * are zero bytes.  Views stay valid until pmx_fastx_free. */
typedef struct pmx_fastx pmx_fastx;
int pmx_fastx_read_paired(const char *path1, const char *path2, pmx_fastx **out);
int pmx_fastx_read(const char *path, pmx_fastx **out);
int64_t pmx_fastx_num_reads(const pmx_fastx *fx);
int pmx_fastx_views(const pmx_fastx *fx, const char **seq_concat, const char **qual_concat, const int64_t **offsets,
                    const char **names_concat, const int64_t **name_offsets);
void pmx_fastx_free(pmx_fastx *fx);

/* ---- BAM egress (host): what alignAndWriteBam does with the results of align_reads_direct
 * (src/conversion.cpp:288-538: build_bam_from_result, compute_sam_flags, compute_tlen, sort by pos, BAM + .bai).
 * reads / quality / read_names / r_lens are the arrays that were handed to the aligner (R2 already reverse-
 * complemented and its qualities reversed).  Writes `bam_path` and `bam_path`.bai.  Returns PMX_OK or PMX_ERR_IO. */
int pmx_write_bam(const char *bam_path, const char *ref_name, int64_t ref_len, int n_reads, const char **reads,
                  const char **quality, const char **read_names, const int *r_lens,
                  const align_pair_result_t *results, bool pairedEndReads);

/* Device-resident form used by the pipeline / benchmark: fixed 32-byte records + CIGAR arena. */
typedef struct {
    int32_t rs, re, qs, qe;
    uint8_t mapq, rev, proper_frag, mapped;
    uint16_t n_cigar;
    uint16_t flags;      /* PMX_ALN_* status bits */
    uint32_t cigar_off;  /* index into the CIGAR arena (uint32 ops) */
    int32_t score;       /* dp_max of the primary */
} pmx_aln_record;

#define PMX_ALN_OVERFLOW 0x1     /* a fixed-capacity work buffer overflowed: record is invalid */
#define PMX_ALN_UNSUPPORTED 0x2  /* hit a reference branch not implemented on the GPU yet */
#define PMX_ALN_HAS_ALN 0x4      /* the record carries an alignment (rs/re/qs/qe/mapq/CIGAR are set) */

typedef struct pmx_aligner pmx_aligner;
/* builds the minimizer index of one reference genome on the device; preset chosen from the mean
   read length exactly as setup_minimap2(for_scoring=1) does (src/mm_align.c:118-188) */
int pmx_aligner_create(pmx_ctx *ctx, const char *reference, int64_t ref_len, int mean_read_len, pmx_aligner **out);
/* re-target an existing aligner at another reference genome (keeps the work buffers) */
int pmx_aligner_set_reference(pmx_ctx *ctx, pmx_aligner *al, const char *reference, int64_t ref_len, int mean_read_len);
/* What the current reference index holds, for checks of the two index builders against each other (the device build of
 * ref_index_kernels.hip is the default; PMX_ALIGN_HOST_INDEX=1 selects the host restatement of mm_idx_str):
 * out[0] minimizer occurrences, out[1] distinct minimizers, out[2] mid_occ, out[3] a digest of every
 * (minimizer, occurrence list) pair, independent of the table's slot order; out[4] = 1 when the index was built on the device. */
int pmx_aligner_index_digest(pmx_ctx *ctx, pmx_aligner *al, uint64_t out[5]);
void pmx_aligner_free(pmx_ctx *ctx, pmx_aligner *al);
/* [hot] map + align every read (pair) of a packed read set.  revcomp_mate2 != 0: odd-indexed reads
   are reverse-complemented on the fly (what readFastqPaired does on the host, src/seeding.cpp:251).
   Results stay on the device until fetched. */
int pmx_align_readset(pmx_ctx *ctx, pmx_aligner *al, const pmx_readset *rs, int paired, int revcomp_mate2);
/* [hot, --refine] score_reads_vs_reference (src/mm_align.c:144-199): maps every read (pair) against the aligner's
 * reference and returns minus the summed count_read_errors (edit distance of the first region: block length - matches +
 * ambiguous bases; the read length without one).  Leaves the records of the run behind like pmx_align_readset.
 * Paired scoring needs an even number of reads. */
int pmx_align_score_reads(pmx_ctx *ctx, pmx_aligner *al, const pmx_readset *rs, int paired, int revcomp_mate2, int64_t *score);
/* Drop-in for the reference's scorer with its own signature (src/mm_align.h:13-17): host strings in (interleaved mates when
 * paired_end, mate 2 as sequenced), minus the total edit distance out, 0 on failure.  An odd read of a paired set is mapped
 * alone (src/mm_align.c:178-185); reads of flagged records count as unmapped (pmx_last_error() says how many). */
int64_t pmx_score_reads_vs_reference(const char *reference, int n_reads, const char **reads, const int *r_lens, int kmer_size,
                                     bool paired_end);
/* The DP kernel on its own (A9: ksw_extd2_sse, src/3rdparty/minimap2/ksw2_extd2_sse.c:28-400, with the aligner's scoring
 * parameters): a batch of (query, target) pairs of nt4 codes (0..3, 4 = N) through the GROUPED DP SERVICE of the short-read
 * tiers (align_kernel_dpg.hip) -- the entry point of its parity tests against the reference function and of its throughput
 * measurement (bench.py `dp_service`).  Sequence i is seqs[q_off[i] .. q_off[i+1]) / seqs[t_off[i] .. t_off[i+1]); w,
 * zdrop, end_bonus, flag (KSW_EZ_* bits) per request as the reference takes them.  out[i].served = 0 for a request the
 * service does not take (a side longer than 128 bases, a band that cuts the matrix, other flag combinations, more than 20
 * CIGAR operations): the align tiers run those on the wave-per-request kernels.  `reps` > 1 repeats the launch (timing);
 * *kernel_ms (may be NULL) receives the duration of one launch of the service kernel. */
typedef struct {
    int32_t served;
    uint32_t max;
    int32_t zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end;
    uint32_t cigar[20];
} pmx_dp_result;
/* the aligner's DP scoring: out[0..8] = a, b, q, e, q2, e2, sc_ambi, zdrop, end_bonus (mm_mapopt_t of the preset the mean
 * read length selected, src/mm_align.c:140-166) */
int pmx_align_scoring(const pmx_aligner *al, int32_t out[9]);
int pmx_align_dp_batch(pmx_ctx *ctx, pmx_aligner *al, const uint8_t *seqs, const int64_t *q_off, const int64_t *t_off, int64_t n,
                       const int32_t *w, const int32_t *zdrop, const int32_t *end_bonus, const int32_t *flag, pmx_dp_result *out,
                       int reps, double *kernel_ms);
/* One chosen DP implementation of the align tiers on a caller's requests (the entry point of their parity tests against the
 * reference's ksw_extd2_sse / ksw_ll_i16; inputs as pmx_align_dp_batch takes them):
 *   SERVE            the wave DP service as a service round launches it: everything else (class 2), then the register-resident
 *                    kernel for sides <= 192 (class 1).  Requests are posted in 480-byte entries ((qlen + 15 & ~15) + tlen <= 480)
 *                    and results hold up to 20 CIGAR operations.
 *   SERVE_ONE_CLASS  the same service with one class: every request through ksw_extd2 of the all-LDS unit.
 *   WAVE_LONG        one request per wave on the layout of the long-read launch (dp_fast LDS copy unless no_dp_fast).
 *   WAVE_GENERAL     the same on the general layout of the wave tiers (no dp_fast: the anti-diagonal kernel on the layout's arrays).
 *   SW_LL            sw_ll (ksw_ll_i16) on the long-read layout: score in .score, .qe / .te / .ok as it leaves them.
 * max_read_len / n_segs: what the layouts are planned from, by the planners the stage itself uses.  no_rows_dp: never the
 * row-by-row DP; no_dp_fast: no LDS copy of small DPs' arrays (the stage itself passes 0 for both).  caps[0] receives the capacities planned (SERVE: class 2,
 * caps[1] class 1) also when n == 0; a request beyond them comes back served = 0.  CIGARs go to cigar_arena (arena_cap words;
 * n * caps[0].max_cigar always suffices) at out[i].cigar_off.  path_taken: PMX_DP_PATH_* of the implementation that ran. */
#define PMX_DP_PROBE_SERVE 0
#define PMX_DP_PROBE_SERVE_ONE_CLASS 1
#define PMX_DP_PROBE_WAVE_LONG 2
#define PMX_DP_PROBE_WAVE_GENERAL 3
#define PMX_DP_PROBE_SW_LL 4
#define PMX_DP_PATH_REG 0x100      /* ksw_extd2_reg, | NC (1..3), | TB_LDS */
#define PMX_DP_PATH_ROWS 0x200     /* ksw_extd2_rows_t, | SW (4, 8, 12, 16), | EXACT */
#define PMX_DP_PATH_DIAG 0x300     /* ksw_extd2_t, | FAST or | TB_LDS */
#define PMX_DP_PATH_KIND 0x300
#define PMX_DP_PATH_EXACT 0x20
#define PMX_DP_PATH_FAST 0x40
#define PMX_DP_PATH_TB_LDS 0x80
#define PMX_DP_PATH_ALL_LDS 0x1000 /* dispatched by the all-LDS unit (SERVE_ONE_CLASS) */
typedef struct {
    int32_t served;
    uint32_t max;
    int32_t zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end;
    int32_t path_taken;
    int32_t ok, qe, te; /* SW_LL */
    int64_t cigar_off;
} pmx_dp_probe_result;
typedef struct {
    int32_t max_qlen, max_tlen, max_cigar, reserved;
    int64_t tb_cap, tb_fast_cap;
} pmx_dp_probe_caps;
int pmx_align_dp_probe(pmx_ctx *ctx, pmx_aligner *al, int path, int max_read_len, int n_segs, int no_rows_dp, int no_dp_fast,
                       const uint8_t *seqs, const int64_t *q_off, const int64_t *t_off, int64_t n, const int32_t *w,
                       const int32_t *zdrop, const int32_t *end_bonus, const int32_t *flag, pmx_dp_probe_result *out,
                       uint32_t *cigar_arena, int64_t arena_cap, pmx_dp_probe_caps caps[2]);
/* TEST ACCESSOR (not on the product path): one operation of the align tiers' anchor sort / chaining code on a batch of anchor lists,
 * exactly as map_frag calls it -- the entry point of the parity tests against the reference's radix_sort_128x / radix_sort_64 /
 * mg_lchain_dp / mg_lchain_rmq.
 *   path  WAVE_LONG / WAVE_GENERAL: one list per wave on the layout of the long-read launch / the general layout of the wave tiers
 *         (the wave forms: rank sort, chain_fill_wave, chain_fill_wide_wave, the ballot backtrack);
 *         LANE: one list per lane on the interleaved arena of the thread-per-pair kernel (the scalar forms, 64 different lists per wave).
 *   op    SORT128 radix_sort_128x, SORT64 radix_sort_64 (the x words; y is ignored and comes back 0), CHAIN_DP chain_dp,
 *         CHAIN_RMQ chain_rmq with the arguments of the long-join pass.  A path that does not compile an operation: PMX_ERR_UNSUPPORTED.
 * par: the chaining parameters; a field set to PMX_CHAIN_PROBE_DEFAULT (floats: NaN) takes the value of the aligner's preset
 * (max_dist_x / max_dist_y: max_gap; n_seg: 1), and the values in force are written back.  anchors: (x, y) word pairs in the
 * reference's packing, list i at [a_off[i], a_off[i + 1]); qlen: two read lengths per list (NULL: 0).  out_anchors / out_u: list i's
 * resulting anchors (out[i].n_a of them) and chains (out[i].n_u words score << 32 | count) from a_off[i] on.  out[i].status: the
 * PMX_ST_* bits the operation left (1 overflow, 2 unsupported).  A list longer than caps->max_anchor is not served (served = 0,
 * nothing written).  caps receives the capacities of the layout also when n == 0. */
#define PMX_CHAIN_PROBE_WAVE_LONG 0
#define PMX_CHAIN_PROBE_WAVE_GENERAL 1
#define PMX_CHAIN_PROBE_LANE 2
#define PMX_CHAIN_PROBE_SORT128 0
#define PMX_CHAIN_PROBE_SORT64 1
#define PMX_CHAIN_PROBE_CHAIN_DP 2
#define PMX_CHAIN_PROBE_CHAIN_RMQ 3
#define PMX_CHAIN_PROBE_DEFAULT INT32_MIN
typedef struct {
    int32_t bw, bw_long, max_gap, max_chain_skip, max_chain_iter, min_cnt, min_chain_score;
    float chn_pen_gap, chn_pen_skip;
    int32_t rmq_inner_dist, rmq_size_cap, max_dist_x, max_dist_y, n_seg;
} pmx_chain_probe_params;
typedef struct {
    int32_t served;
    uint32_t status;
    int64_t n_a;
    int32_t n_u, reserved;
} pmx_chain_probe_result;
typedef struct {
    int32_t max_anchor, max_reg, max_qlen, reserved;
} pmx_chain_probe_caps;
int pmx_align_chain_probe(pmx_ctx *ctx, pmx_aligner *al, int path, int op, int max_read_len, int n_segs, pmx_chain_probe_params *par,
                          const uint64_t *anchors, const int64_t *a_off, const int32_t *qlen, int64_t n, pmx_chain_probe_result *out,
                          uint64_t *out_anchors, uint64_t *out_u, pmx_chain_probe_caps *caps);
int64_t pmx_align_num_records(const pmx_aligner *al);
int64_t pmx_align_cigar_words(pmx_ctx *ctx, pmx_aligner *al);
int pmx_align_fetch(pmx_ctx *ctx, pmx_aligner *al, pmx_aln_record *records, int64_t n_records, uint32_t *cigar_arena,
                    int64_t arena_cap);
/* the same download without waiting for it, on a stream of the caller's choice (hipStream_t as void*; NULL = the context's):
 * the copies start once the results are complete, and the next pmx_align_readset on this aligner waits for them before it
 * overwrites its buffers.  The caller synchronises `stream` before reading the (pinned) host buffers. */
int pmx_align_fetch_async(pmx_ctx *ctx, pmx_aligner *al, pmx_aln_record *records, int64_t n_records, uint32_t *cigar_arena,
                          int64_t arena_cap, void *stream);
/* copy the fixed-size records into a caller-owned DEVICE buffer (for RCCL gathers) */
int pmx_align_copy_records_device(pmx_ctx *ctx, pmx_aligner *al, void *d_records, int64_t n_records);
/* the same for the CIGAR arena (pmx_align_cigar_words() words): records + arena are what rank 0 needs to write the BAM */
int pmx_align_copy_cigars_device(pmx_ctx *ctx, pmx_aligner *al, void *d_cigars, int64_t n_words);
/* Work statistics of the last pmx_align_readset call (no reference counterpart; bench.py reports GCUPS from them):
   DP cells are counted as q * min(t, 2w+1) per ksw2 call. */
typedef struct pmx_align_stats {
    int64_t n_items;        /* pairs (paired) or reads aligned */
    int64_t dp_pairs;       /* items that needed at least one ksw2 DP (the rest were answered by proved shortcuts) */
    int64_t dp_calls;       /* ksw2 DPs run */
    int64_t dp_cells;       /* their cells */
    int64_t dp_rounds;      /* DP-service rounds of the thread-per-pair tier */
    int64_t wave_tier_items;     /* items handed to the wave-per-pair tiers */
    int64_t general_tier_items;  /* ... of which re-run with the general capacities */
    int64_t compact_tier_items;  /* items finished by the compact LDS tier */
    int64_t huge_tier_items;     /* wave-tier items re-run once more with 16x the anchors (what overflowed the general capacities) */
    int64_t simple_chain_items;  /* ... of the compact tier's, the distinct pairs its register-only chain kernel finished (mates that
                                    do not overlap on the reference) */
    int64_t near_chain_items;    /* ... and the ones it finished whose mates' extents overlap while their seeds do not (the near class);
                                    not part of simple_chain_items */
    int64_t reserved[5];
} pmx_align_stats;
int pmx_align_get_stats(pmx_ctx *ctx, pmx_aligner *al, pmx_align_stats *out);
/* device pointers of the last result (for RCCL gathers without a host bounce) */
const void *pmx_align_device_records(const pmx_aligner *al);
const void *pmx_align_device_cigars(const pmx_aligner *al);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: one rank per GPU (a process, or a host thread with its own context), RCCL over xGMI.
 * The reference is a single process; the two exchange steps follow SURVEY.md section 8e.  Reads are sharded by the
 * caller (contiguous, pair-aligned shards), the seed index and the placed genome are replicated per GPU.
 *   rank 0: pmx_dist_unique_id(id); ship the 128 bytes to every rank (a file, a pipe, MPI, a torch store ...)
 *   every rank: pmx_dist_init(ctx, id, rank, world, &d)            -- collective (ncclCommInitRank)
 *   per sample: seed the shard, pmx_dist_merge_histograms(d, pl), pmx_place_score (replicated: same result on every
 *               rank), align the shard, pmx_dist_gather_alignments(d, al, 0, ...), rank 0 writes the BAM.
 * Every call is collective over the ranks of `d` and stream-ordered on the context's stream.  librccl.so.1 is loaded on
 * first use.  PMX_DIST_HOST_DIR=<shared directory>: a file-based transport through host memory for functional tests on a
 * box with fewer GPUs than ranks (RCCL refuses two ranks on one device).
 * ------------------------------------------------------------------------------------------ */
#define PMX_DIST_ID_BYTES 128
typedef struct pmx_dist pmx_dist;
int pmx_dist_unique_id(char id[PMX_DIST_ID_BYTES]);
int pmx_dist_init(pmx_ctx *ctx, const char id[PMX_DIST_ID_BYTES], int rank, int world, pmx_dist **out);
void pmx_dist_free(pmx_dist *d);
int pmx_dist_rank(const pmx_dist *d);
int pmx_dist_world(const pmx_dist *d);
int pmx_dist_barrier(pmx_dist *d);
/* element-wise sum of every rank's n values, on every rank (--refine over shards: candidate scores add up) */
int pmx_dist_sum_i64(pmx_dist *d, int64_t *vals, int64_t n);
/* --dedup over the whole sample (src/placement.cpp:1550-1620 collapses duplicates of ALL reads): every rank thins its shard
 * (exact comparison), the ranks exchange the 128-bit hash pairs of the reads they keep, and a read whose pair a lower rank
 * keeps is dropped.  Then pmx_place_add_reads(..., dedup_reads = 1) on the same read set seeds through that mask.
 * Building blocks (also usable with another transport): pmx_place_dedup_local (mask + the kept reads' hash pairs into two
 * device arrays of n_reads entries; returns their number), pmx_place_dedup_drop_seen, pmx_place_dedup_local_count. */
int pmx_dist_dedup_reads(pmx_dist *d, pmx_place *pl, const pmx_readset *rs, int64_t *n_kept_local);
int64_t pmx_place_dedup_local(pmx_ctx *ctx, pmx_place *pl, const pmx_readset *rs, void *d_h1, void *d_h2, int64_t cap);
int pmx_place_dedup_drop_seen(pmx_ctx *ctx, pmx_place *pl, const pmx_readset *rs, void *d_seen_h1, void *d_seen_h2, int64_t n_seen);
int64_t pmx_place_dedup_local_count(pmx_ctx *ctx, pmx_place *pl, const pmx_readset *rs);
/* all-gather of the ranks' (hash, count) histograms + integer merge: afterwards every rank's placer holds the histogram of
 * the whole sample and pmx_place_score gives the same result on every rank (no floating-point reduction anywhere) */
int pmx_dist_merge_histograms(pmx_dist *d, pmx_place *pl);
/* the records and the CIGAR arena of the aligner's last call, from every rank to `root` (exact sizes, point to point); on
 * the root the records stand in rank order with cigar_off rebased onto the arenas laid back to back.  n_records / n_words:
 * totals on the root, 0 elsewhere. */
int pmx_dist_gather_alignments(pmx_dist *d, pmx_aligner *al, int root, int64_t *n_records, int64_t *n_words);
/* One-node form of step 2 (no traffic between the GPUs, no funnel through the root's PCIe link): the ranks agree on the
 * place of every rank's records / CIGAR words in ONE result set (records in rank order, arenas back to back; one small
 * all-gather of the counts) and each rank downloads its own part -- cigar_off rebased onto the merged arena on the device --
 * to that place in host buffers all ranks map (shared memory; pinned / registered for the copies to be asynchronous).
 * pmx_dist_rank_counts reports the sizes the plan exchanged. */
int pmx_dist_plan_alignments(pmx_dist *d, pmx_aligner *al, int64_t *record_base, int64_t *word_base, int64_t *total_records,
                             int64_t *total_words);
int pmx_dist_fetch_shard_async(pmx_dist *d, pmx_aligner *al, pmx_aln_record *records_all, uint32_t *cigars_all, void *stream);
const void *pmx_dist_gathered_records(const pmx_dist *d);   /* device pointers of the last gather (root) */
const void *pmx_dist_gathered_cigars(const pmx_dist *d);
int pmx_dist_rank_counts(const pmx_dist *d, int64_t *records_per_rank, int64_t *words_per_rank);   /* world entries each */
int pmx_dist_fetch_gathered(pmx_dist *d, pmx_aln_record *records, int64_t n_records, uint32_t *cigar_arena, int64_t arena_cap);
int pmx_dist_fetch_gathered_async(pmx_dist *d, pmx_aln_record *records, int64_t n_records, uint32_t *cigar_arena,
                                  int64_t arena_cap, void *stream);   /* see pmx_align_fetch_async */

/* ------------------------------------------------------------------------------------------
 * --meta: haplotype deconvolution of a mixed sample (BASELINE config 5; src/main.cpp:1192-1313 runDeconvolution,
 * src/mgsr.cpp).  Reads -> seedmer lists (k-min-mer hash + orientation), merged by list; every node's overlap coefficient
 * (:5685-5790); the nodes of the best top_oc distinct coefficients are the candidates (:8010-8060); a parsimony score per
 * (read, candidate) = max(seedmers the node's genome holds in the read's orientation, in the other one) (:7225-7455);
 * candidates with equal score columns merge; P(read | node) = err^(n - s) (1 - err)^s; SQUAREM EM (:4341-4443), nodes under
 * prop_threshold dropped, again (<= em_max_rounds, :4445-4490).  csrc/api_meta.hip says how each step runs on the device.
 * The node side is an ORIENTED index over the same tree as the place stage's index (PMX_INDEX_ORIENTED).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    double error_rate;          /* 0.005 (src/mgsr.hpp:1109) */
    double em_convergence;      /* 1e-5  --em-convergence-threshold: |log-likelihood change| that ends the EM */
    double em_delta_threshold;  /* 0     --em-delta-threshold: > 0 = stop on the largest proportion change instead */
    double prop_threshold;      /* 0.005 propThresholdToRemove (src/mgsr.hpp:1108) */
    double discard;             /* 0     --discard: reads whose best score < discard * seedmers carry no weight */
    int32_t em_max_iterations;  /* 1000 */
    int32_t em_max_rounds;      /* 5 */
    int64_t reserved[2];
} pmx_meta_params;
typedef struct pmx_meta pmx_meta;
int pmx_meta_create(pmx_ctx *ctx, const pmx_index *idx, const pmx_index *idx_oriented, pmx_meta **out);
void pmx_meta_free(pmx_ctx *ctx, pmx_meta *m);
/* reads (concatenated ASCII + n+1 offsets, mates as sequenced): seedmer lists, merge, overlap coefficients of all nodes */
int pmx_meta_set_reads(pmx_ctx *ctx, pmx_meta *m, const char *concat, const int64_t *offsets, int64_t n_reads);
/* candidates = the nodes of the top_oc best distinct overlap coefficients (1000: --top-oc), or exactly the given nodes when
 * n_override > 0; then every (merged read, candidate) parsimony score on the device */
int pmx_meta_score(pmx_ctx *ctx, pmx_meta *m, int64_t top_oc, const uint32_t *cand_override, int64_t n_override);
int pmx_meta_em(pmx_ctx *ctx, pmx_meta *m, const pmx_meta_params *mp);
int64_t pmx_meta_num_reads(const pmx_meta *m);        /* merged reads that have seedmers */
int64_t pmx_meta_num_candidates(const pmx_meta *m);
int pmx_meta_candidates(const pmx_meta *m, uint32_t *dfs_index, int64_t cap);          /* ascending */
int pmx_meta_overlap_coefficients(const pmx_meta *m, double *oc, int64_t cap);         /* per node */
int pmx_meta_read_info(const pmx_meta *m, int64_t *n_seedmers, int64_t *multiplicity, int64_t cap);
int pmx_meta_read_seedmers(const pmx_meta *m, int64_t *offsets, uint64_t *hash, uint8_t *rev, int64_t cap_seedmers);
int pmx_meta_scores(pmx_ctx *ctx, pmx_meta *m, uint16_t *scores, int64_t cap);         /* [reads][candidates]; see pmx_meta_row_range */
/* the estimated haplotypes, by proportion (descending): representative node, proportion, the candidates merged into it */
int64_t pmx_meta_num_haplotypes(const pmx_meta *m);
int pmx_meta_haplotype(const pmx_meta *m, int64_t i, uint32_t *node, double *prop, int64_t *n_members, uint32_t *members,
                       int64_t cap);
int pmx_meta_em_info(const pmx_meta *m, int32_t *rounds, int32_t *iterations, double *log_likelihood);
/* --dust T (src/main.cpp:2059-2061, default 100 = off): pmx_meta_set_reads drops every read whose DUST score is non-zero and
 * greater than T (src/mgsr.cpp:1593-1594, 1833-1834).  pmx_read_dust = mgsr::getDust (src/mgsr.cpp:1505-1568; host, no
 * device): Prinseq-scaled score over base triplets in a sliding window of `window` triplets (the reference uses 64). */
int pmx_meta_set_dust(pmx_meta *m, double threshold);
/* --mask-read-ends N (src/main.cpp:2065; extractReadSequences, src/mgsr.cpp:1274-1280, 1304-1310), 0 = off, kept for the
 * pmx_meta_set_reads calls that follow: a read of length L becomes read[N : L - N] when L > 2N and the empty read otherwise,
 * before anything else looks at it.  The DUST score is the trimmed read's (an empty one scores 0 and stays), the seedmer
 * lists and the overlap coefficients are seeded from the trimmed read (the seeding kernels' per-end trim: no copy of the
 * reads), and a read trimmed to nothing counts wherever a read without seedmers counts: in the kept reads behind the overlap
 * coefficients, in its amplicon group's N, -1 in pmx_meta_raw_to_merged.  When every read ends empty there are no merged
 * reads, every overlap coefficient is 0 and pmx_meta_em leaves no haplotype.  n < 0 or n > INT32_MAX: PMX_ERR_ARG.
 * --gpus N: the same value on every rank, each trims its shard.  pmx_meta_assign on reads set with N > 0 is
 * PMX_ERR_UNSUPPORTED: the reference's reader for --filter-and-assign takes the value and ignores it (src/mgsr.cpp:1575). */
int pmx_meta_set_mask_read_ends(pmx_meta *m, int64_t n);
/* --em-leaves-only (src/main.cpp:2053; squareEM::squareEM, src/mgsr.cpp:8018-8037), for the pmx_meta_score calls that follow
 * without a candidate override (an override stays "exactly these nodes").  A node is a SAMPLE when its id in the plain index
 * does not begin with `node_`, and ELIGIBLE when it, or a node that pmx_index_node_heads folds onto the same head, is a
 * sample.  The candidates are then chosen by walking the nodes by falling overlap coefficient (ascending DFS index within a
 * value), passing over the nodes that are not eligible BEFORE a rank is counted, up to top_oc distinct values among the
 * eligible ones.  Every node is ranked by its own coefficient, as without the switch, and equal score columns are merged
 * after scoring.  No eligible node: PMX_ERR_ARG. */
int pmx_meta_set_em_leaves_only(pmx_meta *m, int on);
/* --mask-reads N / --mask-seeds N (src/main.cpp:2026-2030; initializeQueryData, src/mgsr.cpp:2049-2139), both 0 = off, for the
 * pmx_meta_set_reads calls that follow.  On the merged reads, count[h] = the sum of the multiplicities of the merged reads whose
 * list holds hash h (once per read, either orientation).  mask_reads T > 0: a merged read with an entry of count <= T is
 * dropped; mask_seeds T > 0: every entry of count <= T is removed, the rest keeps its order, a read left empty is dropped and
 * reads that became equal stay apart.  Everything after -- overlap coefficients, candidates, scores, EM, the read getters,
 * pmx_meta_raw_to_merged (-1 for a read of a dropped merged read) -- is of the survivors.  Both > 0: PMX_ERR_ARG, "Only one
 * masking parameter can be set at a time" (src/mgsr.cpp:2049-2053); a negative value: PMX_ERR_ARG.  --gpus N: the same masks
 * on every rank.  pmx_meta_assign on reads set with a mask is PMX_ERR_UNSUPPORTED: the reference's reader for
 * --filter-and-assign never masks (initializeQueryDataBatch, src/mgsr.cpp:1575). */
int pmx_meta_set_masks(pmx_meta *m, int64_t mask_reads, int64_t mask_seeds);
/* of the last pmx_meta_set_reads (src/mgsr.cpp:2049-2139, reported at :2220-2230): numMaskReads (merged reads dropped by
 * mask_reads), numMaskSeeds (entries removed by mask_seeds), numPassedReads (merged reads left); pointers may be NULL */
int pmx_meta_mask_info(const pmx_meta *m, int64_t *reads_dropped, int64_t *seeds_removed, int64_t *reads_left);
/* the distinct hashes of the merged reads BEFORE masking, ascending, with count[h] (kminmerCounts, src/mgsr.cpp:2049-2139:
 * :2055-2060); pmx_meta_mask_num_counts of them (0 when the last pmx_meta_set_reads ran without a mask, and
 * pmx_meta_mask_counts is PMX_ERR_ARG then); either array may be NULL */
int64_t pmx_meta_mask_num_counts(const pmx_meta *m);
int pmx_meta_mask_counts(const pmx_meta *m, uint64_t *hash, int64_t *count, int64_t cap);
/* --amplicon-depth FILE, --mask-reads-relative-frequency X, --mask-seeds-relative-frequency X (src/main.cpp:2032-2040;
 * extractReadSequences, src/mgsr.cpp:1216-1342; initializeQueryData, :1774-2235).  pmx_meta_set_amplicons: the amplicon of every
 * raw read of the pmx_meta_set_reads calls that follow, until cleared with NULL / 0 -- group_of_read[r] in [0, n_groups], the
 * value n_groups meaning "not listed in the file" (the reference's last group).  A set_reads with another n_reads, or with a
 * value out of range, is PMX_ERR_ARG.  With amplicons set:
 *   - reads are merged by seedmer list WITHIN their amplicon: the same list in two amplicons stays two merged reads, each with
 *     its own multiplicity.  Merged reads are ordered by (amplicon, hash list, orientation list);
 *   - a mask counts within the amplicon: count[g][h] = the summed multiplicities of the merged reads of g that carry h, and a
 *     read of g is masked against the threshold of g.  T_g = the absolute parameter of pmx_meta_set_masks, or under a relative
 *     parameter rf (size_t)(rf * (double)N_g), N_g = the raw reads of g passed to set_reads (before --dust, reads without
 *     seedmers included).  The unlisted group always takes the absolute parameter, so a relative parameter leaves it unmasked;
 *     a threshold of 0 masks nothing in its group.  numMaskReads / numMaskSeeds (pmx_meta_mask_info) are summed over the groups,
 *     pmx_meta_mask_counts reports per distinct hash of the sample the sum over the groups;
 *   - amplicons alone (no mask parameter above 0) only change the merge: no mask step runs;
 *   - pmx_meta_raw_to_merged names the merged read of the raw read's own amplicon; pmx_meta_assign is PMX_ERR_UNSUPPORTED
 *     (the reference's batch reader takes no such file).
 * pmx_meta_set_relative_masks: both 0 = off; a negative value is PMX_ERR_ARG; more than one of the four masking parameters
 * above 0 is PMX_ERR_ARG, "Only one masking parameter can be set at a time" (checked by whichever setter is called second and by
 * set_reads).  A relative parameter without amplicons does nothing in the reference (its single group is the unlisted one);
 * here set_reads refuses it with PMX_ERR_ARG.  A read set of 2^32 - 1 list entries or more under amplicons with a mask is
 * PMX_ERR_CAPACITY.  --gpus N: every rank passes the groups of its own shard with the same n_groups; ranks that disagree on
 * n_groups all return PMX_ERR_ARG from set_reads. */
int pmx_meta_set_amplicons(pmx_meta *m, const int32_t *group_of_read, int64_t n_reads, int32_t n_groups);
int pmx_meta_set_relative_masks(pmx_meta *m, double reads_rf, double seeds_rf);
/* of the last pmx_meta_set_reads, when it ran with amplicons (PMX_ERR_ARG otherwise): the amplicon of every merged read (cap >=
 * pmx_meta_num_reads); per group g in [0, n_groups] (cap >= pmx_meta_num_amplicon_groups = n_groups + 1, 0 without amplicons)
 * its raw reads N_g, the threshold applied (0 without a mask), its merged reads before masking and its merged reads left; any
 * pointer may be NULL */
int pmx_meta_read_amplicons(const pmx_meta *m, int32_t *amplicon, int64_t cap);
int32_t pmx_meta_num_amplicon_groups(const pmx_meta *m);
int pmx_meta_amplicon_info(const pmx_meta *m, int64_t *raw_reads, int64_t *threshold, int64_t *merged_before, int64_t *merged_left, int64_t cap);
/* the (group, hash, count) triples BEFORE masking, ascending by (group, hash); pmx_meta_amplicon_num_counts of them (0, and
 * pmx_meta_amplicon_counts PMX_ERR_ARG, unless the last pmx_meta_set_reads ran with amplicons AND a mask); any array may be NULL */
int64_t pmx_meta_amplicon_num_counts(const pmx_meta *m);
int pmx_meta_amplicon_counts(const pmx_meta *m, int32_t *group, uint64_t *hash, int64_t *count, int64_t cap);
/* Host only.  The table of --amplicon-depth: one `read id <TAB> primer id` per line; groups numbered by first appearance of the
 * primer id; a later line for a read id replaces an earlier one (the earlier primer keeps its group, possibly empty); empty
 * lines are skipped.  PMX_ERR_IO: the file cannot be read; PMX_ERR_FORMAT (the message holds the line number): a line that does
 * not have exactly two tab-separated non-empty fields.  pmx_amplicons_lookup: the group of a read name (the FASTQ header up to
 * the first white space), -1 when unlisted. */
typedef struct pmx_amplicons pmx_amplicons;
int pmx_amplicons_load(const char *path, pmx_amplicons **out);
void pmx_amplicons_free(pmx_amplicons *a);
int32_t pmx_amplicons_num_groups(const pmx_amplicons *a);
const char *pmx_amplicons_group_name(const pmx_amplicons *a, int32_t g);
int32_t pmx_amplicons_lookup(const pmx_amplicons *a, const char *read_name);
/* --meta --gpus N: call after pmx_meta_create, before pmx_meta_set_reads (`d` on the same context, kept alive by the caller).
 * From then on set_reads, score and em are COLLECTIVE: every rank calls them in the same order, set_reads with its own shard of
 * the raw reads.  The merged reads, overlap coefficients, candidates, haplotypes and em_info are then those of one rank over the
 * whole sample, bit for bit, on every rank.  pmx_meta_scores returns only this rank's rows: merged reads [first, first + count)
 * (pmx_meta_row_range; without a dist: 0 and num_reads).
 * pmx_meta_assign and pmx_meta_read_best are collective too, for a dist of two ranks or more (a dist of ONE rank stays
 * PMX_ERR_UNSUPPORTED for both, as every dist was before: one GPU runs them without a dist): each sets the row range by the rule of pmx_meta_score (it is 0
 * rows between set_reads and the first of the three) and works on its rank's rows only.  Their per-read getters
 * (pmx_meta_assign_reads / _nodes / _taxa, pmx_meta_assign_num_nodes, pmx_meta_read_best_get) then report this rank's rows, index
 * 0 = `first`, cap >= count; pmx_meta_breadth and pmx_meta_active_nodes are the whole sample's on every rank.  The rules that
 * keep these collectives from hanging (csrc/meta_assign.hip has them in full): every refusal follows from settings that are the
 * same on every rank; pmx_meta_assign begins by exchanging a digest of its settings (discard, breadth on / off, max_taxa, the
 * ambiguity pair, a hash of the taxonomy's node table) and ranks that disagree ALL return PMX_ERR_ARG before any other exchange;
 * no exchange depends on a rank's own number of rows or chunks, and a rank with an empty shard or no rows takes part in all.
 * pmx_meta_assign_gather / pmx_meta_read_best_gather (collective; PMX_ERR_ARG without a dist, before the matching compute call,
 * or a second time after it): every rank's rows to `root`, whose getters then cover all pmx_meta_num_reads merged reads and equal
 * one rank's over the whole sample bit for bit (the CSR offsets rebased, the node lists in row order); the other ranks keep
 * their rows.  pmx_meta_row_range stays the rank's own on every rank.  No run on more than one physical GPU exists: the tests
 * run the ranks as processes on one device. */
int pmx_meta_assign_gather(pmx_ctx *ctx, pmx_meta *m, int root);
/* rows of the breadth hit matrix per exchange of its merge over the ranks (0 = default: what a 1 GiB buffer of world x slab holds);
 * the same value on every rank; the tests force slab edges with it.  rows < 0: PMX_ERR_ARG */
int pmx_meta_set_breadth_slab(pmx_meta *m, int64_t rows);
int pmx_meta_read_best_gather(pmx_ctx *ctx, pmx_meta *m, int root);
int pmx_meta_attach_dist(pmx_meta *m, pmx_dist *d);
int pmx_meta_row_range(const pmx_meta *m, int64_t *first, int64_t *count);
double pmx_read_dust(const char *seq, int64_t len, int32_t window);

/* --meta --filter-and-assign (filterAndAssignBatch, src/main.cpp:720-1016; scoreReadsBatch / assignReadsBatch,
 * src/mgsr.cpp:7477-7575, 6415-6516).  Call after pmx_meta_set_reads (mates are independent reads; --dust as set by
 * pmx_meta_set_dust).  Every merged read is scored against EVERY node, score = max(f, r) as above; with max its best score and
 * n its seedmers (pmx_meta_read_info): max == 0 -> PMX_META_UNMAPPED; 0 < max < (int32)(discard * n) -> PMX_META_DISCARDED
 * (the cast truncates, src/mgsr.cpp:1693); else PMX_META_ASSIGNED, and the read's nodes are ALL nodes with score == max, its LCA
 * node their lowest common ancestor (UINT32_MAX for a read that is not assigned).  Nodes are DFS indices; identical nodes are
 * NOT folded here (pmx_index_node_heads folds at output time).  With an attached dist: collective, see pmx_meta_attach_dist.
 * With a taxonomy (pmx_meta_set_taxonomy, below) an assigned read whose best-scoring or near-best-scoring nodes span more than
 * max_taxa taxa becomes PMX_META_OVER_TAXA instead: no nodes, no LCA.  PMX_ERR_UNSUPPORTED then for discard > 0 together with
 * a non-zero ambiguity threshold.  Without a taxonomy nothing of it runs.
 * Parity with the reference's own run is unpinned, as for --meta; csrc/meta_assign.hip says how it runs on the device. */
#define PMX_META_UNMAPPED 0
#define PMX_META_DISCARDED 1
#define PMX_META_ASSIGNED 2
#define PMX_META_OVER_TAXA 3
int pmx_meta_assign(pmx_ctx *ctx, pmx_meta *m, double discard);
/* per merged read (cap >= pmx_meta_num_reads); any pointer may be NULL.  n_nodes is 0 unless the read is assigned */
int pmx_meta_assign_reads(const pmx_meta *m, uint8_t *state, uint16_t *max_score, uint32_t *lca, uint32_t *n_nodes, int64_t cap);
/* the assigned nodes as a CSR list: read r's nodes at nodes[offsets[r] .. offsets[r + 1]), ascending; num_reads + 1 offsets */
int64_t pmx_meta_assign_num_nodes(const pmx_meta *m);
int pmx_meta_assign_nodes(const pmx_meta *m, int64_t *offsets, uint32_t *nodes, int64_t cap_nodes);
/* The taxonomy filter of --filter-and-assign (--taxonomic-metadata, --maximum-taxon-number; fillTaxonIndices, src/mgsr.cpp:
 * 156-196; checkTaxonIndicesBatch, :6463-6496).  node_taxon: per DFS index of the oriented index the node's own taxon in [0,
 * n_taxa), -1 = none (any node, internal ones included).  S(v) = the taxa in the subtree of v, in the tree as indexed (identical
 * nodes not folded); a node is over when |S(v)| > max_taxa.  A read's taxa are the union of S(v) over the nodes where one of
 * its seedmers changes presence (in either orientation; at the root: is present) and its score is >= lo = max(0, max - amb),
 * amb = max(abs, (int)(max * ratio)) (pmx_meta_set_ambiguous: --ambiguous-score-threshold, -ratio; both 0 = its best nodes);
 * it is over when one of those nodes is, or the union exceeds max_taxa.  max_taxa 0 clears the taxonomy (node_taxon may be
 * NULL); max_taxa > 16 is PMX_ERR_UNSUPPORTED.  Both hold for the pmx_meta_assign calls that follow. */
int pmx_meta_set_taxonomy(pmx_meta *m, const int32_t *node_taxon, int64_t n_nodes, int64_t n_taxa, int32_t max_taxa);
int pmx_meta_set_ambiguous(pmx_meta *m, int32_t abs, double ratio);
/* the taxa of every merged read of the last pmx_meta_assign (cap >= pmx_meta_num_reads reads): n_taxa[r] ids, ascending, at
 * taxa[r * max_taxa] with max_taxa = pmx_meta_assign_max_taxa (0: the call ran without a taxonomy); n_taxa is 0 unless the
 * read is assigned */
int pmx_meta_assign_taxa(const pmx_meta *m, uint32_t *n_taxa, uint32_t *taxa, int64_t cap);
int32_t pmx_meta_assign_max_taxa(const pmx_meta *m);
/* S(v) of the taxonomy that is set: its size (ids[0 .. size) ascending, ids may be NULL), -1 when it exceeds max_taxa, -2 for
 * a bad argument or without a taxonomy */
int64_t pmx_meta_node_taxa(const pmx_meta *m, int64_t v, uint32_t *ids, int64_t cap);
/* Host only.  The taxonomic metadata table (loadTaxonomicMetadata, src/mgsr.cpp:198-256): tokens separated by white space; the
 * header token equal to `rank` names the column, which must not be the first; on every other line the first token is a node
 * identifier and the token in that column its taxon (`.`: the line is skipped; empty lines too); a taxon's index is its order
 * of first appearance; a later line for an identifier replaces an earlier one.  PMX_ERR_IO: the file cannot be read;
 * PMX_ERR_ARG: no such rank in the header, or in its first column; PMX_ERR_FORMAT: no header line, or a line that ends before
 * the column.  pmx_taxonomy_lookup: the taxon of an identifier, -1 when the table has none. */
typedef struct pmx_taxonomy pmx_taxonomy;
int pmx_taxonomy_load(const char *path, const char *rank, pmx_taxonomy **out);
void pmx_taxonomy_free(pmx_taxonomy *t);
int64_t pmx_taxonomy_num_taxa(const pmx_taxonomy *t);
const char *pmx_taxonomy_taxon_name(const pmx_taxonomy *t, int64_t taxon);
int64_t pmx_taxonomy_lookup(const pmx_taxonomy *t, const char *identifier);
/* --breadth-ratio of --filter-and-assign (calculateBreadthRatio, src/mgsr.cpp:6518-6584): whether the reads assigned to a node
 * cover its genome.  pmx_meta_set_breadth(on): the pmx_meta_assign calls that follow also compute it (default off: nothing of it
 * runs or is allocated).  pmx_meta_breadth: per DFS index (cap_nodes >= the index's nodes; any pointer may be NULL), over the
 * assignment of the last pmx_meta_assign (reads that are PMX_META_ASSIGNED; a merged read counts with its multiplicity):
 *   total_ref_seeds  distinct seedmer hashes of the node's genome, either orientation (node->totalRefSeeds, mgsr.cpp:590-610)
 *   observed         distinct hashes among them that some read assigned to the node carries (ObservedBreadthCount)
 *   depth            sum over the reads assigned to the node of multiplicity x (distinct hashes of the read that the node holds)
 * A node folded into its head (pmx_index_node_heads) carries its head's numbers.  The file's four ratios follow on the host:
 * obs / total and depth / total (0 when total is 0), 1 - exp(-mean depth) (0 when that is 0), observed over expected ratio (0 when
 * expected is 0).  PMX_ERR_ARG when the last pmx_meta_assign ran without breadth (pmx_meta_set_reads empties it, like the other
 * results).  pmx_meta_assign with breadth is PMX_ERR_UNSUPPORTED when one bit per (distinct seedmer of the reads, node) exceeds
 * 8 GiB: nothing is approximated. */
int pmx_meta_set_breadth(pmx_meta *m, int on);
int pmx_meta_breadth(const pmx_meta *m, uint64_t *total_ref_seeds, uint64_t *observed, uint64_t *depth, int64_t cap_nodes);
/* The per-read scores behind --write-meta-read-scores-unfiltered / -filtered of the abundance mode (scoreReads, src/mgsr.cpp:
 * 7325-7420: maxScore and epp of every read; collapseIdenticalScoringNodes, :794-847; writeMetaReadScores, src/main.cpp:446-466).
 * pmx_meta_read_best scores every merged read of the last pmx_meta_set_reads against EVERY node, score = max(f, r) as above,
 * and keeps two numbers a read: max_score, its best score over all nodes, and n_best, the number of ACTIVE nodes that reach
 * it (0 when max_score is 0).  A node is active when it is the root or one of its changes in the oriented index has a hash, in
 * either orientation, among the distinct seedmer hashes of the merged reads (after --dust and the masks): the nodes the
 * reference keeps when it collapses the tree for a sample.  An inactive node scores as its nearest active ancestor, so the
 * maximum is the same over either set.  It needs no pmx_meta_score, builds no read -> node list, and runs on reads set with a
 * mask, with amplicons or with masked ends.  PMX_ERR_ARG before pmx_meta_set_reads; with an attached dist it is collective
 * (pmx_meta_attach_dist).  What pmx_meta_assign left on the handle stays, and the other
 * way round; pmx_meta_set_reads empties all of it.
 * pmx_meta_read_best_get: per merged read (cap >= pmx_meta_num_reads; either pointer may be NULL); pmx_meta_active_nodes: one
 * byte per DFS index, 1 = active (cap_nodes >= the index's nodes).  Both PMX_ERR_ARG until pmx_meta_read_best has run since the
 * last pmx_meta_set_reads. */
int pmx_meta_read_best(pmx_ctx *ctx, pmx_meta *m);
int pmx_meta_read_best_get(const pmx_meta *m, uint16_t *max_score, uint32_t *n_best, int64_t cap);
int pmx_meta_active_nodes(const pmx_meta *m, uint8_t *active, int64_t cap_nodes);
/* the reads of the last pmx_meta_set_reads in input order -> their merged read, -1 for a read dropped by --dust, without
 * seedmers or dropped by a low-coverage mask.  With an attached dist: pmx_meta_num_raw_reads is the shard's raw count and the
 * map names, for this rank's raw reads in shard order, their merged read in the WHOLE sample's numbering -- the slice of the
 * one-rank map that the shard covers */
int64_t pmx_meta_num_raw_reads(const pmx_meta *m);
int pmx_meta_raw_to_merged(const pmx_meta *m, int64_t *map, int64_t cap);
/* Host only, no device.  head[v] of an ORIENTED index: v itself when v is the root or carries changes, else the nearest
 * ancestor that does -- a node without changes has its parent's seed set, scores as it, and the reference prints it on that
 * ancestor's line (src/mgsr.cpp:505-532).  pmx_index_lca: the lowest common ancestor of two DFS indices, -1 out of range. */
int pmx_index_node_heads(const pmx_index *idx_oriented, uint32_t *head);
int64_t pmx_index_lca(const pmx_index *idx, int64_t a, int64_t b);

/* ------------------------------------------------------------------------------------------
 * GENOTYPE + CONSENSUS stages (runGenotyping / runConsensus, src/main.cpp:1828-1900).  The reference forks
 * `bcftools mpileup -Ou -B`, `bcftools call --ploidy 1 -m -A`, filters the calls (src/genotyping.cpp:167-279) and forks
 * `bcftools consensus` (src/conversion.cpp:83-255).  Here: a device pileup into integer tables, the htslib error model and
 * the reference's filter restated over those tables, and the two writers.  Substitutions only; DESIGN.md section 7 names
 * what is left out (INDEL records, BAQ, the allele pruning of `call -m`); mpileup's bias annotations are written on request
 * (pmx_pileup_bias + pmx_genotype_annotate).
 *
 * pmx_pileup_* replace createMplpBcf (src/conversion.cpp:83-128).  Tables per 0-based reference position:
 *   hist[pos][q 0..63][strand 0 fwd / 1 rev][base A C G T N]  (PMX_PILEUP_HIST uint32 counters per position): the bases
 *     bcf_call_glfgen hands to errmod_cal, q as it caps it (src/3rdparty/bcftools/bam2bcf.c:425-461);
 *   aux[pos][0..3]: raw depth (INFO/DP), sum of the capped mapping qualities of those bases (MQ = sum / bases), bases of
 *     MQ-0 reads, reads covering the position with a deletion.
 * Reads enter as the BAM of the align stage shows them: the filters of mplp_func (bcftools/mpileup.c:196-299: orphans of
 * paired data are skipped), the depth cap of bam_plp_push in BAM order (htslib-1.20/sam.c:6097-6151) and the
 * reconciliation of overlapping mates (sam.c:5824-6003) are applied.  names_concat / name_offsets (n_reads + 1; names as
 * in the FASTQ, a trailing /1 or /2 is dropped) feed the read-name hash that picks the mate an overlap keeps; NULL = the
 * reads are called r0, r1, ... by read index.
 * ------------------------------------------------------------------------------------------ */
#define PMX_PILEUP_HIST 640
#define PMX_PILEUP_AUX 4
typedef struct {
    int32_t max_depth;    /* 250 (mpileup.c:1367); 0 = no cap */
    int32_t min_baseq;    /* 1   (mpileup.c:1363) */
    int32_t max_baseq;    /* 60  (mpileup.c:1364) */
    int32_t delta_baseq;  /* 30  (mpileup.c:1365) */
    int32_t cap_mapq;     /* 60  (bca->capQ, bam2bcf.c:49) */
    int32_t reserved[3];
} pmx_pileup_params;
void pmx_pileup_default_params(pmx_pileup_params *pp);
typedef struct pmx_pileup pmx_pileup;
int pmx_pileup_create(pmx_ctx *ctx, pmx_pileup **out);
void pmx_pileup_free(pmx_ctx *ctx, pmx_pileup *pu);
/* [hot] the pileup of the results the aligner's last pmx_align_readset left on the device, over the same read set
 * (qualities as attached with pmx_readset_set_qualities; without them every base is 'I'); ref_len = the aligner's genome */
int pmx_pileup_run(pmx_ctx *ctx, pmx_pileup *pu, pmx_aligner *al, const pmx_readset *rs, int64_t ref_len, int paired,
                   int revcomp_mate2, const char *names_concat, const int64_t *name_offsets, const pmx_pileup_params *pp);
/* the same from host arrays (records + CIGAR arena as pmx_align_fetch / pmx_dist_fetch_gathered return them, reads and
 * qualities concatenated with n_records + 1 offsets): what rank 0 of a --gpus N run holds for the whole sample */
int pmx_pileup_run_records(pmx_ctx *ctx, pmx_pileup *pu, const pmx_aln_record *records, int64_t n_records,
                           const uint32_t *cigar_arena, int64_t n_words, const char *concat, const char *qual_concat,
                           const int64_t *offsets, int64_t ref_len, int paired, int revcomp_mate2, const char *names_concat,
                           const int64_t *name_offsets, const pmx_pileup_params *pp);
/* hist: ref_len * PMX_PILEUP_HIST, aux: ref_len * PMX_PILEUP_AUX (either may be NULL) */
int pmx_pileup_fetch(pmx_ctx *ctx, pmx_pileup *pu, uint32_t *hist, uint32_t *aux);
/* per read of the last run: bit 0 = in the pileup, bit 1 = its overlap with its mate was reconciled, bit 2 = it is the
 * second mate in BAM order, bit 3 = it keeps the quality of agreeing bases; rank = its place in the BAM (0xffffffff: not
 * written).  Either may be NULL. */
int pmx_pileup_read_info(const pmx_pileup *pu, uint8_t *flags, uint32_t *bam_rank, int64_t cap);
/* algorithmic HBM bytes of the last run's two kernels (inputs read once + tables written once) */
int64_t pmx_pileup_bytes(const pmx_pileup *pu);
/* [hot] the bias pass: for every listed site, the histograms mpileup's rank tests read (bam2bcf.c:488-527) over exactly the
 * bases the last pmx_pileup_run / pmx_pileup_run_records counted in hist.  PMX_PILEUP_BIAS uint32 counters per site:
 *   [PMX_PLB_POS][is_alt][100]  position in the aligned part of the read, scaled to 0..99 (get_position, bam2bcf.c:144-193)
 *   [PMX_PLB_SCL][is_alt][100]  15 * length of the nearest soft clip / (distance to it + 1), at most 99
 *   [PMX_PLB_MQ ][is_alt][60]   mapping quality (255 -> 20, cap_mapq, at most 59)
 *   [PMX_PLB_BQ ][is_alt][60]   base quality after the neighbour rule and max_baseq, at most 59
 *   [PMX_PLB_MQS][strand][60]   mapping quality by strand of the written record (0 forward, 1 reverse)
 * is_alt = 0 when the reference letter is A C G T (either case) and the base equals it, 1 otherwise.  positions: 0-based,
 * strictly ascending, inside [0, ref_len); ref_bases: one letter per site; out: n_sites * PMX_PILEUP_BIAS.  The state of the
 * last run is read on the device: after pmx_pileup_run the aligner's results and the read set must still be those of that
 * run.  n_sites == 0 does nothing; a call before a run, an unsorted list or a position outside the reference is an error
 * and launches nothing. */
#define PMX_PLB_NPOS 100
#define PMX_PLB_NQUAL 60
#define PMX_PLB_POS 0
#define PMX_PLB_SCL 200
#define PMX_PLB_MQ 400
#define PMX_PLB_BQ 520
#define PMX_PLB_MQS 640
#define PMX_PILEUP_BIAS 760
int pmx_pileup_bias(pmx_ctx *ctx, pmx_pileup *pu, const int32_t *positions, const char *ref_bases, int64_t n_sites, uint32_t *out);

/* pmx_genotype_* replace createVcfWithMutationMatrices / createConsensus (src/conversion.cpp:130-255) and
 * genotyping::applyMutationSpectrum / passesConsensusGate (src/genotyping.cpp:167-279).  Host; positions are few. */
/* IndexBuilder::computeSubstitutionSpectrum (src/index_single_mode.cpp:1408-1558): counts[from * 4 + to] of the
 * substitutions on the tree's branches, the number of branches, and the genome length the rates are normalised with: the
 * median of ten leaf genomes, here the leaves evenly spaced in DFS order (the reference walks a hash map) */
int pmx_genotype_spectrum_counts(const pmx_panman *pm, int64_t counts[16], int64_t *n_branches, int64_t *genome_len);
/* the rates for genome length L turned to phred as loadSubstMatrixFromIndex does (src/main.cpp:290-311); returns 1 when
 * the tree shows no substitution at all (the reference then runs without a spectrum), 0 otherwise */
int pmx_genotype_spectrum_phred(const int64_t counts[16], int64_t n_branches, int64_t genome_len, double phred[16]);
/* one site from its hist[pos] (PMX_PILEUP_HIST counters): errmod_cal (htslib-1.20/errmod.c:143-208) + bcf_call_combine
 * (bam2bcf.c:955-1115).  ref_base: the reference letter.  alleles[0..n_alleles): A C G T N = 0..4, reference first, then
 * the alternatives seen by falling quality sum (the unseen allele is not listed); pl[k] = the likelihood of the homozygote
 * of allele k as mpileup scales it (minimum over ALL its genotypes subtracted, not renormalised); ad[k], adf/adr, dp4. */
typedef struct {
    int32_t n_alleles;
    int32_t alleles[5];
    int32_t pl[5];
    int32_t ad[5];
    int32_t dp4[4];
    int32_t n_bases;      /* bases in the model (sum of hist) */
    int32_t reserved[3];
} pmx_site_call;
int pmx_genotype_site(const uint32_t *hist, char ref_base, pmx_site_call *out);
/* the annotations `bcftools mpileup` adds to a record with an alternative, from one site's hist, aux and bias rows:
 * calc_vdb (bam2bcf.c:596-657), calc_mwu_biasZ with do_Z = 1 (:813-864, called as :1152-1160), calc_SegBias for one
 * sample (:891-927) and MQ0F (:1314), each as the float the reference stores.  Bit k of `present` is set when value[k] is
 * written to the record (a HUGE_VAL result is not, :1288-1309); MQ0F always is. */
enum { PMX_TEST_VDB = 0, PMX_TEST_SGB, PMX_TEST_RPBZ, PMX_TEST_MQBZ, PMX_TEST_MQSBZ, PMX_TEST_BQBZ, PMX_TEST_SCBZ, PMX_TEST_MQ0F, PMX_N_TESTS };
typedef struct {
    float value[PMX_N_TESTS];
    uint32_t present;
    uint32_t reserved[3];
} pmx_site_tests;
int pmx_genotype_site_tests(const uint32_t *hist_row, const uint32_t *aux_row, const uint32_t *bias_row, char ref_base, pmx_site_tests *out);
/* the INFO name of test k ("VDB", "SGB", ...; NULL outside 0..PMX_N_TESTS-1), in the order a record lists them */
const char *pmx_genotype_test_name(int k);
/* a float as htslib's kputd prints it into a VCF (kstring.c:38-140): six significant digits, trailing zeros dropped, %g
 * outside [0.0001, 999999].  Returns the length needed (without the NUL). */
int64_t pmx_genotype_format_float(double v, char *out, int64_t cap);
/* applyMutationSpectrum (src/genotyping.cpp:200-279) on one raw VCF line; phred = NULL: the plain branch of
 * createVcfWithMutationMatrices (src/conversion.cpp:163-178).  Writes the line to keep ("" = dropped) and returns its
 * length, or a negative error (a line the reference throws on). */
int64_t pmx_genotype_filter_line(const char *line, const double *phred16, int min_depth, double min_qual, char *out, int64_t cap);
typedef struct pmx_genotyper pmx_genotyper;
/* calls of a whole genome from the pileup tables: every position where an alternative base has a non-zero quality sum
 * becomes a raw line, goes through pmx_genotype_filter_line, and a line that stays is written with REF and the called
 * allele alone.  Returns the number of records, or a negative error. */
int64_t pmx_genotype_call(const uint32_t *hist, const uint32_t *aux, const char *reference, int64_t ref_len, const char *chrom,
                          const double *phred16, int min_depth, double min_qual, pmx_genotyper **out);
int64_t pmx_genotype_num_records(const pmx_genotyper *g);
const char *pmx_genotype_record(const pmx_genotyper *g, int64_t i);   /* the VCF line without its newline */
/* 0-based reference position of record i (-1: no such record) */
int64_t pmx_genotype_record_pos(const pmx_genotyper *g, int64_t i);
/* rewrites the INFO of the records at `positions` (0-based, ascending; bias: n_sites * PMX_PILEUP_BIAS from
 * pmx_pileup_bias at the same positions) as DP;VDB;SGB;RPBZ;MQBZ;MQSBZ;BQBZ;SCBZ;MQ0F;AC;AN;DP4;MQ, absent tests left out.
 * A position without a record is an error.  pmx_genotype_write_vcf then also writes the eight ##INFO lines. */
int pmx_genotype_annotate(pmx_genotyper *g, const int32_t *positions, const uint32_t *bias, int64_t n_sites);
void pmx_genotype_free(pmx_genotyper *g);
/* `<prefix>.vcf`: header (fileformat, contig, the INFO / FORMAT fields written, #CHROM ... sample_name) + the records */
int pmx_genotype_write_vcf(const pmx_genotyper *g, const char *path, const char *chrom, int64_t ref_len, const char *sample_name);
/* `bcftools consensus -f ref.fa vcf` for substitution records + the header rename of createConsensus
 * (src/conversion.cpp:186-255): the first sequence of ref_fa with every record's ALT in place of its REF, `>header`,
 * 60 bases per line */
int pmx_genotype_write_consensus(const char *vcf_path, const char *ref_fa_path, const char *out_path, const char *header);

/* The library's tuning / testing / diagnostic switches are environment variables PMX_<NAME>, all of them listed with their
 * class and meaning in ONE table (csrc/device/pmx_options.hpp).  The environment is read once, at the first use;
 * pmx_options_reload reads it again (a test that changes a switch inside one process), pmx_options_describe writes the
 * table with the current values ("PMX_NAME [class] meaning (= value)" lines) and returns the bytes it needs. */
void pmx_options_reload(void);
int64_t pmx_options_describe(char *buf, int64_t cap);

/* kernel timing: average duration (ms) of the dominant kernel of the last call, measured with HIP
   events on the context stream; name selects a stage ("pack", "seed", "score", "align") or a kernel of the align stage
   ("align_cseeds" = k_compact_seeds*, "align_dom" = the mapping kernel over every pair, "align_cmulti" = the compact
   tier's second form, k_align_compact*_multi) or a span of --meta ("meta_score" = the bit matrices and the score kernel of
   pmx_meta_score; "meta_assign" = the device work of pmx_meta_assign up to the scan of the node counts, "meta_assign_emit" = its
   list kernel, both summed over the call's chunks; with a taxonomy "meta_assign" ends before the taxonomy kernels and
   "meta_assign_taxa" holds them and that scan; with pmx_meta_set_breadth "meta_breadth" = the breadth kernels, summed likewise, and "meta_breadth_count" = the column
   count kernel among them, and with an attached dist "meta_breadth_merge" = the kernels that OR the ranks' hit matrices into the local one, summed over
   the slabs of the exchange (the exchange itself is not in it); "meta_read_best" = the device work of pmx_meta_read_best, summed over its chunks; "meta_mask" = the mask step of pmx_meta_set_reads, and with amplicons "meta_mask_sort" = the sort
   of its (amplicon, hash) keys inside it); < 0: no such span in the last call */
double pmx_last_kernel_ms(pmx_ctx *ctx, const char *name);

#ifdef __cplusplus
}
#endif
#endif
