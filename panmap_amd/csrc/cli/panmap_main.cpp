// `panmap <panman> [reads1] [reads2] [options]` -- the reference's command line (src/main.cpp:1941-2131, 2225-2276) for
// the stages this library implements, written against the C ABI only (include/panmap_amd.h):
//   index   PanMAN -> seed index, cached as `<panman>.idx` (reused when newer than the PanMAN and built with the same
//           seeding parameters, src/main.cpp:371-396; -f rebuilds; -i loads a given file; --index-out names the output)
//   place   reads -> `<prefix>.placement.tsv` (src/placement.cpp:1952-2003)
//   align   placed genome -> `<prefix>.ref.fa` (+ .fai), reads aligned to it -> `<prefix>.bam` (+ .bai)
//   genotype   device pileup of the alignments -> substitution calls -> `<prefix>.vcf` (runGenotyping, src/main.cpp:1828-1875)
//   consensus  the placed genome with the calls applied -> `<prefix>.consensus.fa` (runConsensus, src/main.cpp:1877-1900)
// `--stop index|place|align|genotype|consensus` ends after that stage (default: consensus).  --meta ->
// `<prefix>.mgsr.abundance.out` (with --write-ocranks also `<prefix>.overlapCoefficients.tsv`, with --write-meta-read-scores-unfiltered / -filtered
// `<prefix>.read_scores_info.unfiltered.tsv` / `.filtered.tsv`); --meta --filter-and-assign --align-reads [--min-num-align N] -> `<prefix>_mgsr_aligned/`: one
// BAM (+ .bai) per node with at least N assigned reads, and their genomes in reference.fa.  Refused with an error, never a silent no-op: the bwa backend (-a), --baq, the options of the
// parts of panmap this build leaves out (--impute, ...), BUILDING a homopolymer-compressed index (one
// given with -i or found at <panman>.idx is placed against as it is), --hpc or such an index with --meta.
// --batch FILE runs the samples of a batch file against what stays resident (the index, or with --meta both indexes and the
// pmx_meta); with --gpus N the samples are DEALT to N processes, one per GPU, which exchange nothing: every sample's files are
// what the one-GPU run writes.  Output prefix: -o, else derived from reads1 as the reference derives it.  Exit code 130 on SIGINT.
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cctype>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <thread>
#include <algorithm>
#include <chrono>
#include <fstream>
#include <iomanip>
#include <memory>
#include <new>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "panmap_amd.h"

namespace {

struct Config {
    std::string panman, reads1, reads2, output, index, index_out, stop = "consensus", aligner = "minimap2", batch;
    int threads = 1, k = 19, s = 8, t = 0, l = 3, flank_mask = 250, zstd_level = 7;
    bool open_syncmer = false, hpc = false, force_reindex = false, index_uncompressed = false, quiet = false;
    double seed_mask_fraction = 0.0;
    bool dedup = false, force_leaf = false;
    int trim_start = 0, trim_end = 0, min_seed_quality = 0, min_read_support = -1;
    bool meta = false;     // --meta: haplotype deconvolution (src/main.cpp:1192-1313)
    bool filter_and_assign = false;   // --meta --filter-and-assign: reads to their best-scoring nodes (src/main.cpp:720-1016)
    // the taxonomy filter of --filter-and-assign (src/main.cpp:2068-2083); `taxonomy_options`: the ones given besides the file
    std::string taxonomic_metadata, taxonomic_rank = "Family";
    int maximum_taxon_number = 1, ambiguous_score = 0;
    double ambiguous_ratio = 0.0;
    std::vector<std::string> taxonomy_options;
    bool breadth_ratio = false;       // --breadth-ratio: <prefix>.mgsr.breadths.out (src/main.cpp:957-1015)
    // --align-reads / --min-num-align N: a BAM per assigned node (alignAssignedReads, src/main.cpp:615-717); `align_options`: the
    // ones given, in order
    bool align_reads = false;
    int min_num_align = 10;
    std::vector<std::string> align_options;
    // --mask-reads N / --mask-seeds N: the low-coverage masks of --meta (src/main.cpp:2026-2030, src/mgsr.cpp:2049-2139);
    // `mask_options`: the ones given, in order
    int64_t mask_reads = 0, mask_seeds = 0;
    std::vector<std::string> mask_options;
    // --amplicon-depth FILE (read id <TAB> primer id) and the masks whose threshold is a share of an amplicon's reads
    // (src/main.cpp:2032-2040, src/mgsr.cpp:1216-1342, 2062-2075); they are listed in mask_options too
    std::string amplicon_depth;
    double mask_reads_rf = 0.0, mask_seeds_rf = 0.0;
    // --mask-read-ends N: bases cut from both ends of every read of --meta (src/main.cpp:2065, src/mgsr.cpp:1274-1280); listed
    // in mask_options too
    int64_t mask_read_ends = 0;
    // --em-leaves-only (src/main.cpp:2053), --write-ocranks (:2115) and the two read-score reports, --write-meta-read-scores-
    // unfiltered / -filtered (src/main.cpp:1225-1227, 1308-1310), switches of the abundance mode; `em_options`: the ones given, in order
    bool em_leaves_only = false, write_ocranks = false, read_scores_unfiltered = false, read_scores_filtered = false;
    std::vector<std::string> em_options;
    int64_t top_oc = 1000;
    double em_convergence = 0.00001, em_delta = 0.0, discard = 0.0, dust = 100.0;
    int em_max_iterations = 1000, em_max_rounds = 5;
    int gpus = 1;          // --gpus N: one process per GPU, reads sharded, RCCL exchange (pmx_dist_*)
    bool refine = false;   // src/main.cpp:186-190, 2002-2011
    double refine_top_pct = 0.01;
    int refine_max_top_n = 150, refine_neighbor_radius = 2, refine_max_neighbor_n = 150;
    int min_depth = 1;       // --min-depth / --min-qual: the consensus gate (src/genotyping.cpp:167-174, 272)
    double min_qual = 30.0;
    bool annotate_vcf = false;   // --annotate-vcf: mpileup's bias annotations in the INFO of the written records
};

void on_sigint(int) { _exit(130); }

struct Fatal { std::string msg; int code; };
[[noreturn]] void die(const std::string& msg, int code = 1) { throw Fatal{msg, code}; }   // main (or the --batch loop) reports it
void check(int rc, const char* what) {
    if (rc != PMX_OK) die(std::string(what) + ": " + pmx_last_error());
}
void say(const Config& c, const char* stage, const std::string& what) {
    if (!c.quiet) fprintf(stderr, "[%s] %s\n", stage, what.c_str());
}
bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
time_t mtime(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 ? st.st_mtime : 0; }

void usage() {
    fputs("Usage: panmap <panman> [reads1.fq[.gz]] [reads2.fq[.gz]] [options]\n"
          "  -o, --output PREFIX        output prefix (default: derived from reads1)\n"
          "  -t, --threads N            accepted (the GPU owns the parallelism)\n"
          "      --stop STAGE           index|place|align|genotype|consensus (default consensus)\n"
          "      --min-depth N          high-quality bases a call needs (default 1)     --min-qual F   lowest QUAL kept (default 30)\n"
          "      --annotate-vcf         add VDB, SGB, RPBZ, MQBZ, MQSBZ, BQBZ, SCBZ and MQ0F to the INFO of the VCF records\n"
          "      --batch FILE           one sample per line: reads1 [reads2] [prefix]; the index stays resident (with --meta: both\n"
          "                             indexes and the device state; not with --amplicon-depth).  With --gpus N (at most 16) the samples\n"
          "                             are dealt to N processes, one per GPU, each sample whole on one GPU: the files of the one-GPU run\n"
          "      --meta                 estimate haplotype abundances of a mixed sample -> <prefix>.mgsr.abundance.out\n"
          "      --meta --filter-and-assign   assign every read to the nodes it scores best on -> <prefix>.mgsr.assignedReads.fastq,\n"
          "                             .mgsr.assignedReads.out, .mgsr.assignedReadsLCANode.out (--discard F, --dust F; also with --gpus N:\n"
          "                             every rank assigns its share of the distinct reads, rank 0 gathers and writes the one-GPU files)\n"
          "      --breadth-ratio        ... and write <prefix>.mgsr.breadths.out: per node the distinct seeds of its genome, how many of them\n"
          "                             the reads assigned to it hit, their depth, and the observed / expected breadth ratios (a switch)\n"
          "      --align-reads          ... and align the reads of every node that has at least --min-num-align N (default 10) of them to that\n"
          "                             node's genome -> <prefix>_mgsr_aligned/<node>.bam (+ .bai) and reference.fa (minimap2 presets)\n"
          "      --taxonomic-metadata TSV     ... and drop the reads whose best-scoring nodes span more than N taxa: node id in the first\n"
          "                             column, the taxa of --taxonomic-rank NAME (default Family) in the column of that name\n"
          "      --maximum-taxon-number N (default 1, at most 16)   --ambiguous-score-threshold N / --ambiguous-score-threshold-ratio F:\n"
          "                             count the nodes within max(N, int(best * F)) of a read's best score too (not with --discard > 0)\n"
          "      --mask-reads N         --meta: drop every read that carries a k-min-mer seen at most N times in the whole sample (counted\n"
          "                             over the distinct reads, each with its number of copies)      --mask-seeds N   remove those\n"
          "                             k-min-mers from the reads instead (one of the two; also with --gpus N; not with --filter-and-assign)\n"
          "      --amplicon-depth TSV   --meta: `read id <TAB> primer id` per line; reads are collapsed and the masks count within the reads\n"
          "                             of a primer (amplicon), the reads that are not listed forming one more group\n"
          "      --mask-reads-relative-frequency F / --mask-seeds-relative-frequency F   as --mask-reads / --mask-seeds with the threshold\n"
          "                             int(F x the reads of the amplicon); needs --amplicon-depth; unlisted reads stay unmasked (one of the four)\n"
          "      --mask-read-ends N     --meta: cut N bases from both ends of every read before anything else looks at it (a read of 2N\n"
          "                             bases or fewer stays in the sample, empty; also with --gpus N and --batch; not with --filter-and-assign)\n"
          "      --em-leaves-only       --meta: take the EM's candidates among the sampled genomes only (ids that do not begin with node_, and\n"
          "                             nodes identical to one); the --top-oc ranks are counted among those (a switch)\n"
          "      --write-ocranks        --meta: write <prefix>.overlapCoefficients.tsv, every node's id, overlap coefficient and rank (a switch)\n"
          "      --write-meta-read-scores-unfiltered / --write-meta-read-scores-filtered   --meta: write <prefix>.read_scores_info.unfiltered.tsv /\n"
          "                             .filtered.tsv, one line per distinct read that maps: its copies, seedmers, best score over ALL nodes, the\n"
          "                             number of nodes that reach it, and the input positions of its copies; the filtered file lacks the reads\n"
          "                             below --discard (switches; also with --gpus N, with or without --batch)\n"
          "      --top-oc N --em-convergence-threshold F --em-delta-threshold F --em-maximum-iterations N --em-maximum-rounds N --discard F --dust F\n"
          "      --gpus N               N processes, one per GPU: reads sharded, seed index replicated, RCCL exchange (with --batch:\n"
          "                             whole samples dealt instead, nothing exchanged).  With --meta, --filter-and-assign included, one sample is\n"
          "                             sharded over the N ranks and rank 0 writes the files of the one-GPU run\n"
          "      --refine               re-rank the top candidates by aligning the reads against them\n"
          "      --refine-top-pct F / --refine-max-top-n N / --refine-neighbor-radius N / --refine-max-neighbor-n N\n"
          "  -i, --index PATH           load a pre-built index       --index-out PATH   write the built index here\n"
          "  -f, --reindex              force rebuild                --zstd-level N     (default 7)   --index-uncompressed\n"
          "  -k N  -s N  -l N  --offset N  --open-syncmer  --flank-mask N  --seed-mask-fraction F\n"
          "      --hpc                  the index must be homopolymer-compressed (one given with -i or found at <panman>.idx is used as\n"
          "                             it is, with or without this flag; this command line does not build one; not with --meta)\n"
          "      --dedup --trim-start N --trim-end N --min-seed-quality N --min-read-support N --force-leaf\n"
          "  -a, --aligner minimap2     -q, --quiet   -h, --help   -V, --version\n", stderr);
}

Config parse(int argc, char** argv) {
    Config c;
    std::vector<std::string> pos;
    auto need = [&](int& i) -> const char* { if (i + 1 >= argc) die(std::string("option ") + argv[i] + " needs a value"); return argv[++i]; };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        std::string val;
        const size_t eq = a.rfind("--", 0) == 0 ? a.find('=') : std::string::npos;   // --opt=value
        bool has_val = false;
        if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_val = true; }
        auto v = [&]() -> std::string { return has_val ? val : std::string(need(i)); };
        if (a == "-h" || a == "--help" || a == "--help-all") { usage(); exit(0); }
        else if (a == "-V" || a == "--version") { puts(pmx_version()); exit(0); }
        else if (a == "-o" || a == "--output") c.output = v();
        else if (a == "-t" || a == "--threads") c.threads = atoi(v().c_str());
        else if (a == "--stop") c.stop = v();
        else if (a == "-i" || a == "--index") c.index = v();
        else if (a == "--index-out") c.index_out = v();
        else if (a == "-f" || a == "--reindex") c.force_reindex = true;
        else if (a == "-k" || a == "--kmer") c.k = atoi(v().c_str());
        else if (a == "-s" || a == "--syncmer") c.s = atoi(v().c_str());
        else if (a == "--offset") c.t = atoi(v().c_str());
        else if (a == "-l" || a == "--lmer") c.l = atoi(v().c_str());
        else if (a == "--open-syncmer") c.open_syncmer = true;
        else if (a == "--hpc") c.hpc = true;
        else if (a == "--flank-mask") c.flank_mask = atoi(v().c_str());
        else if (a == "--seed-mask-fraction") c.seed_mask_fraction = atof(v().c_str());
        else if (a == "--zstd-level") c.zstd_level = atoi(v().c_str());
        else if (a == "--index-uncompressed") c.index_uncompressed = true;
        else if (a == "-a" || a == "--aligner") c.aligner = v();
        else if (a == "--dedup") c.dedup = true;
        else if (a == "--trim-start") c.trim_start = atoi(v().c_str());
        else if (a == "--trim-end") c.trim_end = atoi(v().c_str());
        else if (a == "--min-seed-quality") c.min_seed_quality = atoi(v().c_str());
        else if (a == "--min-read-support") c.min_read_support = atoi(v().c_str());
        else if (a == "--force-leaf") c.force_leaf = true;
        else if (a == "-q" || a == "--quiet") c.quiet = true;
        else if (a == "-v" || a == "--verbose" || a == "--no-color" || a == "--no-progress") {}
        else if (a == "--batch") c.batch = v();
        else if (a == "--gpus") c.gpus = atoi(v().c_str());
        else if (a == "--refine") c.refine = true;
        else if (a == "--refine-top-pct") c.refine_top_pct = atof(v().c_str());
        else if (a == "--refine-max-top-n") c.refine_max_top_n = atoi(v().c_str());
        else if (a == "--refine-neighbor-radius") c.refine_neighbor_radius = atoi(v().c_str());
        else if (a == "--refine-max-neighbor-n") c.refine_max_neighbor_n = atoi(v().c_str());
        else if (a == "--meta") c.meta = true;
        else if (a == "--filter-and-assign") c.filter_and_assign = true;
        else if (a == "--taxonomic-metadata") c.taxonomic_metadata = v();
        else if (a == "--taxonomic-rank") { c.taxonomic_rank = v(); c.taxonomy_options.push_back(a); }
        else if (a == "--maximum-taxon-number") { c.maximum_taxon_number = atoi(v().c_str()); c.taxonomy_options.push_back(a); }
        else if (a == "--ambiguous-score-threshold") { c.ambiguous_score = atoi(v().c_str()); c.taxonomy_options.push_back(a); }
        else if (a == "--ambiguous-score-threshold-ratio") { c.ambiguous_ratio = atof(v().c_str()); c.taxonomy_options.push_back(a); }
        else if (a == "--breadth-ratio") {   // po::bool_switch in the reference: a number after it would silently become a reads file
            const std::string next = has_val ? val : i + 1 < argc ? std::string(argv[i + 1]) : std::string();
            char* end = nullptr;
            if (!next.empty()) (void)strtod(next.c_str(), &end);
            if (has_val || (end && *end == '\0'))
                die("option --breadth-ratio is not accepted with a value (" + next + "): it is a switch, as in the reference");
            c.breadth_ratio = true;
        }
        else if (a == "--align-reads") { c.align_reads = true; c.align_options.push_back(a); }
        else if (a == "--min-num-align") { c.min_num_align = atoi(v().c_str()); c.align_options.push_back(a); }
        else if (a == "--mask-reads") { c.mask_reads = atoll(v().c_str()); c.mask_options.push_back(a); }
        else if (a == "--mask-seeds") { c.mask_seeds = atoll(v().c_str()); c.mask_options.push_back(a); }
        else if (a == "--amplicon-depth") { c.amplicon_depth = v(); c.mask_options.push_back(a); }
        else if (a == "--mask-reads-relative-frequency") { c.mask_reads_rf = atof(v().c_str()); c.mask_options.push_back(a); }
        else if (a == "--mask-seeds-relative-frequency") { c.mask_seeds_rf = atof(v().c_str()); c.mask_options.push_back(a); }
        else if (a == "--mask-read-ends") {
            const std::string n = v();
            char* end = nullptr;
            errno = 0;
            c.mask_read_ends = strtoll(n.c_str(), &end, 10);
            if (n.empty() || *end != '\0' || errno != 0 || c.mask_read_ends < 0 || c.mask_read_ends > INT32_MAX)
                die("option --mask-read-ends is not accepted with the value '" + n + "': it takes a number of bases, 0 or more");
            c.mask_options.push_back(a);
        }
        else if (a == "--em-leaves-only") { c.em_leaves_only = true; c.em_options.push_back(a); }
        else if (a == "--write-ocranks") { c.write_ocranks = true; c.em_options.push_back(a); }
        else if (a == "--write-meta-read-scores-unfiltered") { c.read_scores_unfiltered = true; c.em_options.push_back(a); }
        else if (a == "--write-meta-read-scores-filtered") { c.read_scores_filtered = true; c.em_options.push_back(a); }
        else if (a == "--jplace") die("option " + a + " is not accepted: this build writes no jplace output");
        else if (a == "--top-oc") c.top_oc = atoll(v().c_str());
        else if (a == "--em-convergence-threshold") c.em_convergence = atof(v().c_str());
        else if (a == "--em-delta-threshold") c.em_delta = atof(v().c_str());
        else if (a == "--em-maximum-iterations") c.em_max_iterations = atoi(v().c_str());
        else if (a == "--em-maximum-rounds") c.em_max_rounds = atoi(v().c_str());
        else if (a == "--discard") c.discard = atof(v().c_str());
        else if (a == "--dust") c.dust = atof(v().c_str());
        else if (a == "--min-depth") c.min_depth = atoi(v().c_str());
        else if (a == "--min-qual") c.min_qual = atof(v().c_str());
        else if (a == "--annotate-vcf") c.annotate_vcf = true;
        else if (a == "--baq") die("--baq (base alignment quality) is not implemented in this build; the pileup runs as `mpileup -B` does");
        else if (a == "--impute" || a == "--extent-guard" || a == "--reference-node" ||
                 a == "--dump-sequence" || a == "--dump-all-scores")
            die("option " + a + " belongs to a part of panmap this build does not implement (index / place / align / genotype / consensus only)");
        else if (a.size() > 1 && a[0] == '-') die("unknown option " + a + " (see --help)");
        else pos.push_back(a);
    }
    if (pos.empty()) { usage(); exit(1); }
    c.panman = pos[0];
    if (pos.size() > 1) c.reads1 = pos[1];
    if (pos.size() > 2) c.reads2 = pos[2];
    if (pos.size() > 3) die("at most two read files");
    return c;
}

// src/main.cpp:2253-2276
std::string derive_prefix(const Config& c) {
    if (c.reads1.empty()) return c.panman;
    std::string stem = c.reads1;
    const size_t slash = stem.find_last_of('/');
    if (slash != std::string::npos) stem = stem.substr(slash + 1);
    const size_t dot = stem.find_last_of('.');
    if (dot != std::string::npos && dot > 0) stem = stem.substr(0, dot);            // fs::path::stem()
    auto strip = [&](std::initializer_list<const char*> sfx) {
        for (const char* s : sfx) {
            const size_t n = strlen(s);
            if (stem.size() > n && stem.compare(stem.size() - n, n, s) == 0) { stem.erase(stem.size() - n); return; }
        }
    };
    strip({"_R1", "_R2", "_1", "_2", ".R1", ".R2", ".1", ".2"});
    strip({".fastq", ".fq"});
    return stem;
}

// readBatchFiles (src/main.cpp:1025-1087): one sample per line, `reads1 [reads2] [prefix]`; '#' starts a comment line; a
// single optional field is reads2 when it looks like a FASTQ, else the output prefix; default prefix = reads1 without its
// directory-independent mate suffix and .fastq / .fq
struct BatchEntry { std::string reads1, reads2, prefix; };
std::vector<BatchEntry> read_batch_file(const std::string& path) {
    std::ifstream in(path);
    if (!in.is_open()) die("Cannot open batch file: " + path);
    std::vector<BatchEntry> out;
    std::string line;
    size_t line_no = 0;
    while (std::getline(in, line)) {
        ++line_no;
        const size_t b = line.find_first_not_of(" \t\r\n"), e2 = line.find_last_not_of(" \t\r\n");
        if (b == std::string::npos) continue;
        line = line.substr(b, e2 - b + 1);
        if (line[0] == '#') continue;
        std::istringstream iss(line);
        BatchEntry e;
        std::string f2, f3;
        iss >> e.reads1 >> f2 >> f3;
        if (e.reads1.empty()) continue;
        if (!f2.empty()) {
            if (!f3.empty()) { e.reads2 = f2; e.prefix = f3; }
            else {
                std::string lower = f2;
                for (char& ch : lower) ch = (char)tolower((unsigned char)ch);
                if (lower.find(".fastq") != std::string::npos || lower.find(".fq") != std::string::npos) e.reads2 = f2;
                else e.prefix = f2;
            }
        }
        if (e.prefix.empty()) {
            const size_t slash = e.reads1.find_last_of('/');
            const std::string dir = slash == std::string::npos ? "" : e.reads1.substr(0, slash);
            std::string stem = slash == std::string::npos ? e.reads1 : e.reads1.substr(slash + 1);
            const size_t dot = stem.find_last_of('.');
            if (dot != std::string::npos && dot > 0) stem = stem.substr(0, dot);
            auto strip = [&](std::initializer_list<const char*> sfx) {
                for (const char* sx : sfx) {
                    const size_t n = strlen(sx);
                    if (stem.size() > n && stem.compare(stem.size() - n, n, sx) == 0) { stem.erase(stem.size() - n); return; }
                }
            };
            strip({"_R1", "_R2", "_1", "_2", ".R1", ".R2"});
            strip({".fastq", ".fq"});
            e.prefix = dir.empty() ? stem : dir + "/" + stem;
        }
        if (!exists(e.reads1)) die("Batch line " + std::to_string(line_no) + ": reads file not found: " + e.reads1);
        if (!e.reads2.empty() && !exists(e.reads2)) die("Batch line " + std::to_string(line_no) + ": reads file not found: " + e.reads2);
        out.push_back(e);
    }
    return out;
}
std::vector<BatchEntry> read_samples(const std::string& path) {   // ... of which there must be one
    std::vector<BatchEntry> samples = read_batch_file(path);
    if (samples.empty()) die("No samples found in batch file");
    return samples;
}
void mkdirs(const std::string& dir) {   // fs::create_directories
    std::string cur;
    for (size_t i = 0; i <= dir.size(); ++i) {
        if (i == dir.size() || dir[i] == '/') {
            if (!cur.empty() && !exists(cur)) mkdir(cur.c_str(), 0777);
        }
        if (i < dir.size()) cur += dir[i];
    }
}

// cachedIndexUsable (src/main.cpp:371-396).  The index is authoritative about HPC, as in the reference (the place stage takes
// `hpc` from the index, src/placement.cpp:1095-1101): an index whose header says hpc = 1 is usable when the other parameters
// match, with or without --hpc on the command line -- it is never rebuilt over.  *is_hpc: what the header says.
bool cached_index_usable(const Config& c, bool* is_hpc) {
    if (exists(c.panman) && mtime(c.index) < mtime(c.panman)) {
        fprintf(stderr, "panmap: cached index %s is older than %s; rebuilding.\n", c.index.c_str(), c.panman.c_str());
        return false;
    }
    pmx_index_info h;
    int unc = 0;
    if (pmx_index_read_header(c.index.c_str(), &h, &unc) != PMX_OK) {
        fprintf(stderr, "panmap: cached index %s has no readable param header (old format/corrupt); rebuilding.\n", c.index.c_str());
        return false;
    }
    if (h.k != c.k || h.s != c.s || h.t != c.t || h.l != c.l || (h.open_syncmer != 0) != c.open_syncmer) {
        fprintf(stderr, "panmap: cached index %s was built with different seeding parameters (k/s/t/l/open-syncmer); rebuilding.\n", c.index.c_str());
        return false;
    }
    *is_hpc = h.hpc != 0;
    return true;
}

// --hpc means "the index must be an HPC index"; this command line does not build one (that producer is not pinned to the
// reference's: DESIGN.md section 7)
const char* const kHpcNeedsIndex =
    "--hpc needs a homopolymer-compressed index, and this command line does not build one.  Make it with the reference's "
    "`panmap <panman> --hpc --stop index`, or with pmx_index_build_ex(..., mode | PMX_INDEX_HPC, ...) / Index.build(hpc=True) + "
    "save, and name it with -i (or leave it at <panman>.idx)";

char comp(char b) {   // seeding::reverseComplement (src/seeding.cpp:271-284): A/C/G/T only, everything else kept
    switch (b) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return b; }
}

// What lives as long as the process's GPU work: the tree, its index(es), the device and what is resident on it.  Filled in by
// real_main / run_meta as they go.  close() is an explicit call and NOT a destructor: a rank that dies between two collectives
// must leave the process (Fatal reaches main) without a barrier and with the communicator as it is -- a barrier or a transport
// released while unwinding would block that rank for ever, and fork_ranks' first-failure reaping waits for it to exit.
struct Run {
    std::string panman_path;
    pmx_panman* pm = nullptr;                    // opened by panman(), whoever asks first
    pmx_index *idx = nullptr, *oidx = nullptr;   // (oidx, meta: --meta only)
    pmx_ctx* ctx = nullptr;
    int dev = 0;
    pmx_dist* dist = nullptr;                    // --gpus N: this process is one rank
    pmx_place* pl = nullptr;
    pmx_meta* meta = nullptr;
    bool have_spectrum = false, spectrum_empty = false;
    double phred[16];

    // the PanMAN, opened on first use; nullptr when it does not open (pmx_last_error() says why): what that means is the caller's
    pmx_panman* panman() {
        if (!pm && pmx_panman_open(panman_path.c_str(), &pm) != PMX_OK) pm = nullptr;
        return pm;
    }
    // the substitution spectrum of the tree as phred, counted once from the open PanMAN (the reference keeps it in the
    // index); nullptr when the tree shows no substitution
    const double* spectrum() {
        if (!have_spectrum) {
            int64_t counts[16], n_branches = 0, genome_len = 0;
            check(pmx_genotype_spectrum_counts(pm, counts, &n_branches, &genome_len), "counting the substitution spectrum");
            const int rc = pmx_genotype_spectrum_phred(counts, n_branches, genome_len, phred);
            if (rc < 0) die("substitution spectrum");
            spectrum_empty = rc == 1;
            have_spectrum = true;
        }
        return spectrum_empty ? nullptr : phred;
    }
    // the one teardown list, for the normal ends only (in the parent of the ranks only the host objects exist)
    void close() {
        if (meta) pmx_meta_free(ctx, meta);
        if (dist) { (void)pmx_dist_barrier(dist); pmx_dist_free(dist); }
        if (pl) pmx_place_free(ctx, pl);
        if (ctx) pmx_ctx_destroy(ctx);
        if (idx) pmx_index_close(idx);
        if (oidx) pmx_index_close(oidx);
        if (pm) pmx_panman_close(pm);
    }
};

// One sample's reads on the host, in one list: R1, R2 interleaved as the place stage takes them (extractReadSequences: R2 in
// FASTQ orientation, NOT reverse-complemented), or R2 appended behind R1 as --meta takes them (the score of a read does not
// depend on its place in the list).  off[r] .. off[r + 1] is read r in `concat` and in `quals` (FASTA: zero bytes).
struct Reads {
    enum Layout { INTERLEAVED, APPENDED };
    struct File { pmx_fastx* h = nullptr; ~File() { if (h) pmx_fastx_free(h); } } file1, file2;   // (the views below point into them)
    std::string concat, quals;
    std::vector<int64_t> off;
    const char *nm1 = nullptr, *nm2 = nullptr;   // the name views of the two files
    const int64_t *no1 = nullptr, *no2 = nullptr;
    bool paired = false;
    int64_t n_reads = 0, unit = 1;               // unit: reads that stay together in a shard
    int64_t n_first = 0;                         // reads of the first file

    Reads(const std::string& reads1, const std::string& reads2, Layout layout) {
        pmx_fastx *&f1 = file1.h, *&f2 = file2.h;
        check(pmx_fastx_read(reads1.c_str(), &f1), "reading reads1");
        paired = !reads2.empty();
        if (paired) check(pmx_fastx_read(reads2.c_str(), &f2), "reading reads2");
        const int64_t n1 = pmx_fastx_num_reads(f1), n2 = paired ? pmx_fastx_num_reads(f2) : 0;
        if (paired && layout == INTERLEAVED && n1 != n2) die("File " + reads2 + " does not contain the same number of reads as " + reads1);   // src/placement.cpp:189-192
        const char *s1, *q1, *s2 = nullptr, *q2 = nullptr;
        const int64_t *o1, *o2 = nullptr;
        check(pmx_fastx_views(f1, &s1, &q1, &o1, &nm1, &no1), "reads1 views");
        if (paired) check(pmx_fastx_views(f2, &s2, &q2, &o2, &nm2, &no2), "reads2 views");
        n_reads = n1 + n2;
        n_first = n1;
        unit = paired && layout == INTERLEAVED ? 2 : 1;
        off.reserve((size_t)n_reads + 1);
        concat.reserve((size_t)(o1[n1] + (paired ? o2[n2] : 0)));
        quals.reserve(concat.capacity());
        auto put = [&](const char* s, const char* q, const int64_t* o, int64_t i) {
            off.push_back((int64_t)concat.size());
            concat.append(s + o[i], (size_t)(o[i + 1] - o[i]));
            quals.append(q + o[i], (size_t)(o[i + 1] - o[i]));
        };
        for (int64_t i = 0; i < n1; ++i) {
            put(s1, q1, o1, i);
            if (unit == 2) put(s2, q2, o2, i);
        }
        if (paired && unit == 1) for (int64_t i = 0; i < n2; ++i) put(s2, q2, o2, i);
        off.push_back((int64_t)concat.size());
    }
    int mean_len() const { return (int)(concat.size() / (size_t)std::max<int64_t>(n_reads, 1)); }
    // the shard of `rank`: reads [*lo, *hi), contiguous, mates together
    void shard(int rank, int world, int64_t* lo, int64_t* hi) const {
        const int64_t n_units = n_reads / unit;
        *lo = n_units * rank / world * unit;
        *hi = rank == world - 1 ? n_reads : n_units * (rank + 1) / world * unit;
    }
    std::string name(int64_t r) const {          // (either layout: mates alternate, or the second file follows the first)
        const bool second = unit == 2 ? (r & 1) != 0 : r >= n_first;
        const int64_t i = unit == 2 ? r / 2 : second ? r - n_first : r;
        std::string nm = second ? std::string(nm2 + no2[i], (size_t)(no2[i + 1] - no2[i])) : std::string(nm1 + no1[i], (size_t)(no1[i + 1] - no1[i]));
        while (!nm.empty() && nm.back() == '\0') nm.pop_back();
        return nm;
    }
};

// One sample through place (+ --refine) (+ align, genotype, consensus) against the resident index: c.reads1 / c.reads2 /
// c.output name it.  A call-lifetime struct, one function per step in the order run_sample calls them; it owns the sample's
// device objects and frees them however the sample ends.  With run.dist (--gpus N) this process is one rank: it seeds and
// aligns ITS contiguous, pair-aligned shard of the reads; the histograms are merged over the ranks before the (replicated)
// scoring, candidate scores of --refine are summed, and the records + CIGAR arenas are gathered to rank 0, which writes
// every output file.
struct Sample {
    const Config& c;
    Run& run;
    const Reads& reads;
    pmx_ctx* const ctx;
    pmx_dist* const dist;
    const int rank, world;
    const bool writer, paired;
    const int64_t n_reads;
    const int mean_len;
    const std::string tsv_path, fa_path, bam_path, vcf_path, cons_path;   // each output's name, built here only
    int64_t lo = 0, hi = 0;                      // this rank's shard
    pmx_index_info info;
    // the device objects
    pmx_readset *rs = nullptr, *rs_hpc = nullptr;
    pmx_aligner *al = nullptr, *refine_al = nullptr;   // refine_al: the first refine worker's, which works on `ctx`
    pmx_pileup* pu = nullptr;
    pmx_genotyper* gt = nullptr;
    // what the steps leave for the later ones
    pmx_place_result res;
    pmx_refine_result refined;
    std::string node_id, genome;
    std::vector<pmx_aln_record> recs;            // the whole sample's records and their CIGAR arena (writer)
    std::vector<uint32_t> arena;
    std::vector<std::string> names;

    Sample(const Config& c_, Run& run_, const Reads& reads_)
        : c(c_), run(run_), reads(reads_), ctx(run_.ctx), dist(run_.dist), rank(dist ? pmx_dist_rank(dist) : 0), world(dist ? pmx_dist_world(dist) : 1),
          writer(rank == 0), paired(reads_.paired), n_reads(reads_.n_reads), mean_len(reads_.mean_len()), tsv_path(c_.output + ".placement.tsv"),
          fa_path(c_.output + ".ref.fa"), bam_path(c_.output + ".bam"), vcf_path(c_.output + ".vcf"), cons_path(c_.output + ".consensus.fa") {
        reads.shard(rank, world, &lo, &hi);
        memset(&refined, 0, sizeof(refined));
        check(pmx_index_get_info(run.idx, &info), "index info");
    }
    ~Sample() {
        if (gt) pmx_genotype_free(gt);
        if (pu) pmx_pileup_free(ctx, pu);
        free_refine_aligner();
        if (al) pmx_aligner_free(ctx, al);
        if (rs_hpc) pmx_readset_free(ctx, rs_hpc);
        if (rs) pmx_readset_free(ctx, rs);
    }
    void free_refine_aligner() { if (refine_al) pmx_aligner_free(ctx, refine_al); refine_al = nullptr; }

    // Reads: the shard [lo, hi) of the host reads, the resident placer.  Leaves: `rs` (the shard, packed, on the device; it
    // goes on to --refine, align and the pileup), the placer's node scores (of the whole sample, on every rank) and `res`.
    void place() {
        check(pmx_readset_upload(ctx, reads.concat.data(), reads.off.data() + lo, hi - lo, &rs), "uploading the reads");
        check(pmx_readset_pack(ctx, rs), "packing the reads");
        pmx_place_params pp;
        memset(&pp, 0, sizeof(pp));
        pp.seed_mask_fraction = c.seed_mask_fraction; pp.min_read_support = c.min_read_support; pp.trim_start = c.trim_start; pp.trim_end = c.trim_end;
        pp.dedup_reads = c.dedup; pp.force_leaf = c.force_leaf; pp.min_seed_quality = c.min_seed_quality;
        if (c.min_seed_quality > 0) check(pmx_readset_set_qualities(ctx, rs, reads.quals.data() + reads.off[(size_t)lo]), "attaching the qualities");
        check(pmx_place_reset(ctx, run.pl), "place reset");
        // An HPC index: the placer compresses the reads by itself (the raw reads go on to the align, genotype and consensus stages).
        // Only the dedup over the ranks needs the compressed set in hand: its calls hash the read bytes and are matched to the
        // seeding call by the read set, so the shard is compressed here and that set is given to both.
        pmx_readset* seed_rs = rs;
        const bool dedup_over_ranks = dist && c.dedup && c.min_seed_quality <= 0;
        if (info.hpc && dedup_over_ranks) {
            check(pmx_readset_hpc_compress(ctx, rs, &rs_hpc), "compressing the reads");
            check(pmx_readset_pack(ctx, rs_hpc), "packing the compressed reads");
            seed_rs = rs_hpc;
        }
        if (dedup_over_ranks) check(pmx_dist_dedup_reads(dist, run.pl, seed_rs, nullptr), "collapsing duplicate reads over the ranks");
        check(pmx_place_add_reads(ctx, run.pl, seed_rs, &pp), "seeding the reads");
        if (dist) check(pmx_dist_merge_histograms(dist, run.pl), "merging the ranks' seed histograms");
        check(pmx_place_score(ctx, run.pl, &pp, n_reads, &res), "scoring the tree");
    }

    // one --refine candidate: its genome indexed on `wctx` in `al` (created on the first call, re-referenced after), the shard's
    // reads aligned against it, their score sum -> *score
    int score_candidate(pmx_ctx* wctx, pmx_aligner*& al_w, uint32_t node, int64_t* score) {
        // one reconstruction per candidate: the worker's buffer keeps the size of the previous genome (genomes of one
        // tree differ by a few bases) and grows only when the returned length says so
        thread_local std::string cand;
        if (cand.size() < 1024) cand.resize(1024);
        int64_t len = pmx_panman_node_genome(run.pm, (int64_t)node, &cand[0], (int64_t)cand.size());
        if (len > (int64_t)cand.size()) {
            cand.resize((size_t)len + (size_t)len / 64);
            len = pmx_panman_node_genome(run.pm, (int64_t)node, &cand[0], (int64_t)cand.size());
        }
        if (len <= 0) { *score = 0; return PMX_OK; }   // (scoreNodeByAlignment returns 0 for an empty genome, src/placement.cpp:496-499)
        const int rc = al_w ? pmx_aligner_set_reference(wctx, al_w, cand.data(), len, mean_len) : pmx_aligner_create(wctx, cand.data(), len, mean_len, &al_w);
        if (rc != PMX_OK) return rc;
        return pmx_align_score_reads(wctx, al_w, rs, paired ? 1 : 0, 0, score);
    }

    // --refine (refineTopCandidates, src/placement.cpp:516-698, called at :1910-1914): every candidate's genome is indexed on the
    // device and the reads -- as extractReadSequences leaves them, mate 2 as sequenced -- are aligned against it.
    // Reads: the placer's node scores, `res`, `rs`, the PanMAN.  Leaves: `refined` (ran = 0 when there was nothing to refine or
    // the PanMAN does not open, which switches the refinement off); no aligner.
    void refine() {
        if (!run.panman()) {
            fprintf(stderr, "panmap: warning: Failed to load full tree for refinement, disabling refinement\n");
            return;
        }
        std::vector<double> scores5((size_t)info.n_nodes * 5);
        check(pmx_place_node_outputs(ctx, run.pl, scores5.data(), nullptr, nullptr), "node scores");
        pmx_refine_params rp;
        memset(&rp, 0, sizeof(rp));
        rp.top_pct = c.refine_top_pct; rp.max_top_n = c.refine_max_top_n; rp.neighbor_radius = c.refine_neighbor_radius; rp.max_neighbor_n = c.refine_max_neighbor_n;
        std::vector<uint32_t> cands((size_t)info.n_nodes);
        const int64_t n_cand = pmx_refine_candidates(pmx_index_parents(run.idx), info.n_nodes, scores5.data(), res.best_index, &rp, cands.data(), (int64_t)cands.size());
        if (n_cand < 0) die(std::string("refining the placement: ") + pmx_last_error());
        cands.resize((size_t)n_cand);
        // The candidates are independent: a few aligners, each with its own context (stream) and host thread, score them
        // concurrently -- one sample's reads do not fill the GPU.  The first one runs alone (it also computes the read set's
        // locality order, which the others then share read-only).
        std::vector<int64_t> cand_score((size_t)n_cand, 0);
        if (n_cand > 0) {
            check(score_candidate(ctx, refine_al, cands[0], &cand_score[0]), "refining the placement");
            check(pmx_ctx_synchronize(ctx), "refining the placement");
            int n_workers = 4;
            if (const char* e = getenv("PMX_REFINE_STREAMS")) n_workers = std::max(1, atoi(e));
            n_workers = (int)std::min<int64_t>(n_workers, std::max<int64_t>(n_cand - 1, 1));
            std::atomic<int64_t> next{1};
            std::atomic<int> failed{0};
            std::string fail_msg;
            std::mutex fail_mu;
            std::vector<std::thread> pool;
            for (int wk = 0; wk < n_workers; ++wk)
                pool.emplace_back([&, wk]() {    // worker 0 goes on with `ctx` and refine_al; the others release what they made, on every path
                    pmx_ctx* wctx = ctx;
                    pmx_aligner* own = nullptr;
                    if (wk > 0 && pmx_ctx_create(run.dev, &wctx) != PMX_OK) { failed = 1; return; }
                    pmx_aligner*& al_w = wk == 0 ? refine_al : own;
                    for (;;) {
                        const int64_t i = next.fetch_add(1);
                        if (i >= n_cand || failed.load()) break;
                        if (score_candidate(wctx, al_w, cands[(size_t)i], &cand_score[(size_t)i]) != PMX_OK) {
                            std::lock_guard<std::mutex> lock(fail_mu);
                            if (!failed.exchange(1)) fail_msg = pmx_last_error();
                            break;
                        }
                    }
                    if (wk > 0) { if (own) pmx_aligner_free(wctx, own); pmx_ctx_destroy(wctx); }
                });
            for (auto& t : pool) t.join();
            if (failed.load()) die("refining the placement: " + fail_msg);
        }
        free_refine_aligner();
        if (dist) check(pmx_dist_sum_i64(dist, cand_score.data(), (int64_t)cand_score.size()), "summing the candidate scores over the ranks");
        struct Lookup { const std::vector<uint32_t>* nodes; const std::vector<int64_t>* scores; } lk{&cands, &cand_score};
        auto lookup = [](void* user, uint32_t node, int64_t* score) -> int {
            const Lookup& l = *(const Lookup*)user;
            const auto it = std::lower_bound(l.nodes->begin(), l.nodes->end(), node);
            if (it == l.nodes->end() || *it != node) return PMX_ERR_ARG;
            *score = (*l.scores)[(size_t)(it - l.nodes->begin())];
            return PMX_OK;
        };
        check(pmx_refine_top_candidates(pmx_index_parents(run.idx), info.n_nodes, scores5.data(), res.best_index, &rp, lookup, &lk, &refined, nullptr, nullptr, 0),
              "refining the placement");
        if (!refined.ran) fprintf(stderr, "panmap: warning: Refinement skipped: no nodes with positive scores\n");
        else say(c, "place", "refined against " + std::to_string(refined.n_candidates) + " candidates");
    }

    // Reads: `res`, the placer's tie lists, `refined`.  Leaves: `<prefix>.placement.tsv` (writer) and, on every rank, `node_id`,
    // the log_containment placement; none is Fatal "No placement found", after the file is written.
    void write_placement() {
        static const char* metric_names[5] = {"log_raw", "log_cosine", "containment", "weighted_containment", "log_containment"};
        if (writer) {
            FILE* f = fopen(tsv_path.c_str(), "w");
            if (!f) die("cannot write " + tsv_path);
            fputs("metric\tscore\tnodes\n", f);
            for (int m = 0; m < 5; ++m) {
                std::string ids;
                if (res.n_tied[m] > 0) {
                    std::vector<uint32_t> tied((size_t)res.n_tied[m]);
                    check(pmx_place_tied(run.pl, m, tied.data(), (int64_t)tied.size()), "tied nodes");
                    for (size_t j = 0; j < tied.size(); ++j) { if (j) ids += ","; ids += pmx_index_node_id(run.idx, tied[j]); }
                } else if (res.best_index[m] != UINT32_MAX) ids = pmx_index_node_id(run.idx, res.best_index[m]);
                fprintf(f, "%s\t%.6f\t%s\n", metric_names[m], res.best_score[m], ids.c_str());
            }
            if (refined.ran)   // src/placement.cpp:1987-2000
                for (int m = 0; m < 5; ++m)
                    if (refined.node[m] != UINT32_MAX)
                        fprintf(f, "refined_%s\t%.0f\t%s\n", metric_names[m], (double)refined.score[m], pmx_index_node_id(run.idx, refined.node[m]));
            fclose(f);
            say(c, "place", tsv_path);
        }
        if (res.best_index[4] == UINT32_MAX) die("No placement found");
        node_id = pmx_index_node_id(run.idx, res.best_index[4]);
        say(c, "place", node_id + " (log_containment " + std::to_string(res.best_score[4]) + ")");
    }

    // Reads: `node_id`, the PanMAN (a tree that does not open ends the sample).  Leaves: `genome`, the placed node's, and on
    // the writer `<prefix>.ref.fa` + `.fai`.
    void placed_genome() {
        pmx_panman* pm = run.panman();
        if (!pm) die(std::string("opening the PanMAN: ") + pmx_last_error());
        const int64_t node = pmx_panman_find_node(pm, node_id.c_str());
        if (node < 0) die("placed node '" + node_id + "' is not in the PanMAN");
        genome.assign((size_t)pmx_panman_node_genome(pm, node, nullptr, 0), '\0');
        pmx_panman_node_genome(pm, node, &genome[0], (int64_t)genome.size());
        if (genome.empty()) die("Empty sequence for node '" + node_id + "', cannot align");
        if (!writer) return;
        FILE* f = fopen(fa_path.c_str(), "w");
        if (!f) die("Cannot write reference file: " + fa_path);
        fprintf(f, ">%s\n%s\n", node_id.c_str(), genome.c_str());
        fclose(f);
        FILE* fai = fopen((fa_path + ".fai").c_str(), "w");   // faidx: name, length, offset of the first base, bases per line, bytes per line
        if (fai) { fprintf(fai, "%s\t%zu\t%zu\t%zu\t%zu\n", node_id.c_str(), genome.size(), node_id.size() + 2, genome.size(), genome.size() + 1); fclose(fai); }
        say(c, "align", fa_path);
    }

    // Reads: `genome`, `rs`.  Leaves: `al` with the shard's alignments on the device (the one-rank pileup runs over it) and,
    // on the writer, the whole sample's `recs` + `arena` on the host (--gpus N: gathered; the other ranks are done here).
    void align() {
        check(pmx_aligner_create(ctx, genome.data(), (int64_t)genome.size(), mean_len, &al), "indexing the placed genome");
        check(pmx_align_readset(ctx, al, rs, paired ? 1 : 0, paired ? 1 : 0), "aligning");   // mate 2 reverse-complemented on the device
        if (dist) {
            int64_t g_records = 0, g_words = 0;
            check(pmx_dist_gather_alignments(dist, al, 0, &g_records, &g_words), "gathering the ranks' alignments");
            if (!writer) return;
            if (g_records != n_reads) die("the gathered alignment records do not cover the sample");
            recs.resize((size_t)n_reads);
            arena.resize((size_t)std::max<int64_t>(g_words, 1));
            check(pmx_dist_fetch_gathered(dist, recs.data(), n_reads, arena.data(), (int64_t)arena.size()), "fetching the gathered alignments");
        } else {
            recs.resize((size_t)n_reads);
            arena.resize((size_t)std::max<int64_t>(pmx_align_cigar_words(ctx, al), 1));
            check(pmx_align_fetch(ctx, al, recs.data(), n_reads, arena.data(), (int64_t)arena.size()), "fetching the alignments");
        }
    }

    // Reads: the host reads, `recs`, `arena`.  Leaves: `<prefix>.bam` (+ .bai) and `names`, the reads' names in read order.
    void write_bam() {
        // what alignAndWriteBam holds after the aligner call: R2 reverse-complemented, its qualities reversed (src/seeding.cpp:231-269)
        std::vector<std::string> seq_s((size_t)n_reads), qual_s((size_t)n_reads);
        names.resize((size_t)n_reads);
        for (int64_t r = 0; r < n_reads; ++r) {
            names[(size_t)r] = reads.name(r);
            std::string sq(reads.concat, (size_t)reads.off[(size_t)r], (size_t)(reads.off[(size_t)r + 1] - reads.off[(size_t)r]));
            std::string ql(reads.quals, (size_t)reads.off[(size_t)r], sq.size());
            for (char& ch : ql) if (ch == '\0') ch = 'I';   // FASTA input: missing qualities
            if (paired && (r & 1)) {
                std::string rc(sq.rbegin(), sq.rend());
                for (char& ch : rc) ch = comp(ch);
                sq.swap(rc);
                std::string rq(ql.rbegin(), ql.rend());
                ql.swap(rq);
            }
            seq_s[(size_t)r].swap(sq);
            qual_s[(size_t)r].swap(ql);
        }
        std::vector<const char*> seq_p((size_t)n_reads), qual_p((size_t)n_reads), name_p((size_t)n_reads);
        std::vector<int> lens((size_t)n_reads);
        for (int64_t r = 0; r < n_reads; ++r) { seq_p[(size_t)r] = seq_s[(size_t)r].c_str(); qual_p[(size_t)r] = qual_s[(size_t)r].c_str(); name_p[(size_t)r] = names[(size_t)r].c_str(); lens[(size_t)r] = (int)seq_s[(size_t)r].size(); }
        const int64_t n_items = paired ? n_reads / 2 : n_reads;
        std::vector<align_pair_result_t> results((size_t)std::max<int64_t>(n_items, 1));
        int64_t n_mapped = 0, n_withheld = 0;
        auto fill = [&](const pmx_aln_record& r, read_align_t* o) {
            memset(o, 0, sizeof(*o));
            if (r.mapped && (r.flags & PMX_ALN_HAS_ALN)) {
                o->pos = r.rs + 1; o->rs = r.rs; o->re = r.re; o->qs = r.qs; o->qe = r.qe;
                o->mapq = r.mapq; o->rev = r.rev; o->proper_frag = r.proper_frag; o->n_cigar = r.n_cigar;
                o->cigar = arena.data() + r.cigar_off;   // (points into the arena: nothing to free)
            } else o->pos = INT_MAX;
        };
        for (int64_t k = 0; k < n_items; ++k) {
            align_pair_result_t& out = results[(size_t)k];
            memset(&out, 0, sizeof(out));
            const pmx_aln_record& a = recs[(size_t)(paired ? 2 * k : k)];
            const bool invalid = paired ? ((a.flags | recs[(size_t)(2 * k + 1)].flags) & 3) != 0 : (a.flags & 3) != 0;
            out.r1.pos = out.r2.pos = INT_MAX;
            if (invalid) { ++n_withheld; continue; }
            if (!a.mapped) continue;
            out.mapped = 1;
            ++n_mapped;
            fill(a, &out.r1);
            if (paired) fill(recs[(size_t)(2 * k + 1)], &out.r2);
        }
        check(pmx_write_bam(bam_path.c_str(), node_id.c_str(), (int64_t)genome.size(), (int)n_reads, seq_p.data(), qual_p.data(), name_p.data(), lens.data(),
                            results.data(), paired), "writing the BAM");
        say(c, "align", bam_path + " (" + std::to_string(n_mapped) + " of " + std::to_string(n_items) + (paired ? " pairs" : " reads") + " mapped" +
                        (n_withheld ? ", " + std::to_string(n_withheld) + " invalid records withheld" : "") + ")");
    }

    // One rank: the pileup runs over what the align stage left on the device.  --gpus N: rank 0 holds the gathered records
    // and the whole sample's reads on the host and uploads them.  Same tables either way.
    // Reads: `al` + `rs`, or `recs` + `arena` + the host reads; `names`, `genome`, the tree's spectrum.  Leaves: `pu` (the
    // pileup, on the device), `gt` (the calls) and `<prefix>.vcf`.
    void genotype() {
        std::string names_concat;
        std::vector<int64_t> name_off((size_t)n_reads + 1, 0);
        for (int64_t r = 0; r < n_reads; ++r) { names_concat += names[(size_t)r]; name_off[(size_t)r + 1] = (int64_t)names_concat.size(); }
        names_concat.push_back('\0');
        check(pmx_pileup_create(ctx, &pu), "creating the pileup");
        if (dist) {
            check(pmx_pileup_run_records(ctx, pu, recs.data(), n_reads, arena.data(), (int64_t)arena.size(), reads.concat.data(), reads.quals.data(), reads.off.data(),
                                         (int64_t)genome.size(), paired ? 1 : 0, paired ? 1 : 0, names_concat.data(), name_off.data(), nullptr), "pileup");
        } else {
            check(pmx_readset_set_qualities(ctx, rs, reads.quals.data()), "attaching the qualities");
            check(pmx_pileup_run(ctx, pu, al, rs, (int64_t)genome.size(), paired ? 1 : 0, paired ? 1 : 0, names_concat.data(), name_off.data(), nullptr), "pileup");
        }
        std::vector<uint32_t> hist(genome.size() * PMX_PILEUP_HIST), aux(genome.size() * PMX_PILEUP_AUX);
        check(pmx_pileup_fetch(ctx, pu, hist.data(), aux.data()), "fetching the pileup tables");
        const int64_t n_calls = pmx_genotype_call(hist.data(), aux.data(), genome.data(), (int64_t)genome.size(), node_id.c_str(), run.spectrum(),
                                                  c.min_depth, c.min_qual, &gt);
        if (n_calls < 0) die(std::string("calling variants: ") + pmx_last_error());
        if (c.annotate_vcf && n_calls > 0) {
            // the written records' sites go through the bias pass of the pileup that is still on the device
            std::vector<int32_t> sites((size_t)n_calls);
            std::string letters((size_t)n_calls, 'N');
            for (int64_t i = 0; i < n_calls; ++i) {
                sites[(size_t)i] = (int32_t)pmx_genotype_record_pos(gt, i);
                letters[(size_t)i] = genome[(size_t)sites[(size_t)i]];
            }
            std::vector<uint32_t> bias((size_t)n_calls * PMX_PILEUP_BIAS);
            check(pmx_pileup_bias(ctx, pu, sites.data(), letters.data(), n_calls, bias.data()), "pileup bias pass");
            check(pmx_genotype_annotate(gt, sites.data(), bias.data(), n_calls), "annotating the records");
        }
        check(pmx_genotype_write_vcf(gt, vcf_path.c_str(), node_id.c_str(), (int64_t)genome.size(), bam_path.c_str()), "writing the VCF");
        say(c, "call", vcf_path + " (" + std::to_string(n_calls) + " variants)");
    }

    // Reads: `<prefix>.vcf` and `<prefix>.ref.fa` as written.  Leaves: `<prefix>.consensus.fa`.
    void consensus() {
        std::string sample = c.output.substr(c.output.find_last_of("/\\") + 1);   // src/main.cpp:1889-1892
        if (sample.empty()) sample = "sample";
        check(pmx_genotype_write_consensus(vcf_path.c_str(), fa_path.c_str(), cons_path.c_str(), (sample + "_consensus ref=" + node_id).c_str()), "writing the consensus");
        say(c, "consensus", cons_path);
    }
};

// Returns the placed node; throws Fatal.  `stop`: 1 place, 2 align, 3 genotype, 4 consensus.
std::string run_sample(const Config& c, int stop, Run& run) {
    const Reads reads(c.reads1, c.reads2, Reads::INTERLEAVED);
    Sample s(c, run, reads);
    s.place();
    if (c.refine) s.refine();
    s.write_placement();
    if (stop == 1) return s.node_id;
    s.placed_genome();
    s.align();
    if (!s.writer) return s.node_id;             // --gpus N: rank 0 has everything now and writes the rest
    s.write_bam();
    if (stop < 3) return s.node_id;
    s.genotype();
    if (stop < 4) return s.node_id;
    s.consensus();
    return s.node_id;
}

// ------------------------------------------------------------------------------------------------ --gpus N
// One process per GPU, forked before any GPU call: what the caller holds in memory (the indexes, the PanMAN, the reads) every
// rank inherits, and each rank opens its own device.  The ranks meet through RCCL (pmx_dist_*); the communicator's id travels
// through a file in a private directory.  The parent only waits.
struct Ranks {
    int rank = 0, world = 1;
    std::string meet_dir;
};

// -> true in a rank (rk filled in), false in the parent once the ranks have ended (*code = the run's exit code).
// rendezvous = false: ranks that never meet (--batch) get no directory
bool fork_ranks(int n, Ranks& rk, int* code, bool rendezvous = true) {
    if (n <= 1) return true;
    char tmpl[] = "/tmp/panmap_ranks_XXXXXX";
    if (rendezvous) {
        if (!mkdtemp(tmpl)) die("cannot create a rendezvous directory under /tmp");
        rk.meet_dir = tmpl;
    }
    fflush(stdout); fflush(stderr);
    std::vector<pid_t> kids;
    for (int r = 0; r < n; ++r) {
        const pid_t pid = fork();
        if (pid < 0) die("fork failed");
        if (pid == 0) { rk.rank = r; rk.world = n; return true; }
        kids.push_back(pid);
    }
    // Wait for whichever rank ends first.  A rank that fails (no such device, unreadable reads, any die() between two
    // collectives) leaves the others blocked in ncclCommInitRank / a collective for ever: the first failure ends the
    // run -- the remaining children (and only they) get SIGTERM, are reaped, and its code is returned.
    int worst = 0;
    size_t left = kids.size();
    while (left > 0) {
        int st = 0;
        const pid_t k = waitpid(-1, &st, 0);
        if (k < 0) {
            if (errno == EINTR) continue;
            worst = worst ? worst : 1;
            break;
        }
        auto it = std::find(kids.begin(), kids.end(), k);
        if (it == kids.end()) continue;
        *it = -1;
        --left;
        const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
        if (code && !worst) {
            worst = code;
            for (pid_t o : kids) if (o > 0) kill(o, SIGTERM);
        }
    }
    if (rendezvous) {
        unlink((rk.meet_dir + "/uid.tmp").c_str());
        unlink((rk.meet_dir + "/uid").c_str());
        rmdir(rk.meet_dir.c_str());
    }
    *code = worst;
    return false;
}

// The GPUs a rank of this run could open, counted in a child of its own: the parent must not touch the GPU before it forks
// the ranks (each rank opens its own device in a fresh process state).
int visible_gpus() {
    fflush(stdout); fflush(stderr);
    const pid_t pid = fork();
    if (pid < 0) return 0;
    if (pid == 0) _exit(std::min(pmx_device_count(), 255));
    int st = 0;
    while (waitpid(pid, &st, 0) < 0 && errno == EINTR) {}
    return WIFEXITED(st) ? WEXITSTATUS(st) : 0;
}

// one sample sharded over --gpus N needs a GPU per rank (PMX_DEVICE names the first; PMX_DIST_SAME_DEVICE: the ranks share it)
bool gpus_for_every_rank(int n, int* have) {
    if (getenv("PMX_DIST_SAME_DEVICE")) return true;
    *have = visible_gpus();
    const char* e = getenv("PMX_DEVICE");
    return (e ? atoi(e) : 0) + n <= *have;
}

int rank_device(const Ranks& rk) {
    int dev = 0;
    if (const char* e = getenv("PMX_DEVICE")) dev = atoi(e);
    if (rk.world > 1 && !getenv("PMX_DIST_SAME_DEVICE")) dev += rk.rank;   // (PMX_DIST_SAME_DEVICE: functional test on a one-GPU box)
    return dev;
}

// the rendezvous: rank 0 makes the communicator id and publishes it in the directory, every rank joins (NULL for one rank)
pmx_dist* join_ranks(pmx_ctx* ctx, const Ranks& rk) {
    if (rk.world <= 1) return nullptr;
    char uid[PMX_DIST_ID_BYTES];
    const std::string uid_path = rk.meet_dir + "/uid";
    if (rk.rank == 0) {
        check(pmx_dist_unique_id(uid), "creating the communicator id");
        FILE* f = fopen((uid_path + ".tmp").c_str(), "wb");
        if (!f || fwrite(uid, 1, sizeof(uid), f) != sizeof(uid)) die("cannot write the communicator id");
        fclose(f);
        if (rename((uid_path + ".tmp").c_str(), uid_path.c_str()) != 0) die("cannot publish the communicator id");
    } else {
        FILE* f = nullptr;
        for (int tries = 0; tries < 600000 && !(f = fopen(uid_path.c_str(), "rb")); ++tries) usleep(500);
        if (!f || fread(uid, 1, sizeof(uid), f) != sizeof(uid)) die("rank 0 never published the communicator id");
        fclose(f);
    }
    pmx_dist* dist = nullptr;
    check(pmx_dist_init(ctx, uid, rk.rank, rk.world, &dist), "joining the ranks (RCCL)");
    return dist;
}

// ------------------------------------------------------------------------------------------------ --batch
// The samples of a batch file are DEALT, not sharded: each one runs whole, on one GPU, against what that process keeps
// resident, exactly as it runs under --gpus 1 -- so its files are the one-GPU run's by construction.  With --gpus N the ranks
// never meet (no rendezvous, no pmx_dist): all they share is this block, mapped by the parent before the fork.  A rank takes
// the next sample of the file until none is left, and adds each sample to one of the two counts the parent reports at the
// end.  One process (--gpus 1) runs the same loop alone: the file's order.
struct Deal {
    std::atomic<int64_t> next, done, failed;
    static_assert(std::atomic<int64_t>::is_always_lock_free, "the batch counters are shared between processes");

    static Deal* map() {
        void* p = mmap(nullptr, sizeof(Deal), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) die("cannot map the counters of the batch");
        Deal* d = new (p) Deal;
        d->next.store(0); d->done.store(0); d->failed.store(0);
        return d;
    }
};

// One rank's (or the only process's) part of the batch.  run_one(sample) runs one sample and returns what its report line
// says behind `->`; a Fatal is that sample's failure and the batch goes on (runBatchPlacement, src/main.cpp:1464-1666).  The
// line -- `[position in the file/samples] prefix -> ... (NNNms)` -- leaves in one write(2), so the lines of several ranks
// cannot interleave.
template <class RunOne>
void run_dealt(const std::vector<BatchEntry>& samples, Deal& deal, RunOne&& run_one) {
    const int64_t n = (int64_t)samples.size();
    for (int64_t i; (i = deal.next.fetch_add(1)) < n;) {
        const BatchEntry& e = samples[(size_t)i];
        const size_t slash = e.prefix.find_last_of('/');
        if (slash != std::string::npos && slash > 0) mkdirs(e.prefix.substr(0, slash));
        const auto t0 = std::chrono::steady_clock::now();
        std::string what;
        bool ok = true;
        try { what = run_one(e); }
        catch (const Fatal& f) { ok = false; what = f.msg == "No placement found" ? std::string("NO PLACEMENT") : "failed: " + f.msg; }
        const long long ms = (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        const std::string line = "[" + std::to_string(i + 1) + "/" + std::to_string(n) + "] " + e.prefix + " -> " + what + " (" + std::to_string(ms) + "ms)\n";
        if (write(2, line.data(), line.size()) < 0) {}   // (nowhere to report it)
        (ok ? deal.done : deal.failed).fetch_add(1);
    }
}

// The end of the batch, in the parent of the ranks or in the only process.  code: what fork_ranks returned -- non-zero when a
// rank could not start or died; its samples are not dealt again, and nothing more is started after a GPU process has died.
int end_batch(Deal* deal, int code, size_t n_samples, const char* verb) {
    const long long done = (long long)deal->done.load(), failed = (long long)deal->failed.load();
    munmap(deal, sizeof(Deal));
    if (code) {
        fprintf(stderr, "panmap: error: a rank ended with code %d; %lld of %zu samples had been reported, the others are not run\n", code, done + failed, n_samples);
        return code;
    }
    fprintf(stderr, "Batch complete: %lld %s, %lld failed\n", done, verb, failed);
    return failed ? 1 : 0;
}

// the id of node `head` and, comma-joined behind it, the ids of the n nodes that share its line: those folded into it
// (identical nodes, src/mgsr.cpp:505-532) or the haplotypes merged with it
std::string joined_ids(const pmx_index* idx, uint32_t head, const uint32_t* others, size_t n) {
    std::string ids = pmx_index_node_id(idx, head);
    for (size_t i = 0; i < n; ++i) { ids += ","; ids += pmx_index_node_id(idx, others[i]); }
    return ids;
}

// What one --meta process keeps for all its samples (runDeconvolution, src/main.cpp:1192-1313; --filter-and-assign:
// filterAndAssignBatch, :720-1016): the Run with the PanMAN, the two indexes of the tree (the place stage's and its oriented
// form, without flank mask, built in memory), the context and the pmx_meta with its settings; the two tables; the ranks.  One
// function per step in the order run_meta calls them.  --gpus N without --batch: one rank per GPU, each with a contiguous shard
// of the one sample's reads (R1 then R2); every rank ends with the whole sample's result (pmx_meta_attach_dist), rank 0 writes
// it.  With --batch the ranks never meet: each runs whole samples.  run.close() is run_meta's call at the normal ends.
struct MetaRun {
    Config c;                                    // (quiet in the ranks above 0)
    Run run;
    struct Amplicons { pmx_amplicons* a = nullptr; ~Amplicons() { pmx_amplicons_free(a); } } amplicons;   // --amplicon-depth
    struct Taxonomy { pmx_taxonomy* t = nullptr; ~Taxonomy() { pmx_taxonomy_free(t); } } taxonomy;        // --taxonomic-metadata
    Ranks rk;

    explicit MetaRun(const Config& c_) : c(c_) {}

    // the refusals that need no file
    void refuse_options() const {
        if (c.reads1.empty() && c.batch.empty()) die("--meta needs reads");
        // one sample of --filter-and-assign, or with the read-score reports, over --gpus N is sharded over N ranks that gather
        // to rank 0; decided here, before anything is built, when the machine cannot give every rank a GPU
        int have = 0;
        if (c.filter_and_assign && c.gpus > 1 && c.batch.empty() && !gpus_for_every_rank(c.gpus, &have))
            die("--filter-and-assign over --gpus " + std::to_string(c.gpus) + " shards the sample over " + std::to_string(c.gpus) +
                " ranks and needs one GPU per rank: this machine shows " + std::to_string(have) + "; lower --gpus");
        if (!c.batch.empty() && !c.amplicon_depth.empty())
            die("option --amplicon-depth is not accepted with --batch: one table cannot name the reads of several samples");
        if (c.discard < 0.0 || c.discard > 1.0) die("--discard must be between 0 and 1");   // src/main.cpp:1358-1361
        if (c.dust > 100.0) die("--dust must be <= 100");                                    // src/main.cpp:1353-1356
        if (c.l < 2) die("--meta needs l >= 2 in this build (the orientation of a lone syncmer is not indexed)");
        if (!c.mask_options.empty() && c.filter_and_assign)   // (initializeQueryDataBatch, src/mgsr.cpp:1575, never masks)
            die("option " + c.mask_options[0] + " is not accepted with --filter-and-assign: the reference's reader for that mode " +
                (c.mask_options[0] == "--mask-read-ends" ? "takes the value and ignores it" : "never masks"));
        if (!c.em_options.empty() && c.filter_and_assign)
            die("option " + c.em_options[0] + " is not accepted with --filter-and-assign: that mode ranks no candidates and runs no EM");
        if ((c.read_scores_unfiltered || c.read_scores_filtered) && !c.filter_and_assign && c.gpus > 1 && c.batch.empty() && !gpus_for_every_rank(c.gpus, &have))
            die(std::string("option ") + (c.read_scores_unfiltered ? "--write-meta-read-scores-unfiltered" : "--write-meta-read-scores-filtered") +
                " is not accepted with one sample over --gpus " + std::to_string(c.gpus) + " on this machine: the ranks gather their rows of the reads to rank 0 and need a GPU each, it shows " +
                std::to_string(have) + "; lower --gpus");
        if (c.mask_reads < 0 || c.mask_seeds < 0) die("--mask-reads and --mask-seeds must not be negative");
        if (c.mask_reads_rf < 0.0 || c.mask_seeds_rf < 0.0)
            die("--mask-reads-relative-frequency and --mask-seeds-relative-frequency must not be negative");
        if ((c.mask_reads > 0) + (c.mask_seeds > 0) + (c.mask_reads_rf > 0.0) + (c.mask_seeds_rf > 0.0) > 1)
            die("Only one masking parameter can be set at a time");   // src/mgsr.cpp:2049-2053
    }

    // The amplicons: the table is read before anything else is opened.  (A relative mask without the file does nothing in the
    // reference, whose single group is then the unlisted one: refused.)  Leaves: amplicons.a, null without --amplicon-depth.
    void load_amplicons() {
        if (c.amplicon_depth.empty()) {
            for (const std::string& o : c.mask_options)
                if (o == "--mask-reads-relative-frequency" || o == "--mask-seeds-relative-frequency")
                    die("option " + o + " is not accepted without --amplicon-depth: its threshold is a share of the reads of amplicon groups, which this "
                        "build does not make without that file");
            return;
        }
        const int rc = pmx_amplicons_load(c.amplicon_depth.c_str(), &amplicons.a);
        if (rc == PMX_ERR_IO)
            die("option --amplicon-depth is not accepted: cannot read " + c.amplicon_depth + ", the file that names the amplicon groups, which this build "
                "does not make by itself");
        if (rc != PMX_OK) die(std::string("option --amplicon-depth is not accepted: ") + pmx_last_error());
    }

    // The taxonomy filter: its refusals, then the table, read before anything else is opened.  Leaves: taxonomy.t, null
    // without --taxonomic-metadata.
    void load_taxonomy() {
        const bool with_taxonomy = !c.taxonomic_metadata.empty();
        if ((with_taxonomy || !c.taxonomy_options.empty()) && !c.filter_and_assign)
            die("option " + (with_taxonomy ? std::string("--taxonomic-metadata") : c.taxonomy_options[0]) + " is not accepted without --filter-and-assign");
        if (!with_taxonomy && !c.taxonomy_options.empty()) die("option " + c.taxonomy_options[0] + " is not accepted without --taxonomic-metadata");
        if (!with_taxonomy) return;
        if (c.maximum_taxon_number < 1 || c.maximum_taxon_number > 16) die("--maximum-taxon-number must be between 1 and 16");
        if (c.ambiguous_score < 0 || c.ambiguous_ratio < 0.0) die("--ambiguous-score-threshold and --ambiguous-score-threshold-ratio must not be negative");
        if (c.discard > 0.0 && (c.ambiguous_score > 0 || c.ambiguous_ratio > 0.0))
            die("--discard above 0 cannot be combined with --ambiguous-score-threshold or --ambiguous-score-threshold-ratio: which near-best nodes "
                "count would then depend on the order of a node's seed changes in the reference");
        const int rc = pmx_taxonomy_load(c.taxonomic_metadata.c_str(), c.taxonomic_rank.c_str(), &taxonomy.t);
        if (rc == PMX_ERR_IO) die("option --taxonomic-metadata is not accepted: cannot read " + c.taxonomic_metadata);
        check(rc, "--taxonomic-metadata");
    }

    // Leaves: the open PanMAN, run.idx and run.oidx; the two builds are independent: side by side.
    void build_indexes() {
        run.panman_path = c.panman;
        pmx_panman* pm = run.panman();
        if (!pm) die(std::string("opening the PanMAN: ") + pmx_last_error());
        int rc1 = PMX_OK, rc2 = PMX_OK;
        std::string e2;
        std::thread th([&]() { rc2 = pmx_index_build_ex(pm, c.k, c.s, c.t, c.l, c.open_syncmer ? 1 : 0, 0, PMX_INDEX_ORIENTED, -1, &run.oidx); if (rc2 != PMX_OK) e2 = pmx_last_error(); });
        rc1 = pmx_index_build_ex(pm, c.k, c.s, c.t, c.l, c.open_syncmer ? 1 : 0, 0, 0, -1, &run.idx);
        th.join();
        check(rc1, "building the index");
        if (rc2 != PMX_OK) die("building the oriented index: " + e2);
        say(c, "index", "seed index + oriented seed index (in memory)");
    }

    // n ranks; meet: they join each other (one sample, sharded) -- or never meet (--batch: whole samples, dealt).
    // -> true in a rank, false in the parent once the ranks have ended (*code = the run's exit code).
    // In a rank, leaves: rk, the rank's device open and, when they meet, the ranks joined (run.ctx, run.dist).
    bool open_rank(int n, bool meet, int* code) {
        if (!fork_ranks(n, rk, code, meet)) return false;
        if (rk.rank > 0) c.quiet = true;
        run.dev = rank_device(rk);
        check(pmx_ctx_create(run.dev, &run.ctx), "opening the GPU");
        if (meet) run.dist = join_ranks(run.ctx, rk);
        return true;
    }

    // Leaves: run.meta with the indexes on the device, the ranks attached, --dust, the masks and what --filter-and-assign is
    // run with: the taxonomy, the ambiguity thresholds, --breadth-ratio.  None of it depends on a sample's reads.
    void configure() {
        pmx_meta*& m = run.meta;
        check(pmx_meta_create(run.ctx, run.idx, run.oidx, &m), "uploading the indexes");
        if (run.dist) check(pmx_meta_attach_dist(m, run.dist), "attaching the ranks");
        check(pmx_meta_set_dust(m, c.dust), "--dust");
        check(pmx_meta_set_mask_read_ends(m, c.mask_read_ends), "--mask-read-ends");
        if (c.mask_read_ends > 0)
            say(c, "meta", "Mask-read-ends " + std::to_string(c.mask_read_ends) + " turned on: " + std::to_string(c.mask_read_ends) +
                               " bases are cut from both ends of every read before seeding");
        check(pmx_meta_set_em_leaves_only(m, c.em_leaves_only ? 1 : 0), "--em-leaves-only");
        check(pmx_meta_set_masks(m, c.mask_reads, c.mask_seeds), "--mask-reads / --mask-seeds");
        check(pmx_meta_set_relative_masks(m, c.mask_reads_rf, c.mask_seeds_rf), "--mask-reads-relative-frequency / --mask-seeds-relative-frequency");
        if (!c.filter_and_assign) return;
        if (taxonomy.t) {
            std::vector<int32_t> node_taxon;
            for (int64_t v = 0; pmx_index_node_id(run.idx, v); ++v) node_taxon.push_back((int32_t)pmx_taxonomy_lookup(taxonomy.t, pmx_index_node_id(run.idx, v)));
            check(pmx_meta_set_taxonomy(m, node_taxon.data(), (int64_t)node_taxon.size(), pmx_taxonomy_num_taxa(taxonomy.t), c.maximum_taxon_number), "--taxonomic-metadata");
            check(pmx_meta_set_ambiguous(m, c.ambiguous_score, c.ambiguous_ratio), "--ambiguous-score-threshold");
        }
        check(pmx_meta_set_breadth(m, c.breadth_ratio ? 1 : 0), "--breadth-ratio");
    }
};

// One sample of a --meta process: its reads, this rank's shard of them, and what the steps leave for one another.  A
// call-lifetime struct, one function per step in the order meta_steps calls them.  Nothing of a sample outlives it: the
// tallies and lists below start empty for every sample of a batch.  `c`: the sample's reads1 / reads2 / output (--batch: a
// copy of the run's with those three set, and quiet).
struct MetaSample {
    const Config& c;
    Run& run;
    const MetaRun::Amplicons& amplicons;
    const MetaRun::Taxonomy& taxonomy;
    std::unique_ptr<const Reads> reads_p;        // mates as sequenced, one after the other
    int64_t lo = 0, hi = 0;                      // this rank's shard
    // --filter-and-assign, what assign() leaves for the writers: per merged read its state, LCA node and nodes [off[r], off[r + 1])
    // of `nodes`; per read of the input its merged read; per node its head, per head the nodes folded into it
    int64_t n_merged = 0, n_nodes = 0;
    std::vector<uint8_t> state;
    std::vector<uint32_t> lca, nodes, head;
    std::vector<int64_t> off, merged;
    std::vector<std::vector<uint32_t>> folded;
    // ... and write_fastq: per merged read the FASTQ positions of its copies (ascending: input order), the four tallies
    std::string fq_path;
    std::vector<std::vector<int64_t>> copies;
    int64_t n_written = 0, n_unmapped = 0, n_discarded = 0, n_over = 0;
    // ... write_fastq and write_node_lists for --align-reads: per FASTQ position its read of the input, per head the FASTQ
    // positions of its reads (ascending)
    std::vector<int64_t> fq_read;
    std::vector<std::vector<int64_t>> by_node;
    // the read-score reports, what score_all_nodes() leaves for the two writers (and `merged`, n_merged)
    std::vector<uint16_t> rs_max;
    std::vector<uint32_t> rs_nbest;
    std::vector<int64_t> rs_seedmers, rs_mult;
    std::vector<std::vector<int64_t>> rs_copies;

    MetaSample(MetaRun& mr, const Config& c_) : c(c_), run(mr.run), amplicons(mr.amplicons), taxonomy(mr.taxonomy) {}
    ~MetaSample() {                              // (a sample that failed inside --align-reads)
        if (al_rs) pmx_readset_free(run.ctx, al_rs);
        if (al_fa) fclose(al_fa);
    }
    const Reads& reads() const { return *reads_p; }
    bool masking() const { return c.mask_reads > 0 || c.mask_seeds > 0 || c.mask_reads_rf > 0.0 || c.mask_seeds_rf > 0.0; }
    std::string ids_of_head(uint32_t h) const { return joined_ids(run.idx, h, folded[h].data(), folded[h].size()); }

    // Leaves: the whole sample's reads on the host (one sample over --gpus N: before the fork, every rank inherits them).
    void read_reads() { reads_p.reset(new Reads(c.reads1, c.reads2, Reads::APPENDED)); }

    // Leaves: the shard [lo, hi) of rank `rank` of `world` (a dealt sample: all of it, 0 of 1).
    void take_shard(int rank, int world) { reads().shard(rank, world, &lo, &hi); }

    // --amplicon-depth.  Leaves: in run.meta the amplicon of every read of this rank's shard, by its own name (mates one by one);
    // unlisted: the last group.
    void set_amplicons() {
        pmx_meta* m = run.meta;
        if (!amplicons.a) return;
        const int32_t n_groups = pmx_amplicons_num_groups(amplicons.a);
        std::vector<int32_t> group((size_t)(hi - lo));
        for (int64_t r = lo; r < hi; ++r) {
            const int32_t g = pmx_amplicons_lookup(amplicons.a, reads().name(r).c_str());
            group[(size_t)(r - lo)] = g < 0 ? n_groups : g;
        }
        check(pmx_meta_set_amplicons(m, group.data(), hi - lo, n_groups), "--amplicon-depth");
        if (c.quiet) return;
        int64_t unlisted = 0;   // (over the whole sample, whatever the shard)
        for (int64_t r = 0; r < reads().n_reads; ++r) unlisted += pmx_amplicons_lookup(amplicons.a, reads().name(r).c_str()) < 0;
        say(c, "meta", "Amplicons: " + std::to_string(n_groups) + " groups in " + c.amplicon_depth + ", " + std::to_string(unlisted) + " of " +
                           std::to_string(reads().n_reads) + " reads not listed");
    }

    // Reads: the shard.  Leaves: the merged reads of the whole sample in run.meta, masked when a mask is set.
    void set_reads() { check(pmx_meta_set_reads(run.ctx, run.meta, reads().concat.data(), reads().off.data() + lo, hi - lo), "seeding the reads"); }

    // the reference's two lines (src/mgsr.cpp:2220-2230)
    void report_masks() const {
        if (!masking()) return;
        int64_t dropped = 0, removed = 0, left = 0;
        check(pmx_meta_mask_info(run.meta, &dropped, &removed, &left), "the numbers of the masks");
        char rf[64];   // (a relative parameter as the reference's stream prints a double)
        snprintf(rf, sizeof(rf), "%g", c.mask_reads_rf > 0.0 ? c.mask_reads_rf : c.mask_seeds_rf);
        const bool whole_reads = c.mask_reads > 0 || c.mask_reads_rf > 0.0;
        const std::string value = c.mask_reads > 0 ? std::to_string(c.mask_reads) : c.mask_seeds > 0 ? std::to_string(c.mask_seeds) : std::string(rf);
        say(c, "meta", whole_reads ? "Mask-reads " + value + " turned on: " + std::to_string(dropped) +
                                         " reads containing low coverage kminmers will be skipped during placement and EM... Total reads to process: " +
                                         std::to_string(left)
                                   : "Mask-seeds " + value + " turned on: " + std::to_string(removed) +
                                         " seeds are removed during placement and EM... Total reads to process: " + std::to_string(left));
    }

    // ---- --filter-and-assign (writeAssignedReadsOut, src/main.cpp:522-558, :889-903), after set_reads: every read against every
    // node, then the files.  `<prefix>.mgsr.assignedReads.fastq` holds the assigned reads in input order (FASTA input: quality
    // `I`); `.mgsr.assignedReads.out` and `.mgsr.assignedReadsLCANode.out` hold one line per head node that has reads,
    // `head[,nodes folded into it]<TAB>.<TAB>count<TAB>indices into the FASTQ`, by ascending DFS index of the head (the reference's
    // orders come from hash-map iteration: DESIGN.md section 4.3).  With --taxonomic-metadata the reads spanning more than
    // --maximum-taxon-number taxa are in none of the files, and the second column holds the taxon names of the head's subtree by
    // ascending taxon index, `.` when there are none or too many.

    // Leaves: `merged`, per read of the WHOLE input its merged read.  One sample over --gpus N (collective): every rank holds the
    // slice of its shard, in the whole sample's numbering; the shards are contiguous in input order, so the map is their
    // concatenation -- a zero-filled array with the slice (+ 1) at the shard's place, summed over the ranks.
    void whole_raw_to_merged() {
        pmx_meta* m = run.meta;
        merged.assign((size_t)std::max<int64_t>(reads().n_reads, 1), 0);
        if (!run.dist) {
            check(pmx_meta_raw_to_merged(m, merged.data(), reads().n_reads), "the reads' merged reads");
            return;
        }
        if (pmx_meta_num_raw_reads(m) != hi - lo) die("the shard's raw -> merged map does not cover the shard");
        std::vector<int64_t> mine((size_t)std::max<int64_t>(hi - lo, 1));
        check(pmx_meta_raw_to_merged(m, mine.data(), hi - lo), "the shard's merged reads");
        for (int64_t r = lo; r < hi; ++r) merged[(size_t)r] = mine[(size_t)(r - lo)] + 1;
        check(pmx_dist_sum_i64(run.dist, merged.data(), reads().n_reads), "assembling the reads' merged reads over the ranks");
        for (int64_t& x : merged) --x;
    }

    // Leaves: the assignment on the device's side done and downloaded: state / lca / off / nodes / merged, head / folded.
    // One sample over --gpus N: every rank assigns its rows of the merged reads, rank 0 gathers them (the other ranks return
    // after the collective calls, with nothing to write).
    void assign() {
        pmx_meta* m = run.meta;
        check(pmx_meta_assign(run.ctx, m, c.discard), "assigning the reads to nodes");
        if (run.dist) {
            check(pmx_meta_assign_gather(run.ctx, m, 0), "gathering the ranks' assignments");
            whole_raw_to_merged();
            if (pmx_dist_rank(run.dist) != 0) return;
        }
        n_merged = pmx_meta_num_reads(m);
        state.resize((size_t)std::max<int64_t>(n_merged, 1));
        lca.resize(state.size());
        nodes.resize((size_t)std::max<int64_t>(pmx_meta_assign_num_nodes(m), 1));
        off.resize((size_t)n_merged + 1);
        check(pmx_meta_assign_reads(m, state.data(), nullptr, lca.data(), nullptr, n_merged), "the reads' states");
        check(pmx_meta_assign_nodes(m, off.data(), nodes.data(), (int64_t)nodes.size()), "the reads' nodes");
        if (!run.dist) whole_raw_to_merged();
        pmx_index_info info;
        check(pmx_index_get_info(run.oidx, &info), "index info");
        n_nodes = info.n_nodes;
        head.resize((size_t)n_nodes);
        check(pmx_index_node_heads(run.oidx, head.data()), "folding identical nodes");
        folded.resize((size_t)n_nodes);
        for (uint32_t v = 0; v < (uint32_t)n_nodes; ++v)
            if (head[v] != v) folded[head[v]].push_back(v);
    }

    // Reads: state, merged, the reads.  Leaves: the FASTQ, `copies`, the four tallies.
    void write_fastq() {
        const Reads& rd = reads();
        fq_path = c.output + ".mgsr.assignedReads.fastq";
        FILE* fq = fopen(fq_path.c_str(), "w");
        if (!fq) die("cannot write " + fq_path);
        copies.resize((size_t)n_merged);
        for (int64_t r = 0; r < rd.n_reads; ++r) {
            const int64_t mr = merged[(size_t)r];
            const int st = mr < 0 ? PMX_META_UNMAPPED : state[(size_t)mr];
            if (st != PMX_META_ASSIGNED) { (st == PMX_META_OVER_TAXA ? n_over : st == PMX_META_DISCARDED ? n_discarded : n_unmapped)++; continue; }
            const size_t at = (size_t)rd.off[(size_t)r], len = (size_t)(rd.off[(size_t)r + 1] - rd.off[(size_t)r]);
            const std::string qual = len > 0 && rd.quals[at] == '\0' ? std::string(len, 'I') : rd.quals.substr(at, len);   // src/main.cpp:889-903
            fprintf(fq, "@%s\n%.*s\n+\n%s\n", rd.name(r).c_str(), (int)len, rd.concat.data() + at, qual.c_str());
            copies[(size_t)mr].push_back(n_written++);
            if (c.align_reads) fq_read.push_back(r);
        }
        fclose(fq);
    }

    // one of the two node-list files: a line per head with reads (`groups[h]`: their FASTQ positions, sorted here)
    void write_node_list(const std::string& path, std::vector<std::vector<int64_t>>& groups) const {
        FILE* f = fopen(path.c_str(), "w");
        if (!f) die("cannot write " + path);
        for (uint32_t h = 0; h < (uint32_t)n_nodes; ++h) {
            std::vector<int64_t>& g = groups[h];
            if (g.empty()) continue;
            std::sort(g.begin(), g.end());
            std::string taxa;
            uint32_t tx[16];
            const int64_t n_tx = taxonomy.t ? pmx_meta_node_taxa(run.meta, h, tx, 16) : 0;
            for (int64_t i = 0; i < n_tx; ++i) { if (i) taxa += ","; taxa += pmx_taxonomy_taxon_name(taxonomy.t, tx[i]); }
            fprintf(f, "%s\t%s\t%zu\t", ids_of_head(h).c_str(), taxa.empty() ? "." : taxa.c_str(), g.size());
            for (size_t i = 0; i < g.size(); ++i) fprintf(f, i ? ",%lld" : "%lld", (long long)g[i]);
            fputc('\n', f);
        }
        fclose(f);
    }

    // Reads: off / nodes / lca / head, copies.  Read -> nodes inverted to head -> reads, for the assigned nodes and for the LCA
    // node.  Leaves: the two node-list files and `by_node`, each head's list sorted.
    void write_node_lists() {
        std::vector<std::vector<int64_t>> by_lca((size_t)n_nodes);
        by_node.assign((size_t)n_nodes, {});
        for (int64_t mr = 0; mr < n_merged; ++mr) {
            if (copies[(size_t)mr].empty()) continue;
            uint32_t prev = UINT32_MAX;
            std::vector<uint32_t> hs;
            for (int64_t q = off[(size_t)mr]; q < off[(size_t)mr + 1]; ++q) hs.push_back(head[nodes[(size_t)q]]);
            std::sort(hs.begin(), hs.end());
            for (uint32_t h : hs) {
                if (h != prev) by_node[h].insert(by_node[h].end(), copies[(size_t)mr].begin(), copies[(size_t)mr].end());
                prev = h;
            }
            std::vector<int64_t>& l = by_lca[head[lca[(size_t)mr]]];
            l.insert(l.end(), copies[(size_t)mr].begin(), copies[(size_t)mr].end());
        }
        write_node_list(c.output + ".mgsr.assignedReads.out", by_node);
        write_node_list(c.output + ".mgsr.assignedReadsLCANode.out", by_lca);
    }

    // --breadth-ratio (src/main.cpp:992-1013, calculateBreadthRatio, src/mgsr.cpp:6518-6584): a line per head node, with or without
    // reads, in the pre-order of the collapsed tree (= ascending DFS index of the heads); the header alone when no read was assigned
    void write_breadths() const {
        const std::string path = c.output + ".mgsr.breadths.out";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) die("cannot write " + path);
        fputs("NodeId\tTotalRefSeeds\tObservedBreadthCount\tObservedBreadthRatio\tTotalDepth\tMeanDepth\tExpectedBreadthRatio\tObservedToExpectedBreadthRatio\n", f);
        std::vector<uint64_t> total((size_t)n_nodes), observed((size_t)n_nodes), depth((size_t)n_nodes);
        check(pmx_meta_breadth(run.meta, total.data(), observed.data(), depth.data(), n_nodes), "the breadth of the nodes");
        for (uint32_t h = 0; n_written > 0 && h < (uint32_t)n_nodes; ++h) {
            if (head[h] != h) continue;
            const double t = (double)total[h];
            const double ratio = total[h] > 0 ? (double)observed[h] / t : 0.0, mean = total[h] > 0 ? (double)depth[h] / t : 0.0;
            const double expected = mean > 0 ? 1.0 - std::exp(-mean) : 0.0;
            fprintf(f, "%s\t%llu\t%llu\t%g\t%llu\t%g\t%g\t%g\n", ids_of_head(h).c_str(), (unsigned long long)total[h], (unsigned long long)observed[h], ratio,
                    (unsigned long long)depth[h], mean, expected, expected > 0 ? ratio / expected : 0.0);
        }
        fclose(f);
        say(c, "meta", path);
    }

    // ---- --align-reads (alignAssignedReads, src/main.cpp:615-717, called at :943-946), after write_node_lists: every head with at
    // least --min-num-align reads (negative: 0) gets those reads -- single-end, a mate 2 as sequenced, ascending FASTQ position --
    // aligned to its own ungapped genome: `<prefix>_mgsr_aligned/<sanitised id>.bam` (+ .bai), and the genomes in
    // `<prefix>_mgsr_aligned/reference.fa` as `>id` + lines of at most 80 bases.  Heads by ascending DFS index (the reference
    // iterates a hash map); the aligner is this library's, not bwa (DESIGN.md sections 4.3 and 7).  The assigned reads go to the
    // device once; a node's reads are one pmx_readset_select of that set.
    std::string al_dir;
    std::vector<uint32_t> al_todo;               // the qualifying heads, ascending
    int64_t al_skipped = 0;                      // heads with reads, but fewer than --min-num-align
    std::vector<std::string> al_seq, al_qual, al_name;   // the records of the FASTQ (a name ends at its first white space, as kseq reads it)
    pmx_readset* al_rs = nullptr;                // ... on the device, with their qualities
    FILE* al_fa = nullptr;                       // reference.fa: a node's text is written once every node before it has been
    std::vector<std::string> al_fa_text;
    std::vector<char> al_fa_ready;
    size_t al_fa_next = 0;
    std::mutex al_fa_mu;
    std::atomic<int64_t> al_done{0};

    static std::string sanitize(const std::string& id) {
        std::string out = id;
        for (char& ch : out)
            if (ch == '/' || ch == '\\' || isspace((unsigned char)ch)) ch = '_';
        return out;
    }

    // Reads: by_node, fq_read, the reads.  Leaves: al_todo / al_skipped, the directory with an empty reference.fa open, the
    // records of the FASTQ on the host and in al_rs.  Two qualifying heads with one file name end the run here.
    void align_reads_setup() {
        const size_t k = (size_t)std::max(c.min_num_align, 0);
        for (uint32_t h = 0; h < (uint32_t)n_nodes; ++h) {
            if (by_node[h].empty()) continue;
            if (by_node[h].size() < k) ++al_skipped;
            else al_todo.push_back(h);
        }
        std::vector<std::pair<std::string, uint32_t>> stems;
        for (uint32_t h : al_todo) stems.emplace_back(sanitize(pmx_index_node_id(run.idx, h)), h);
        std::sort(stems.begin(), stems.end());
        for (size_t i = 1; i < stems.size(); ++i)
            if (stems[i].first == stems[i - 1].first)
                die("--align-reads: the nodes '" + std::string(pmx_index_node_id(run.idx, stems[i - 1].second)) + "' and '" +
                    pmx_index_node_id(run.idx, stems[i].second) + "' would both be written to " + stems[i].first + ".bam");
        al_dir = c.output + "_mgsr_aligned";
        mkdirs(al_dir);
        const std::string fa_path = al_dir + "/reference.fa";
        al_fa = fopen(fa_path.c_str(), "w");
        if (!al_fa) die("cannot write " + fa_path);
        al_fa_text.resize(al_todo.size());
        al_fa_ready.assign(al_todo.size(), 0);
        if (al_todo.empty()) return;
        const Reads& rd = reads();
        std::string concat, quals;
        std::vector<int64_t> offs(1, 0);
        for (int64_t r : fq_read) {
            const size_t at = (size_t)rd.off[(size_t)r], len = (size_t)(rd.off[(size_t)r + 1] - rd.off[(size_t)r]);
            al_seq.emplace_back(rd.concat, at, len);
            al_qual.push_back(len > 0 && rd.quals[at] == '\0' ? std::string(len, 'I') : rd.quals.substr(at, len));   // (as write_fastq wrote them)
            std::string nm = rd.name(r);
            for (size_t i = 0; i < nm.size(); ++i)
                if (isspace((unsigned char)nm[i])) { nm.resize(i); break; }
            al_name.push_back(nm);
            concat += al_seq.back();
            quals += al_qual.back();
            offs.push_back((int64_t)concat.size());
        }
        check(pmx_readset_upload(run.ctx, concat.data(), offs.data(), (int64_t)fq_read.size(), &al_rs), "uploading the assigned reads");
        check(pmx_readset_set_qualities(run.ctx, al_rs, quals.data()), "attaching the qualities of the assigned reads");
    }

    // node i's text of reference.fa is known: write it, and what waited for it, in node order
    void publish_reference(size_t i, const std::string& id, const char* genome, int64_t len) {
        std::string text = ">" + id + "\n";
        for (int64_t at = 0; at < len; at += 80) { text.append(genome + at, (size_t)std::min<int64_t>(80, len - at)); text += '\n'; }
        std::lock_guard<std::mutex> lock(al_fa_mu);
        al_fa_text[i].swap(text);
        al_fa_ready[i] = 1;
        for (; al_fa_next < al_fa_text.size() && al_fa_ready[al_fa_next]; ++al_fa_next) {
            fwrite(al_fa_text[al_fa_next].data(), 1, al_fa_text[al_fa_next].size(), al_fa);
            std::string().swap(al_fa_text[al_fa_next]);
        }
    }

    // one qualifying head on `wctx`: its genome into reference.fa, its reads selected into `sel_w` and aligned by `al_w` (both made
    // on the first call, reused after), the records fetched, the BAM written.  -> a PMX code; pmx_last_error() says why
    int align_node(pmx_ctx* wctx, pmx_aligner*& al_w, pmx_readset*& sel_w, size_t i) {
        const uint32_t h = al_todo[i];
        const std::vector<int64_t>& idx = by_node[h];
        const int64_t n = (int64_t)idx.size();
        const std::string id = pmx_index_node_id(run.idx, h);
        thread_local std::string genome;   // (one reconstruction per node: score_candidate's way)
        if (genome.size() < 1024) genome.resize(1024);
        int64_t len = pmx_panman_node_genome(run.pm, (int64_t)h, &genome[0], (int64_t)genome.size());
        if (len > (int64_t)genome.size()) {
            genome.resize((size_t)len + (size_t)len / 64);
            len = pmx_panman_node_genome(run.pm, (int64_t)h, &genome[0], (int64_t)genome.size());
        }
        publish_reference(i, id, genome.data(), std::max<int64_t>(len, 0));
        if (len <= 0) {   // (the reference's aligner call fails on it: a warning, the node is not counted)
            fprintf(stderr, "panmap: warning: Alignment/BAM write failed for node %s\n", id.c_str());
            return PMX_OK;
        }
        int64_t bases = 0;
        for (int64_t j : idx) bases += (int64_t)al_seq[(size_t)j].size();
        const int mean_len = (int)(bases / std::max<int64_t>(n, 1));   // (of this node's reads: the reference's call sees only those)
        int rc = pmx_readset_select(wctx, al_rs, idx.data(), n, &sel_w);
        if (rc == PMX_OK) rc = pmx_readset_pack(wctx, sel_w);
        if (rc == PMX_OK) rc = al_w ? pmx_aligner_set_reference(wctx, al_w, genome.data(), len, mean_len) : pmx_aligner_create(wctx, genome.data(), len, mean_len, &al_w);
        if (rc == PMX_OK) rc = pmx_align_readset(wctx, al_w, sel_w, 0, 0);
        if (rc != PMX_OK) return rc;
        const int64_t words = pmx_align_cigar_words(wctx, al_w);
        if (words < 0) return (int)words;
        std::vector<pmx_aln_record> recs((size_t)std::max<int64_t>(n, 1));
        std::vector<uint32_t> arena((size_t)std::max<int64_t>(words, 1));
        rc = pmx_align_fetch(wctx, al_w, recs.data(), n, arena.data(), (int64_t)arena.size());
        if (rc != PMX_OK) return rc;
        std::vector<const char*> seq_p((size_t)n), qual_p((size_t)n), name_p((size_t)n);
        std::vector<int> lens((size_t)n);
        std::vector<align_pair_result_t> results((size_t)std::max<int64_t>(n, 1));
        for (int64_t q = 0; q < n; ++q) {
            const size_t j = (size_t)idx[(size_t)q];
            seq_p[(size_t)q] = al_seq[j].c_str(); qual_p[(size_t)q] = al_qual[j].c_str(); name_p[(size_t)q] = al_name[j].c_str(); lens[(size_t)q] = (int)al_seq[j].size();
            align_pair_result_t& out = results[(size_t)q];
            memset(&out, 0, sizeof(out));
            out.r1.pos = out.r2.pos = INT_MAX;
            const pmx_aln_record& r = recs[(size_t)q];
            if ((r.flags & 3) != 0 || !r.mapped) continue;   // (an invalid record is withheld: Sample::write_bam)
            out.mapped = 1;
            if (r.flags & PMX_ALN_HAS_ALN) {
                read_align_t& o = out.r1;
                o.pos = r.rs + 1; o.rs = r.rs; o.re = r.re; o.qs = r.qs; o.qe = r.qe;
                o.mapq = r.mapq; o.rev = r.rev; o.proper_frag = r.proper_frag; o.n_cigar = r.n_cigar;
                o.cigar = arena.data() + r.cigar_off;   // (points into the arena: nothing to free)
            }
        }
        rc = pmx_write_bam((al_dir + "/" + sanitize(id) + ".bam").c_str(), id.c_str(), len, (int)n, seq_p.data(), qual_p.data(), name_p.data(), lens.data(), results.data(), false);
        if (rc == PMX_OK) ++al_done;
        return rc;
    }

    // Work layout of Sample::refine(): the first node on the run's context, then a few workers, each with a context, an aligner
    // and a selected read set of its own, take the nodes from a counter; the first failure stops them all.
    // Leaves: the BAMs, reference.fa closed, the reference's closing line.
    void align_reads() {
        align_reads_setup();
        const int64_t n_todo = (int64_t)al_todo.size();
        pmx_aligner* al0 = nullptr;
        pmx_readset* sel0 = nullptr;
        std::atomic<int> failed{0};
        std::string fail_msg;
        if (n_todo > 0) {
            if (align_node(run.ctx, al0, sel0, 0) != PMX_OK) { failed = 1; fail_msg = pmx_last_error(); }
            int n_workers = 4;
            if (const char* e = getenv("PMX_ALIGN_READS_STREAMS")) n_workers = std::max(1, atoi(e));
            n_workers = (int)std::min<int64_t>(n_workers, std::max<int64_t>(n_todo - 1, 1));
            std::atomic<int64_t> next{1};
            std::mutex fail_mu;
            std::vector<std::thread> pool;
            for (int wk = 0; wk < n_workers && !failed.load() && n_todo > 1; ++wk)
                pool.emplace_back([&, wk]() {    // worker 0 goes on with the run's context, al0 and sel0; the others release what they made, on every path
                    pmx_ctx* wctx = run.ctx;
                    pmx_aligner* own_al = nullptr;
                    pmx_readset* own_sel = nullptr;
                    if (wk > 0 && pmx_ctx_create(run.dev, &wctx) != PMX_OK) {
                        std::lock_guard<std::mutex> lock(fail_mu);
                        if (!failed.exchange(1)) fail_msg = pmx_last_error();
                        return;
                    }
                    pmx_aligner*& al_w = wk == 0 ? al0 : own_al;
                    pmx_readset*& sel_w = wk == 0 ? sel0 : own_sel;
                    for (;;) {
                        const int64_t i = next.fetch_add(1);
                        if (i >= n_todo || failed.load()) break;
                        if (align_node(wctx, al_w, sel_w, (size_t)i) != PMX_OK) {
                            std::lock_guard<std::mutex> lock(fail_mu);
                            if (!failed.exchange(1)) fail_msg = pmx_last_error();
                            break;
                        }
                    }
                    if (wk > 0) {
                        if (own_al) pmx_aligner_free(wctx, own_al);
                        if (own_sel) pmx_readset_free(wctx, own_sel);
                        pmx_ctx_destroy(wctx);
                    }
                });
            for (auto& t : pool) t.join();
        }
        if (al0) pmx_aligner_free(run.ctx, al0);
        if (sel0) pmx_readset_free(run.ctx, sel0);
        if (al_rs) pmx_readset_free(run.ctx, al_rs);
        al_rs = nullptr;
        fclose(al_fa);
        al_fa = nullptr;
        if (failed.load()) die("aligning the assigned reads: " + fail_msg);
        say(c, "meta", "Aligned reads for " + std::to_string(al_done.load()) + " nodes (" + std::to_string(al_skipped) + " below minNumAlign=" +
                           std::to_string(std::max(c.min_num_align, 0)) + ")");
    }

    // the line that ends the mode: the FASTQ's name and the four tallies of write_fastq
    void report_assigned() const {
        say(c, "meta", fq_path + " (" + std::to_string(n_written) + " assigned, " + std::to_string(n_discarded) + " discarded, " + std::to_string(n_unmapped) +
                           " unmapped reads" +
                           (taxonomy.t ? ", " + std::to_string(n_over) + " spanning more than " + std::to_string(c.maximum_taxon_number) + " taxa" : std::string()) + ")");
    }

    // --write-ocranks (writeOCRanks, src/main.cpp:430-444): `<prefix>.overlapCoefficients.tsv`, one line per node of the index,
    // id <TAB> coefficient with six decimals <TAB> rank; by falling coefficient, ascending DFS index within a value; the rank
    // starts at 0 and goes up by one whenever the coefficient differs from the line before.  Every node, also under
    // --em-leaves-only.  Reads: the overlap coefficients set_reads left (--gpus N: the same on every rank).
    void write_ocranks() const {
        pmx_index_info info;
        check(pmx_index_get_info(run.idx, &info), "the index's size");
        std::vector<double> oc((size_t)info.n_nodes);
        check(pmx_meta_overlap_coefficients(run.meta, oc.data(), info.n_nodes), "the overlap coefficients");
        std::vector<uint32_t> by_oc(oc.size());
        std::iota(by_oc.begin(), by_oc.end(), 0u);
        std::stable_sort(by_oc.begin(), by_oc.end(), [&](uint32_t a, uint32_t b) { return oc[a] > oc[b]; });
        const std::string path = c.output + ".overlapCoefficients.tsv";
        std::ofstream out(path);
        if (!out.is_open()) die("cannot write " + path);
        out << std::fixed << std::setprecision(6);
        uint32_t rank = 0;
        double cur = oc.empty() ? 0.0 : oc[by_oc[0]];
        for (uint32_t v : by_oc) {
            if (oc[v] != cur) { cur = oc[v]; ++rank; }
            out << pmx_index_node_id(run.idx, v) << '\t' << oc[v] << '\t' << rank << '\n';
        }
        out.close();
        if (!out) die("cannot write " + path);
        say(c, "meta", path + " (" + std::to_string(oc.size()) + " nodes, " + std::to_string(oc.empty() ? 0 : rank + 1) + " ranks)");
    }

    // ---- the read-score reports of the abundance mode (writeMetaReadScores, src/main.cpp:446-466; the discard loop, :1229-1243).
    // One line per merged read that maps, by ascending merged index: index, copies, seedmers, best score over ALL nodes, the
    // number of active nodes that reach it, (filtered file only: OvermaximumTaxonNumber, always 0 in this mode,) the positions of
    // its copies in the input, ascending and comma-joined.  The filtered file lacks the reads whose best score is below
    // (int)(seedmers * --discard): the all-node maximum, as in the reference; which reads the EM keeps is pmx_meta_em's matter
    // (DESIGN.md section 4.3).

    // Leaves: rs_max / rs_nbest / rs_seedmers / rs_mult per merged read and rs_copies, the input positions of every merged read's copies.
    // One sample over --gpus N: every rank scores its rows, rank 0 gathers them and holds what the writers need.
    void score_all_nodes() {
        pmx_meta* m = run.meta;
        check(pmx_meta_read_best(run.ctx, m), "scoring the reads against every node");
        if (run.dist) {
            check(pmx_meta_read_best_gather(run.ctx, m, 0), "gathering the ranks' read scores");
            whole_raw_to_merged();
            if (pmx_dist_rank(run.dist) != 0) return;
        }
        n_merged = pmx_meta_num_reads(m);
        const size_t n = (size_t)std::max<int64_t>(n_merged, 1);
        rs_max.resize(n); rs_nbest.resize(n); rs_seedmers.resize(n); rs_mult.resize(n);
        check(pmx_meta_read_best_get(m, rs_max.data(), rs_nbest.data(), n_merged), "the reads' best scores");
        check(pmx_meta_read_info(m, rs_seedmers.data(), rs_mult.data(), n_merged), "the reads' seedmers");
        const int64_t n_raw = reads().n_reads;
        if (!run.dist) whole_raw_to_merged();
        rs_copies.assign((size_t)n_merged, std::vector<int64_t>());
        for (int64_t r = 0; r < n_raw; ++r)
            if (merged[(size_t)r] >= 0) rs_copies[(size_t)merged[(size_t)r]].push_back(r);
    }
    bool below_discard(int64_t r) const { return (int)rs_max[(size_t)r] < (int)((double)rs_seedmers[(size_t)r] * c.discard); }

    void write_read_scores(bool filtered) const {
        const std::string path = c.output + (filtered ? ".read_scores_info.filtered.tsv" : ".read_scores_info.unfiltered.tsv");
        std::ofstream out(path);
        if (!out.is_open()) die("cannot write " + path);
        out << "ReadIndex\tNumDuplicates\tTotalScore\tMaxScore\tNumMaxScoreNodes\t" << (filtered ? "OvermaximumTaxonNumber\t" : "") << "RawReadsIndices\n";
        int64_t n_lines = 0;
        for (int64_t r = 0; r < n_merged; ++r) {
            if (rs_max[(size_t)r] == 0 || (filtered && below_discard(r))) continue;
            const std::vector<int64_t>& copies = rs_copies[(size_t)r];
            out << r << '\t' << copies.size() << '\t' << rs_seedmers[(size_t)r] << '\t' << rs_max[(size_t)r] << '\t' << rs_nbest[(size_t)r] << '\t';
            if (filtered) out << "0\t";
            for (size_t j = 0; j < copies.size(); ++j) out << (j ? "," : "") << copies[j];
            out << '\n';
            ++n_lines;
        }
        out.close();
        if (!out) die("cannot write " + path);
        say(c, "meta", path + " (" + std::to_string(n_lines) + " reads)");
    }

    // the reference's three tallies over the merged reads (src/main.cpp:1240-1243)
    void report_read_scores() const {
        int64_t unmapped = 0, discarded = 0;
        for (int64_t r = 0; r < n_merged; ++r) {
            if (rs_max[(size_t)r] == 0) ++unmapped;
            else if (below_discard(r)) ++discarded;
        }
        say(c, "meta", std::to_string(unmapped) + " reads unmapped... ");
        say(c, "meta", std::to_string(discarded) + " reads discarded due to low parsimony score... ");
        say(c, "meta", std::to_string(n_merged - unmapped - discarded) + " reads mapped to nodes...");
    }

    // ---- the abundances.  Reads: the merged reads.  Leaves: the candidates scored and the EM's haplotypes in run.meta, on every rank.
    void estimate() {
        pmx_meta* m = run.meta;
        check(pmx_meta_score(run.ctx, m, c.top_oc, nullptr, 0), "scoring the reads against the candidate nodes");
        say(c, "meta", std::to_string(pmx_meta_num_reads(m)) + " distinct reads x " + std::to_string(pmx_meta_num_candidates(m)) + " candidate nodes");
        pmx_meta_params mp;
        memset(&mp, 0, sizeof(mp));
        mp.error_rate = 0.005; mp.em_convergence = c.em_convergence; mp.em_delta_threshold = c.em_delta; mp.prop_threshold = 0.005; mp.discard = c.discard;
        mp.em_max_iterations = c.em_max_iterations; mp.em_max_rounds = c.em_max_rounds;
        check(pmx_meta_em(run.ctx, m, &mp), "estimating the abundances");
    }

    // `<prefix>.mgsr.abundance.out`, one line per estimated haplotype: node id (+ the nodes merged into it, comma-joined) <TAB>
    // proportion with five decimals, by proportion
    void write_abundance() const {
        pmx_meta* m = run.meta;
        const std::string path = c.output + ".mgsr.abundance.out";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) die("cannot write " + path);
        const int64_t n_h = pmx_meta_num_haplotypes(m);
        if (n_h == 0) fprintf(stderr, "No reads remain for node scoring and EM after discarding low-score reads... Exiting... \n");   // src/main.cpp:1244-1247
        for (int64_t i = 0; i < n_h; ++i) {
            uint32_t node = 0;
            double prop = 0;
            int64_t n_mem = 0;
            check(pmx_meta_haplotype(m, i, &node, &prop, &n_mem, nullptr, 0), "haplotype");
            std::vector<uint32_t> mem((size_t)std::max<int64_t>(n_mem, 1));
            check(pmx_meta_haplotype(m, i, nullptr, nullptr, nullptr, mem.data(), (int64_t)mem.size()), "haplotype members");
            fprintf(f, "%s\t%.5f\n", joined_ids(run.idx, node, mem.data(), (size_t)n_mem).c_str(), prop);
        }
        fclose(f);
        say(c, "meta", path + " (" + std::to_string(n_h) + " haplotypes)");
    }
};

// one sample whose reads and shard are in hand, against the configured run; writer: this process writes the abundances (every
// rank of a sharded sample ends with them)
void meta_steps(MetaSample& s, bool writer) {
    s.set_reads();
    s.report_masks();
    if (s.c.filter_and_assign) {
        s.assign();
        if (!writer) return;   // (one sample over --gpus N: rank 0 gathered, writes and aligns alone; the others wait at the run's last barrier)
        s.write_fastq();
        s.write_node_lists();
        if (s.c.align_reads) s.align_reads();
        if (s.c.breadth_ratio) s.write_breadths();
        s.report_assigned();
    } else {
        const bool read_scores = s.c.read_scores_unfiltered || s.c.read_scores_filtered;
        if (writer && s.c.write_ocranks) s.write_ocranks();
        if (read_scores) s.score_all_nodes();
        if (writer && s.c.read_scores_unfiltered) s.write_read_scores(false);
        if (writer && read_scores) s.report_read_scores();
        s.estimate();
        if (writer) s.write_abundance();
        if (writer && s.c.read_scores_filtered) s.write_read_scores(true);
    }
}

int run_meta(const Config& c) {
    MetaRun mr(c);
    mr.refuse_options();
    const bool batch = !c.batch.empty();
    std::vector<BatchEntry> samples;
    if (batch) samples = read_samples(c.batch);
    mr.load_amplicons();
    mr.load_taxonomy();
    mr.build_indexes();
    int code = 0;
    if (!batch) {   // one sample, sharded over the ranks
        MetaSample s(mr, mr.c);
        s.read_reads();
        if (!mr.open_rank(c.gpus, true, &code)) { mr.run.close(); return code; }
        mr.configure();
        s.take_shard(mr.rk.rank, mr.rk.world);
        s.set_amplicons();
        meta_steps(s, mr.rk.rank == 0);
        mr.run.close();
        return 0;
    }
    // --batch: the samples dealt to ranks that never meet, as in real_main; the rank that takes a sample reads its reads
    fprintf(stderr, "Batch mode: %zu samples\n", samples.size());
    fflush(stderr);
    Deal* deal = Deal::map();
    if (!mr.open_rank((int)std::min<size_t>((size_t)c.gpus, samples.size()), false, &code)) {
        mr.run.close();
        return end_batch(deal, code, samples.size(), "done");
    }
    mr.configure();
    run_dealt(samples, *deal, [&](const BatchEntry& e) {
        Config sc = mr.c;
        sc.reads1 = e.reads1; sc.reads2 = e.reads2; sc.output = e.prefix; sc.quiet = true;
        MetaSample s(mr, sc);
        s.read_reads();
        s.take_shard(0, 1);
        meta_steps(s, true);
        return c.filter_and_assign ? std::to_string(s.n_written) + " assigned reads" : std::to_string(pmx_meta_num_haplotypes(mr.run.meta)) + " haplotypes";
    });
    const int rc = mr.rk.world == 1 ? end_batch(deal, 0, samples.size(), "done") : 0;
    mr.run.close();
    return rc;
}

int real_main(int argc, char** argv) {
    signal(SIGINT, on_sigint);
    Config c = parse(argc, argv);
    if (c.s <= 0 || c.s > c.k) die("Invalid syncmer s=" + std::to_string(c.s) + " (must be in 1..k, k=" + std::to_string(c.k) + ")");
    if (c.t < 0 || c.t > c.k - c.s) die("Invalid syncmer offset=" + std::to_string(c.t) + " (must be in 0..k-s = 0.." + std::to_string(c.k - c.s) + ")");
    if (c.aligner != "minimap2") die("aligner '" + c.aligner + "' is not implemented in this build (minimap2 only)");
    int stop = c.stop == "index" ? 0 : c.stop == "place" ? 1 : c.stop == "align" ? 2 : c.stop == "genotype" ? 3 : c.stop == "consensus" ? 4 : -1;
    if (stop < 0) die("--stop expects index|place|align|genotype|consensus");
    if (c.index.empty()) c.index = c.index_out.empty() ? c.panman + ".idx" : c.index_out;
    else if (!exists(c.index)) die("index file not found: " + c.index + " (--index expects a pre-built index; use --index-out to build at a custom path)");
    if (c.output.empty()) c.output = derive_prefix(c);
    if (!c.batch.empty() && !c.reads1.empty()) die("--batch takes the read files from the batch file, not from the command line");
    if (c.gpus < 1) die("--gpus expects a positive number");
    if (!c.batch.empty() && c.gpus > 16) die("--batch deals its samples to at most 16 ranks: --gpus " + std::to_string(c.gpus) + " is too many");

    if (c.breadth_ratio && !c.filter_and_assign) die("option --breadth-ratio is not accepted without --filter-and-assign");
    if (!c.align_options.empty() && !c.filter_and_assign) die("option " + c.align_options[0] + " is not accepted without --filter-and-assign");
    if (!c.align_options.empty() && !c.align_reads) die("option --min-num-align is not accepted without --align-reads");
    if (c.filter_and_assign && !c.meta) die("--filter-and-assign needs --meta");
    if (!c.mask_options.empty() && !c.meta) die("option " + c.mask_options[0] + " is not accepted without --meta");
    if (!c.em_options.empty() && !c.meta) die("option " + c.em_options[0] + " is not accepted without --meta");
    if (c.meta) {   // the reference's --meta has no HPC
        pmx_index_info h;
        if (c.hpc) die("--meta has no homopolymer-compressed form: drop --hpc");
        if (exists(c.index) && pmx_index_read_header(c.index.c_str(), &h, nullptr) == PMX_OK && h.hpc) die("--meta cannot use the homopolymer-compressed index " + c.index);
        return run_meta(c);
    }
    // the batch file is read, and found wanting, before anything is built or opened
    std::vector<BatchEntry> samples;
    if (!c.batch.empty() && stop != 0) samples = read_samples(c.batch);

    // ------------------------------------------------------------------------------------------------ index
    Run run;
    run.panman_path = c.panman;
    bool idx_hpc = false;
    if (exists(c.index) && !c.force_reindex && cached_index_usable(c, &idx_hpc)) {
        if (c.hpc && !idx_hpc) die(std::string(kHpcNeedsIndex) + "; " + c.index + " is not one");
        check(pmx_index_load(c.index.c_str(), &run.idx), "loading the index");
        say(c, "index", c.index + " (cached)" + (idx_hpc ? ", homopolymer-compressed" : ""));
    } else {
        if (c.hpc) die(kHpcNeedsIndex);
        if (!run.panman()) die(std::string("opening the PanMAN: ") + pmx_last_error());
        check(pmx_index_build(run.pm, c.k, c.s, c.t, c.l, c.open_syncmer ? 1 : 0, c.flank_mask, &run.idx), "building the index");
        check(pmx_index_save(run.idx, c.index.c_str(), c.zstd_level, c.index_uncompressed ? 1 : 0), "writing the index");
        say(c, "index", c.index + " (built)");
    }
    if (stop == 0 || (c.reads1.empty() && c.batch.empty())) { run.close(); return 0; }

    // ------------------------------------------------------------------------------------------------ --gpus N
    // forked HERE: the index (and the PanMAN, when it was opened) is in memory and nothing has touched a GPU yet.  One sample
    // is sharded over the ranks, which meet through RCCL; the samples of --batch are dealt to ranks that never meet, and no
    // more of those than there are samples
    const bool batch = !c.batch.empty();
    Ranks rk;
    Deal* deal = nullptr;
    if (batch) {
        fprintf(stderr, "Batch mode: %zu samples\n", samples.size());
        fflush(stderr);
        deal = Deal::map();
    }
    if (c.gpus > 1) {
        int code = 0;
        const int n_ranks = batch ? (int)std::min<size_t>((size_t)c.gpus, samples.size()) : c.gpus;
        if (!fork_ranks(n_ranks, rk, &code, !batch)) {
            run.close();
            return batch ? end_batch(deal, code, samples.size(), "placed") : code;
        }
        if (rk.rank > 0) c.quiet = true;
    }

    // ------------------------------------------------------------------------------------------------ samples
    run.dev = rank_device(rk);
    check(pmx_ctx_create(run.dev, &run.ctx), "opening the GPU");
    if (!batch) run.dist = join_ranks(run.ctx, rk);
    check(pmx_place_create(run.ctx, run.idx, &run.pl), "uploading the index");
    int rc = 0;
    if (!batch) run_sample(c, stop, run);
    else {
        // runBatchPlacement (src/main.cpp:1464-1666): the samples this process takes, one after the other against the index
        // that stays on the device; one line per sample on stderr, a failed sample does not stop the batch.  A rank exits 0
        // whatever its samples did: the counts are in the shared block, and the parent reports them
        run_dealt(samples, *deal, [&](const BatchEntry& e) {
            Config sc = c;
            sc.reads1 = e.reads1; sc.reads2 = e.reads2; sc.output = e.prefix; sc.quiet = true;
            return run_sample(sc, stop, run);
        });
        if (rk.world == 1) rc = end_batch(deal, 0, samples.size(), "placed");
    }
    run.close();
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return real_main(argc, argv);
    } catch (const Fatal& f) {
        fprintf(stderr, "panmap: error: %s\n", f.msg.c_str());
        return f.code;
    }
}
