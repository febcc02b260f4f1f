// options.hpp -- `movi query` / `movi view` command line, mirroring the reference's
// flag table (src/movi_parser.cpp:82-223, handling :340-439) and defaults
// (include/movi_options.hpp:225-294) for the actions this engine implements.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace movi_host {

struct Options {
    std::string command;          // "query" | "view" | "null" | "plan" | "build" | "rlbwt" | "build-SA" | "color"
    std::string index_dir;        // -i / --index
    std::string read_file;        // -r / --read ("-" = stdin)
    std::string out_file;         // -o / --out-file
    std::string bpf_file;         // view --bpf
    std::string ref_file;         // null --gen-reads -f/--fasta; build -f/--fasta
    std::string index_type = "regular-thresholds";   // build --type (DEFAULT_INDEX_TYPE, src/movi_launcher.cpp:17)
    bool separators = false;      // build --separators
    bool preprocessed = false;    // build --preprocessed: REF.bwt.heads + REF.bwt.len (+ REF.thr_pos) instead of a FASTA, built on the GPU
    bool gpu_build = false;       // build --gpu-build: suffix array, BWT, LCP and thresholds of the FASTA's text on the GPU, then the table there too
    bool verify = false;          // build --gpu-build --verify: the builder's verify stage (src/movi_parser.cpp:105)
    bool keep = false;            // build --gpu-build --keep: REF.bwt.heads, REF.bwt.len and REF.thr_pos stay beside the FASTA (:113)
    std::string bwt_file;         // rlbwt --bwt-file
    bool gen_reads = false;       // null --gen-reads
    bool pml = true;              // default query type (movi_options.hpp:243)
    bool count = false;
    bool zml = false;             // --zml: Ziv-Merhav cross parse lengths, same outputs as PML
    bool mem = false;             // --mem: maximal exact matches (src/mem_finder.cpp), one line per MEM
    bool kmer = false;            // --kmer: k-mer presence (src/sequitur.cpp:322-421), one line per read
    bool kmer_occ = false;        // --kmer-occ: occurrences of every k-mer in the text (include/movi_hip.h: movi_kmer_occ_host), one line per read
    bool locate = false;          // --locate: text positions of the count / MEM hits beside the ordinary file (needs INDEX/ssa.movi: build-SA)
    uint32_t max_occ = 100;       // --max-occ: positions listed per match at most (1 .. 2^32 - 1)
    bool sa_entries = false;      // --sa-entries: one suffix-array entry per base beside the PML file (needs INDEX/ssa.movi: build-SA)
    bool multi_classify = false;  // --multi-classify: PML walk + document scoring, one report line per read (needs INDEX/doc_sets_flat.bin: movi color)
    uint32_t min_len = 1;         // --min-len (uint8_t, movi_options.hpp: min_match_len)
    bool report_all = false;      // --report-all
    float min_diff_frac = 0.05f;  // --min-diff-frac
    float min_score_frac = 0.0f;  // --min-score-frac (non-zero turns the min-diff-frac mode off)
    bool color = false;           // build --color: ref.fa.doc_offsets + the colour step
    uint64_t sample_rate = 100;   // build-SA --sample-rate (movi_options.hpp: SA_sample_rate)
    uint32_t k = 31;              // -k / --k-length (movi_options.hpp:254)
    uint32_t min_mem_length = 25; // -l / --min-mem-length (movi_options.hpp:255)
    long ftab_k = -1;             // --ftab-k K: the engine's interval table at min(K, 12) ("ftab_k"); -1 = not given
    bool classify = false;
    bool filter = false;
    bool invert = false;
    bool write_stdout = false;    // --stdout
    bool no_output = false;
    bool prefetch = true;         // -n / --no-prefetch clears it (affects record order only)
    bool reverse = false;
    bool verbose = false;
    bool no_header = false;       // view: headerless BPF
    bool small_bpf = false, large_bpf = false;
    int ignore_illegal_chars = 0; // 1 = substitute 'A'; 2 (random) is rejected
    size_t strands = 16;
    size_t threads = 1;
    size_t bin_width = 150;
    int gpus = 1;                 // extension: --gpus N shards the reads across N devices
    bool logs = false;            // --logs: <prefix>.costs / .scans / .fastforwards next to the PML output (src/utils.cpp:376-382)
    bool gpus_given = false;      //   (given explicitly, N == 1 included: the index goes through the RCCL replication path)
    int device = 0;               // extension: --device D
    int ahead_rows = -1;          // extension: --ahead-rows 0|1: look-ahead rows off / built whatever the device's free memory says (default: the engine's policy)
    long seg_len = -1;            // extension: --seg-len N: segment length of the segment-parallel long-read walk (0 = off; default: the engine's)

    // derived predicates, same names as the reference (movi_options.hpp:57-58)
    bool write_output_allowed() const { return !no_output && !filter; }
    bool write_stdout_enabled() const { return write_stdout && !classify; }
    bool ml() const { return pml || zml; }                                // per-base matching lengths
    std::string query_type() const { return kmer_occ ? "kmer_occ" : kmer ? "kmers" : mem ? "mem" : count ? "count" : (zml ? "zml" : "pml"); }   // src/utils.cpp:47-67
};

struct UsageError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// Throws UsageError with the reference's message texts where they exist.
Options parse_args(int argc, char **argv);
std::string usage();
int run_build(const Options &o);  // build_cmd.cpp (writes DIR/ref.fa.doc_offsets too when o.color; --preprocessed: from a run-length BWT; --gpu-build: from the FASTA on the GPU)
int run_rlbwt(const Options &o);  // build_cmd.cpp

}  // namespace movi_host
