#include "options.hpp"

#include <cerrno>
#include <cstdlib>
#include <map>
#include <set>

namespace movi_host {

namespace {

struct Spec {
    const char *long_name;
    char short_name;     // 0 = none
    bool takes_value;
};

// Flags of the actions we serve (src/movi_parser.cpp:82-223).  Flags of the reference that
// select features outside this engine's scope are recognised so that the error is explicit.
const Spec kSpecs[] = {
    {"index", 'i', true},        {"read", 'r', true},       {"out-file", 'o', true},
    {"threads", 't', true},      {"strands", 's', true},    {"pml", 0, false},
    {"count", 0, false},         {"classify", 0, false},    {"filter", 0, false},
    {"invert", 'v', false},      {"stdout", 0, false},      {"no-output", 0, false},
    {"no-prefetch", 'n', false}, {"reverse", 0, false},     {"verbose", 0, false},
    {"bin-width", 0, true},      {"ignore-illegal-chars", 0, true},
    {"bpf", 0, true},            {"small-bpf", 0, false},   {"large-bpf", 0, false},
    {"no-header", 0, false},     {"help", 'h', false},      {"gpus", 0, true},
    {"device", 0, true},         {"type", 0, true},         {"debug", 'd', false},
    {"logs", 0, false},          {"mmap", 0, false},        {"gen-reads", 0, false},
    {"fasta", 'f', true},          {"separators", 0, false},  {"seg-len", 0, true},
    {"ahead-rows", 0, true},        {"sample-rate", 0, true},
    {"gpu-build", 0, false},     {"verify", 0, false},      {"keep", 0, false},   // build on the GPU from the FASTA; the reference's --verify / --keep (src/movi_parser.cpp:105, :113)
    {"preprocessed", 0, false},  {"bwt-file", 0, true},     // build from a run-length BWT; movi rlbwt (src/movi_parser.cpp:112, :202-203)
    // Movi Color, default colour mode (src/movi_parser.cpp:119-121, 164-179, 193-199)
    {"multi-classify", 0, false}, {"min-len", 0, true},     {"report-all", 0, false},
    {"min-diff-frac", 0, true},  {"min-score-frac", 0, true}, {"color", 0, false},
    // ... and the flags of its other modes: recognised, refused by name
    {"full", 0, false},          {"compress", 0, false},    {"freq-compress", 0, false},
    {"tree-compress", 0, false}, {"color-vectors", 0, false}, {"pvalue-scoring", 0, false},
    {"early-stop", 0, false},    {"report-colors", 0, false}, {"report-color-ids", 0, false},
    {"color-move-rows", 0, false},
    // recognised but unsupported query types / features
    {"zml", 0, false},           {"mem", 0, false},         {"rpml", 0, false},
    {"kmer", 0, false},          {"kmer-count", 0, false},  {"sa-entries", 0, false},
    {"kmer-occ", 0, false},      // occurrences per k-mer: this engine's own query (not the reference's --kmer-count)
    {"locate", 0, false},        {"max-occ", 0, true},      // text positions of count / MEM hits: this engine's own (include/movi_hip.h)
    {"ftab-k", 0, true},         {"multi-ftab", 0, false},
    {"k-length", 'k', true},     {"min-mem-length", 'l', true},
};

const Spec *find_long(const std::string &n) {
    for (const Spec &s : kSpecs)
        if (n == s.long_name) return &s;
    return nullptr;
}
const Spec *find_short(char c) {
    for (const Spec &s : kSpecs)
        if (s.short_name && s.short_name == c) return &s;
    return nullptr;
}

float to_float(const std::string &name, const std::string &v) {
    char *end = nullptr;
    const float x = std::strtof(v.c_str(), &end);
    if (v.empty() || (end && *end)) throw UsageError("Argument '" + v + "' failed to parse for option '" + name + "'");
    return x;
}

// The colour modes this engine does not serve: each refusal names its flag
void refuse_color_modes(const std::map<std::string, std::vector<std::string>> &seen) {
    for (const char *bad : {"full", "compress", "freq-compress", "tree-compress", "color-vectors", "pvalue-scoring", "early-stop",
                            "report-colors", "report-color-ids", "color-move-rows"})
        if (seen.count(bad))
            throw UsageError(std::string("--") + bad + " is not supported by the MI355X engine: Movi Color is served in its default colour mode only "
                             "(flat colour table, one document set per run)");
}

long to_int(const std::string &name, const std::string &v) {
    char *end = nullptr;
    long x = std::strtol(v.c_str(), &end, 10);
    if (v.empty() || (end && *end)) throw UsageError("Argument '" + v + "' failed to parse for option '" + name + "'");
    return x;
}

}  // namespace

std::string usage() {
    return "movi (MI355X engine): movi query -i DIR -r FILE|- [-o PREFIX] [--pml|--zml|--count] [--classify] [--filter [-v]]\n"
           "                      [--stdout] [--no-output] [-s N] [-t N] [-n] [--reverse] [--bin-width N] [--ftab-k K]\n"
           "                      [--ignore-illegal-chars 1] [--gpus N] [--device D] [--seg-len N] [--ahead-rows 0|1] [--verbose]\n"
           "       movi query -i DIR -r FILE|- --mem --ftab-k K [-l MIN_MEM_LENGTH] [-o PREFIX] [--stdout] [--no-output]\n"
           "                      [--reverse] [--ignore-illegal-chars 1] [--gpus N] [--device D]\n"
           "       movi query -i DIR -r FILE|- --kmer [-k K] [--ftab-k K'] [-o PREFIX] [--stdout] [--no-output]\n"
           "                      [--reverse] [--ignore-illegal-chars 1] [--gpus N] [--device D]   (--kmer-count, --rpml: not supported)\n"
           "       movi query -i DIR -r FILE|- --kmer-occ [-k K] [--ftab-k K'] ...   (occurrences of every k-mer in the text -> <prefix>.kmer_occ.<k>)\n"
           "       movi query -i DIR -r FILE|- --count|--mem ... --locate [--max-occ N]   (text positions of the hits -> <prefix>.matches.locs /\n"
           "                      <prefix>.mems.locs, at most N per match, default 100; after build-SA)\n"
           "       movi query -i DIR -r FILE|- --sa-entries [-o PREFIX] [--no-output] ...   (PML + <prefix>.sa_entries.bpf; after build-SA)\n"
           "       movi query -i DIR -r FILE|- --multi-classify -o REPORT|--stdout [--min-len N] [--report-all [--min-diff-frac F | --min-score-frac F]]\n"
           "                      [--no-output] [--reverse] [--gpus N] [--device D]   (after movi color; default colour mode only)\n"
           "       movi build-SA -i DIR [--sample-rate N] [--device D]\n"
           "       movi color -i DIR [--device D]   (DIR/ref.fa.doc_offsets [+ ref.fa.doc_ids] -> DIR/doc_sets_flat.bin)\n"
           "       movi view --bpf FILE\n"
           "       movi null -i DIR [--gen-reads -f REF.fasta] [--pml|--zml]\n"
           "       movi build -i DIR -f REF.fasta [--type regular-thresholds|blocked-thresholds|sampled-thresholds|regular|blocked|sampled]\n"
           "                  [--separators] [--color]\n"
           "       movi build -i DIR -f REF.fasta --gpu-build [--type ...] [--separators] [--color] [--device D] [--verify] [--keep]\n"
           "                  (suffix array, BWT, LCP and thresholds on the GPU: texts up to 2^32 - 2^20 characters; --verify checks them there;\n"
           "                  --keep writes REF.fasta.bwt.heads, .bwt.len and .thr_pos for a later --preprocessed build of another type)\n"
           "       movi build -i DIR -f REF --preprocessed [--type ...] [--device D]   (REF.bwt.heads + REF.bwt.len [+ REF.thr_pos] -> DIR/index.movi,\n"
           "                  built on the GPU; --separators is recognised from the alphabet)\n"
           "       movi rlbwt --bwt-file FILE   (FILE -> FILE.heads + FILE.len)\n";
}

Options parse_args(int argc, char **argv) {
    Options o;
    std::map<std::string, std::vector<std::string>> seen;
    std::vector<std::string> positional;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            std::string name = a.substr(2), val;
            bool has_val = false;
            size_t eq = name.find('=');
            if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
            const Spec *s = find_long(name);
            if (!s) throw UsageError("Option '" + name + "' does not exist");
            if (s->takes_value && !has_val) {
                if (i + 1 >= argc) throw UsageError("Option '" + name + "' is missing an argument");
                val = argv[++i];
            }
            seen[s->long_name].push_back(val);
        } else if (a.size() >= 2 && a[0] == '-' && a != "-") {
            // short options: -t1, -t 1, grouped booleans -nv
            for (size_t p = 1; p < a.size(); p++) {
                const Spec *s = find_short(a[p]);
                if (!s) throw UsageError(std::string("Option '") + a[p] + "' does not exist");
                if (s->takes_value) {
                    std::string val = a.substr(p + 1);
                    if (val.empty()) {
                        if (i + 1 >= argc) throw UsageError(std::string("Option '") + s->long_name + "' is missing an argument");
                        val = argv[++i];
                    }
                    seen[s->long_name].push_back(val);
                    break;
                }
                seen[s->long_name].push_back("");
            }
        } else {
            positional.push_back(a);
        }
    }
    auto has = [&](const char *n) { return seen.count(n) > 0; };
    auto val = [&](const char *n) { return seen[n].back(); };
    if (has("help") || positional.empty()) { o.command = "help"; return o; }
    o.command = positional[0];
    o.verbose = has("verbose");
    o.logs = has("logs");
    o.no_header = has("no-header");
    if (o.command == "query") {
        // src/movi_parser.cpp:341, :431-434
        if (seen["index"].size() != 1 || seen["read"].size() != 1)
            throw UsageError("Please include one index directory and one read file.");
        o.index_dir = val("index");
        o.read_file = val("read");
        if (has("out-file")) o.out_file = val("out-file");
        for (const char *bad : {"rpml", "kmer-count", "multi-ftab"})
            if (has(bad))
                throw UsageError(std::string("--") + bad + " is not supported by the MI355X engine (PML, ZML, count, MEM and "
                                 "k-mer presence queries, --sa-entries and --multi-classify with PML, only)");
        refuse_color_modes(seen);
        // --mmap (src/movi_parser.cpp: "Use memory mapping to read the index") is accepted and implied: movi_index_load
        // always maps the file and uploads the rows straight from the page cache
                if (has("bin-width")) o.bin_width = (size_t)to_int("bin-width", val("bin-width"));
        // movi_parser.cpp:353-355 applies set_count, set_zml, set_pml in this order and each setter
        // clears the other query types (movi_options.hpp:108-110), so the last one applied wins
        // (the "only specify count or pml" check at :407-410 can never fire)
        // (set_kmer, :350, then set_mem, :352, come first: --kmer or --mem followed by a later one of the list is that other query)
        // (--kmer-occ is applied where --kmer is and wins over it: `--kmer --kmer-occ` is the occurrence query)
        if (has("kmer")) { o.kmer = true; o.pml = false; o.count = false; o.zml = false; o.mem = false; }
        if (has("kmer-occ")) { o.kmer_occ = true; o.kmer = false; o.pml = false; o.count = false; o.zml = false; o.mem = false; }
        if (has("mem")) { o.mem = true; o.pml = false; o.count = false; o.zml = false; o.kmer = false; o.kmer_occ = false; }
        if (has("count")) { o.count = true; o.pml = false; o.zml = false; o.mem = false; o.kmer = false; o.kmer_occ = false; }
        if (has("zml")) { o.zml = true; o.pml = false; o.count = false; o.mem = false; o.kmer = false; o.kmer_occ = false; }
        if (has("pml")) { o.pml = true; o.count = false; o.zml = false; o.mem = false; o.kmer = false; o.kmer_occ = false; }
        if (has("k-length")) {
            const long v = to_int("k-length", val("k-length"));
            if (v < 0 || v > 0xFFFFFFFFl) throw UsageError("Argument '" + val("k-length") + "' failed to parse for option 'k-length'");
            o.k = (uint32_t)v;
        }
        if (has("min-mem-length")) {
            const long v = to_int("min-mem-length", val("min-mem-length"));
            if (v < 0 || v > 0xFFFFFFFFl) throw UsageError("Argument '" + val("min-mem-length") + "' failed to parse for option 'min-mem-length'");
            o.min_mem_length = (uint32_t)v;
        }
        if (has("ftab-k")) {
            o.ftab_k = to_int("ftab-k", val("ftab-k"));
            if (o.ftab_k < 0) throw UsageError("Argument '" + val("ftab-k") + "' failed to parse for option 'ftab-k'");
        }
        o.classify = has("classify");
        o.filter = has("filter");
        if (o.filter) o.classify = true;                          // set_filter(), movi_options.hpp:122-125
        o.invert = has("invert");
        o.reverse = has("reverse");
        if (has("ignore-illegal-chars")) {
            long v = to_int("ignore-illegal-chars", val("ignore-illegal-chars"));
            if (v != 1 && v != 2)
                throw UsageError("ignore-illegal-chars should be either 1 (set illegal chars to 'A') or 2 (set illegal chars to a random char).");
            if (v == 2)
                throw UsageError("--ignore-illegal-chars 2 (random substitution) is not reproducible and is not supported; use 1");
            o.ignore_illegal_chars = (int)v;
        }
        if (has("no-prefetch")) o.prefetch = false;
        if (has("strands")) o.strands = (size_t)to_int("strands", val("strands"));
        if (has("threads")) o.threads = (size_t)to_int("threads", val("threads"));
        if (o.strands == 0) o.strands = 1;
        o.write_stdout = has("stdout");
        o.no_output = has("no-output");
        if (has("gpus")) { o.gpus = (int)to_int("gpus", val("gpus")); o.gpus_given = true; }
        if (has("device")) o.device = (int)to_int("device", val("device"));
        if (has("seg-len")) o.seg_len = (long)to_int("seg-len", val("seg-len"));
        if (has("ahead-rows")) {
            o.ahead_rows = (int)to_int("ahead-rows", val("ahead-rows"));
            if (o.ahead_rows < 0 || o.ahead_rows > 1) throw UsageError("--ahead-rows must be 0 or 1");
        }
        if (o.gpus < 1) throw UsageError("--gpus must be >= 1");
        if (o.classify && o.count) throw UsageError("--classify needs PML or ZML queries");
        if (has("sample-rate")) throw UsageError("--sample-rate belongs to build-SA: a query takes the rate from ssa.movi");
        if (o.kmer_occ) {
            if (o.classify || o.logs || has("sa-entries") || has("multi-classify"))
                throw UsageError("--kmer-occ cannot be combined with --classify, --filter, --logs, --sa-entries or --multi-classify");
            if (o.k == 0) throw UsageError("-k / --k-length must be at least 1");
            o.prefetch = false;                                   // file order, as --kmer
        }
        o.locate = has("locate");
        if (o.locate) {
            if (!o.count && !o.mem) throw UsageError("--locate reports the text positions of count or MEM hits: it needs --count or --mem");
            if (o.classify || o.logs) throw UsageError("--locate cannot be combined with --classify, --filter or --logs");
        }
        if (has("max-occ")) {
            if (!o.locate) throw UsageError("--max-occ belongs to --locate");
            const std::string &mv = val("max-occ");
            char *end = nullptr;
            errno = 0;
            const unsigned long long v = std::strtoull(mv.c_str(), &end, 10);
            if (mv.empty() || mv[0] < '0' || mv[0] > '9' || (end && *end) || errno || v < 1 || v > 0xFFFFFFFFull)
                throw UsageError("--max-occ must be between 1 and 4294967295");
            o.max_occ = (uint32_t)v;
        }
        o.sa_entries = has("sa-entries");
        if (o.sa_entries) {
            // (the reference opens an empty .sa_entries.bpf beside the other query types' files: only query_pml records entries)
            if (!o.pml) throw UsageError("--sa-entries reports the positions of the PML walk: it cannot be combined with --zml, --count, --mem or --kmer");
            if (o.classify || o.logs) throw UsageError("--sa-entries cannot be combined with --classify, --filter or --logs");
        }
        o.multi_classify = has("multi-classify");
        if (has("min-len")) {                                     // cxxopts::value<uint8_t>, src/movi_parser.cpp:172
            const long v = to_int("min-len", val("min-len"));
            if (v < 0 || v > 255) throw UsageError("Argument '" + val("min-len") + "' failed to parse for option 'min-len'");
            o.min_len = (uint32_t)v;
        }
        o.report_all = has("report-all");
        if (has("min-diff-frac")) o.min_diff_frac = to_float("min-diff-frac", val("min-diff-frac"));
        if (has("min-score-frac")) o.min_score_frac = to_float("min-score-frac", val("min-score-frac"));
        if (o.multi_classify) {
            if (!o.pml || o.sa_entries)
                throw UsageError("--multi-classify scores the PML walk: it cannot be combined with --zml, --count, --mem, --kmer or --sa-entries");
            if (o.classify || o.logs) throw UsageError("--multi-classify cannot be combined with --classify, --filter or --logs");
            if (o.out_file.empty() && !o.write_stdout && !o.no_output)
                throw UsageError("--multi-classify writes its report to the file given with -o / --out-file (or to --stdout)");
        } else if (o.report_all || has("min-len") || has("min-diff-frac") || has("min-score-frac")) {
            throw UsageError("--min-len, --report-all, --min-diff-frac and --min-score-frac belong to --multi-classify");
        }
        if (o.kmer) {
            if (o.classify || o.logs) throw UsageError("--kmer cannot be combined with --classify, --filter or --logs");
            if (o.k == 0) throw UsageError("-k / --k-length must be at least 1");
            o.prefetch = false;                                   // movi_parser.cpp:350: file order
        }
        if (o.mem) {                                              // src/movi.cpp:235-247
            if (o.classify || o.logs) throw UsageError("--mem cannot be combined with --classify, --filter or --logs");
            if (o.ftab_k <= 0)
                throw UsageError("MEM finding requires ftab. Please build the ftab using the ./movi ftab --ftab-k <k>, then pass "
                                 "--ftab-k <k> to the query step. (MEM finding without --ftab-k is not supported.)");
            o.prefetch = false;                                   // MEM finding does not support prefetching: file order
        }
    } else if (o.command == "plan") {
        // host-only helper (no GPU): prints how the reads are batched and in which order
        // their records will be emitted, one `batch<TAB>id<TAB>length` line per read.
        if (seen["read"].size() != 1) throw UsageError("Please include one read file.");
        o.read_file = val("read");
        if (has("no-prefetch")) o.prefetch = false;
        if (has("strands")) o.strands = (size_t)to_int("strands", val("strands"));
        if (o.strands == 0) o.strands = 1;
    } else if (o.command == "null") {
        // src/movi_parser.cpp:524-541
        if (seen["index"].size() != 1) throw UsageError("Please specify the index directory file.");
        o.index_dir = val("index");
        if (has("gen-reads")) {
            o.gen_reads = true;
            if (!has("fasta")) throw UsageError("Please specify the reference fasta file.");
            o.ref_file = val("fasta");
        }
        if (has("zml")) { o.zml = true; o.pml = false; }
        if (has("pml")) { o.pml = true; o.zml = false; }
        if (has("device")) o.device = (int)to_int("device", val("device"));
    } else if (o.command == "build") {
        // src/movi_parser.cpp:441-470: one index directory and one reference
        if (seen["index"].size() != 1) throw UsageError("Please specify the index directory file.");
        if (seen["fasta"].size() != 1) throw UsageError("Please specify the reference fasta file.");
        o.index_dir = val("index");
        o.ref_file = val("fasta");
        if (has("type")) o.index_type = val("type");
        o.separators = has("separators");
        o.color = has("color");                                   // src/movi_parser.cpp:119-121
        refuse_color_modes(seen);
        if (has("device")) o.device = (int)to_int("device", val("device"));
        o.preprocessed = has("preprocessed");                     // src/movi_parser.cpp:289-291
        if (o.preprocessed && o.color)
            throw UsageError("--color cannot be combined with --preprocessed: the document offsets come from the FASTA, which is not read");
        o.gpu_build = has("gpu-build");
        o.verify = has("verify");
        o.keep = has("keep");
        if (o.gpu_build && o.preprocessed)
            throw UsageError("--gpu-build cannot be combined with --preprocessed: one builds from the FASTA, the other from a run-length BWT");
        if ((o.verify || o.keep) && !o.gpu_build)
            throw UsageError(std::string(o.verify ? "--verify" : "--keep") + " belongs to --gpu-build");
    } else if (o.command == "rlbwt") {
        // src/movi_parser.cpp:440-446
        if (seen["bwt-file"].size() != 1) throw UsageError("Please specify one bwt file.");
        o.bwt_file = val("bwt-file");
    } else if (o.command == "color") {
        // src/movi_parser.cpp:193-199, handled at :319-330
        if (seen["index"].size() != 1) throw UsageError("Please specify the index directory file.");
        o.index_dir = val("index");
        refuse_color_modes(seen);
        if (has("device")) o.device = (int)to_int("device", val("device"));
    } else if (o.command == "build-SA") {
        // src/movi_parser.cpp:308-317
        if (seen["index"].size() != 1) throw UsageError("Please specify the index directory file.");
        o.index_dir = val("index");
        if (has("sample-rate")) {
            const std::string v = val("sample-rate");
            char *end = nullptr;
            const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v[0] == '-' || (end && *end)) throw UsageError("Argument '" + v + "' failed to parse for option 'sample-rate'");
            if (x == 0 || x > (1ull << 24)) throw UsageError("--sample-rate must be between 1 and 16777216");
            o.sample_rate = x;
        }
        if (has("device")) o.device = (int)to_int("device", val("device"));
    } else if (o.command == "view") {
        if (seen["bpf"].size() != 1) throw UsageError("Please specify one mls file.");
        o.bpf_file = val("bpf");
        o.small_bpf = has("small-bpf");
        o.large_bpf = has("large-bpf");
    } else {
        throw UsageError("The '" + o.command + "' action is not part of the MI355X engine (query, view, null, build, rlbwt, build-SA and color only); use "
                         "the reference movi for inspect / ftab.");
    }
    return o;
}

}  // namespace movi_host
