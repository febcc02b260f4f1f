// movi_main.cpp -- the `movi` host binary of the MI355X engine: `movi query` and
// `movi view` with the reference's command line, input rules and output bytes
// (driver: src/movi.cpp:221-400 query(), :402-503 view(), :561-748 main()).
//
// All query arithmetic happens on the GPU behind the C-ABI of include/movi_hip.h; this
// file only parses, batches, orders and writes.  One binary serves both index modes (the
// reference ships one binary per mode and a launcher, src/movi_launcher.cpp:244-254).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/movi_hip.h"
#include "nulldb.hpp"
#include "options.hpp"
#include "output.hpp"
#include "query_kind.hpp"
#include "reads.hpp"

using namespace movi_host;

namespace {

struct EngineError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

void check(int rc, const char *what) {
    if (rc != MOVI_OK) throw EngineError(std::string(what) + ": " + movi_last_error());
}

const char *index_type_name(uint32_t mode) {                          // program(), src/utils.cpp:10-40
    return mode == MOVI_MODE_REGULAR_THRESHOLDS ? "regular-thresholds"
           : mode == MOVI_MODE_SAMPLED_THRESHOLDS ? "sampled-thresholds"
           : mode == MOVI_MODE_SAMPLED ? "sampled"
           : mode == MOVI_MODE_REGULAR ? "regular"
           : mode == MOVI_MODE_BLOCKED ? "blocked" : "blocked-thresholds";
}

// Contiguous shards of [0, n) balanced by bases.
std::vector<size_t> shard_bounds(const ReadSet &rs, int parts) {
    std::vector<size_t> b(1, 0);
    const uint64_t total = rs.offsets.back();
    for (int p = 1; p < parts; p++) {
        const uint64_t target = total * p / parts;
        size_t i = std::lower_bound(rs.offsets.begin(), rs.offsets.end(), target) - rs.offsets.begin();
        b.push_back(std::min(std::max(i, b.back()), rs.size()));
    }
    b.push_back(rs.size());
    return b;
}

// Rounds the strand scheduler spends on a read in prefetch mode (see reads.hpp).  PML: one
// round per base.  Count: ReadProcessor::backward_search (src/read_processor.cpp:1096-1175)
// returns in the round of the last LF when it stops at position 0 or at an illegal base, and
// one round later when the interval became empty.
uint64_t count_rounds(const ReadSet &rs, size_t i, uint64_t matched, const uint8_t *code_of) {
    const uint64_t len = rs.len(i);
    const uint8_t *R = rs.bases.data() + rs.offsets[i];
    if (len == 0 || code_of[R[len - 1]] == 0xFF) return 1;
    if (matched >= len) return std::max<uint64_t>(len - 1, 1);
    if (code_of[R[len - matched - 1]] == 0xFF) return std::max<uint64_t>(matched - 1, 1);
    return std::max<uint64_t>(matched, 1);
}

// ZML: one round per ReadProcessor::backward_search call (src/read_processor.cpp:1096-1175 driven
// by :667-714).  A round either extends the phrase by one base (and also ends it there when the
// next base is illegal or position 0 is reached) or finds the interval empty / the first
// extension impossible and ends the phrase without moving.  Derived from the match lengths:
// base p-1 extended the phrase of p iff z[p-1] == z[p] + 1 (or both sit at the u16 clamp).
uint64_t zml_rounds(const ReadSet &rs, size_t i, const uint16_t *z, const uint8_t *code_of) {
    const int64_t len = (int64_t)rs.len(i);
    const uint8_t *R = rs.bases.data() + rs.offsets[i];
    auto legal = [&](int64_t p) { return code_of[R[p]] != 0xFF; };
    auto val = [&](int64_t p) { return z[len - 1 - p]; };
    int64_t pos = len - 1;
    while (pos >= 0 && !legal(pos)) pos--;                             // reset_backward_search at load
    if (pos < 0) return 1;
    uint64_t rounds = 0;
    bool first = true;
    for (;;) {
        rounds++;
        if (pos == 0) return rounds;                                   // first iteration at position 0 ends the read
        bool ended = false;
        if (first && !legal(pos - 1)) ended = true;                    // :1119-1121, no LF in this round
        first = false;
        if (!ended) {
            const bool extended = legal(pos - 1) && (val(pos - 1) == (uint16_t)(val(pos) + 1) ||
                                                     (val(pos) == 65535 && val(pos - 1) == 65535));
            if (!extended) {
                ended = true;                                          // empty interval: :1142-1146
            } else {
                pos--;
                if (pos == 0) return rounds;                           // :1148-1156
                if (!legal(pos - 1)) ended = true;                     // :1159-1163, same round
            }
        }
        if (ended) {                                                   // :688-700
            pos--;
            while (pos >= 0 && !legal(pos)) pos--;
            if (pos < 0) return rounds + 1;                            // one more round on the empty range
            first = true;
        }
    }
}

// ---- the three-stage host pipeline of `movi query`: parse (thread) -> GPU calls (caller) -> order + write (thread).
// Three Jobs circulate; each carries a chunk of reads and everything the engine returns for it, so the parser can fill
// chunk k+1 and the writer can drain chunk k-1 while the GPU works on chunk k.  Record order is untouched: chunks are
// parsed, processed and written strictly in input order.
// Result buffer of one job: grow-only, never zero-filled (the engine writes every entry) -- but its pages are TOUCHED,
// by several threads, when it is allocated: a device-to-host copy into memory that has never been touched takes the
// driver's page-fault path and ran at a third of the PCIe rate (1 Gbase of 10 kbp reads: 0.24 s of GPU calls, 0.10 s
// with resident pages).
struct MlBuf {
    uint16_t *p = nullptr;
    size_t cap = 0;
    bool pinned = false;                                              // page-locked (movi_host_alloc): the engine overlaps its transfers
    ~MlBuf() { release(); }
    void release() {
        if (p) { if (pinned) movi_host_free(p); else std::free(p); }
        p = nullptr;
        cap = 0;
    }
    uint16_t *data() const { return p; }
    void ensure(size_t n, bool want_pinned) {
        if (n <= cap) return;
        release();
        cap = n + (n >> 4);
        const size_t bytes = ((cap * sizeof(uint16_t) + (2u << 20) - 1) >> 21) << 21;
        void *q = nullptr;
        if (want_pinned && movi_host_alloc(bytes, &q) == MOVI_OK && q) {   // resident and pinned as it comes
            p = static_cast<uint16_t *>(q);
            pinned = true;
            return;
        }
        pinned = false;
        if (posix_memalign(&q, 2u << 20, bytes) != 0 || !q) { cap = 0; throw std::bad_alloc(); }
        p = static_cast<uint16_t *>(q);
        madvise(q, bytes, MADV_HUGEPAGE);                              // fewer, larger faults where THP is on
        const unsigned T = bytes >= (64u << 20) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
        auto touch = [&](unsigned t) {
            volatile uint8_t *b = static_cast<volatile uint8_t *>(q);
            for (size_t off = bytes / T * t, end = t + 1 == T ? bytes : bytes / T * (t + 1); off < end; off += 4096) b[off] = 0;
        };
        if (T == 1) touch(0);
        else {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < T; t++) th.emplace_back(touch, t);
            for (auto &x : th) x.join();
        }
    }
};

void *pinned_alloc(size_t bytes) {
    void *q = nullptr;
    return movi_host_alloc(bytes, &q) == MOVI_OK ? q : nullptr;
}
void pinned_free(void *q) { movi_host_free(q); }

// The chunks' read buffers: page-locked up to the size of an ordinary chunk -- allocated by the parser's warm-up while the index loads --,
// plain memory beyond it (a chunk of long reads grows to a GB: page-locking that much inside the run costs more than it gives).
// Why (tools/r05_stall.sh, the engine's MOVI_TRACE_HOST_CALLS=1): the upload of a chunk's 33.5 MB from PAGEABLE memory takes 0.6 ms when
// nothing else runs, 1.1 - 2.9 ms beside the parser's threads, and now and then 20 - 30 ms (one run in five on some boxes: the runtime's
// pageable path against the parser's page faults); from page-locked memory it is one direct DMA.  25 runs each on one box, ms per
// 150 Mbases: --no-output 14.6 - 38.7 (median 18.4) -> 12.4 - 19.9 (13.5); with the BPF file 32.0 - 69.8 (35.7) -> 31.0 - 44.9 (32.8).
// The calls are kept whole ("host_overlap" 0: the engine would otherwise cut a call on page-locked buffers into overlapped pieces,
// which chunk-sized calls never earn back -- the MOVI_PINNED=1 measurement above).  MOVI_PINNED=0: pageable buffers (A/B).
constexpr size_t kPinnedChunkLimit = 96u << 20;
std::mutex g_pinned_m;
std::vector<void *> g_pinned_ptrs;
void *chunk_alloc(size_t bytes) {
    if (bytes <= kPinnedChunkLimit) {
        void *q = pinned_alloc(bytes);
        if (q) { std::lock_guard<std::mutex> g(g_pinned_m); g_pinned_ptrs.push_back(q); return q; }
    }
    return std::malloc(bytes);
}
void chunk_free(void *q) {
    {
        std::lock_guard<std::mutex> g(g_pinned_m);
        auto it = std::find(g_pinned_ptrs.begin(), g_pinned_ptrs.end(), q);
        if (it != g_pinned_ptrs.end()) { g_pinned_ptrs.erase(it); movi_host_free(q); return; }
    }
    std::free(q);
}

struct Job {
    ReadSet rs;
    MlBuf pml;                                                        // PML / ZML values, emission order per read
    std::vector<uint16_t> log_ff, log_scan;                           // --logs: per-base fast-forwards / scan rows
    std::vector<uint64_t> matched, counts;                            // --count
    std::vector<uint32_t> n_mems;                                     // --mem: MEMs per read ...
    std::vector<movi_mem_t> mems;                                     // ... and all of them, read by read (file order)
    std::vector<uint32_t> n_runs, kmers_found;                        // --kmer: runs and found k-mers per read ...
    std::vector<movi_kmer_run_t> runs;                                // ... and all the runs, read by read (file order)
    std::vector<uint64_t> occ, occ_sum;                               // --kmer-occ: one count per base (a read's last k - 1: 0), the sums per read ...
    std::vector<uint32_t> occ_found;                                  // ... and the found k-mers per read
    std::vector<movi_mc_read_t> mc;                                   // --multi-classify: best / second / counts per read ...
    std::vector<uint32_t> mc_counts;                                  // ... and, with --report-all, its counter row (num_species per read)
    std::vector<uint64_t> sa;                                         // --sa-entries: one suffix-array entry per base, emission order like pml
    std::vector<uint64_t> loc_occ, loc_first, loc_pos;                // --locate: per item (a read with matched > 0, in read order; a MEM) its occurrences, and
                                                                      // the positions of item k in loc_pos[loc_first[k] .. loc_first[k + 1])
    std::vector<uint8_t> err;                                         // per-read error byte
    RawBytes original;                                                // reads as given (--filter after --ignore-illegal-chars 1)
    std::vector<uint32_t> bins_above, bins_below;                     // verdict-only classification
    std::vector<uint64_t> bins_sum;
    bool verdict_only = false;
    bool ml_vector = false;                                           // the engine gets a PML / ZML vector to fill (else NULL: the walk alone)
    // The one-read Job of the warm-up call (warm_up_engine).  It keeps that call what it always was where a real chunk's differs: a
    // walk-only query still hands the engine a vector (so the first real chunk finds the handle's staging as before), --report-all
    // asks for no counter rows, and a MEM / k-mer call gets room for one result per base -- all a read can hold, so it never runs twice.
    bool warm_up = false;

    uint16_t *ml_out() const { return ml_vector ? pml.data() : nullptr; }
    // Sizes what the engine returns for the chunk in `rs`.  assign(): zero-filled per chunk; resize() / ensure(): the engine writes every entry.
    void prepare(const QueryPlan &plan, const Options &o, uint32_t num_species, bool pinned) {
        const size_t n = rs.size();
        verdict_only = plan.verdict_only;
        bins_above.assign(verdict_only ? n : 0, 0);
        bins_below.assign(verdict_only ? n : 0, 0);
        bins_sum.assign(verdict_only ? n : 0, 0);
        ml_vector = plan.result_vector ||
                    (warm_up && (plan.kind == QueryKind::SaEntries || plan.kind == QueryKind::Pml || plan.kind == QueryKind::Zml));
        pml.ensure(ml_vector ? rs.bases.size() : 0, pinned);
        if (plan.logs) { log_ff.resize(rs.bases.size()); log_scan.resize(rs.bases.size()); }
        if (o.sa_entries) sa.resize(rs.bases.size());
        if (o.multi_classify) {
            mc.resize(n);
            mc_counts.resize(o.report_all && !warm_up ? n * (size_t)num_species : 0);
        }
        matched.assign(o.count ? n : 0, 0);
        counts.assign(o.count ? n : 0, 0);
        n_mems.assign(o.mem ? n : 0, 0);
        n_runs.assign(o.kmer ? n : 0, 0);
        kmers_found.assign(o.kmer ? n : 0, 0);
        if (o.kmer_occ) occ.resize(rs.bases.size());
        occ_found.assign(o.kmer_occ ? n : 0, 0);
        occ_sum.assign(o.kmer_occ ? n : 0, 0);
        err.assign(n, 0);
    }
};

template <typename T>
class HandOff {                                                       // unbounded FIFO between two pipeline stages
public:
    void push(T v) {
        { std::lock_guard<std::mutex> g(m_); q_.push_back(v); }
        cv_.notify_all();
    }
    // false once close() was called and the queue is drained -- or at once after abandon()
    bool pop(T &v) {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return !q_.empty() || closed_ || abandoned_; });
        if (abandoned_ || q_.empty()) return false;
        v = q_.front();
        q_.erase(q_.begin());
        return true;
    }
    void close() {
        { std::lock_guard<std::mutex> g(m_); closed_ = true; }
        cv_.notify_all();
    }
    void abandon() {
        { std::lock_guard<std::mutex> g(m_); abandoned_ = true; }
        cv_.notify_all();
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<T> q_;
    bool closed_ = false, abandoned_ = false;
};

// A regular read file is memory-mapped: the parser then cuts lines and batches without copying a byte, and its worker
// threads copy the sequences straight from the page cache into the chunk; pipes and stdin go through the stream.
// (InputMapping: reads.hpp)
std::unique_ptr<BatchReader> open_reader(const std::string &path, std::istream &in, size_t min_reads, InputMapping &map) {
    // (populating the mapping ahead of the parser from a helper thread -- MADV_POPULATE_READ, 16 MB at a time -- was
    // measured and dropped: it contends with the parser's own faults for the address-space lock; scan 14 -> 23 ms)
    if (path != "-" && !std::getenv("MOVI_NO_MMAP")) (void)map.map(path);
    if (map.p != MAP_FAILED) return std::unique_ptr<BatchReader>(new BatchReader(static_cast<const char *>(map.p), map.n, min_reads));
    return std::unique_ptr<BatchReader>(new BatchReader(in, min_reads));
}

// Every output stream of `movi query` (open_output_files, src/utils.cpp:319-384), opened from the plan by open_outputs.
struct Outputs {
    // stream buffers first: they must outlive the streams that flush through them on destruction
    std::vector<char> out_buf2 = std::vector<char>(1u << 20);
    std::ofstream report_file, matches_file, sa_file, locs_file;
    std::unique_ptr<WorkerPool> bpf_pool;                             // the writer stage's helper threads (record order, BPF gather; built by the writer thread, outlives mls_file)
    BpfWriter mls_file;
    // --multi-classify writes one report, to the -o file itself (open_output_files, src/utils.cpp:323-326) or to --stdout; the PML
    // file the reference opens beside it stays empty there and is not created here
    std::ofstream mc_file;
    std::ofstream costs_file, scans_file, ff_file;                    // --logs
    std::ostream *report = nullptr;                                   // the classification report: report_file or stdout
};

void open_or_throw(std::ofstream &f, const std::string &name, std::ios::openmode mode = std::ios::out) {
    f.open(name, mode);
    if (!f.good()) throw std::runtime_error("Failed to open the output file: " + name);
}

void open_outputs(const Options &o, const QueryPlan &plan, const std::string &index_type, Classifier &classifier, Outputs &f) {
    f.matches_file.rdbuf()->pubsetbuf(f.out_buf2.data(), (std::streamsize)f.out_buf2.size());
    if (o.classify) {
        classifier.load_null_db(o.index_dir, o.query_type(), o.verbose);
        if (!o.filter) {                                              // src/classifier.cpp:39-61
            if (!o.write_stdout) {
                const std::string name = o.read_file + "." + index_type + plan.report_suffix;
                std::cerr << "[movi] Report file name: " << name << "\n";
                f.report_file.open(name);
                f.report = &f.report_file;
            } else {
                f.report = &std::cout;
            }
            classifier.write_report_header(*f.report);
        }
    }
    if (plan.mc_to_out_file) open_or_throw(f.mc_file, o.out_file);
    const std::string prefix = !o.out_file.empty() ? o.out_file : o.read_file + "." + index_type;
    if (!plan.matches_suffix.empty()) open_or_throw(f.matches_file, prefix + plan.matches_suffix);
    if (!plan.locs_suffix.empty()) open_or_throw(f.locs_file, prefix + plan.locs_suffix);
    if (!plan.bpf_suffix.empty()) f.mls_file.open(prefix + plan.bpf_suffix, 16);
    if (!plan.sa_suffix.empty()) open_or_throw(f.sa_file, prefix + plan.sa_suffix, std::ios::out | std::ios::binary);
    // --logs (src/utils.cpp:376-382: opened with the other output files, written by output_logs :268-289 per read)
    if (plan.logs) {
        const std::string stem = prefix + plan.logs_stem;
        f.costs_file.open(stem + ".costs");
        f.scans_file.open(stem + ".scans");
        f.ff_file.open(stem + ".fastforwards");
        if (!f.costs_file.good() || !f.scans_file.good() || !f.ff_file.good()) throw std::runtime_error("Failed to open the log files: " + stem + ".costs/.scans/.fastforwards");
    } else if (plan.logs_ignored) {
        std::cerr << "[movi] --logs is only collected for PML queries that write their output to files; ignored here.\n";
    }
}

struct WarmJoin { std::thread &t; ~WarmJoin() { if (t.joinable()) t.join(); } };
struct Closer {
    std::vector<movi_index_t *> &h;
    ~Closer() { for (auto *x : h) movi_index_destroy(x); }
};

// What the steps of `movi query` and its three pipeline stages share.  The members stand in the order the command sets them up and
// go away in the reverse one: the output streams before the handles, the handles before the parser's warm-up thread and the chunks.
struct QueryRun {
    const Options &o;
    const QueryPlan plan;
    DocInfo docs;                                                     // --multi-classify
    uint32_t num_species = 0;
    bool share_gpu = false;
    std::chrono::steady_clock::time_point t0, t1;                      // "loading the index" starts at t0, "processing the reads" at t1
    double warm_seconds = 0;
    std::ifstream file_in;
    std::istream *in = &std::cin;
    InputMapping map;
    std::unique_ptr<BatchReader> reader;
    Job jobs[3];
    uint64_t chunk_bases = 1ull << 25, chunk_min_reads = 1ull << 15, chunk_hard_max = 1ull << 30;
    std::string pinned_env;
    bool pin_buffers = false;
    bool pin_chunks = false;                                           // read buffers page-locked at warm-up, one direct upload per chunk (chunk_alloc)
    std::thread warmer;
    WarmJoin warm_join{warmer};
    std::vector<movi_index_t *> handles;
    Closer closer{handles};
    movi_index_desc_t desc;
    Classifier classifier;
    Outputs out;
    bool bpf_serial = false;                                           // A/B: the one-thread gather-and-write loop (BpfWriter::append(records))
    unsigned bpf_threads = 4;                                          // (8 measured the same: the stage is bound by its write()s)
    HandOff<Job *> free_q, parsed_q, done_q;
    std::exception_ptr parse_error, write_error;
    std::mutex err_m;
    uint64_t reads_done = 0, bases_done = 0;
    uint64_t occ_found_total = 0, occ_sum_total = 0;                   // --kmer-occ: found k-mers and the sum of their counts, all reads
    double gpu_seconds = 0, parse_seconds = 0, write_seconds = 0;
    std::vector<double> chunk_parse_s, chunk_gpu_s;                    // --verbose: the first chunks' stage times one by one
    std::vector<BatchReader::PhaseTimes> chunk_phases;                 // (cumulative parser phases after each chunk)

    explicit QueryRun(const Options &opts) : o(opts), plan(query_plan(opts)), handles((size_t)opts.gpus, nullptr) {}
    int dev_of(int g) const { return share_gpu ? o.device : o.device + g; }
};

// What the query needs beside the index, and the devices it asks for: checked before anything is loaded.
void check_inputs_and_devices(QueryRun &q) {
    const Options &o = q.o;
    if ((o.sa_entries || o.locate) && !std::ifstream(o.index_dir + "/ssa.movi").good())      // deserialize_sampled_SA, src/move_structure_io.cpp:727-730
        throw std::runtime_error("[deserialize sampled SA] Failed to open sampled SA entries file at " + o.index_dir + "/ssa.movi" +
                                 "\nBuild the sampled SA by running the build-SA command.");
    if (o.multi_classify) {
        // the index first, so that a missing one is reported as such; then deserialize_doc_sets_flat (src/move_structure_io.cpp:587-592)
        // and load_document_info (:643-649), each with the reference's message
        struct stat sb;
        if (stat(o.index_dir.c_str(), &sb) != 0 ||
            (S_ISDIR(sb.st_mode) && !std::ifstream(o.index_dir + "/index.movi").good() && !std::ifstream(o.index_dir + "/movi_index.bin").good()))
            throw std::runtime_error("The index does not exist at " + o.index_dir + " (no index.movi in it)");
        if (!std::ifstream(o.index_dir + "/doc_sets_flat.bin").good())
            throw std::runtime_error("[deserialize doc sets flat] Failed to open document sets flat file at " + o.index_dir + "/doc_sets_flat.bin");
        q.docs = load_doc_info(o.index_dir);
        if (q.docs.to_taxon_id.empty() || q.docs.to_taxon_id.size() > 0xFFFF)
            throw std::runtime_error("ref.fa.doc_offsets / ref.fa.doc_ids name " + std::to_string(q.docs.to_taxon_id.size()) + " species: between 1 and 65535 are served");
    }
    q.num_species = (uint32_t)q.docs.to_taxon_id.size();
    int n_dev = 0;
    check(movi_device_count(&n_dev), "no usable GPU");
    if (n_dev < 1) throw EngineError("no usable GPU: the MI355X engine has no CPU fallback");
    // test hook for 1-GPU boxes: MOVI_SHARE_GPU=1 puts every logical GPU of --gpus N on --device
    q.share_gpu = std::getenv("MOVI_SHARE_GPU") && std::string(std::getenv("MOVI_SHARE_GPU")) == "1";
    if (!q.share_gpu && o.device + o.gpus > n_dev)
        throw EngineError("requested devices " + std::to_string(o.device) + ".." + std::to_string(o.device + o.gpus - 1) +
                          " but only " + std::to_string(n_dev) + " visible");
}

// Round 5: the read file is mapped and the parser WARMED while the index loads (BatchReader::warm_up: the worker pool, the first
// window's newline scan -- and with it the mapping's page faults --, the three circulating chunks' buffers sized and first
// touched by the pool's pinned threads).  A run of 1 M x 150 bp is 4.5 chunks, three of them used to be parsed into fresh memory:
// chunk 1 took 7.4 ms, chunks 2 - 3 3.9 - 4.3 ms, a warm chunk 2.8 ms (tools/r05_cli.sh).  (Touching the buffers from helper
// threads of THIS thread instead made the parse slower, 0.024 - 0.028 s against 0.020 s: first touch by threads on another NUMA node
// than the parser's pinned pool.)  Round 6 (advisor finding): the warm-up no longer reads the input -- round 5's scanned the first
// window while the index loaded, outside the "processing the reads" clock the reference keeps its whole parse inside -- : its tables
// are sized from the line density of the file's first MiB (the probe below), and the first window's scan, page faults included, is
// the first chunk's own, inside the clock.  What stays outside is set-up of the engine's host side -- the worker pool, sizing and
// page-locking the three circulating chunks' buffers --, like the device staging reserved with the index.  (Should a warm-up ever scan
// -- no line density known --, its seconds are added to the reported time.)  MOVI_NO_WARM_PARSER=1: A/B.
void open_input_and_warm_parser(QueryRun &q) {
    const Options &o = q.o;
    if (const char *e = std::getenv("MOVI_CHUNK_BASES")) {             // test hook: many small chunks
        q.chunk_bases = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
        q.chunk_min_reads = 1;
    }
    q.pinned_env = std::getenv("MOVI_PINNED") ? std::getenv("MOVI_PINNED") : "";
    q.pin_buffers = q.pinned_env == "1";
    if (o.read_file == "-") return;
    q.file_in.open(o.read_file.c_str());
    if (!q.file_in.good()) return;                                     // (a missing file is reported where it always was: after the index)
    q.in = &q.file_in;
    q.reader = open_reader(o.read_file, *q.in, o.prefetch ? 4 * o.strands : 1, q.map);   // src/movi.cpp:283, :326
    const bool warm = q.map.p != MAP_FAILED && !q.pin_buffers && !std::getenv("MOVI_NO_WARM_PARSER") && !std::getenv("MOVI_CHUNK_BASES");
    // (only where the warm-up allocates them, outside the run -- and only for short lines: a chunk of long reads outgrows the
    // warmed buffers at once, and giving page-locked memory back inside the run cost 100 k x 10 kbp 20 %: 0.094 - 0.135 -> 0.134 - 0.159 s,
    // tools/r05_pin_ab.sh)
    bool short_lines = false;
    double lines_per_byte = 0.0;                                       // (of the file's first MiB: sizes the warm-up's tables without a scan of the input)
    if (warm) {
        const char *m = static_cast<const char *>(q.map.p);
        const size_t probe = std::min<size_t>(q.map.n, 1u << 20);
        size_t nl = 0;
        for (const char *p = m; (p = static_cast<const char *>(std::memchr(p, '\n', (size_t)(m + probe - p)))) != nullptr; ++p) nl++;
        short_lines = nl * 1024 >= probe;                              // at least a line per KiB (the scan-ahead's own test for long reads)
        lines_per_byte = probe ? (double)(nl + 1) / (double)probe : 0.0;
    }
    q.pin_chunks = warm && short_lines && q.pinned_env != "0";
    if (q.pin_chunks)
        for (Job &j : q.jobs) j.rs.bases.set_allocator(chunk_alloc, chunk_free);
    if (warm)
        q.warmer = std::thread([&q, lines_per_byte] {
            ReadSet *sets[3] = {&q.jobs[0].rs, &q.jobs[1].rs, &q.jobs[2].rs};
            try { q.reader->warm_up(sets, 3, q.chunk_bases, lines_per_byte); } catch (...) { /* no memory for it: the chunks allocate as they come */ }
            q.warm_seconds = q.reader->warm_input_seconds();           // (read after the join) the part that read the input
        });
}

void load_handles(QueryRun &q) {
    const Options &o = q.o;
    if (!o.gpus_given) {
        check(movi_index_load(o.device, o.index_dir.c_str(), &q.handles[0]), "loading the index");
    } else if (!q.share_gpu) {
        // --gpus N: the index file is mapped once, its rows cross PCIe once (to the first GPU) and reach the others
        // through ONE RCCL broadcast over xGMI; every GPU then builds its resident layout (include/movi_hip.h)
        std::vector<int> devs((size_t)o.gpus);
        for (int g = 0; g < o.gpus; g++) devs[(size_t)g] = q.dev_of(g);
        check(movi_index_load_replicated(o.index_dir.c_str(), devs.data(), o.gpus, q.handles.data()), "replicating the index");
    } else {
        // MOVI_SHARE_GPU=1 (test hook for 1-GPU boxes: every logical GPU of --gpus N is the same device, which RCCL cannot
        // serve as N ranks): N independent loads, so that the read sharding and the per-GPU host threads can be exercised
        for (int g = 0; g < o.gpus; g++) check(movi_index_load(q.dev_of(g), o.index_dir.c_str(), &q.handles[(size_t)g]), "loading the index");
    }
}

// The side tables and options of every handle, then what "loading the index" builds ahead of the first chunk.
void configure_handles(QueryRun &q) {
    const Options &o = q.o;
    const std::vector<movi_index_t *> &handles = q.handles;
    if (o.sa_entries || o.locate)                                      // deserialize_sampled_SA, src/move_structure_io.cpp:724-744 (every GPU holds the samples beside its table)
        for (auto *hd : handles) check(movi_ssa_load(hd, (o.index_dir + "/ssa.movi").c_str()), "loading the sampled suffix array");
    if (o.multi_classify)                                              // deserialize_doc_sets_flat: every GPU holds the colour tables beside its table
        for (auto *hd : handles) {
            if (const char *e = std::getenv("MOVI_COLOR_SCRATCH_BYTES"))           // test hook: reads through the counter scratch in several chunks
                check(movi_set_option(hd, "color_scratch_bytes", std::atoll(e)), "MOVI_COLOR_SCRATCH_BYTES");
            check(movi_color_load(hd, (o.index_dir + "/doc_sets_flat.bin").c_str(), q.num_species), "loading the colour tables");
        }
    if (o.seg_len >= 0)
        for (auto *hd : handles) check(movi_set_option(hd, "seg_len", o.seg_len), "--seg-len");
    // (the ZML parse does not walk on the look-ahead rows unless "zml_ahead" asks for it: `--zml --ahead-rows 1` builds nothing)
    if (o.zml && o.ahead_rows == 1)
        std::cerr << "[movi] --ahead-rows 1 is ignored with --zml: the ZML parse walks on the plain rows (the engine's \"zml_ahead\" option is opt-in and no faster).\n";
    if (o.ahead_rows >= 0 && !(o.zml && o.ahead_rows == 1))
        for (auto *hd : handles) check(movi_set_option(hd, "ahead_rows", o.ahead_rows), "--ahead-rows");
    // --ftab-k K: the engine's interval table at min(K, 12) -- speed only, never answers (an index outside its scope keeps none)
    if (o.ftab_k >= 0)
        for (auto *hd : handles) (void)movi_set_option(hd, "ftab_k", std::min<long>(o.ftab_k, 12));
    if (q.pin_chunks)
        for (auto *hd : handles) check(movi_set_option(hd, "host_overlap", 0), "host_overlap");
    // (the command's own pipeline keeps the host's cores busy -- parser pool, record order, BPF gather and write --: the PML vector comes
    // down as it is instead of as reset masks for the engine's worker threads to expand beside them; tools/r06_l.sh: GPU calls 13 - 15 ms
    // against 35 - 40 ms in three runs of five.  MOVI_PML_VIA_MASK=1 forces the mask route: the parity suite's re-run.)
    if (!std::getenv("MOVI_PML_VIA_MASK")) {
        const char *hm = std::getenv("MOVI_HOST_MASKS");                      // (A/B: -1 = the engine's own policy, 1 = every call)
        for (auto *hd : handles) (void)movi_set_option(hd, "host_masks", hm ? std::atoi(hm) : 0);
    }
    // Round 5: the handles' derived tables -- top-of-walk / interval table, look-ahead rows (16 bytes per row: 16 GB and ~0.3 s of
    // allocation + build for a 1 B-row index), row-start checkpoints -- are part of LOADING THE INDEX (movi_index_prepare), not of the
    // first chunk's GPU call: rounds 3 - 4 built them inside the read-processing clock, behind the first chunk's parse, which a
    // 14 M-row index hides and a 1 B-row one does not (bench.py big_table.cli_path: 0.31 s of "processing" for 0.03 s of work).
    for (auto *hd : handles) {                                         // (errors here are not the query's: the real calls report)
        if (q.plan.prepare == QueryPlan::kNoPrepare) continue;         // --logs runs on the first kernel, which uses none of the derived tables
        (void)movi_index_prepare(hd, (uint32_t)q.plan.prepare, nullptr, nullptr);
        // ... and so is the device staging of a chunk's host call (three hipMallocs: 1.2 ms of the first chunk's 3 ms call otherwise):
        // a chunk's bases with the slack of its last batch, its result vector when one comes back, reads down to 64 bases long
        const int64_t cb = (int64_t)std::min<uint64_t>(q.chunk_bases + (q.chunk_bases >> 3), 1ull << 31) / (o.gpus > 0 ? o.gpus : 1);
        // (a reservation that does not fit is not an error: the staging then grows inside the first call, as it did before round 5)
        bool reserved = movi_set_option(hd, "reserve_host_bases", cb) == MOVI_OK;
        reserved = movi_set_option(hd, "reserve_host_reads", cb / 64) == MOVI_OK && reserved;
        if (q.plan.reserve_results)
            reserved = movi_set_option(hd, "reserve_host_results", cb) == MOVI_OK && reserved;
        if (!reserved && o.verbose) std::cerr << "[movi] The device staging could not be reserved up front (" << movi_last_error() << "); it grows with the first chunk.\n";
    }
}

// ---- the engine call of one shard of a chunk

struct ShardOut {                                                     // what a shard returns beside the Job's own arrays
    std::vector<movi_mem_t> mems;                                     // --mem / --kmer: the shard's results, sized by what it found
    std::vector<movi_kmer_run_t> runs;
    std::vector<uint64_t> loc_occ, loc_first, loc_pos;                // --locate: the shard's items (loc_first: relative to the shard, one more than items)
};

// MEM and k-mer results: room for a few per read first; a shard that finds more is run again with room for exactly what it found.
// call(results, cap, &total) is the engine call.
template <typename T, typename Call>
int call_with_room(const Job &job, size_t a, size_t b, std::vector<T> &v, Call call) {
    const uint64_t bases = job.rs.offsets[b] - job.rs.offsets[a];
    const uint64_t cap = job.warm_up ? bases : (b - a) * 8 + bases / 16;
    uint64_t total = 0;
    v.resize(cap);
    int rc = call(v.data(), cap, &total);
    if (rc == MOVI_ERR_ARG && total > cap) {
        v.resize(total);
        rc = call(v.data(), total, &total);
    }
    v.resize(rc == MOVI_OK ? total : 0);
    return rc;
}

// --locate: the shard's hits, after its ordinary query -- one item (i, len - matched, len) per read with matched > 0 of a count query,
// one per MEM of a MEM query -- through movi_locate_matches_host, which uploads the shard's reads a second time (include/movi_hip.h).
int locate_shard(const QueryRun &q, movi_index_t *h, const Job &job, size_t a, size_t b, ShardOut &out) {
    std::vector<movi_match_t> items;
    if (q.plan.kind == QueryKind::Count) {
        for (size_t i = a; i < b; i++)
            if (job.matched[i] > 0) {
                const uint64_t len = job.rs.len(i);
                items.push_back(movi_match_t{(uint32_t)(i - a), (uint32_t)(len - std::min<uint64_t>(job.matched[i], len)), (uint32_t)len});
            }
    } else {
        size_t k = 0;
        for (size_t i = a; i < b; i++)
            for (uint32_t j = 0; j < job.n_mems[i]; j++, k++) items.push_back(movi_match_t{(uint32_t)(i - a), out.mems[k].start, out.mems[k].end});
    }
    const uint64_t ni = items.size();
    out.loc_occ.assign(ni, 0);
    out.loc_first.assign(ni + 1, 0);
    // room for a few positions per item first; a shard that lists more is run again with room for exactly what it lists
    uint64_t cap = std::min<uint64_t>(ni * q.o.max_occ, ni * 4 + 1024), total = 0;
    out.loc_pos.resize(cap);
    auto call = [&]() {
        return movi_locate_matches_host(h, job.rs.bases.data(), job.rs.offsets.data() + a, b - a, items.data(), ni, q.o.max_occ, out.loc_occ.data(),
                                        out.loc_first.data(), out.loc_pos.data(), cap, &total, nullptr, nullptr);
    };
    int rc = call();
    if (rc == MOVI_ERR_ARG && total > cap) {
        cap = total;
        out.loc_pos.resize(cap);
        rc = call();
    }
    out.loc_pos.resize(rc == MOVI_OK ? total : 0);
    return rc;
}

int run_shard_query(const QueryRun &q, movi_index_t *h, Job &job, size_t a, size_t b, ShardOut &out);

// Reads [a, b) of the job's chunk on one handle.
int run_shard(const QueryRun &q, movi_index_t *h, Job &job, size_t a, size_t b, ShardOut &out) {
    const int rc = run_shard_query(q, h, job, a, b, out);
    if (rc != MOVI_OK || !q.plan.locate) return rc;
    return locate_shard(q, h, job, a, b, out);
}

// The ordinary query of a shard: the only place that names the engine's query entry points (locate_shard's beside it).
int run_shard_query(const QueryRun &q, movi_index_t *h, Job &job, size_t a, size_t b, ShardOut &out) {
    const Options &o = q.o;
    const uint8_t *bases = job.rs.bases.data();
    const uint64_t *offs = job.rs.offsets.data() + a;
    const uint64_t n = b - a;
    uint8_t *err = job.err.data() + a;
    switch (q.plan.kind) {
    case QueryKind::PmlVerdictBins:
        return movi_pml_classify_host(h, bases, offs, n, (uint32_t)o.bin_width, q.classifier.max_value_thr, job.bins_above.data() + a,
                                      job.bins_below.data() + a, job.bins_sum.data() + a, err, nullptr);
    case QueryKind::PmlLogs:
        return movi_pml_logs_host(h, bases, offs, n, job.pml.data(), job.log_ff.data(), job.log_scan.data(), err, nullptr);
    case QueryKind::MultiClassify:
        return movi_multi_classify_host(h, bases, offs, n, o.min_len, job.mc.data() + a,
                                        job.mc_counts.empty() ? nullptr : job.mc_counts.data() + a * (size_t)q.num_species, nullptr, err, nullptr);
    case QueryKind::SaEntries:                                        // (--no-output: computed and discarded, as the reference does)
        return movi_sa_entries_host(h, bases, offs, n, job.ml_out(), job.sa.data(), err, nullptr);
    case QueryKind::Pml:
        return movi_pml_host(h, bases, offs, n, job.ml_out(), err, nullptr);
    case QueryKind::Zml:
        return movi_zml_host(h, bases, offs, n, job.ml_out(), err, nullptr);
    case QueryKind::Mem:
        return call_with_room(job, a, b, out.mems, [&](movi_mem_t *v, uint64_t cap, uint64_t *total) {
            return movi_mem_host(h, bases, offs, n, o.min_mem_length, job.n_mems.data() + a, v, cap, total, err, nullptr);
        });
    case QueryKind::Kmer:
        return call_with_room(job, a, b, out.runs, [&](movi_kmer_run_t *v, uint64_t cap, uint64_t *total) {
            return movi_kmer_host(h, bases, offs, n, o.k, job.n_runs.data() + a, job.kmers_found.data() + a, v, cap, total, nullptr);
        });
    case QueryKind::Count:
        return movi_count_host(h, bases, offs, n, job.matched.data() + a, job.counts.data() + a, err, nullptr);
    case QueryKind::KmerOcc:                                          // (the counts lie relative to the shard's first base)
        return movi_kmer_occ_host(h, bases, offs, n, o.k, job.occ.data() + offs[0], job.occ_found.data() + a, job.occ_sum.data() + a, err, nullptr);
    }
    return MOVI_ERR_ARG;
}

// ---- warm-up, while the parser works on the first chunk (the derived tables were built with the index, above):
// one one-read query of the same kind through the host entry point: what the FIRST host call does once -- the handle's
// device staging, the page-locked block of its small results, the walk kernels' code object (a translation unit of its own
// since round 5: the builders' launches do not load it) -- cost the first chunk 20 - 30 ms without it (tools/r05_cli.sh:
// GPU calls of 1 M x 150 bp 0.035 - 0.045 s with the preparation alone, 0.012 - 0.014 s with the warm-up call).
void warm_up_engine(const QueryRun &q) {
    if (q.plan.prepare == QueryPlan::kNoPrepare) return;               // --logs runs on the first kernel, which uses none of the derived tables
    const uint8_t wb[32] = {'A','C','G','T','A','C','G','T','A','C','G','T','A','C','G','T','A','C','G','T','A','C','G','T','A','C','G','T','A','C','G','T'};
    Job w;
    w.warm_up = true;                                                 // (what that changes: Job::warm_up)
    w.rs.bases.resize_uninitialized(sizeof wb);
    std::memcpy(w.rs.bases.data(), wb, sizeof wb);
    w.rs.offsets = {0, sizeof wb};
    w.rs.batch_of = {0};
    w.prepare(q.plan, q.o, q.num_species, false);
    for (auto *hd : q.handles) {                                       // (errors here are not the query's: the real calls report)
        ShardOut out;
        (void)run_shard(q, hd, w, 0, 1, out);
    }
}

// ---- stage 1: parse
// (round 5, measured and dropped: keeping the parser's threads off the cache domain of the GPU-call and writer threads --
// inside the command every parser phase runs 2 x slower than in tools/parse_bench -- changed nothing: 0.027 - 0.036 s against
// 0.026 s per 150 Mbases.  tools/r05_cli.sh)
void parse_stage(QueryRun &q) {
    BatchReader &reader = *q.reader;
    try {
        reader.adopt_pool();                                           // (a pool built by the warm-up: this thread joins its cache domain)
        Job *j = nullptr;
        // (round 5, measured and dropped: smaller FIRST chunks -- a quarter, then half of the steady size, to shorten the
        // pipeline's fill -- tripled the GPU stage, 0.011 -> 0.035 s per 150 Mbases: every growth of a chunk re-allocates the
        // engine's device staging, and hipFree waits for the device.  tools/r05_cli.sh.  Tried again with the staging reserved up
        // front ("reserve_host_*"): nothing to see through the box's own noise, 15 runs each, BPF 30 - 40 against 30 - 39 and 32 - 35
        // against 34 - 37 ms, --no-output worse in one round and better in the other)
        while (q.free_q.pop(j)) {
            const auto tp = std::chrono::steady_clock::now();
            const bool more = reader.next_chunk(j->rs, q.chunk_bases, q.chunk_min_reads, q.chunk_hard_max);
            const double dtp = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
            q.parse_seconds += dtp;
            if (q.chunk_parse_s.size() < 64) { q.chunk_parse_s.push_back(dtp); q.chunk_phases.push_back(reader.phase_times()); }
            if (!more) break;
            q.parsed_q.push(j);
        }
    } catch (...) {
        std::lock_guard<std::mutex> g(q.err_m);
        q.parse_error = std::current_exception();
    }
    q.parsed_q.close();
}

// ---- stage 3: record order + writers (everything that touches the output streams lives on this thread)

// record order: strand scheduler emulation in prefetch mode, file order otherwise
std::vector<uint32_t> record_order(QueryRun &q, const Job &job) {
    const Options &o = q.o;
    const ReadSet &rs = job.rs;
    const size_t n = rs.size();
    WorkerPool *pool = q.out.bpf_pool.get();
    std::vector<uint32_t> order;
    if (o.prefetch) {
        std::vector<uint64_t> cost(n);
        auto cost_of = [&](size_t i) -> uint64_t {
            return o.pml ? rs.len(i)
                 : o.zml ? zml_rounds(rs, i, job.pml.data() + rs.offsets[i], q.desc.code_of)
                         : count_rounds(rs, i, job.matched[i], q.desc.code_of);
        };
        if (pool) {
            const unsigned P = pool->size() * 2u;
            pool->run(P, [&](unsigned p) { for (size_t i = n * p / P, e = n * (p + 1) / P; i < e; i++) cost[i] = cost_of(i); });
        } else {
            for (size_t i = 0; i < n; i++) cost[i] = cost_of(i);
        }
        order = strand_order(rs, cost, o.strands, pool);
    } else {
        order.resize(n);
        for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    }
    return order;
}

// write_mls, src/read_processor.cpp:489-562: one line per read, the PML records' order
void write_multi_classify_lines(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    const Options &o = q.o;
    const ReadSet &rs = job.rs;
    std::string txt;
    txt.reserve(rs.size() * 24);
    for (uint32_t i : order)
        append_mls_line(txt, rs.id(i), rs.len(i), job.mc[i], o.report_all ? job.mc_counts.data() + (size_t)i * q.num_species : nullptr,
                        q.docs.to_taxon_id, o.report_all, o.min_diff_frac, o.min_score_frac);
    std::ostream &out = o.write_stdout ? static_cast<std::ostream &>(std::cout) : q.out.mc_file;
    out.write(txt.data(), (std::streamsize)txt.size());
}

// output_base_stats(DataType::sa_entry), src/utils.cpp:212-246: the PML records' order
void write_sa_records(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    const ReadSet &rs = job.rs;
    std::string rec;
    for (uint32_t i : order) {
        rec.clear();
        append_sa_record(rec, rs.id(i), job.sa.data() + rs.offsets[i], rs.len(i));
        q.out.sa_file.write(rec.data(), (std::streamsize)rec.size());
    }
}

// the plain BPF file: records gathered from the chunk's arrays by a pool of this thread's, written behind it (output.cpp)
void write_bpf_pooled(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    const ReadSet &rs = job.rs;
    if (!q.out.bpf_pool) q.out.bpf_pool.reset(new WorkerPool(q.bpf_threads));
    q.out.mls_file.append(BpfWriter::Chunk{order.data(), rs.size(), rs.offsets.data(), job.pml.data(), rs.id_off.data(), rs.id_bytes.data()}, *q.out.bpf_pool);
}

// plain `--stdout`: the text of a chunk is formatted by worker threads (ranges balanced by bases), written in order
void write_stdout_parallel(const Job &job, const std::vector<uint32_t> &order) {
    const ReadSet &rs = job.rs;
    const size_t n = rs.size();
    const unsigned T = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::string> txt(T);
    std::vector<size_t> cut(T + 1, n);
    cut[0] = 0;
    uint64_t acc = 0;
    unsigned t = 1;
    for (size_t k = 0; k < n && t < T; k++) {
        acc += rs.len(order[k]);
        while (t < T && acc >= rs.bases.size() * (uint64_t)t / T) cut[t++] = k + 1;
    }
    std::vector<std::thread> th;
    for (unsigned u = 0; u < T; u++)
        th.emplace_back([&, u] {
            for (size_t k = cut[u]; k < cut[u + 1]; k++) {
                const uint32_t i = order[k];
                append_stdout_pmls(txt[u], rs.id(i), job.pml.data() + rs.offsets[i], rs.len(i));
            }
        });
    for (auto &x : th) x.join();
    for (unsigned u = 0; u < T; u++) std::cout.write(txt[u].data(), (std::streamsize)txt[u].size());
}

// output_logs, src/utils.cpp:268-289
void write_log_lines(QueryRun &q, const Job &job, uint32_t i) {
    const ReadSet &rs = job.rs;
    // costs: the wall-clock nanoseconds a CPU strand spent per base -- nothing a GPU lane has; zeros
    std::string tc, ts, tf;
    for (std::string *t : {&tc, &ts, &tf}) { t->push_back('>'); t->append(rs.id(i)); t->push_back('\n'); }
    const uint16_t *sc = job.log_scan.data() + rs.offsets[i], *ff = job.log_ff.data() + rs.offsets[i];
    for (uint64_t k = 0, len = rs.len(i); k < len; k++) {
        tc += "0 ";
        ts += std::to_string(sc[k]); ts.push_back(' ');
        tf += std::to_string(ff[k]); tf.push_back(' ');
    }
    q.out.costs_file << tc << "\n";
    q.out.scans_file << ts << "\n";
    q.out.ff_file << tf << "\n";
}

// The general PML / ZML form, read by read: classification, --filter, text on stdout or the BPF records (one-thread writer), --logs.
void write_per_read(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    const Options &o = q.o;
    const ReadSet &rs = job.rs;
    std::vector<BpfWriter::Record> bpf;                               // the chunk's records, in emission order
    if (q.plan.to_bpf) bpf.reserve(rs.size());
    for (uint32_t i : order) {
        const uint64_t len = rs.len(i);
        const uint16_t *p = job.verdict_only ? nullptr : job.pml.data() + rs.offsets[i];
        if (o.classify) {                                             // write_mls, src/read_processor.cpp:565-578
            const bool found = job.verdict_only
                ? (job.bins_above[i] / (job.bins_above[i] + job.bins_below[i] + 0.0) > 0.50)      // classifier.cpp:119
                : q.classifier.classify(rs.id(i), p, len, o.bin_width, o.write_output_allowed() ? q.out.report : nullptr);
            if (o.filter && !o.no_output && (found != o.invert)) {
                const uint8_t *seq = (job.original.empty() ? rs.bases.data() : job.original.data()) + rs.offsets[i];
                std::cout << ">" << rs.id(i) << "\n";
                std::cout.write(reinterpret_cast<const char *>(seq), (std::streamsize)len);
                std::cout << "\n";
            }
        }
        if (o.write_output_allowed()) {
            if (o.write_stdout_enabled()) write_stdout_pmls(std::cout, rs.id(i), p, len);
            else bpf.push_back(BpfWriter::Record{rs.id(i), p, len});
            if (q.plan.logs) write_log_lines(q, job, i);
        }
    }
    if (q.plan.to_bpf) q.out.mls_file.append(bpf);
}

// A chunk's lines of a count, MEM or k-mer query in one write
void write_text(QueryRun &q, const std::string &txt) {
    if (txt.empty()) return;
    std::ostream &out = q.o.write_stdout_enabled() ? static_cast<std::ostream &>(std::cout) : q.out.matches_file;
    out.write(txt.data(), (std::streamsize)txt.size());
}

// --locate: a chunk's .locs lines in one write -- to stdout in place of the ordinary lines, or to the file beside theirs
void write_locs_text(QueryRun &q, const std::string &txt) {
    if (txt.empty()) return;
    std::ostream &out = q.o.write_stdout_enabled() ? static_cast<std::ostream &>(std::cout) : q.out.locs_file;
    out.write(txt.data(), (std::streamsize)txt.size());
}

void write_count_lines(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    std::string txt;
    if (!(q.plan.locate && q.o.write_stdout_enabled())) {
        txt.reserve(job.rs.size() * 32);
        for (uint32_t i : order) append_count_line(txt, job.rs.id(i), job.rs.len(i), job.matched[i], job.counts[i]);
        write_text(q, txt);
    }
    if (!q.plan.locate) return;
    const size_t n = job.rs.size();
    std::vector<uint64_t> item(n + 1, 0);                              // the item of read i, if it has one: the reads with matched > 0 before it
    for (size_t i = 0; i < n; i++) item[i + 1] = item[i] + (job.matched[i] > 0 ? 1u : 0u);
    txt.clear();
    txt.reserve(n * 48 + job.loc_pos.size() * 10);
    for (uint32_t i : order) {
        const bool has = job.matched[i] > 0;
        const uint64_t k = item[i], f = has ? job.loc_first[k] : 0;
        append_count_locs_line(txt, job.rs.id(i), job.rs.len(i), job.matched[i], has ? job.loc_occ[k] : 0, job.loc_pos.data() + f,
                               has ? job.loc_first[k + 1] - f : 0);
    }
    write_locs_text(q, txt);
}

// output_mems, src/utils.cpp:306-316 (file order: no prefetch)
void write_mem_lines(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    const size_t n = job.rs.size();
    std::string txt;
    txt.reserve(n * 32);
    std::vector<uint64_t> first(n + 1, 0);
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + job.n_mems[i];
    if (!(q.plan.locate && q.o.write_stdout_enabled())) {
        for (uint32_t i : order)
            for (uint64_t k = first[i]; k < first[i + 1]; k++) append_mem_line(txt, job.rs.id(i), job.mems[k]);
        write_text(q, txt);
    }
    if (!q.plan.locate) return;
    txt.clear();
    txt.reserve(job.mems.size() * 48 + job.loc_pos.size() * 10);
    for (uint32_t i : order)
        for (uint64_t k = first[i]; k < first[i + 1]; k++)
            append_mem_locs_line(txt, job.rs.id(i), job.mems[k].start, job.mems[k].end, job.loc_occ[k], job.loc_pos.data() + job.loc_first[k],
                                 job.loc_first[k + 1] - job.loc_first[k]);
    write_locs_text(q, txt);
}

// output_kmers, src/utils.cpp:258-266 (file order: no prefetch)
void write_kmer_lines(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    const size_t n = job.rs.size();
    std::string txt;
    txt.reserve(n * 32);
    std::vector<uint64_t> first(n + 1, 0);
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + job.n_runs[i];
    for (uint32_t i : order)
        append_kmer_line(txt, job.rs.id(i), job.rs.len(i), q.o.k, job.kmers_found[i], job.runs.data() + first[i], job.n_runs[i]);
    write_text(q, txt);
}

// one line per read (file order: no prefetch)
void write_kmer_occ_lines(QueryRun &q, const Job &job, const std::vector<uint32_t> &order) {
    std::string txt;
    txt.reserve(job.rs.size() * 32 + job.rs.bases.size() * 2);
    for (uint32_t i : order)
        append_kmer_occ_line(txt, job.rs.id(i), job.rs.len(i), q.o.k, job.occ_found[i], job.occ_sum[i], job.occ.data() + job.rs.offsets[i]);
    write_text(q, txt);
}

void write_job(QueryRun &q, Job &job) {
    const Options &o = q.o;
    const QueryPlan &plan = q.plan;
    const size_t n = job.rs.size();
    // nothing to write for this chunk (`--no-output` without a report or a filter): no record order needed either
    if (!o.write_output_allowed() && !(o.classify && (o.filter || q.out.report))) return;
    if (!q.out.bpf_pool && n >= 4096) q.out.bpf_pool.reset(new WorkerPool(q.bpf_threads));   // this stage's helpers (order, BPF gather)
    const std::vector<uint32_t> order = record_order(q, job);
    switch (plan.kind) {
    case QueryKind::MultiClassify: return write_multi_classify_lines(q, job, order);
    case QueryKind::Mem: return write_mem_lines(q, job, order);
    case QueryKind::Kmer: return write_kmer_lines(q, job, order);
    case QueryKind::Count: return write_count_lines(q, job, order);
    case QueryKind::KmerOcc: return write_kmer_occ_lines(q, job, order);
    default: break;                                                   // the PML / ZML forms
    }
    if (q.out.sa_file.is_open()) write_sa_records(q, job, order);
    if (plan.to_bpf && !o.classify && !plan.logs && !q.bpf_serial) return write_bpf_pooled(q, job, order);
    if (!o.classify && o.write_stdout_enabled() && job.rs.bases.size() >= (1u << 22)) return write_stdout_parallel(job, order);
    write_per_read(q, job, order);
}

void write_stage(QueryRun &q) {
    Job *j = nullptr;
    while (q.done_q.pop(j)) {
        bool failed;
        { std::lock_guard<std::mutex> g(q.err_m); failed = q.write_error != nullptr; }
        if (!failed) {
            try {
                const auto tw = std::chrono::steady_clock::now();
                write_job(q, *j);
                q.write_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
            } catch (...) {
                std::lock_guard<std::mutex> g(q.err_m);
                q.write_error = std::current_exception();
            }
        }
        q.free_q.push(j);
    }
}

// whatever happens in run_query, the two threads are released and joined before the streams and jobs go away
struct Joiner {
    HandOff<Job *> &free_q, &done_q;
    std::thread &parser, &writer;
    ~Joiner() {
        free_q.abandon();                                             // parser: stop taking jobs
        done_q.close();                                               // writer: drain what was handed over, then stop
        if (parser.joinable()) parser.join();
        if (writer.joinable()) writer.join();
    }
};

// ---- stage 2: the GPU calls, in input order
void gpu_stage(QueryRun &q) {
    const Options &o = q.o;
    Job *jp = nullptr;
    while (q.parsed_q.pop(jp)) {
        Job &job = *jp;
        ReadSet &rs = job.rs;
        const size_t n = rs.size();
        { std::lock_guard<std::mutex> g(q.err_m); if (q.write_error) std::rethrow_exception(q.write_error); }
        if (n == 0) { q.free_q.push(jp); continue; }
        if (o.reverse)                                                // src/read_processor.cpp:49-51
            for (size_t i = 0; i < n; i++) std::reverse(rs.bases.begin() + rs.offsets[i], rs.bases.begin() + rs.offsets[i + 1]);
        job.original.clear();                                         // --filter echoes the read as given
        if (o.ignore_illegal_chars == 1) {                            // check_alphabet, src/move_structure.cpp:389-395
            if (o.filter) job.original.assign(rs.bases);
            for (auto &c : rs.bases)
                if (q.desc.code_of[c] == 0xFF) c = 'A';
        }
        job.prepare(q.plan, o, q.num_species, q.pin_buffers);
        const std::vector<size_t> sb = shard_bounds(rs, o.gpus);
        std::vector<std::string> errors((size_t)o.gpus);
        std::vector<ShardOut> shards((size_t)o.gpus);
        auto tg = std::chrono::steady_clock::now();
        auto work = [&](int g) {
            const size_t a = sb[g], b = sb[g + 1];
            if (a == b) return;
            if (run_shard(q, q.handles[g], job, a, b, shards[(size_t)g]) != MOVI_OK) errors[g] = movi_last_error();
        };
        if (o.gpus == 1) {
            work(0);
        } else {
            std::vector<std::thread> th;
            for (int g = 0; g < o.gpus; g++) th.emplace_back(work, g);
            for (auto &t : th) t.join();
        }
        { const double dtg = std::chrono::duration<double>(std::chrono::steady_clock::now() - tg).count(); q.gpu_seconds += dtg; if (q.chunk_gpu_s.size() < 64) q.chunk_gpu_s.push_back(dtg); }
        for (const auto &e : errors)
            if (!e.empty()) throw EngineError(e);
        if (o.kmer) {                                                 // the shards' runs in read order
            job.runs.clear();
            for (auto &s : shards) job.runs.insert(job.runs.end(), s.runs.begin(), s.runs.end());
        }
        if (o.mem) {                                                  // the shards' MEMs in read order
            job.mems.clear();
            for (auto &s : shards) job.mems.insert(job.mems.end(), s.mems.begin(), s.mems.end());
        }
        if (q.plan.locate) {                                          // the shards' items in read order, their firsts made the chunk's
            job.loc_occ.clear(); job.loc_pos.clear();
            job.loc_first.assign(1, 0);
            for (auto &s : shards) {
                const uint64_t base = job.loc_pos.size();
                job.loc_occ.insert(job.loc_occ.end(), s.loc_occ.begin(), s.loc_occ.end());
                for (size_t k = 1; k < s.loc_first.size(); k++) job.loc_first.push_back(base + s.loc_first[k]);
                job.loc_pos.insert(job.loc_pos.end(), s.loc_pos.begin(), s.loc_pos.end());
            }
        }
        if (o.kmer_occ)                                               // the summary's totals (--no-output still prints them)
            for (size_t i = 0; i < n; i++) { q.occ_found_total += job.occ_found[i]; q.occ_sum_total += job.occ_sum[i]; }
        q.reads_done += n;
        q.bases_done += rs.bases.size();
        q.done_q.push(jp);
    }
}

void report_run(const QueryRun &q) {
    const Options &o = q.o;
    // (the parser's warm-up touched the input before t1: its seconds count as read processing, although they ran beside the index load)
    const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - q.t1).count() + q.warm_seconds;
    std::cerr << "[movi] " << q.reads_done << " reads are processed.\n";
    std::cerr << "[movi] Time measured for processing the reads: " << total << " s (" << q.bases_done << " bases; GPU calls "
              << q.gpu_seconds << " s; input scanned ahead of the clock and added to it: " << q.warm_seconds << " s)\n";
    if (o.verbose) {
        const BatchReader::PhaseTimes pt = q.reader->phase_times();
        std::cerr << "[movi] Parser phases: newline scan " << pt.prescan << " s, batch cut " << pt.cut << " s, lengths " << pt.lengths
                  << " s, copy " << pt.copy << " s; " << pt.bulk_reads << " of " << pt.reads << " reads cut in bulk (" << pt.closed_reads << " by the closed form)\n";
    }
    if (o.verbose) {                                                   // chunk by chunk: the first chunk's parse runs alone, the others beside the GPU calls
        std::cerr << "[movi] Chunks: parse";
        for (double x : q.chunk_parse_s) std::cerr << " " << x;
        std::cerr << " s; GPU calls";
        for (double x : q.chunk_gpu_s) std::cerr << " " << x;
        std::cerr << " s\n";
        std::cerr << "[movi] Chunk phases (cut [of which waiting for the scan-ahead] / lengths / copy | the scan-ahead helper's own time, ms):";
        BatchReader::PhaseTimes prev;
        for (const auto &p : q.chunk_phases) {
            std::cerr << " " << (p.cut - prev.cut) * 1e3 << "[" << (p.scan_wait - prev.scan_wait) * 1e3 << "]/" << (p.lengths - prev.lengths) * 1e3 << "/"
                      << (p.copy - prev.copy) * 1e3 << "|" << (p.scan_busy - prev.scan_busy) * 1e3;
            prev = p;
        }
        std::cerr << "\n";
    }
    if (o.verbose && q.out.bpf_pool) {
        const BpfWriter::Times bt = q.out.mls_file.times();
        std::cerr << "[movi] BPF writer: gather " << bt.gather << " s, waiting for a free slab " << bt.wait << " s (" << q.out.bpf_pool->size()
                  << " threads); write() " << bt.write << " s on its own thread\n";
    }
    if (o.verbose)                                                     // the three pipeline stages run side by side: the slowest one bounds the command
        std::cerr << "[movi] Stage times: parse " << q.parse_seconds << " s, GPU calls " << q.gpu_seconds << " s, order + write "
                  << q.write_seconds << " s (page-locked chunk buffers: " << (q.pin_buffers ? "yes" : (q.pin_chunks ? "reads" : "no")) << ")\n";
}

int run_query(const Options &o) {
    QueryRun q(o);
    check_inputs_and_devices(q);
    q.t0 = std::chrono::steady_clock::now();
    open_input_and_warm_parser(q);
    load_handles(q);
    configure_handles(q);
    check(movi_index_get_desc(q.handles[0], &q.desc), "index description");
    const std::string index_type = index_type_name(q.desc.mode);
    std::cerr << "[movi] The " << index_type << " index is being used (r = " << q.desc.r << ").\n";
    std::cerr << "[movi] Time measured for loading the index: "
              << std::chrono::duration<double>(std::chrono::steady_clock::now() - q.t0).count() << " s\n";

    // input: file or stdin (setup_input_file, src/movi.cpp:106-118) -- opened above, while the index loaded
    if (o.read_file != "-" && !q.file_in.good()) throw std::runtime_error("The input file " + o.read_file + " does not exist.");
    open_outputs(o, q.plan, index_type, q.classifier, q.out);

    if (q.warmer.joinable()) q.warmer.join();
    q.t1 = std::chrono::steady_clock::now();
    if (!q.reader) q.reader = open_reader(o.read_file, *q.in, o.prefetch ? 4 * o.strands : 1, q.map);   // (stdin) src/movi.cpp:283, :326
    // chunks of >= 2^25 bases and >= 2^15 reads (long reads: up to 2^30 bases): one GPU lane walks one read, so a chunk needs
    // READS to fill the lanes (2^25 bases of 150 bp reads = 224 k reads: more than the 147 k lanes the PML kernel keeps
    // resident) -- but the host stages (text parsing ~1.4 GB/s, BPF writing) are what bounds the command, and they only overlap
    // the GPU calls and each other across chunks: better several half-filled launches than one full one

    // Page-locked chunk buffers (MOVI_PINNED=1): with the reads and the result vector in page-locked memory the engine's
    // *_host entry points cut a call into pieces whose upload, walk and download overlap (include/movi_hip.h).  Measured
    // in this command and NOT the default (profiles/r03_cli_path.txt): its chunks (2^25 bases of short reads, 2^15 long
    // reads) are a quarter of what the overlapped path needs to pay -- each piece must still fill the GPU -- and a run makes
    // a handful of calls, so the path's one-time set-up (six streams with staging) is never earned back: GPU calls of
    // 1 M x 150 bp 0.021 s pageable, 0.084 s page-locked; 100 k x 10 kbp 0.15 s / 0.31 s.  (Round 5: page-locked read buffers with
    // the calls NOT cut into pieces -- one direct upload per chunk -- 8.1 - 9.5 against 8.6 - 9.9 ms of GPU calls per 150 Mbases, the
    // command 12.0 - 13.1 against 12.5 - 12.6 ms, and with the BPF file 50 - 57 against 32 - 36 ms: dropped.  tools/r05_scan.sh)  The command's own pipeline
    // (parse | GPU calls | order + write, three chunks in flight) already overlaps the transfers with the other stages.
    if (q.pin_buffers)
        for (Job &j : q.jobs) j.rs.bases.set_allocator(pinned_alloc, pinned_free);
    for (Job &j : q.jobs) q.free_q.push(&j);
    q.bpf_serial = std::getenv("MOVI_BPF_SERIAL") != nullptr;
    if (const char *e = std::getenv("MOVI_BPF_THREADS")) q.bpf_threads = (unsigned)std::max(1, std::atoi(e));

    std::thread parser(parse_stage, std::ref(q));
    std::thread writer(write_stage, std::ref(q));
    Joiner joiner{q.free_q, q.done_q, parser, writer};
    warm_up_engine(q);
    gpu_stage(q);
    // end of input (or a parse error, which surfaces after every earlier chunk has been written)
    q.done_q.close();
    writer.join();
    q.free_q.abandon();
    parser.join();
    if (q.write_error) std::rethrow_exception(q.write_error);
    if (q.parse_error) std::rethrow_exception(q.parse_error);
    q.out.mls_file.close();
    if (q.out.sa_file.is_open()) q.out.sa_file.close();
    if (q.out.locs_file.is_open()) q.out.locs_file.close();
    report_run(q);
    if (o.kmer_occ) {                                                  // the two totals the reference's --kmer-count prints (include/sequitur.hpp:12-14)
        std::ostream &sum_out = o.write_stdout ? std::cerr : std::cout;   // (--stdout: the lines own stdout)
        sum_out << "Number of kmers found in the index:\t" << q.occ_found_total << "\n"
                << "Sum of the counts of found k-mers:\t" << q.occ_sum_total << "\n";
    }
    std::cout.flush();
    return 0;
}

// `movi null`: Classifier::generate_null_statistics (src/classifier.cpp:12-22, driver src/movi.cpp:732-736).
int run_null(const Options &o) {
    const std::string pattern_file = o.index_dir + "/null_reads.fasta";
    if (o.gen_reads) {
        unsigned seed = (unsigned)std::time(nullptr);                 // srand(time(0)), src/utils.cpp:431
        if (const char *e = std::getenv("MOVI_NULL_SEED")) seed = (unsigned)std::strtoul(e, nullptr, 10);
        const size_t n = generate_null_reads(o.ref_file, pattern_file, seed);
        std::cerr << "[movi] " << n << " null reads written to " << pattern_file << "\n";
    }
    movi_index_t *h = nullptr;
    check(movi_index_load(o.device, o.index_dir.c_str(), &h), "loading the index");
    struct Closer { movi_index_t *h; ~Closer() { movi_index_destroy(h); } } closer{h};
    const std::vector<std::string> seqs = read_fasta_sequences(pattern_file);
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets(1, 0);
    for (const std::string &s : seqs) {
        bases.insert(bases.end(), s.begin(), s.end());
        offsets.push_back(bases.size());
    }
    std::vector<uint16_t> ml(bases.size());
    check(o.zml ? movi_zml_host(h, bases.data(), offsets.data(), seqs.size(), ml.data(), nullptr, nullptr)
                : movi_pml_host(h, bases.data(), offsets.data(), seqs.size(), ml.data(), nullptr, nullptr),
          "null statistics");
    const std::vector<uint64_t> values(ml.begin(), ml.end());        // ml_stats, emission order per read
    const NullStats st = compute_null_stats(values);
    const std::string name = o.index_dir + "/movi." + o.query_type() + ".nulldb";
    write_null_db(name, st, values);
    std::cerr << "[movi] Null database statistics: mean_null_stat: " << st.mean << " percentile_value: " << st.percentile_value
              << " (" << st.num_values << " values) -> " << name << "\n";
    return 0;
}

// `movi build-SA` (src/movi.cpp:640-..., find_sampled_SA_entries + serialize_sampled_SA): INDEX/ssa.movi from index.movi alone --
// nothing is fetched from the text; the array is built on the GPU (movi_ssa_build).
int run_build_sa(const Options &o) {
    const auto t0 = std::chrono::steady_clock::now();
    movi_index_t *h = nullptr;
    check(movi_index_load(o.device, o.index_dir.c_str(), &h), "loading the index");
    struct Closer { movi_index_t *h; ~Closer() { movi_index_destroy(h); } } closer{h};
    const auto t1 = std::chrono::steady_clock::now();
    check(movi_ssa_build(h, o.sample_rate, nullptr), "building the sampled suffix array");
    const auto t2 = std::chrono::steady_clock::now();
    const std::string name = o.index_dir + "/ssa.movi";
    check(movi_ssa_save(h, name.c_str()), "writing ssa.movi");
    uint64_t n_samples = 0;
    check(movi_ssa_get(h, nullptr, nullptr, 0, &n_samples), "the sampled suffix array");
    std::cerr << "[movi] " << n_samples << " sampled SA entries (sample rate " << o.sample_rate << ") written to " << name << " (index load "
              << std::chrono::duration<double>(t1 - t0).count() << " s, build " << std::chrono::duration<double>(t2 - t1).count() << " s)\n";
    return 0;
}

// `movi color` (src/movi.cpp: build_doc_pats + build_doc_sets + flat_and_serialize_colors_vectors): INDEX/doc_sets_flat.bin from index.movi and
// INDEX/ref.fa.doc_offsets (+ ref.fa.doc_ids), on the GPU.
int run_color(const Options &o) {
    const DocInfo docs = load_doc_info(o.index_dir);
    if (docs.offsets.empty()) throw std::runtime_error(o.index_dir + "/ref.fa.doc_offsets holds no document");
    const auto t0 = std::chrono::steady_clock::now();
    movi_index_t *h = nullptr;
    check(movi_index_load(o.device, o.index_dir.c_str(), &h), "loading the index");
    struct Closer { movi_index_t *h; ~Closer() { movi_index_destroy(h); } } closer{h};
    if (const char *e = std::getenv("MOVI_COLOR_CHUNK_KEYS"))           // test hook: several chunks on a small text
        check(movi_set_option(h, "color_chunk_keys", std::atoll(e)), "MOVI_COLOR_CHUNK_KEYS");
    // a sampled suffix array that `movi build-SA` left in the directory is used as it is (any rate); without one the build makes its own
    const bool have_ssa = std::ifstream(o.index_dir + "/ssa.movi").good();
    if (have_ssa) check(movi_ssa_load(h, (o.index_dir + "/ssa.movi").c_str()), "loading the sampled suffix array");
    const auto t1 = std::chrono::steady_clock::now();
    check(movi_color_build(h, docs.offsets.data(), docs.ids.empty() ? nullptr : docs.ids.data(), docs.offsets.size(), nullptr), "building the document sets");
    const auto t2 = std::chrono::steady_clock::now();
    const std::string name = o.index_dir + "/doc_sets_flat.bin";
    check(movi_color_save(h, name.c_str()), "writing doc_sets_flat.bin");
    const auto t3 = std::chrono::steady_clock::now();
    uint64_t flat_size = 0;
    uint32_t species = 0;
    check(movi_color_get(h, &flat_size, nullptr, 0, nullptr, 0, &species, nullptr, 0), "the colour tables");
    double walk = 0, sort = 0, number = 0, chunks = 0;
    (void)movi_index_info(h, "color_walk_seconds", &walk);
    (void)movi_index_info(h, "color_sort_seconds", &sort);
    (void)movi_index_info(h, "color_number_seconds", &number);
    (void)movi_index_info(h, "color_chunks", &chunks);
    std::cerr << "[movi] The flat color table (flat_colors.size(): " << flat_size << ", " << docs.offsets.size() << " documents, " << species
              << " species) is written to " << name << " (index load " << std::chrono::duration<double>(t1 - t0).count() << " s, build "
              << std::chrono::duration<double>(t2 - t1).count() << " s" << (have_ssa ? " on ssa.movi" : ", its own sampled suffix array included") << ": walk " << walk << " s, sort " << sort << " s in " << (uint64_t)chunks
              << " chunk(s), numbering " << number << " s; write " << std::chrono::duration<double>(t3 - t2).count() << " s)\n";
    return 0;
}

// `movi plan`: the host-side batching + record order, without any GPU work.
int run_plan(const Options &o) {
    std::ifstream file_in;
    std::istream *in = &std::cin;
    if (o.read_file != "-") {
        file_in.open(o.read_file.c_str());
        if (!file_in.good()) throw std::runtime_error("The input file " + o.read_file + " does not exist.");
        in = &file_in;
    }
    InputMapping map;
    std::unique_ptr<BatchReader> reader_ptr = open_reader(o.read_file, *in, o.prefetch ? 4 * o.strands : 1, map);
    BatchReader &reader = *reader_ptr;
    ReadSet rs;
    uint64_t plan_chunk = 1ull << 28;
    if (const char *e = std::getenv("MOVI_CHUNK_BASES")) plan_chunk = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));   // test hook
    std::unique_ptr<WorkerPool> plan_pool;                             // test hook: the record order by a pool, as `movi query`'s writer stage computes it
    if (const char *e = std::getenv("MOVI_PLAN_THREADS")) plan_pool.reset(new WorkerPool((unsigned)std::max(1, std::atoi(e))));
    while (reader.next_chunk(rs, plan_chunk)) {
        std::vector<uint64_t> cost(rs.size());
        for (size_t i = 0; i < rs.size(); i++) cost[i] = rs.len(i);
        std::vector<uint32_t> order;
        if (o.prefetch) order = strand_order(rs, cost, o.strands, plan_pool.get());
        else for (size_t i = 0; i < rs.size(); i++) order.push_back((uint32_t)i);
        for (uint32_t i : order) std::cout << rs.batch_of[i] << "\t" << rs.id(i) << "\t" << rs.len(i) << "\n";
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::ios::sync_with_stdio(false);
    try {
        Options o = parse_args(argc, argv);
        if (o.command == "help") {
            std::cerr << usage();
            return 0;
        }
        if (o.command == "view") return view_bpf(o, std::cout);
        if (o.command == "plan") return run_plan(o);
        if (o.command == "null") return run_null(o);
        if (o.command == "build") {                                    // --color: the document offsets with the index, then the colour step
            const int rc = run_build(o);
            return (rc == 0 && o.color) ? run_color(o) : rc;
        }
        if (o.command == "rlbwt") return run_rlbwt(o);
        if (o.command == "color") return run_color(o);
        if (o.command == "build-SA") return run_build_sa(o);
        return run_query(o);
    } catch (const UsageError &e) {
        std::cerr << "Error parsing command line options: " << e.what() << "\n" << usage();
        return 1;
    } catch (const std::exception &e) {                               // src/movi.cpp:744-747
        std::cerr << "Error: " << e.what() << "\n";
        return 1;
    }
}
