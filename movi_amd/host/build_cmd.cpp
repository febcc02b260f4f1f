// build_cmd.cpp -- `movi build`: FASTA -> DIR/index.movi, in memory, without the reference's external pipeline
// (prepare_ref + pfp-thresholds + movi-<type> build, src/movi_launcher.cpp:190-242).  The constructor is the one the tests
// hold to the reference's index-size known answers (constructor.hpp: SA-IS, Kasai LCP, leftmost-minimum thresholds, the
// run-length BWT, rows, blocked / sampled ids), compiled into the host binary; texts up to 2^31 characters.
// `movi build --preprocessed`: REF.bwt.heads + REF.bwt.len (+ REF.thr_pos) -> DIR/index.movi, the reference's route for texts the
// in-memory constructor cannot take (an external BWT tool, then `movi rlbwt`, then this; src/move_structure_build.cpp:143-202,
// src/utils.cpp:150-200).  The files are parsed and checked here; the table is built on the GPU (movi_build_from_rlbwt).
// `movi build --gpu-build`: the FASTA's text as above, then suffix array, BWT, LCP, thresholds and the table on the GPU
// (movi_build_from_text): texts up to 2^32 - 2^20 characters, no external tool.
// `movi rlbwt`: build_rlbwt, src/movi.cpp:505-559.
#include <chrono>
#include <iostream>
#include <memory>

#include "../../include/movi_hip.h"
#include "../csrc/movi_build.hpp"
#include "constructor.hpp"
#include "options.hpp"
#include "reads.hpp"

namespace movi_host {

namespace {

using namespace movi_constructor;

struct HostFree { void operator()(void *p) const { (void)movi_host_free(p); } };   // what the engine hands out (movi_host_alloc)
template <typename T> using HostPtr = std::unique_ptr<T, HostFree>;

double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// The FASTA's text as the CPU constructor cleans it, and where its documents end.
std::vector<uint8_t> read_text(const Options &o, std::vector<uint64_t> &doc_ends) {
    std::vector<uint8_t> text;
    if (!text_from_fasta(o.ref_file, o.separators, text, &doc_ends)) throw std::runtime_error("cannot open " + o.ref_file);
    if (text.empty()) throw std::runtime_error("no sequence in " + o.ref_file);
    return text;
}

// The table of a run-length BWT that has passed rlbwt_check, built on the GPU.
HostPtr<void> gpu_image(const Options &o, int mode, const uint8_t *heads, const uint64_t *lens, const uint64_t *thr, uint64_t R, size_t &bytes) {
    void *image = nullptr;
    if (movi_build_from_rlbwt(o.device, (uint32_t)mode, heads, lens, thr, R, &image, &bytes) != MOVI_OK)
        throw std::runtime_error(std::string("building the index on the GPU: ") + movi_last_error());
    return HostPtr<void>(image);
}

void report(const Options &o) {
    std::cerr << "[movi] The " << o.index_type << " index is written to " << o.index_dir << "/index.movi\n";
    if (o.color) std::cerr << "[movi] The document offsets are written to " << o.index_dir << "/ref.fa.doc_offsets\n";
}

int run_build_cpu(const Options &o, int mode) {
    std::vector<uint64_t> doc_ends;
    std::vector<uint8_t> text = read_text(o, doc_ends);
    if ((uint64_t)text.size() + 1 >= (1ull << 31))
        throw std::runtime_error("text too long for the in-memory constructor (2^31 characters, reverse complements included)");
    const std::vector<uint8_t> image = image_from_rlbwt(rlbwt_from_text(text), mode);
    write_index_dir(o.index_dir, image.data(), image.size(), o.color ? &doc_ends : nullptr);
    report(o);
    return 0;
}

int run_build_preprocessed(const Options &o, int mode) {
    const bool with_thr = movi::build_mode_thresholds((uint32_t)mode);
    const Rlbwt rl = read_rlbwt_files(o.ref_file, with_thr);
    const uint64_t R = rl.heads.size(), *thr = with_thr ? rl.thr.data() : nullptr;
    movi::RlbwtInfo info;
    movi::RlbwtArray which;
    std::string why;
    if (!movi::rlbwt_check(rl.heads.data(), rl.lens.data(), thr, R, info, which, why))
        throw std::runtime_error(o.ref_file + (which == movi::kRlbwtHeads ? ".bwt.heads" : which == movi::kRlbwtLens ? ".bwt.len" : ".thr_pos") + ": " + why);
    const auto t0 = std::chrono::steady_clock::now();
    size_t image_bytes = 0;
    const HostPtr<void> image = gpu_image(o, mode, rl.heads.data(), rl.lens.data(), thr, R, image_bytes);
    const double build_s = seconds_since(t0);
    write_index_dir(o.index_dir, image.get(), image_bytes, nullptr);
    std::cerr << "[movi] The " << o.index_type << " index (" << R << " BWT runs, " << info.n << " characters" << (info.sep ? ", separators" : "")
              << ") is written to " << o.index_dir << "/index.movi (build on the GPU " << build_s << " s)\n";
    return 0;
}

// `movi build --gpu-build`: the text as the CPU constructor cleans it, everything after it on the GPU.
int run_build_gpu(const Options &o, int mode) {
    std::vector<uint64_t> doc_ends;
    const std::vector<uint8_t> text = read_text(o, doc_ends);
    movi_text_build_opts_t opts;
    memset(&opts, 0, sizeof(opts));
    opts.verify = o.verify ? 1u : 0u;
    movi_text_build_stats_t st;
    memset(&st, 0, sizeof(st));
    const auto t0 = std::chrono::steady_clock::now();
    HostPtr<void> image;
    size_t image_bytes = 0;
    if (o.keep) {                                                  // the three arrays come down, are written, and go up again
        uint8_t *heads = nullptr;
        uint64_t *lens = nullptr, *thr = nullptr, R = 0;
        if (movi_rlbwt_from_text(o.device, text.data(), text.size(), &opts, &heads, &lens, &thr, &R, &st) != MOVI_OK)
            throw std::runtime_error(std::string("building the run-length BWT on the GPU: ") + movi_last_error());
        const HostPtr<uint8_t> heads_owner(heads);
        const HostPtr<uint64_t> lens_owner(lens), thr_owner(thr);
        write_rlbwt_files(o.ref_file, heads, lens, thr, R);
        image = gpu_image(o, mode, heads, lens, thr, R, image_bytes);
    } else {
        void *p = nullptr;
        if (movi_build_from_text(o.device, (uint32_t)mode, text.data(), text.size(), &opts, &p, &image_bytes, &st) != MOVI_OK)
            throw std::runtime_error(std::string("building the index on the GPU: ") + movi_last_error());
        image.reset(p);
    }
    const double build_s = seconds_since(t0);
    write_index_dir(o.index_dir, image.get(), image_bytes, o.color ? &doc_ends : nullptr);
    report(o);
    if (o.keep) std::cerr << "[movi] The run-length BWT and the thresholds are kept in " << o.ref_file << ".bwt.heads, .bwt.len and .thr_pos\n";
    std::cerr << "[movi] built on the GPU: " << text.size() << " characters, " << st.original_r << " BWT runs, " << st.rounds
              << " doubling rounds" << (st.verified ? ", verified" : "") << "; seconds: upload " << st.seconds[0] << ", suffix sort " << st.seconds[1]
              << ", BWT and runs " << st.seconds[2] << ", LCP " << st.seconds[3] << ", thresholds " << st.seconds[4] << ", verify " << st.seconds[5]
              << ", whole build " << build_s << "\n";
    return 0;
}

}  // namespace

// build_rlbwt, src/movi.cpp:505-559: FILE.heads (one byte per maximal run) and FILE.len (five little-endian bytes per run).  As there,
// the file is read as chars until EOF: a byte 0xFF ends it, and an empty file gives one run of that byte with length 0.
int run_rlbwt(const Options &o) {
    if (!std::ifstream(o.bwt_file).good()) throw std::runtime_error("[build_rlbwt] Failed to open the BWT file: " + o.bwt_file);
    InputMapping map;
    (void)map.map(o.bwt_file);
    const uint8_t *b = map.bytes();
    size_t n = map.p != MAP_FAILED ? map.n : 0;
    if (const void *eof = n ? memchr(b, 0xFF, n) : nullptr) n = (size_t)(static_cast<const uint8_t *>(eof) - b);
    std::ofstream len_file(o.bwt_file + ".len", std::ios::out | std::ios::binary);
    if (!len_file.good()) throw std::runtime_error("[build_rlbwt] Failed to open the length file: " + o.bwt_file + ".len");
    std::ofstream heads_file(o.bwt_file + ".heads", std::ios::out | std::ios::binary);
    if (!heads_file.good()) throw std::runtime_error("[build_rlbwt] Failed to open the heads file: " + o.bwt_file + ".heads");
    std::vector<char> heads, lens;
    auto flush = [&]() {
        heads_file.write(heads.data(), (std::streamsize)heads.size());
        len_file.write(lens.data(), (std::streamsize)lens.size());
        heads.clear();
        lens.clear();
    };
    uint64_t r = 0;
    auto put_run = [&](uint8_t c, uint64_t len) {
        heads.push_back((char)c);
        for (int k = 0; k < 5; k++) lens.push_back((char)(len >> (8 * k)));
        r += 1;
        if (heads.size() >= (1u << 20)) flush();
    };
    if (n == 0) put_run(0xFF, 0);
    for (size_t i = 0, j = 0; i < n; i = j) {
        while (j < n && b[j] == b[i]) j++;
        put_run(b[i], j - i);
    }
    flush();
    heads_file.close();
    len_file.close();
    if (!heads_file.good() || !len_file.good()) throw std::runtime_error("cannot write " + o.bwt_file + ".heads / .len");
    std::cerr << "[movi] " << r << " runs written to " << o.bwt_file << ".heads and " << o.bwt_file << ".len\n";
    return 0;
}

int run_build(const Options &o) {
    static const struct { const char *name; int mode; } kTypes[] = {                   // src/movi_launcher.cpp:56-66
        {"regular-thresholds", 6}, {"blocked-thresholds", 8}, {"sampled-thresholds", 7},
        {"regular", 3}, {"blocked", 2}, {"sampled", 5},
    };
    int mode = -1;
    for (const auto &t : kTypes)
        if (o.index_type == t.name) mode = t.mode;
    if (mode < 0)
        throw UsageError("index type '" + o.index_type + "' is not supported (regular-thresholds, blocked-thresholds, "
                         "sampled-thresholds, regular, blocked, sampled)");
    if (o.preprocessed) return run_build_preprocessed(o, mode);
    if (o.gpu_build) return run_build_gpu(o, mode);
    return run_build_cpu(o, mode);
}

}  // namespace movi_host
