// build_cmd.cpp -- `movi build`: FASTA -> DIR/index.movi, in memory, without the reference's external pipeline
// (prepare_ref + pfp-thresholds + movi-<type> build, src/movi_launcher.cpp:190-242).  The constructor is the one the tests
// hold to the reference's index-size known answers (tools/build_index.cpp: SA-IS, Kasai LCP, leftmost-minimum
// thresholds, rows, blocked / sampled ids), compiled into the host binary; texts up to 2^31 characters.
// `movi build --preprocessed`: REF.bwt.heads + REF.bwt.len (+ REF.thr_pos) -> DIR/index.movi, the reference's route for texts the
// in-memory constructor cannot take (an external BWT tool, then `movi rlbwt`, then this; src/move_structure_build.cpp:143-202,
// src/utils.cpp:150-200).  The files are parsed and checked here; the table is built on the GPU (movi_build_from_rlbwt).
// `movi build --gpu-build`: the FASTA's text as above, then suffix array, BWT, LCP, thresholds and the table on the GPU
// (movi_build_from_text): texts up to 2^32 - 2^20 characters, no external tool.
// `movi rlbwt`: build_rlbwt, src/movi.cpp:505-559.
#define MOVI_BUILD_INDEX_NO_MAIN 1
#include "../../tools/build_index.cpp"

#include <chrono>

#include "../../include/movi_hip.h"
#include "../csrc/movi_build.hpp"
#include "options.hpp"
#include "reads.hpp"

namespace movi_host {

namespace {

uint64_t get5(const uint8_t *p) {                                  // a 5-byte little-endian value
    uint64_t v = 0;
    memcpy(&v, p, 5);
    return v;
}

int run_build_preprocessed(const Options &o, int mode) {
    const std::string heads_path = o.ref_file + ".bwt.heads", len_path = o.ref_file + ".bwt.len", thr_path = o.ref_file + ".thr_pos";
    const bool with_thr = movi::build_mode_thresholds((uint32_t)mode);
    // compute_length_from_bwt, src/move_structure_build.cpp:152-181
    InputMapping heads_map, len_map, thr_map;
    if (!std::ifstream(heads_path).good()) throw std::runtime_error("[build] Failed to open the heads file: " + heads_path);
    if (!heads_map.map(heads_path)) throw std::runtime_error(heads_path + ": holds no run");
    if (!std::ifstream(len_path).good()) throw std::runtime_error("[build] Failed to open the len file: " + len_path);
    (void)len_map.map(len_path);
    const uint64_t R = heads_map.n, len_bytes = len_map.p != MAP_FAILED ? len_map.n : 0;
    if (len_bytes % 5 != 0) throw std::runtime_error(len_path + ": " + std::to_string(len_bytes) + " bytes is not a multiple of 5 (one 5-byte length per run)");
    if (len_bytes / 5 != R)
        throw std::runtime_error(len_path + " holds " + std::to_string(len_bytes / 5) + " lengths but " + heads_path + " holds " + std::to_string(R) + " run heads");
    std::vector<uint64_t> lens(R), thr;
    for (uint64_t k = 0; k < R; k++) lens[k] = get5(len_map.bytes() + 5 * k);
    if (with_thr) {                                                // read_thresholds, src/utils.cpp:150-200; not opened for the other types
        if (!std::ifstream(thr_path).good()) throw std::runtime_error("[read_thresholds] open() file " + thr_path + " failed");
        (void)thr_map.map(thr_path);
        const uint64_t thr_bytes = thr_map.p != MAP_FAILED ? thr_map.n : 0;
        if (thr_bytes % 5 != 0)
            throw std::runtime_error("[read_thresholds] invilid file " + thr_path + ": " + std::to_string(thr_bytes) + " bytes is not a multiple of 5");
        if (thr_bytes / 5 != R)
            throw std::runtime_error(thr_path + " holds " + std::to_string(thr_bytes / 5) + " thresholds but " + heads_path + " holds " + std::to_string(R) + " run heads");
        thr.resize(R);
        // when the thresholds overflow 5 bytes the reference recovers the true values: a sudden drop to less than a tenth of the last
        // value, which was not small itself, is one more wrap (:172-196; unsigned arithmetic as there)
        const uint64_t kMax5 = 1ull << 40;
        uint64_t wraps = 0;
        for (uint64_t k = 0; k < R; k++) {
            const uint64_t t = get5(thr_map.bytes() + 5 * k);
            if (k > 0 && t != 0 && t < (thr[k - 1] - wraps * kMax5) / 10 && (thr[k - 1] - wraps * kMax5) > kMax5 / 10) wraps += 1;
            thr[k] = t + wraps * kMax5;
        }
    }
    movi::RlbwtInfo info;
    movi::RlbwtArray which;
    std::string why;
    if (!movi::rlbwt_check(heads_map.bytes(), lens.data(), with_thr ? thr.data() : nullptr, R, info, which, why))
        throw std::runtime_error((which == movi::kRlbwtHeads ? heads_path : which == movi::kRlbwtLens ? len_path : thr_path) + ": " + why);
    const auto t0 = std::chrono::steady_clock::now();
    void *image = nullptr;
    size_t image_bytes = 0;
    if (movi_build_from_rlbwt(o.device, (uint32_t)mode, heads_map.bytes(), lens.data(), with_thr ? thr.data() : nullptr, R, &image, &image_bytes) != MOVI_OK)
        throw std::runtime_error(std::string("building the index on the GPU: ") + movi_last_error());
    const auto t1 = std::chrono::steady_clock::now();
    mkdir(o.index_dir.c_str(), 0777);
    const std::string name = o.index_dir + "/index.movi";
    std::ofstream f(name, std::ios::binary);
    f.write(static_cast<const char *>(image), (std::streamsize)image_bytes);
    f.close();
    const bool ok = f.good();
    (void)movi_host_free(image);
    if (!ok) throw std::runtime_error("cannot write " + name);
    std::cerr << "[movi] The " << o.index_type << " index (" << R << " BWT runs, " << info.n << " characters" << (info.sep ? ", separators" : "")
              << ") is written to " << name << " (build on the GPU " << std::chrono::duration<double>(t1 - t0).count() << " s)\n";
    return 0;
}

// `movi build --gpu-build`: the text as the CPU constructor cleans it, everything after it on the GPU.
int run_build_gpu(const Options &o, int mode) {
    std::vector<uint8_t> text;
    std::vector<uint64_t> doc_ends;
    if (!text_from_fasta(o.ref_file, o.separators, text, &doc_ends)) throw std::runtime_error("cannot open " + o.ref_file);
    if (text.empty()) throw std::runtime_error("no sequence in " + o.ref_file);
    movi_text_build_opts_t opts;
    memset(&opts, 0, sizeof(opts));
    opts.verify = o.verify ? 1u : 0u;
    movi_text_build_stats_t st;
    memset(&st, 0, sizeof(st));
    const auto t0 = std::chrono::steady_clock::now();
    void *image = nullptr;
    size_t image_bytes = 0;
    if (o.keep) {                                                  // the three arrays come down, are written, and go up again
        uint8_t *heads = nullptr;
        uint64_t *lens = nullptr, *thr = nullptr, R = 0;
        if (movi_rlbwt_from_text(o.device, text.data(), text.size(), &opts, &heads, &lens, &thr, &R, &st) != MOVI_OK)
            throw std::runtime_error(std::string("building the run-length BWT on the GPU: ") + movi_last_error());
        std::ofstream hf(o.ref_file + ".bwt.heads", std::ios::binary), lf(o.ref_file + ".bwt.len", std::ios::binary),
            tf(o.ref_file + ".thr_pos", std::ios::binary);
        hf.write(reinterpret_cast<const char *>(heads), (std::streamsize)R);
        for (uint64_t k = 0; k < R; k++) {                         // five little-endian bytes per run, as tools/build_index --emit-rlbwt
            lf.write(reinterpret_cast<const char *>(&lens[k]), 5);
            tf.write(reinterpret_cast<const char *>(&thr[k]), 5);
        }
        hf.close(); lf.close(); tf.close();
        const bool files_ok = hf.good() && lf.good() && tf.good();
        const int rc = files_ok ? movi_build_from_rlbwt(o.device, (uint32_t)mode, heads, lens, thr, R, &image, &image_bytes) : MOVI_OK;
        (void)movi_host_free(heads);
        (void)movi_host_free(lens);
        (void)movi_host_free(thr);
        if (!files_ok) throw std::runtime_error("cannot write " + o.ref_file + ".bwt.heads / .bwt.len / .thr_pos");
        if (rc != MOVI_OK) throw std::runtime_error(std::string("building the index on the GPU: ") + movi_last_error());
    } else if (movi_build_from_text(o.device, (uint32_t)mode, text.data(), text.size(), &opts, &image, &image_bytes, &st) != MOVI_OK) {
        throw std::runtime_error(std::string("building the index on the GPU: ") + movi_last_error());
    }
    const auto t1 = std::chrono::steady_clock::now();
    mkdir(o.index_dir.c_str(), 0777);
    const std::string name = o.index_dir + "/index.movi";
    std::ofstream f(name, std::ios::binary);
    f.write(static_cast<const char *>(image), (std::streamsize)image_bytes);
    f.close();
    const bool ok = f.good();
    (void)movi_host_free(image);
    if (!ok) throw std::runtime_error("cannot write " + name);
    if (o.color) {
        std::ofstream d(o.index_dir + "/ref.fa.doc_offsets");
        for (uint64_t e : doc_ends) d << e << "\n";
        d.close();
        if (!d.good()) throw std::runtime_error("cannot write " + o.index_dir + "/ref.fa.doc_offsets");
    }
    std::cerr << "[movi] The " << o.index_type << " index is written to " << name << "\n";
    if (o.color) std::cerr << "[movi] The document offsets are written to " << o.index_dir << "/ref.fa.doc_offsets\n";
    if (o.keep) std::cerr << "[movi] The run-length BWT and the thresholds are kept in " << o.ref_file << ".bwt.heads, .bwt.len and .thr_pos\n";
    std::cerr << "[movi] built on the GPU: " << text.size() << " characters, " << st.original_r << " BWT runs, " << st.rounds
              << " doubling rounds" << (st.verified ? ", verified" : "") << "; seconds: upload " << st.seconds[0] << ", suffix sort " << st.seconds[1]
              << ", BWT and runs " << st.seconds[2] << ", LCP " << st.seconds[3] << ", thresholds " << st.seconds[4] << ", verify " << st.seconds[5]
              << ", whole build " << std::chrono::duration<double>(t1 - t0).count() << "\n";
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
    const std::string err = movi_build_index_from_fasta(o.ref_file, mode, o.index_dir, o.separators, o.color);
    if (!err.empty()) throw std::runtime_error(err);
    std::cerr << "[movi] The " << o.index_type << " index is written to " << o.index_dir << "/index.movi\n";
    if (o.color) std::cerr << "[movi] The document offsets are written to " << o.index_dir << "/ref.fa.doc_offsets\n";
    return 0;
}

}  // namespace movi_host
