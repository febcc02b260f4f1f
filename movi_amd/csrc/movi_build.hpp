// movi_build.hpp -- index.movi from a run-length BWT (movi_build_from_rlbwt, `movi build --preprocessed`).
// Plain C++: the library (movi_walk_build.hip, movi_abi.hip) and the host CLI (host/build_cmd.cpp) both hold the input to the
// rules below, the CLI with the file's name in front of the finding and before any device call.
#pragma once
#include <cstdint>
#include <string>

namespace movi {

constexpr uint64_t kBuildMaxItems = 0x7FFFFFFFull - 1;   // 2^31 - 2: hipcub's item counts are int, and the sums take one item more
constexpr uint64_t kBuildMaxN = 1ull << 40;              // lengths and thresholds are 5-byte values

// MAX_RUN_LENGTH, include/move_row_configs.hpp:51,101,135,117,31,72; 0 = not a mode of this engine
inline uint32_t build_max_run(uint32_t mode) {
    return mode == 6 ? 2047u : mode == 3 ? 4095u : mode == 7 ? 511u : (mode == 8 || mode == 2 || mode == 5) ? 1023u : 0u;
}
inline bool build_mode_thresholds(uint32_t mode) { return mode == 6 || mode == 7 || mode == 8; }   // USE_THRESHOLDS, include/utils.hpp:146

// What the run heads and lengths say about the text (build_alphabet, src/move_structure_build.cpp:428-447; use_separator,
// src/move_structure.cpp:547-552).
struct RlbwtInfo {
    uint64_t n = 0;              // characters, terminator included
    uint32_t sigma = 0;          // symbols other than the terminator
    uint32_t sep = 0;            // 1: five symbols led by '%'
    uint8_t alphabet[8] = {0};
    uint64_t counts[8] = {0};
    uint8_t code_of[256] = {0};  // byte -> code; the terminator's is 0 (MoveRow::set_c: alphamap[0] == 256 shifts out)
    uint64_t end_run = 0;        // the terminator's run
};

enum RlbwtArray { kRlbwtHeads = 0, kRlbwtLens = 1, kRlbwtThr = 2 };

// Everything that could make a kernel of the builder read or write out of bounds, or that the reference's constructor would turn
// into a wrong index without saying so.  thr may be NULL (the types without thresholds).  On a finding: false, `which` = the array
// (file) at fault, `why` = the finding.
inline bool rlbwt_check(const uint8_t *heads, const uint64_t *lens, const uint64_t *thr, uint64_t original_r, RlbwtInfo &info,
                        RlbwtArray &which, std::string &why) {
    info = RlbwtInfo();
    which = kRlbwtHeads;
    if (original_r == 0) { why = "holds no run"; return false; }
    if (original_r > kBuildMaxItems) {
        why = std::to_string(original_r) + " runs: the builder's device scans and sorts are 32-bit indexed, at most 2^31 - 2 runs are served";
        return false;
    }
    uint64_t cnt[256] = {0}, terminators = 0;
    for (uint64_t k = 0; k < original_r; k++) {
        if (lens[k] == 0) { which = kRlbwtLens; why = "run " + std::to_string(k) + " has length zero"; return false; }
        if (lens[k] >= kBuildMaxN || info.n + lens[k] >= kBuildMaxN) {
            which = kRlbwtLens;
            why = "the lengths add up to 2^40 characters or more at run " + std::to_string(k);
            return false;
        }
        if (k > 0 && heads[k] == heads[k - 1]) {
            why = "runs " + std::to_string(k - 1) + " and " + std::to_string(k) + " have the same head: the runs are not maximal";
            return false;
        }
        if (heads[k] == 0) { terminators += lens[k]; info.end_run = k; }
        cnt[heads[k]] += lens[k];
        info.n += lens[k];
    }
    if (terminators != 1) {
        why = "the terminator (byte 0) appears " + std::to_string(terminators) + " times: exactly one is expected";
        return false;
    }
    uint32_t distinct = 0;
    for (int c = 1; c < 256; c++) distinct += cnt[c] ? 1u : 0u;
    const bool sep = distinct == 5 && cnt[(int)'%'] != 0 && [&] { for (int c = 1; c < '%'; c++) if (cnt[c]) return false; return true; }();
    if (distinct == 0 || (distinct > 4 && !sep)) {
        why = "alphabet has " + std::to_string(distinct) + " symbols: only DNA (<= 4) and separator ('%' + ACGT) indexes are supported";
        return false;
    }
    for (int c = 1; c < 256; c++)
        if (cnt[c]) {
            info.code_of[c] = (uint8_t)info.sigma;
            info.alphabet[info.sigma] = (uint8_t)c;
            info.counts[info.sigma++] = cnt[c];
        }
    info.sep = sep ? 1u : 0u;
    if (thr)
        for (uint64_t k = 0; k < original_r; k++)
            if (thr[k] > info.n) {
                which = kRlbwtThr;
                why = "threshold " + std::to_string(k) + " is " + std::to_string(thr[k]) + ", greater than the text's length " + std::to_string(info.n);
                return false;
            }
    return true;
}

// The builder proper (movi_walk_build.hip).  The arrays have passed rlbwt_check and `info` is what it filled in; the current device is
// the one to build on.  *h_image: page-locked (hipHostMalloc).  Returns a MOVI_* code of include/movi_hip.h, with `why` on failure.
// With MOVI_BUILD_PROFILE=1 in the environment it waits after every stage and prints the stages' seconds and the peak device bytes.
int build_from_rlbwt(uint32_t mode, const uint8_t *h_heads, const uint64_t *h_lens, const uint64_t *h_thr, uint64_t original_r,
                     const RlbwtInfo &info, void **h_image, size_t *image_bytes, std::string &why);

}  // namespace movi
