// movi_text.hpp -- the run-length BWT and the thresholds from a text (movi_rlbwt_from_text, movi_build_from_text, `movi build --gpu-build`).
// Plain C++: the checks the library makes before any device call and the size formulas of the plan, shared by movi_abi.hip,
// movi_walk_text.hip and the tests (through movi_text_device_bytes).  No HIP in here.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

namespace movi {

// 32-bit ranks and positions: N = n + 1 BWT positions must stay below 2^32 with room for rank + 1 and the padded words.
constexpr uint64_t kTextMaxChars = (1ull << 32) - (1ull << 20);          // MOVI_TEXT_MAX_CHARS of include/movi_hip.h

// The text on the device: N bytes (the terminator 0 appended), then zeros to a multiple of 8 and two words more, so that an 8-byte
// window that starts at any of the N positions lies inside.
inline uint64_t text_padded_bytes(uint64_t N) { return ((N + 7) & ~7ull) + 16; }

// hipcub's scratch is granted this much and held to it.  The largest taker is the radix sort: per pass and block of a batch of at most
// 2^30 items one 4-byte look-back state per digit value (2^8 of them), with a thousand items or more per block.
inline uint64_t text_scratch_bytes(uint64_t N) { return (N < (1ull << 30) ? N : 1ull << 30) + (32ull << 20); }

// Peak device bytes of a build, over N alone; reached in the suffix sort and, with verify, again in the verifier:
//   text                    text_padded_bytes(N)
//   ranks (the inverse)     4 N
//   sort keys, two buffers  2 * 8 (N + 2)     (later: LCP and run starts in one, BWT, run heads and thresholds in the other)
//   suffixes, two buffers   2 * 4 N
//   verifier's bitmap       N / 8 + 8
//   scratch                 text_scratch_bytes(N)
//   counters                64
// The threshold pass runs after text, ranks and suffixes are released and holds 8 bytes per run and 4 per run longer than 256 beside
// the two key buffers: less than the above for every run count (R <= N).
inline uint64_t text_device_bytes(uint64_t N) {
    return text_padded_bytes(N) + 4 * N + 16 * (N + 2) + 8 * N + (N / 8 + 8) + text_scratch_bytes(N) + 64;
}

// Text positions per lane of the LCP pass when the caller names none: long enough that the restart at h = 0 (up to the longest repeat
// per lane) is paid seldom, short enough that a large text still fills the device (2^17 lanes).
inline uint32_t text_default_lcp_chunk(uint64_t N) {
    const uint64_t c = N >> 17;
    return (uint32_t)(c < 64 ? 64 : c > 1024 ? 1024 : c);
}

// Host-side refusals, before any device call.  On a finding: false and `why`, which names the argument.
inline bool text_check(const uint8_t *text, uint64_t n, std::string &why) {
    if (!text) { why = "h_text is NULL"; return false; }
    if (n == 0) { why = "n is 0: the text holds no character"; return false; }
    if (n > kTextMaxChars) {
        why = "n is " + std::to_string(n) + ": longer than the limit of " + std::to_string(kTextMaxChars) +
              " characters (2^32 - 2^20; ranks and positions are 32 bits)";
        return false;
    }
    if (const void *z = memchr(text, 0, n)) {
        why = "h_text holds a byte 0 at position " + std::to_string((uint64_t)(static_cast<const uint8_t *>(z) - text)) +
              ": the terminator is the builder's to append";
        return false;
    }
    return true;
}

struct TextBuildStats {
    uint64_t n_positions = 0, original_r = 0, device_bytes = 0;
    uint32_t rounds = 0, verified = 0;
    double seconds[6] = {0, 0, 0, 0, 0, 0};   // upload | suffix sort | BWT and runs | LCP | thresholds | verify
};

// The stages (movi_walk_text.hip).  The text has passed text_check; the current device is the one to build on.  with_thr = false
// skips the LCP and the threshold passes and leaves *h_thr NULL.  The three arrays are page-locked (hipHostMalloc); on failure none
// is returned.  Returns a MOVI_* code of include/movi_hip.h, with `why` on failure.
int rlbwt_from_text(const uint8_t *h_text, uint64_t n, bool with_thr, uint32_t lcp_chunk, bool verify, uint64_t max_device_bytes,
                    uint8_t **h_heads, uint64_t **h_lens, uint64_t **h_thr, uint64_t *original_r, TextBuildStats &stats, std::string &why);

}  // namespace movi
