// Field map of the chain rows (the PML walk's 32-byte rows: pml_kernel_chain, movi_walk.hpp): what a row's eight dwords hold, packed and
// unpacked in one place.  Plain C++ (host tests compile it as it stands); chain_rows_kernel writes rows with chain_pack, the walk reads
// them with the chain_get_* helpers, which are the same expressions chain_unpack uses.
//
// Window q = rows 2q and 2q + 1 = 64 bytes at byte 64 q (two windows per 128-byte line); the last window of a table of odd r is padded.
// Row i, with j1 = id(i), j2 = id(j1), j3 = id(j2), j4 = id(j3) -- up to FOUR bases per gather: the base at i, and one more at each of
// j1, j2, j3 while the next base is c(j) and the offset arrives below n(j).  Ids are 28 bits, all ones = not a row (r < 2^28 - 1).
//   D0 = j1 | thr0 << 28 | thr1 << 29 | thr2 << 30 | n(j4)[10] << 31
//   D1 = n(i) | off(i) << 11 | c(i) << 22 | c(j1) << 25 | c(j2) << 28
//   D2 = j2 | hint0 << 28
//   D3 = n(j1) | off(j1) << 11
//   D4 = j3 | hint1 << 28
//   D5 = n(j2) | off(j2) << 11 | c(j3) << 22
//   D6 = j4 | hint2 << 28
//   D7 = n(j3) | off(j3) << 11 | n(j4)[9:0] << 22
// Laid out for their readers: the one-base step reads D0 and D1 alone (the first 16-byte load of the row); every ride reads the id dword
// and the dword behind it; the hint of threshold slot k is the top four bits of the id dword D(2 + 2k), and what the fast-forward skip
// behind the last ride needs, n(j4), sits beside that ride's own entry.
// An entry (c, n, off of a target) is INVALID -- c = 7, n = 0, which no base code and no offset passes -- where the target is no row or is
// the '$' row, where the id behind it (the gather's address after that ride) is no row, and behind any invalid entry.  n(j4) = 0 likewise.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MOVI_CHAIN_HD __host__ __device__ inline
#else
#define MOVI_CHAIN_HD inline
#endif

constexpr uint32_t kChainIdMask = 0x0FFFFFFFu;              // the mask of an id and the id that is no row
constexpr uint64_t kChainMaxRows = (1ull << 28) - 2;        // every row index is below the "not a row" value
constexpr uint32_t kChainHintBits = 4u, kChainHintReach = 15u;
constexpr uint32_t kChainRowBytes = 32u, kChainWindowRows = 2u;

MOVI_CHAIN_HD uint64_t chain_rows_bytes_of(uint64_t r) { return ((r + 1) / 2) * 64; }

struct ChainFields {
    uint32_t j[4];                 // j1 .. j4 (any value >= 2^28 - 1 is stored as "not a row")
    uint32_t thr;                  // three threshold bits
    uint32_t n, off, c;            // the row itself
    uint32_t cj[3], nj[3], offj[3];   // the entries of j1, j2, j3 (c = 7, n = 0: no entry)
    uint32_t nj4;                  // n(j4): 0 = the skip behind the last ride is not known
    uint32_t hints;                // three 4-bit hints: slot k at 4 k
};

MOVI_CHAIN_HD void chain_pack(const ChainFields &f, uint32_t d[8]) {
    uint32_t j[4];
    for (int t = 0; t < 4; ++t) j[t] = f.j[t] < kChainIdMask ? f.j[t] : kChainIdMask;
    d[0] = j[0] | ((f.thr & 7u) << 28) | (((f.nj4 >> 10) & 1u) << 31);
    d[1] = (f.n & 0x7FFu) | ((f.off & 0x7FFu) << 11) | ((f.c & 7u) << 22) | ((f.cj[0] & 7u) << 25) | ((f.cj[1] & 7u) << 28);
    d[2] = j[1] | ((f.hints & 15u) << 28);
    d[3] = (f.nj[0] & 0x7FFu) | ((f.offj[0] & 0x7FFu) << 11);
    d[4] = j[2] | (((f.hints >> 4) & 15u) << 28);
    d[5] = (f.nj[1] & 0x7FFu) | ((f.offj[1] & 0x7FFu) << 11) | ((f.cj[2] & 7u) << 22);
    d[6] = j[3] | (((f.hints >> 8) & 15u) << 28);
    d[7] = (f.nj[2] & 0x7FFu) | ((f.offj[2] & 0x7FFu) << 11) | ((f.nj4 & 0x3FFu) << 22);
}

// ---- the walk's readers (arguments: the row's dwords as loaded) ----
MOVI_CHAIN_HD uint32_t chain_get_id(uint32_t d_id) { return d_id & kChainIdMask; }               // D0, D2, D4, D6 -> j1 .. j4
MOVI_CHAIN_HD uint32_t chain_get_hint(uint32_t d_id) { return d_id >> 28; }                      // D2, D4, D6 -> the hint of slot 0, 1, 2
MOVI_CHAIN_HD uint32_t chain_get_thr(uint32_t d0, uint32_t k) { return (d0 >> (28u + k)) & 1u; }
MOVI_CHAIN_HD uint32_t chain_get_n(uint32_t d) { return d & 0x7FFu; }                            // D1, D3, D5, D7 -> n of i, j1, j2, j3
MOVI_CHAIN_HD uint32_t chain_get_off(uint32_t d) { return (d >> 11) & 0x7FFu; }                  // ... and off
MOVI_CHAIN_HD uint32_t chain_get_c(uint32_t d1) { return (d1 >> 22) & 7u; }
MOVI_CHAIN_HD uint32_t chain_get_cj1(uint32_t d1) { return (d1 >> 25) & 7u; }
MOVI_CHAIN_HD uint32_t chain_get_cj2(uint32_t d1) { return (d1 >> 28) & 7u; }
MOVI_CHAIN_HD uint32_t chain_get_cj3(uint32_t d5) { return (d5 >> 22) & 7u; }
MOVI_CHAIN_HD uint32_t chain_get_nj4(uint32_t d0, uint32_t d7) { return (d7 >> 22) | ((d0 >> 31) << 10); }

MOVI_CHAIN_HD ChainFields chain_unpack(const uint32_t d[8]) {
    ChainFields f;
    for (int t = 0; t < 4; ++t) f.j[t] = chain_get_id(d[2 * t]);
    f.thr = (d[0] >> 28) & 7u;
    f.n = chain_get_n(d[1]); f.off = chain_get_off(d[1]); f.c = chain_get_c(d[1]);
    f.cj[0] = chain_get_cj1(d[1]); f.cj[1] = chain_get_cj2(d[1]); f.cj[2] = chain_get_cj3(d[5]);
    for (int t = 0; t < 3; ++t) { f.nj[t] = chain_get_n(d[3 + 2 * t]); f.offj[t] = chain_get_off(d[3 + 2 * t]); }
    f.nj4 = chain_get_nj4(d[0], d[7]);
    f.hints = chain_get_hint(d[2]) | (chain_get_hint(d[4]) << 4) | (chain_get_hint(d[6]) << 8);
    return f;
}

// The fields of row i of a table seen through row_of(t, id, n, off, c, thr) (t < r): the chain of ids, every entry's validity (the rule
// above) and n(j4).  Hints are the caller's (chain_hint_of).  A row beyond r - 1 (padding): no ids, c = 7, n = 0.
template <class RF>
MOVI_CHAIN_HD ChainFields chain_fields_of(RF row_of, uint64_t r, uint64_t end_row, uint64_t i) {
    ChainFields f;
    for (int t = 0; t < 4; ++t) f.j[t] = 0xFFFFFFFFu;
    for (int t = 0; t < 3; ++t) { f.cj[t] = 7u; f.nj[t] = 0; f.offj[t] = 0; }
    f.thr = 0; f.n = 0; f.off = 0; f.c = 7u; f.nj4 = 0; f.hints = 0;
    if (i >= r) return f;
    uint64_t id = 0;
    uint32_t thr_ = 0;
    row_of(i, id, f.n, f.off, f.c, f.thr);
    uint64_t at = id;                                    // j(t + 1), as the table has it
    bool ok = true;                                      // every entry so far is valid
    for (int t = 0; t < 4; ++t) {
        if (at >= r) break;                              // not a row: the id stays all ones, and so does everything behind it
        f.j[t] = (uint32_t)at;
        uint64_t nid = 0;
        uint32_t n = 0, off = 0, c = 7u;
        row_of(at, nid, n, off, c, thr_);
        ok = ok && at != end_row;
        if (t == 3) { f.nj4 = ok ? n : 0u; break; }
        ok = ok && nid < r;                              // the gather behind this ride needs an address
        if (ok) { f.cj[t] = c; f.nj[t] = n; f.offj[t] = off; }
        at = nid;
    }
    return f;
}

// The builder's hint rule for one threshold slot of row i (deep_hint_of's rule for windows of two rows): rows beyond the edge of i's
// window at which the nearest run of `a` lies in the scan's direction, 1 .. reach, or 0 = inside the window, further, or nowhere.
template <class CF>
MOVI_CHAIN_HD uint32_t chain_hint_of(CF c_of, uint64_t r, uint64_t i, uint32_t a, bool down, uint32_t reach) {
    const uint64_t wb = i & ~1ull;
    if (down) {
        const uint64_t edge = wb + 1;
        for (uint64_t t = i + 1; t <= edge && t < r; ++t) if (c_of(t) == a) return 0u;
        for (uint64_t t = edge + 1; t <= edge + reach && t < r; ++t) if (c_of(t) == a) return (uint32_t)(t - edge);
    } else {
        for (uint64_t t = wb; t < i; ++t) if (c_of(t) == a) return 0u;
        for (uint64_t t = 1; t <= reach && t <= wb; ++t) if (c_of(wb - t) == a) return (uint32_t)t;
    }
    return 0u;
}
