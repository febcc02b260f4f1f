// Field maps of the deep rows (DevIndex::rows3): what a row's five dwords and ten extra bits hold, packed and unpacked in one place.
// Plain C++ (host tests compile it as it stands); deep_rows_kernel writes rows with deep_pack, the walk reads them with the deep_get_*
// helpers, which are the same expressions deep_unpack uses.
//
// Row i, with j = id(i), j2 = id(j), j3 = id(j2); W = width of an id, H = 32 - W, B = bits of one reposition hint (three hints a row):
//   D0 = j (W bits; all ones = not a row) | thr0 << 28 | thr1 << 29 | thr2 << 30 | n(j2)[10] << 31       (bits 27 : W are zero)
//   D1 = n(i) | off(i) << 11 | c(i) << 22 | c(j) << 25 | c(j2) << 28 | off(j2)[0] << 31
//   D2 = j2 (W bits) | hints[H - 1 : 0] << W
//   D3 = n(j) | off(j) << 11 | n(j2)[9:0] << 22
//   D4 = hints[3 B - 1 : H] | j3 << (3 B - H)
//   X  = off(j2)[10:1]                                                                                   (ten bits of the window's dword 15)
//
//   wide ids   (r < 2^28 - 1; the only map of tables of 2^26 rows and more):  W = 28, H = 4, B = 2: D4 = hints[5:4]  | j3 << 2
//   narrow ids (r <= 2^26 - 1):                                              W = 26, H = 6, B = 4: D4 = hints[11:6] | j3 << 6
//
// Both maps put the hints' low part on top of D2 and their high part at the bottom of D4, so that one funnel shift of D4 : D2 by W puts
// all 3 B bits side by side, and the hint of threshold slot k is the B bits at B k of that.  The walk tells the maps apart by three
// wave-uniform numbers (id mask, W, shift of j3) -- no code of its own for either.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MOVI_DEEP_HD __host__ __device__ inline
#else
#define MOVI_DEEP_HD inline
#endif

struct DeepMap {
    uint32_t id_bits;      // W
    uint32_t id_mask;      // 2^W - 1: the mask of an id and the id that is no row
    uint32_t hint_bits;    // B
    uint32_t j3_shift;     // 3 B - (32 - W)
};

constexpr uint64_t kDeepNarrowMaxRows = (1ull << 26) - 1;   // narrow ids: every row index is below the 26-bit "not a row" value
constexpr uint64_t kDeepWideMaxRows = (1ull << 28) - 2;     // (deep_rows_eligible: r < 2^28 - 1)

// The map of a table of r rows: narrow ids with 4-bit hints where the row indexes fit and 4-bit hints are asked for, else today's wide ids.
MOVI_DEEP_HD DeepMap deep_map_for(uint64_t r, int want_hint_bits) {
    if (want_hint_bits == 4 && r <= kDeepNarrowMaxRows) return DeepMap{26u, 0x03FFFFFFu, 4u, 6u};
    return DeepMap{28u, 0x0FFFFFFFu, 2u, 2u};
}

struct DeepFields {
    uint32_t j, j2, j3;            // ids (any value >= 2^W - 1 is stored as "not a row")
    uint32_t thr;                  // three threshold bits
    uint32_t n, off, c;            // the row itself
    uint32_t cj, cj2;              // c(j), c(j2) (7 = no entry)
    uint32_t nj, offj, nj2, offj2; // 11 bits each
    uint32_t hints;                // 3 B bits: slot k at B k
};

MOVI_DEEP_HD void deep_pack(const DeepMap &m, const DeepFields &f, uint32_t d[5], uint32_t &x) {
    const uint32_t H = 32u - m.id_bits, hmask = (1u << (3u * m.hint_bits)) - 1u, h = f.hints & hmask;
    const uint32_t j = f.j < m.id_mask ? f.j : m.id_mask, j2 = f.j2 < m.id_mask ? f.j2 : m.id_mask, j3 = f.j3 < m.id_mask ? f.j3 : m.id_mask;
    d[0] = j | ((f.thr & 7u) << 28) | (((f.nj2 >> 10) & 1u) << 31);
    d[1] = (f.n & 0x7FFu) | ((f.off & 0x7FFu) << 11) | ((f.c & 7u) << 22) | ((f.cj & 7u) << 25) | ((f.cj2 & 7u) << 28) | ((f.offj2 & 1u) << 31);
    d[2] = j2 | ((h & ((1u << H) - 1u)) << m.id_bits);
    d[3] = (f.nj & 0x7FFu) | ((f.offj & 0x7FFu) << 11) | ((f.nj2 & 0x3FFu) << 22);
    d[4] = (h >> H) | (j3 << m.j3_shift);
    x = (f.offj2 >> 1) & 0x3FFu;
}

// ---- the walk's readers (arguments: the row's dwords as loaded) ----
MOVI_DEEP_HD uint32_t deep_get_j(uint32_t d0, uint32_t id_mask) { return d0 & id_mask; }
MOVI_DEEP_HD uint32_t deep_get_j2(uint32_t d2, uint32_t id_mask) { return d2 & id_mask; }
MOVI_DEEP_HD uint32_t deep_get_j3(uint32_t d4, uint32_t j3_shift) { return d4 >> j3_shift; }
MOVI_DEEP_HD uint32_t deep_get_nj2(uint32_t d0, uint32_t d3) { return (d3 >> 22) | ((d0 >> 31) << 10); }
MOVI_DEEP_HD uint32_t deep_get_offj2(uint32_t d1, uint32_t x) { return (x << 1) | (d1 >> 31); }
// all 3 B hint bits side by side (bits above them: id bits of j3, never looked at)
MOVI_DEEP_HD uint32_t deep_get_hints(uint32_t d2, uint32_t d4, uint32_t id_bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(d4, d2, id_bits);
#else
    return (uint32_t)((((uint64_t)d4 << 32) | d2) >> id_bits);
#endif
}
// hint of threshold slot k at width w (w = B, or 0 = hints switched off: 0)
MOVI_DEEP_HD uint32_t deep_get_hint(uint32_t hints, uint32_t k, uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ubfe(hints, k * w, w);
#else
    return w ? (hints >> (k * w)) & ((1u << w) - 1u) : 0u;
#endif
}

MOVI_DEEP_HD DeepFields deep_unpack(const DeepMap &m, const uint32_t d[5], uint32_t x) {
    DeepFields f;
    f.j = deep_get_j(d[0], m.id_mask); f.j2 = deep_get_j2(d[2], m.id_mask); f.j3 = deep_get_j3(d[4], m.j3_shift);
    f.thr = (d[0] >> 28) & 7u;
    f.n = d[1] & 0x7FFu; f.off = (d[1] >> 11) & 0x7FFu; f.c = (d[1] >> 22) & 7u; f.cj = (d[1] >> 25) & 7u; f.cj2 = (d[1] >> 28) & 7u;
    f.nj = d[3] & 0x7FFu; f.offj = (d[3] >> 11) & 0x7FFu;
    f.nj2 = deep_get_nj2(d[0], d[3]); f.offj2 = deep_get_offj2(d[1], x & 0x3FFu);
    f.hints = deep_get_hints(d[2], d[4], m.id_bits) & ((1u << (3u * m.hint_bits)) - 1u);
    return f;
}

// The builder's hint rule for one threshold slot of row i, whose scan for base `a` goes down (threshold 0 <= offset: reposition_down) or up:
// rows beyond the edge of i's three-row window at which the nearest run of `a` lies, 1 .. reach, or 0 = inside the window, further, or
// nowhere.  The scan stops AT that row: what it passes lies strictly between -- never row r - 1 going down, never row 0 going up, and the
// target is a row of the table.  c_of(t) = the base of row t.
template <class CF>
MOVI_DEEP_HD uint32_t deep_hint_of(CF c_of, uint64_t r, uint64_t i, uint32_t a, bool down, uint32_t reach) {
    const uint64_t wb = (i / 3) * 3;
    if (down) {
        const uint64_t edge = wb + 2;
        for (uint64_t t = i + 1; t <= edge && t < r; ++t) if (c_of(t) == a) return 0u;
        for (uint64_t t = edge + 1; t <= edge + reach && t < r; ++t) if (c_of(t) == a) return (uint32_t)(t - edge);
    } else {
        for (uint64_t t = wb; t < i; ++t) if (c_of(t) == a) return 0u;
        for (uint64_t t = 1; t <= reach && t <= wb; ++t) if (c_of(wb - t) == a) return (uint32_t)t;
    }
    return 0u;
}
