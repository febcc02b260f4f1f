// movi_search.hpp -- the backward-search interval step shared by the count kernels (movi_kernels.hip) and the MEM kernel
// (movi_walk_mem.hip): the row / window / look-ahead entry readers, update_interval (shrink_interval, shrink_interval_rows) and
// the row-start checkpoints behind MoveInterval::count (row_start).  Moved here unchanged from movi_kernels.hip.
#pragma once
#include "movi_device.hpp"

namespace movi {

// update_interval, src/move_structure_search.cpp:48-61 (get_char: the '$' row never equals a base): move the interval's
// start down to the first row of character b and its end up to the last one.  If [rs, re] holds such a row both searches
// find one and start <= end; if it holds none the interval is empty, and that is all the callers use (the reference lets
// the start run past the end instead).  So the two searches are independent, each bounded by the OTHER end's original row,
// and each takes the 4-row window around its next row per trip (window base clamped to r - 4: never outside the table)
// instead of one row: the trips of this loop -- max over the wave's lanes -- were most of a ZML step on divergent reads.
// Row / window / look-ahead entry of the table the count query walks on: AH = 0 the plain rows, AH = 1 the look-ahead copy
// (DevIndex::rows2: 8 rows + their 8 entries per 128-byte line, the last window in a line of its own).
// (The copy's reposition hints -- DevIndex::hints: y[31:28] of a row, y[30:25] of an entry -- are the PML walk's business: masked
// off here, which leaves the 32-bit ids of that form as they are.)
template <int MODE, int AH>
__device__ __forceinline__ uint2 tab_row(const DevIndex &ix, uint64_t i) {
    if (!AH) return load_row<MODE>(ix.rows, i);
    uint2 v;
    __builtin_memcpy(&v, ix.rows2 + (i >> 3) * 128u + (i & 7u) * 8u, 8);
    v.y &= ix.hints ? 0x0FFFFFFFu : 0xFFFFFFFFu;
    return v;
}
__device__ __forceinline__ uint2 tab_entry(const DevIndex &ix, uint64_t i) {
    uint2 v;
    __builtin_memcpy(&v, ix.rows2 + (i >> 3) * 128u + 64u + (i & 7u) * 8u, 8);
    v.y &= ix.hints ? ~(0x3Fu << 25) : 0xFFFFFFFFu;
    return v;
}
template <int MODE, int AH>
__device__ __forceinline__ void tab_window(const DevIndex &ix, uint64_t wb, uint2 (&w)[4]) {   // wb: aligned, or r - 4 (the last window)
    if (!AH) { load_window<MODE>(ix.rows, wb, w); return; }
    load_window<MODE>(ix.rows2 + (wb < ix.r - 4 ? (wb >> 3) * 128u + (wb & 4u) * 8u : ix.rows2_tail), 0, w);
    const uint32_t ym = ix.hints ? 0x0FFFFFFFu : 0xFFFFFFFFu;
#pragma unroll
    for (int t = 0; t < 4; ++t) w[t].y &= ym;
}

template <int MODE, int AH = 0>
__device__ __forceinline__ void shrink_interval(const DevIndex &ix, bool act, uint32_t b, uint64_t &rs, uint32_t &os,
                                                uint2 &rws, uint64_t &re, uint32_t &oe, uint2 &rwe,
                                                uint32_t &scan_total) {
    uint32_t gs = 0, ge = 0, dead = 0;
    if (act) {
        gs = (rs == ix.end_bwt_idx || row_c<MODE>(rws) != b) ? 1u : 0u;
        ge = (re == ix.end_bwt_idx || row_c<MODE>(rwe) != b) ? 1u : 0u;
    }
    const uint64_t lo = rs, hi = re, wb_last = ix.r - 4;
    while (wave_any((gs | ge) != 0u)) {
        if (gs) {
            if (rs >= hi) { dead = 1; gs = 0; ge = 0; }                  // no row of b in [lo, hi]
            else {
                uint64_t wb = (rs + 1) & ~3ull;
                if (wb > wb_last) wb = wb_last;
                uint2 w[4];
                tab_window<MODE, AH>(ix, wb, w);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (gs && wb + (uint64_t)t == rs + 1) {
                        rs += 1;
                        scan_total += 1;
                        if (rs != ix.end_bwt_idx && row_c<MODE>(w[t]) == b) { rws = w[t]; gs = 0; }
                        else if (rs >= hi) { dead = 1; gs = 0; ge = 0; }
                    }
                }
                os = 0;
            }
        }
        if (ge) {
            if (re <= lo) { dead = 1; gs = 0; ge = 0; }
            else {
                uint64_t wb = (re - 1) & ~3ull;
                if (wb > wb_last) wb = wb_last;
                uint2 w[4];
                tab_window<MODE, AH>(ix, wb, w);
#pragma unroll
                for (int t = 3; t >= 0; --t) {
                    if (ge && wb + (uint64_t)t + 1 == re) {
                        re -= 1;
                        scan_total += 1;
                        if (re != ix.end_bwt_idx && row_c<MODE>(w[t]) == b) { rwe = w[t]; oe = row_n<MODE>(w[t]) - 1; ge = 0; }
                        else if (re <= lo) { dead = 1; gs = 0; ge = 0; }
                    }
                }
            }
        }
    }
    if (dead) { rs = 1; re = 0; os = 0; oe = 0; }                        // empty, whatever the rows were
}

// The same, one row per end and trip (tables too small for a window).
template <int MODE>
__device__ __forceinline__ void shrink_interval_rows(const DevIndex &ix, bool act, uint32_t b, uint64_t &rs, uint32_t &os,
                                                     uint2 &rws, uint64_t &re, uint32_t &oe, uint2 &rwe,
                                                     uint32_t &scan_total) {
    uint32_t gs = 0, ge = 0;
    if (act) {
        gs = (rs == ix.end_bwt_idx || row_c<MODE>(rws) != b) ? 1u : 0u;
        ge = (re == ix.end_bwt_idx || row_c<MODE>(rwe) != b) ? 1u : 0u;
    }
    while (wave_any((gs | ge) != 0u)) {
        uint2 ws = rws, we = rwe;
        if (gs && rs + 1 < ix.r) ws = load_row<MODE>(ix.rows, rs + 1);
        if (ge && re > 0) we = load_row<MODE>(ix.rows, re - 1);
        if (gs) {
            rs += 1; os = 0; scan_total += 1;
            if (rs >= ix.r || rs > re) { gs = 0; ge = 0; }
            else { rws = ws; gs = (rs == ix.end_bwt_idx || row_c<MODE>(rws) != b) ? 1u : 0u; }
        }
        if (ge) {
            if (re == 0) { ge = 0; gs = 0; rs = 1; }          // nothing above row 0: empty
            else {
                re -= 1; scan_total += 1;
                rwe = we;
                oe = row_n<MODE>(rwe) - 1;
                if (re < rs) { ge = 0; gs = 0; }
                else ge = (re == ix.end_bwt_idx || row_c<MODE>(rwe) != b) ? 1u : 0u;
            }
        }
    }
}

// BWT position of (row k, offset 0) from the 32-row checkpoints.
template <int MODE>
__device__ __forceinline__ uint64_t row_start(const DevIndex &ix, uint64_t k) {
    uint64_t j = (k >> kPrefixShift) << kPrefixShift;
    uint64_t p = ix.row_start_ckpt[k >> kPrefixShift];
    for (; j < k; ++j) p += row_n<MODE>(load_row<MODE>(ix.rows, j));
    return p;
}

}  // namespace movi
