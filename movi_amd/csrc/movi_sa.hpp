// movi_sa.hpp -- locate: what movi_walk_sa.hip's kernels share (MoveStructure::get_SA_entries, src/move_structure.cpp:35-48,
// and the builder of the sampled suffix array, find_sampled_SA_entries, src/move_structure_build.cpp:1174-1212).
//   * a packed BWT position (row, offset) in one u64 -- the MOVI_POS_* macros of include/movi_hip.h;
//   * the LOCATE ROWS (LocArgs::rows): 16 bytes per row = the row's own 8 bytes + one u64 with all_p[i] / rate in the high 40 bits and
//     all_p[i] % rate in the low 24 (all_p[i] = BWT position of the row's first character; rate <= 2^24).  "Is all_p[idx] + offset a
//     multiple of rate" is then 32-bit arithmetic on the one 16-byte gather a step makes anyway, and the sample's index at the end of a
//     walk is quotient + (remainder + offset) / rate;
//   * loc_lf_step: LF_move + fast_forward (src/move_structure.cpp:59-87) on those rows.
#pragma once
#include "movi_device.hpp"

namespace movi {

constexpr uint32_t kPosOffBits = 12;                     // offsets are below 4096 in both resident layouts (MOVI_POS_OFFSET_BITS)
constexpr uint64_t kPosNone = ~0ull;                     // MOVI_POS_NONE: no position (a read that hit a throw); locate leaves it alone
constexpr uint32_t kLocRemBits = 24;                     // rate <= 2^24

__device__ __forceinline__ uint64_t pos_pack(uint64_t row, uint32_t off) { return (row << kPosOffBits) | (uint64_t)off; }

// A locate row as loaded: x, y = the row; z, w = the second word.
__device__ __forceinline__ uint4 loc_load(const uint4 *rows, uint64_t i) { return rows[i]; }
__device__ __forceinline__ uint2 loc_row(const uint4 &v) { return make_uint2(v.x, v.y); }
__device__ __forceinline__ uint32_t loc_rem(const uint4 &v) { return v.z & ((1u << kLocRemBits) - 1u); }
__device__ __forceinline__ uint64_t loc_quot(const uint4 &v) { return (uint64_t)(v.z >> kLocRemBits) | ((uint64_t)v.w << (32 - kLocRemBits)); }
__device__ __forceinline__ uint4 loc_make(uint2 row, uint64_t all_p, uint64_t rate) {
    const uint64_t w = ((all_p / rate) << kLocRemBits) | (all_p % rate);
    return make_uint4(row.x, row.y, (uint32_t)w, (uint32_t)(w >> 32));
}

// LF_move + fast_forward for the lanes with `live`, on the locate rows: on entry v is rows[idx], on exit the new idx's.  The gather of
// the target is issued first; `before` (the caller's bookkeeping of the step) runs under it.  Returns a kErr* code.
template <int MODE, typename Before>
__device__ __forceinline__ uint32_t loc_lf_step(const uint4 *__restrict__ rows, uint64_t r, bool live, uint64_t &idx, uint32_t &off,
                                                uint4 &v, uint32_t &ff_total, Before before) {
    uint32_t errc = kErrNone;
    uint64_t j = idx;
    uint32_t n = 0, ff = 0, going = 0;
    uint4 nv = v;
    bool step = false;
    if (live) {
        const uint2 row = loc_row(v);
        j = (uint64_t)row.x | ((uint64_t)(row.y >> 28) << 32);          // row_id<6 / 3>: the id sits in the row
        if (j >= r) {                                                     // move_structure.cpp:63-65
            errc = kErrIdRange;
            j = idx;
        } else {
            nv = loc_load(rows, j);                                       // THE dependent random gather
            off += row_off<MODE>(row);
            step = true;
        }
    }
    before();
    if (step) {
        v = nv;
        n = row_n<MODE>(loc_row(v));
        going = (j < r - 1 && off >= n) ? 1u : 0u;
    }
    while (wave_any(going != 0u)) {                                       // fast_forward: the next row mostly sits in the same line
        if (going) {
            const uint64_t jj = j + 1;
            const uint4 w = loc_load(rows, jj < r ? jj : r - 1);
            off -= n;
            j += 1;
            ff += 1;
            v = w;
            n = row_n<MODE>(loc_row(v));
            going = (j < r - 1 && off >= n && ff < 65535u) ? 1u : 0u;
        }
    }
    if (ff >= 65535u) errc = kErrFastForward;                             // move_structure.cpp:72-75
    ff_total += ff;
    idx = j;
    return errc;
}

// The lane's counters to DevStats (may be null), one atomic per wavefront and counter; errs = items of the lane that failed.
__device__ __forceinline__ void flush_lane_stats_sa(DevStats *stats, uint32_t ff_total, uint32_t errs, uint64_t lane_steps, uint64_t wave_steps) {
    const uint32_t erw = wave_sum(errs);
    unsigned long long ffw = ff_total, lsw = lane_steps;              // summed in 64 bits: 64 lanes of long walks pass 2^32
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        ffw += __shfl_xor(ffw, s, 64);
        lsw += __shfl_xor(lsw, s, 64);
    }
    if ((threadIdx.x & 63) == 0 && stats) {
        if (ffw) atomicAdd(&stats->fast_forwards, ffw);
        if (erw) atomicAdd(&stats->errors, (unsigned long long)erw);
        atomicAdd(&stats->lane_steps, lsw);
        atomicAdd(&stats->wave_steps, (unsigned long long)wave_steps);
    }
}

}  // namespace movi
