// movi_sa.hpp -- locate: what movi_walk_sa.hip's kernels share (MoveStructure::get_SA_entries, src/move_structure.cpp:35-48,
// and the builder of the sampled suffix array, find_sampled_SA_entries, src/move_structure_build.cpp:1174-1212).
//   * a packed BWT position (row, offset) in one u64 -- the MOVI_POS_* macros of include/movi_hip.h;
//   * the LOCATE ROWS (LocArgs::rows): 16 bytes per row = the row's own 8 bytes + one u64 with all_p[i] / rate in the high 40 bits and
//     all_p[i] % rate in the low 24 (all_p[i] = BWT position of the row's first character; rate <= 2^24).  "Is all_p[idx] + offset a
//     multiple of rate" is then 32-bit arithmetic on the one 16-byte gather a step makes anyway, and the sample's index at the end of a
//     walk is quotient + (remainder + offset) / rate;
//   * loc_lf_step: LF_move + fast_forward (src/move_structure.cpp:59-87) on those rows;
//   * locate_walk: the loop over loc_lf_step that locate_kernel and hits_walk_kernel (movi_walk_hits.hip) share.
#pragma once
#include "movi_lists.hpp"

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

// The locate walks of the items [0, n_items) of `pos`, in place: the loop of locate_kernel (movi_walk_sa.hip) and hits_walk_kernel
// (movi_walk_hits.hip), on the lanes' lists (movi_lists.hpp).  Walk lengths are roughly geometric with mean `rate`; every iteration of
// a lane is one dependent gather, a 16-byte locate row.  A walk ends on the first position that is a multiple of the rate -- in
// successor mode (a.succ) not on the one it starts from -- : on_hit(item, s, dist) stores the answer for sample s reached after dist
// steps and returns false where it had to refuse it; on_fail(item) stores the failure of a walk that broke an invariant of the table
// (the reference's throws; more than n steps: an error, not a hang).  An item that is kPosNone stays; one that is not a position of
// the table becomes kPosNone.  Every refusal and failure is counted in DevStats::errors.
template <int MODE, typename IdxT, typename OnHit, typename OnFail>
__device__ __forceinline__ void locate_walk(const DevIndex &ix, const LocArgs &a, uint64_t *__restrict__ pos, uint64_t n_items, DevStats *stats,
                                            OnHit on_hit, OnFail on_fail) {
    LaneList ls(n_items);
    IdxT kidx = 0;
    uint32_t off = 0, ff_total = 0, errs = 0;
    uint64_t dist = 0, lane_steps = 0, wave_steps = 0;      // (64 bits: a rate above n on a large table makes walks of n steps)
    uint4 v = make_uint4(0, 0, 0, 0);
    const uint32_t rate = a.rate;
    while (ls.any()) {
        wave_steps += 1;
        if (ls.state == 1u) {                             // the lane's next item
            const uint64_t p = pos[ls.item];
            const uint64_t row = p >> kPosOffBits;
            if (p != kPosNone && row < ix.r) {
                kidx = (IdxT)row;
                off = (uint32_t)p & ((1u << kPosOffBits) - 1u);
                v = loc_load(a.rows, row);
                dist = 0;
                ls.state = 2u;
            } else {
                if (p != kPosNone) { errs += 1; pos[ls.item] = kPosNone; }
                ls.next();
            }
        }
        uint32_t t = 0;
        bool hit = false;
        if (ls.state == 2u) {
            t = loc_rem(v) + off;                         // < 2^24 + 2^12
            hit = (t % rate == 0u) && !(a.succ != 0u && dist == 0);
        }
        if (hit) {
            if (!on_hit(ls.item, loc_quot(v) + t / rate, dist)) errs += 1;
            ls.next();
        }
        const bool walk = ls.state == 2u;                 // (a lane that took up an item above steps in this same iteration)
        uint64_t idx = kidx;
        const uint32_t e = loc_lf_step<MODE>(a.rows, ix.r, walk, idx, off, v, ff_total, [&]() {
            lane_steps += walk ? 1u : 0u;
            dist += walk ? 1u : 0u;
        });
        kidx = (IdxT)idx;
        if (walk && (e != 0u || dist > a.n)) {            // a corrupt table
            errs += 1;
            on_fail(ls.item);
            ls.next();
        }
    }
    flush_list_stats(stats, ff_total, 0u, errs, lane_steps, wave_steps);
}

}  // namespace movi
