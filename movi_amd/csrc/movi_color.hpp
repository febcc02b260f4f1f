// movi_color.hpp -- Movi Color, default colour mode: what movi_walk_color.hip's two kernels share.
//   * the COLOUR TABLES (MoveStructure::flat_colors / doc_set_flat_inds, include/move_structure.hpp:290-296, written by
//     flat_and_serialize_colors_vectors, src/move_structure_io.cpp:513-548): `flat` is every distinct document set stored as its size
//     followed by its sorted members, u16 each; `inds[row]` is the offset of the row's set in `flat` (u64 on the device, the file's
//     5-byte MoveTally on disk);
//   * a builder key: (row << 16) | document, one per BWT position (build_doc_pats + build_doc_sets, src/move_structure_color.cpp:4-72);
//   * lf_step_pre: LF_move + fast_forward (src/move_structure.cpp:59-87) whose first gather the caller may have issued already.
#pragma once
#include "movi_sa.hpp"

namespace movi {

constexpr uint32_t kDocNone = 0xFFFFu;                   // std::numeric_limits<uint16_t>::max(): no best / second-best document yet
constexpr uint32_t kColorKeyDocBits = 16;

// lf_step (movi_device.hpp) for the lanes with `live`; where `have_pre`, `pre` already is rows[row_id(row)] -- the caller loaded it
// while it still had other work to do -- and no gather is made here.
template <int MODE>
__device__ __forceinline__ uint32_t lf_step_pre(const DevIndex &ix, bool live, uint64_t &idx, uint32_t &off, uint2 &row, bool have_pre,
                                                uint2 pre, uint32_t &ff_total) {
    uint32_t errc = kErrNone;
    uint64_t j = idx;
    uint32_t n = 0, ff = 0, going = 0;
    if (live) {
        j = row_id<MODE>(row, idx, ix);
        if (j >= ix.r) {                                // move_structure.cpp:63-65
            errc = kErrIdRange;
            j = idx;
        } else {
            off += row_off<MODE>(row);
            uint2 w = pre;
            if (!have_pre) w = load_row<MODE>(ix.rows, j);
            row = w;
            n = row_n<MODE>(row);
            going = (j < ix.r - 1 && off >= n) ? 1u : 0u;
        }
    }
    while (wave_any(going != 0u)) {                     // fast_forward, :67-86
        if (going) {
            const uint64_t jj = j + 1;
            const uint2 w = load_row<MODE>(ix.rows, jj < ix.r ? jj : ix.r - 1);
            off -= n;
            j += 1;
            ff += 1;
            row = w;
            n = row_n<MODE>(row);
            going = (j < ix.r - 1 && off >= n && ff < 65535u) ? 1u : 0u;
        }
    }
    if (ff >= 65535u) errc = kErrFastForward;           // move_structure.cpp:72-75
    ff_total += ff;
    idx = j;
    return errc;
}

}  // namespace movi
