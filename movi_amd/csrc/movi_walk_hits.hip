// movi_walk_hits.hip -- locate count and MEM hits: for every match item (read, start, end) the number of occurrences of
// X = P[start .. end) in the indexed text and the text positions of the first min(occ, max_occ) of them in BWT order.  The contract
// is stated in include/movi_hip.h (movi_locate_matches_device); the reference has no such mode.
//
// Why the positions are what they are.  Backward search starts from the F-column range of X's last base -- the suffixes that start
// with it -- and every update_interval + LF pair turns the range of the suffixes that start with Y into that of the suffixes that start
// with cY.  So the final interval [s, e] is the range of BWT positions p whose suffix T[SA[p] ..] starts with X: occ = e - s + 1, and
// the hits in BWT order are SA[s], SA[s + 1], ...  get_SA_entries of p is SA[p], or SA[p] + n where the walk passed text position 0
// (it stops at BWT position 0, whose sample is n - 1): t = entry mod n, and no other shift is needed.
//
// Four steps on the caller's stream:
//   hits_interval_kernel   the searches.  Blocks of one wavefront; a lane owns the items lane, lane + stride, ... and takes up its
//                          next item in the iteration after a search ends, because item lengths differ widely: search_lists
//                          (movi_search.hpp) over P[end - 1] down to P[start] with lim = end - start, so the interval table serves
//                          the first K bases.  Stores per item the interval's two packed ends and the BWT position of its start
//                          (HitsInterval, in the caller's work area), occ (interval_count), and listed = min(occ, max_occ) for
//                          the scan;
//   the scan               hipcub::DeviceScan::ExclusiveSum over the n_items + 1 values of `listed` (the last one 0) into d_first,
//                          64-bit values, its temporary storage from the work area.  n_items + 1 < 2^31: one 32-bit-indexed scan;
//   hits_expand_kernel     slot j < min(total, cap): its item by an upper bound over d_first, its BWT position = the interval's start
//                          + (j - first[item]), its row from the item's first row and the 32-row checkpoints, then
//                          pos_pack(row, offset).  Neighbouring lanes hold neighbouring slots: the stores are coalesced;
//   hits_walk_kernel       the locate walks in place on those slots: locate_walk (movi_sa.hpp), the loop locate_kernel
//                          (movi_walk_sa.hip) runs, with two differences.  The number of slots is min(d_first[n_items], cap), read
//                          on the device -- locate_kernel takes its count from the host, which does not know the total without
//                          waiting for the stream, and a launch over the caller's whole cap would walk, and overwrite, slots past
//                          the total.  And the entry is stored as a text position, t = entry mod n; a sample that does not give
//                          one (a corrupt array) becomes kPosNone and is counted in DevStats::errors.  kPosNone stays.
// The grids of the last two are sized from positions_cap and the kernels read the total from d_first[n_items]: nothing comes back
// to the host, so the call can be captured, and no slot at or past min(total, cap) is read or written.
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"
#include "movi_sa.hpp"

#include <hipcub/hipcub.hpp>

namespace movi {

// The final interval of an item: its two ends as packed positions and the BWT position of the start.  occ == 0: unspecified.
struct HitsInterval {
    uint64_t s_pack, e_pack, p0;
};
static_assert(sizeof(HitsInterval) == kHitsIntervalBytes, "HitsInterval and hits_work_layout differ");

// search_lists over the items: a bad item (outside its read, or empty) is answered in `take`; a search that ends on the whole of X
// stores the interval and its size, interval_count.  A corrupt table never yields a count beyond the text.
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void hits_interval_kernel(DevIndex ix, const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offs,
                                                           uint64_t n_reads, const HitsItem *__restrict__ items, uint64_t n_items,
                                                           uint32_t max_occ, uint64_t n_text, HitsInterval *__restrict__ iv, uint64_t *__restrict__ occ,
                                                           uint64_t *__restrict__ listed, uint8_t *__restrict__ item_err, DevStats *stats) {
    if (blockIdx.x == 0 && threadIdx.x == 0) listed[n_items] = 0;      // the scan's last input: d_first[n_items] = the total
    search_lists<MODE, IdxT>(ix, n_items, stats,
        [&](uint64_t g, const uint8_t *&last, uint32_t &lim) {
            const HitsItem it = items[g];
            bool ok = it.read < n_reads && it.start < it.end;
            if (ok) {
                const uint64_t beg = offs[it.read], fin = offs[(uint64_t)it.read + 1];
                ok = fin >= beg && it.end <= fin - beg;   // (no base outside the read is read)
                last = bases + (beg + it.end - 1u);
                lim = it.end - it.start;
            }
            if (!ok) {                                    // a bad item
                occ[g] = 0; listed[g] = 0;
                if (item_err) item_err[g] = 0xFFu;
            }
            return ok;
        },
        [&](uint64_t g, const SearchStep &st, uint64_t rs, uint32_t os, uint2 rws, uint64_t re, uint32_t oe) {
            uint64_t v = 0;
            uint32_t code = st.err;
            HitsInterval h{0, 0, 0};
            if (!code && st.taken != 0u) {
                if (rs >= ix.r || re >= ix.r || rs > re) code = kErrIdRange;
                else {
                    const uint64_t p0 = row_start<MODE>(ix, rs) + os;
                    v = interval_count<MODE>(ix, rs, os, rws, re, oe);
                    if (p0 >= n_text || v - 1 >= n_text - p0) { code = kErrIdRange; v = 0; }
                    else { h.s_pack = pos_pack(rs, os); h.e_pack = pos_pack(re, oe); h.p0 = p0; }
                }
            }
            iv[g] = h;
            occ[g] = v;
            listed[g] = v < (uint64_t)max_occ ? v : (uint64_t)max_occ;
            if (item_err) item_err[g] = (uint8_t)code;
            return code == 0u;
        });
}

// Slot j of the position list -> the packed position of its BWT position.  A grid-stride loop over [0, min(total, cap)).
// The row of BWT position q inside the item's interval [rs, re]: the last checkpoint block at or below q among those the interval
// touches (a binary search over row_start_ckpt), then at most 32 rows forward -- from the item's first row where that is its block.
// Every index is bounded: blocks by the interval's rows, rows by re < r, the walk by 32 steps; a slot whose offset does not fall
// inside its row (a corrupt table) becomes kPosNone and is counted.
template <int MODE>
__global__ __launch_bounds__(256) void hits_expand_kernel(DevIndex ix, const HitsInterval *__restrict__ iv, const uint64_t *__restrict__ first,
                                                          uint64_t n_items, uint64_t cap, uint64_t *__restrict__ pos, DevStats *stats) {
    const uint64_t total = first[n_items], lim = total < cap ? total : cap;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t errs = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < lim; j += stride) {
        uint64_t lo = 0, hi = n_items;                    // the last item with first[item] <= j: first[0] = 0 <= j < total = first[n_items]
        while (hi - lo > 1) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (first[mid] <= j) lo = mid; else hi = mid;
        }
        const HitsInterval h = iv[lo];
        const uint64_t rs = h.s_pack >> kPosOffBits, re = h.e_pack >> kPosOffBits;
        const uint32_t os = (uint32_t)h.s_pack & ((1u << kPosOffBits) - 1u);
        const uint64_t q = h.p0 + (j - first[lo]);        // the slot's BWT position
        uint64_t out = kPosNone;
        if (rs <= re && re < ix.r && h.p0 >= os) {
            uint64_t row = rs, p = h.p0 - os;             // p: BWT position of (row, 0)
            uint64_t cl = rs >> kPrefixShift, ch = re >> kPrefixShift;
            while (cl < ch) {                             // the last block in (cl, ch] whose checkpoint is <= q, if any
                const uint64_t mid = cl + ((ch - cl + 1) >> 1);
                if (ix.row_start_ckpt[mid] <= q) cl = mid; else ch = mid - 1;
            }
            if (cl > (rs >> kPrefixShift)) { row = cl << kPrefixShift; p = ix.row_start_ckpt[cl]; }
            uint32_t n = row_n<MODE>(load_row<MODE>(ix.rows, row));
            for (int t = 0; t < (1 << kPrefixShift) && row < re && p + n <= q; ++t) {
                p += n;
                row += 1;
                n = row_n<MODE>(load_row<MODE>(ix.rows, row));
            }
            if (q >= p && q - p < n && q - p < (1u << kPosOffBits)) out = pos_pack(row, (uint32_t)(q - p));
        }
        if (out == kPosNone) errs += 1;
        pos[j] = out;
    }
    if (errs && stats) atomicAdd(&stats->errors, (unsigned long long)errs);
}

// locate_walk (movi_sa.hpp) in place on the slots [0, min(total, cap)): see the head of this file for what differs from locate_kernel.
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void hits_walk_kernel(DevIndex ix, LocArgs a, const uint64_t *__restrict__ first, uint64_t n_first,
                                                       uint64_t cap, uint64_t *__restrict__ pos, DevStats *stats) {
    const uint64_t total = first[n_first];
    a.succ = 0u;                                          // (no successor mode here)
    locate_walk<MODE, IdxT>(ix, a, pos, total < cap ? total : cap, stats,
        [&](uint64_t item, uint64_t s, uint64_t dist) {
            uint64_t e = kPosNone;
            if (s < a.n_entries) {
                e = a.samples[s] + dist;                  // get_SA_entries: SA[p], or SA[p] + n
                if (e >= a.n) e -= a.n;
                if (e >= a.n) e = kPosNone;               // (a corrupt sample)
            }
            pos[item] = e;
            return e != kPosNone;
        },
        [&](uint64_t item) { pos[item] = kPosNone; });
}

namespace {
struct HitsIntervalFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &hits_interval_kernel<MODE, IdxT>; }
};
struct HitsWalkFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &hits_walk_kernel<MODE, IdxT>; }
};
}  // namespace

hipError_t launch_locate_matches(int mode, const DevIndex &ix, const LocArgs &loc, const uint8_t *d_bases, const uint64_t *d_offsets,
                                 uint64_t n_reads, const HitsItem *d_items, uint64_t n_items, uint32_t max_occ, uint64_t *d_occ,
                                 uint64_t *d_first, uint64_t *d_positions, uint64_t positions_cap, uint8_t *d_item_err, void *d_work,
                                 uint64_t work_bytes, int stages, DevStats *d_stats, int num_cus, hipStream_t stream, LaunchInfo *info) {
    if ((mode != 6 && mode != 3) || max_occ == 0u || n_items >= kHitsMaxItems) return hipErrorInvalidValue;
    const HitsWorkLayout w = hits_work_layout(n_items);
    if (work_bytes < w.total) return hipErrorInvalidValue;
    HitsInterval *d_iv = reinterpret_cast<HitsInterval *>(static_cast<uint8_t *>(d_work) + w.intervals);
    uint64_t *d_listed = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(d_work) + w.listed);
    void *d_temp = static_cast<uint8_t *>(d_work) + w.scan_temp;
    if (n_items == 0) return hipMemsetAsync(d_first, 0, 8, stream);      // d_first[0] = the total = 0
    hipError_t e = launch_lane_lists<HitsIntervalFamily>("hits_interval_kernel", 0, mode, ix, n_items, kHitsWaves, num_cus, stream, info, d_bases,
                                                         d_offsets, n_reads, d_items, n_items, max_occ, loc.n, d_iv, d_occ, d_listed, d_item_err,
                                                         d_stats);
    if (e != hipSuccess) return e;
    size_t need = 0, have = (size_t)(w.total - w.scan_temp);
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_listed, d_first, (int)(n_items + 1), stream);
    if (e == hipSuccess && need > have) e = hipErrorInvalidValue;            // (hits_work_layout's room for it is an upper bound: never met)
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d_temp, have, d_listed, d_first, (int)(n_items + 1), stream);
    if (e != hipSuccess || positions_cap == 0 || stages < 2) return e;       // (info: the interval kernel's)
    // the total stays on the device: the grids come from the cap, the kernels stop at min(total, cap)
    const uint64_t want = (positions_cap + 255) / 256, gcap = (uint64_t)(num_cus > 0 ? num_cus : 256) * 8u;
    const unsigned blocks = (unsigned)(want < gcap ? want : gcap);
    char nm[96];
    snprintf(nm, sizeof(nm), "hits_expand_kernel<%d>", mode);
    note_walk_launch(nm);
    if (mode == 6) hipLaunchKernelGGL(hits_expand_kernel<6>, dim3(blocks), dim3(256), 0, stream, ix, d_iv, d_first, n_items, positions_cap, d_positions, d_stats);
    else hipLaunchKernelGGL(hits_expand_kernel<3>, dim3(blocks), dim3(256), 0, stream, ix, d_iv, d_first, n_items, positions_cap, d_positions, d_stats);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (stages < 3) {
        if (info) {
            *info = LaunchInfo();
            snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
            info->variant = 0; info->block_threads = 256; info->idx64 = ix.idx32 ? 0 : 1;
        }
        return hipSuccess;
    }
    if (loc.rate == 0u || !loc.rows || !loc.samples) return hipErrorInvalidValue;
    // as launch_locate, over the cap
    return launch_lane_lists<HitsWalkFamily>("hits_walk_kernel", 0, mode, ix, positions_cap, kLocateWaves, num_cus, stream, info, loc, d_first,
                                             n_items, positions_cap, d_positions, d_stats);
}

hipError_t preload_hits(int mode, bool idx32) {
    hipFuncAttributes at;
    hipError_t e = preload_family<HitsIntervalFamily>(mode, idx32);
    if (e == hipSuccess) e = hipFuncGetAttributes(&at, mode == 6 ? (const void *)hits_expand_kernel<6> : (const void *)hits_expand_kernel<3>);
    if (e == hipSuccess) e = preload_family<HitsWalkFamily>(mode, idx32);
    return e;
}

}  // namespace movi
