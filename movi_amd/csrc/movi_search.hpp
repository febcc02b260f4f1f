// movi_search.hpp -- backward search on intervals, shared by the count kernels and ftab_kernel (movi_kernels.hip), the MEM kernel
// (movi_walk_mem.hip) and the k-mer kernel (movi_walk_kmer.hip):
//   * the row / window / look-ahead entry readers, update_interval (shrink_interval, shrink_interval_rows) and the row-start
//     checkpoints behind MoveInterval::count (row_start);
//   * the entry of the interval table (DevIndex::ftab): FtabEntry, ftab_encode, ftab_decode -- its bit layout is stated there only;
//   * for the lane-per-read queries (MEM, k-mers): the prologue (read_lane), the interval step (search_step), the counters' way
//     out (flush_lane_stats) and the launch (launch_lane_per_read);
//   * for the queries whose lanes own lists of patterns (k-mer occurrences, the hits' intervals): the loop (search_lists) and the
//     interval's size (interval_count);
//   * the launch of a MODE x IdxT kernel family: family_kernel, launch_lane_per_read, launch_lane_lists, preload_family.
#pragma once
#include "movi_lists.hpp"

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

// MoveInterval::count (include/move_intervals.hpp:47-58) of the non-empty interval from (rs, os) to (re, oe), rws = row rs: inside one
// row from the offsets, inside a checkpoint block's reach from the rows between the ends, else from the checkpoints.
template <int MODE>
__device__ __forceinline__ uint64_t interval_count(const DevIndex &ix, uint64_t rs, uint32_t os, uint2 rws, uint64_t re, uint32_t oe) {
    if (rs == re) return (uint64_t)oe - os + 1;
    if (re - rs < (1ull << kPrefixShift)) {
        uint64_t v = (uint64_t)row_n<MODE>(rws) - os + oe + 1;
        for (uint64_t j = rs + 1; j < re; ++j) v += row_n<MODE>(load_row<MODE>(ix.rows, j));
        return v;
    }
    return (row_start<MODE>(ix, re) + oe) - (row_start<MODE>(ix, rs) + os) + 1;
}

// ---- entry of the interval table (DevIndex::ftab): the interval after the K bases of its index, and what reaching it cost.
//   x       rs[31:0]                      y       re[31:0]
//   z[3:0]  rs[35:32]   z[7:4]  re[35:32]   z[19:8]  os (< 4096)   z[31:20]  oe (< 4096)
//   w[14:0] fast-forwards   w[30:15] rows scanned   w[31] valid (a cleared entry: the K-mer is absent, or a field overflowed)
struct FtabEntry {
    uint64_t rs, re;
    uint32_t os, oe, ff, scans;
};
__device__ __forceinline__ bool ftab_fits(uint32_t os, uint32_t oe, uint32_t ff, uint32_t scans) {
    return ff < (1u << 15) && scans < (1u << 16) && os < 4096u && oe < 4096u;
}
__device__ __forceinline__ uint4 ftab_encode(const FtabEntry &f) {           // ftab_fits(...) holds
    uint4 e4;
    e4.x = (uint32_t)f.rs;
    e4.y = (uint32_t)f.re;
    e4.z = (uint32_t)(f.rs >> 32) | ((uint32_t)(f.re >> 32) << 4) | (f.os << 8) | (f.oe << 20);
    e4.w = f.ff | (f.scans << 15) | (1u << 31);
    return e4;
}
__device__ __forceinline__ bool ftab_valid(const uint4 &e4) { return (e4.w >> 31) != 0u; }
__device__ __forceinline__ FtabEntry ftab_decode(const uint4 &e4) {          // ftab_valid(e4)
    FtabEntry f;
    f.rs = (uint64_t)e4.x | ((uint64_t)(e4.z & 15u) << 32);
    f.re = (uint64_t)e4.y | ((uint64_t)((e4.z >> 4) & 15u) << 32);
    f.os = (e4.z >> 8) & 0xFFFu;
    f.oe = e4.z >> 20;
    f.ff = e4.w & 0x7FFFu;
    f.scans = (e4.w >> 15) & 0xFFFFu;
    return f;
}

// ---- one lane per read (MEM, k-mers): prologue, step, epilogue, launch

// The block's copy of DevIndex::code_of in LDS (s_code) and the lane's read: rid (through `order`, if given), its first base and length.
struct ReadLane {
    bool valid;
    uint64_t rid, beg;
    uint32_t m;
};
__device__ __forceinline__ ReadLane read_lane(const DevIndex &ix, uint8_t (&s_code)[256], const uint64_t *__restrict__ offs,
                                              uint64_t n_reads, const uint32_t *__restrict__ order) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();
    ReadLane r;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    r.valid = t < n_reads;
    r.rid = (r.valid && order) ? order[t] : t;
    r.beg = r.valid ? offs[r.rid] : 0;
    r.m = r.valid ? (uint32_t)(offs[r.rid + 1] - r.beg) : 0u;
    return r;
}

// One backward-search step of a lane inside a phase -- a run of bases searched from an empty pattern, of which `l` are taken so far
// (the interval is non-empty after each) and `lim` may be taken.  base_at(i) is the code of the i-th base from the phase's next one
// (0xFF: illegal), direction and complement being the caller's; it is asked for i = 0, and for i < K at the phase's start.
//   l == 0   the first K = DevIndex::ftab_k bases by one lookup in the interval table, when they are all legal, stay inside the
//            phase's range and the entry is valid (a cleared entry is not "absent": counter overflow clears it too);
//            else initialize_backward_search (src/move_structure_search.cpp:284-291) on the first base;
//   l > 0    update_interval + two LF moves (:311-333); keep(rs, re, os, oe) sees the interval before them.
// The interval lives in the caller's rs / os / rws (start: row, offset, the row's words) and re / oe / rwe (end) across the call only:
// what it is kept in between iterations is the caller's choice.  The wave-uniform loops inside are entered by all lanes.
struct SearchStep {
    uint32_t b;        // the base the step was on (0xFF: illegal, or the lane is idle)
    uint32_t taken;    // bases taken: K, 1, or 0 -- the phase died on b
    bool ext;          // the step was an update_interval on a legal base
    uint32_t err;      // kErr* of the LF moves: the read is over
};
template <int MODE, typename BaseAt, typename Keep>
__device__ __forceinline__ SearchStep search_step(const DevIndex &ix, bool live, uint32_t lim, uint32_t &l, BaseAt base_at, Keep keep,
                                                  uint64_t &rs, uint32_t &os, uint2 &rws, uint64_t &re, uint32_t &oe, uint2 &rwe,
                                                  uint32_t &ff_total, uint32_t &scan_total) {
    const uint32_t K = ix.ftab_k;
    SearchStep r;
    r.b = live ? base_at(0u) : 0xFFu;
    r.taken = 0;
    r.err = 0;
    bool stepped = false;
    if (K != 0u && live && l == 0 && K <= lim) {
        uint32_t kidx = 0, bad = 0;
        for (uint32_t i = 0; i < K; ++i) {              // K is wave-uniform
            const uint32_t cc = base_at(i) - ix.sep;
            bad |= (uint32_t)(cc > 3u);
            kidx |= (cc & 3u) << (2u * i);
        }
        uint4 e4 = make_uint4(0, 0, 0, 0);
        if (!bad) e4 = ix.ftab[kidx];
        if (ftab_valid(e4)) {
            const FtabEntry f = ftab_decode(e4);
            rs = f.rs; re = f.re; os = f.os; oe = f.oe;
            ff_total += f.ff;
            scan_total += f.scans;
            rws = load_row<MODE>(ix.rows, rs);
            rwe = load_row<MODE>(ix.rows, re);
            r.taken = K;
            stepped = true;
        }
    }
    const uint32_t b = r.b;
    const bool init = live && !stepped && l == 0 && b != 0xFFu;
    r.ext = live && !stepped && l > 0 && b != 0xFFu;
    bool ne_init = false;
    if (init) {
        rs = ix.first_runs[b + 1]; re = ix.last_runs[b + 1];
        os = (uint32_t)ix.first_offsets[b + 1]; oe = (uint32_t)ix.last_offsets[b + 1];
        ne_init = (rs < re) || (rs == re && os <= oe);
        if (ne_init) {
            rws = load_row<MODE>(ix.rows, rs);
            rwe = load_row<MODE>(ix.rows, re);
        }
    }
    if (r.ext) keep(rs, re, os, oe);
    if (ix.r >= 8) shrink_interval<MODE>(ix, r.ext && rs <= re, b, rs, os, rws, re, oe, rwe, scan_total);
    else shrink_interval_rows<MODE>(ix, r.ext && rs <= re, b, rs, os, rws, re, oe, rwe, scan_total);
    bool ne = r.ext && ((rs < re) || (rs == re && os <= oe));
    r.err = lf_step2<MODE>(ix, ne, rs, os, rws, re, oe, rwe, ff_total);
    if (r.err) ne = false;
    if (ne && !((rs < re) || (rs == re && os <= oe))) ne = false;
    if (ne || ne_init) r.taken = 1;
    l += r.taken;
    return r;
}

// The lane's counters to DevStats (may be null), one atomic per wavefront and counter.
__device__ __forceinline__ void flush_lane_stats(DevStats *stats, uint32_t ff_total, uint32_t scan_total, uint32_t failed,
                                                 uint32_t lane_steps, uint32_t wave_steps) {
    const uint32_t ffw = wave_sum(ff_total), scw = wave_sum(scan_total), erw = wave_sum(failed ? 1u : 0u), lsw = wave_sum(lane_steps);
    if ((threadIdx.x & 63) == 0 && stats) {
        if (ffw) atomicAdd(&stats->fast_forwards, (unsigned long long)ffw);
        if (scw) atomicAdd(&stats->scans, (unsigned long long)scw);
        if (erw) atomicAdd(&stats->errors, (unsigned long long)erw);
        atomicAdd(&stats->lane_steps, (unsigned long long)lsw);
        atomicAdd(&stats->wave_steps, (unsigned long long)wave_steps);
    }
}

// The searches of a launch whose lanes own lists of patterns (movi_lists.hpp), one pattern per item, searched leftwards from its last
// base by search_step -- the interval table's lookup first where K <= lim -- until it dies, hits one of the reference's LF throws or
// all its lim bases are taken.
//   take(item, last, lim)                  false: the item holds no pattern (one iteration); else the address of the pattern's last
//                                          base and its length;
//   done(item, st, rs, os, rws, re, oe)    the search is over: st.err != 0, st.taken == 0 (the pattern does not occur) or else the
//                                          interval of the whole pattern.  Returns false where the item failed (DevStats::errors).
// IdxT: the type the lane's interval rows are kept in between iterations (uint32_t when DevIndex::idx32).
template <int MODE, typename IdxT, typename Take, typename Done>
__device__ __forceinline__ void search_lists(const DevIndex &ix, uint64_t n_items, DevStats *stats, Take take, Done done) {
    __shared__ uint8_t s_code[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();
    LaneList ls(n_items);
    uint32_t l = 0, lim = 0;                              // bases of the pattern taken (the interval is non-empty after each), its length
    const uint8_t *last = nullptr;                        // the pattern's last base
    uint32_t ff_total = 0, scan_total = 0, errs = 0;
    uint64_t lane_steps = 0, wave_steps = 0;
    IdxT krs = 0, kre = 0;
    uint32_t os = 0, oe = 0;
    uint2 rws = make_uint2(0, 0), rwe = make_uint2(0, 0);
    while (ls.any()) {
        wave_steps += 1;
        if (ls.state == 1u) {                             // the lane's next item
            if (take(ls.item, last, lim)) { l = 0; ls.state = 2u; }
            else ls.next();
        }
        const bool live = ls.state == 2u;                 // (a lane that took up an item above steps in this same iteration)
        lane_steps += live ? 1u : 0u;
        // ---- one step leftwards on the pattern's next base: last[-l - i], i < lim - l
        uint64_t rs = krs, re = kre;
        const uint8_t *R = last - l;
        auto base_at = [&](uint32_t i) { return (uint32_t)s_code[*(R - i)]; };
        auto keep = [](uint64_t, uint64_t, uint32_t, uint32_t) {};
        const SearchStep st = search_step<MODE>(ix, live, lim, l, base_at, keep, rs, os, rws, re, oe, rwe, ff_total, scan_total);
        krs = (IdxT)rs; kre = (IdxT)re;
        if (live && (st.err != 0u || st.taken == 0u || l == lim)) {
            if (!done(ls.item, st, rs, os, rws, re, oe)) errs += 1;
            ls.next();
        }
    }
    flush_list_stats(stats, ff_total, scan_total, errs, lane_steps, wave_steps);
}

// ---- the launch of a kernel family F: F::kernel<MODE, IdxT>() = the __global__ function (DevIndex, args...), MODE in {6, 3} x IdxT
// in {uint32_t, uint64_t (DevIndex::idx32 == 0)}, in blocks of one wavefront; noted and reported as "<name><MODE, IdxT>".
template <typename F>
auto family_kernel(int mode, bool idx32) {                // mode: 6 or 3
    return mode == 6 ? (idx32 ? F::template kernel<6, uint32_t>() : F::template kernel<6, uint64_t>())
                     : (idx32 ? F::template kernel<3, uint32_t>() : F::template kernel<3, uint64_t>());
}
inline void note_family_launch(const char *name, int variant, int mode, const DevIndex &ix, int waves, LaunchInfo *info) {
    char nm[96];
    snprintf(nm, sizeof(nm), "%s<%d, %s>", name, mode, ix.idx32 ? "unsigned int" : "unsigned long");
    note_walk_launch(nm);
    if (info) {
        *info = LaunchInfo();
        snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
        info->variant = variant; info->block_threads = 64; info->idx64 = ix.idx32 ? 0 : 1; info->waves_per_cu = waves;
    }
}

// One lane per read.
template <typename F, typename... Args>
hipError_t launch_lane_per_read(const char *name, int variant, int mode, const DevIndex &ix, uint64_t n_reads, hipStream_t stream,
                                LaunchInfo *info, Args... args) {
    if (n_reads == 0) return hipSuccess;
    if (mode != 6 && mode != 3) return hipErrorInvalidValue;
    const uint64_t blocks = (n_reads + 63) / 64;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    note_family_launch(name, variant, mode, ix, 0, info);
    hipLaunchKernelGGL(family_kernel<F>(mode, ix.idx32 != 0u), dim3((unsigned)blocks), dim3(64), 0, stream, ix, args...);
    return hipGetLastError();
}

// A list of the n_items items per lane (movi_lists.hpp): at most `waves` one-wavefront blocks per CU, so that a lane's list holds many
// items wherever there are many.  n_items: the host's count, or its upper bound where only the device knows the count
// (hits_walk_kernel); 0 is noted and reported, not launched (the k-mer occurrences of reads without bases).
template <typename F, typename... Args>
hipError_t launch_lane_lists(const char *name, int variant, int mode, const DevIndex &ix, uint64_t n_items, int waves, int num_cus,
                             hipStream_t stream, LaunchInfo *info, Args... args) {
    if (mode != 6 && mode != 3) return hipErrorInvalidValue;
    note_family_launch(name, variant, mode, ix, waves, info);
    if (n_items == 0) return hipSuccess;
    const uint64_t want = (n_items + 63) / 64, cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * (uint64_t)waves;
    hipLaunchKernelGGL(family_kernel<F>(mode, ix.idx32 != 0u), dim3((unsigned)(want < cap ? want : cap)), dim3(64), 0, stream, ix, args...);
    return hipGetLastError();
}

// Loads the family's code object now (movi_index_prepare: a first call may then be captured).
template <typename F>
hipError_t preload_family(int mode, bool idx32) {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, (const void *)family_kernel<F>(mode, idx32));
}

}  // namespace movi
