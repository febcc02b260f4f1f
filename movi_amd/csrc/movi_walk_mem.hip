// movi_walk_mem.hip -- maximal exact matches: MoveStructure::query_mems, src/mem_finder.cpp:7-145 (the BML loop of query_mem_bml,
// :27-103; query_all_mems, :105-145, is the same loop at L' = 1 on legal reads).  The contract -- the two per-read arrays bw / fw,
// the loop over them, where it deviates from the reference -- is stated in include/movi_hip.h (movi_mem_device).
//
// One lane per read, blocks of one wavefront.  Every iteration every lane with work takes ONE backward-search step
// (update_interval + two LF moves, src/move_structure_search.cpp:311-333, or initialize_backward_search :284-291 on the first
// base of a phase) on the base its phase asks for:
//   window   P[w], P[w-1], ..., P[pos]          (w = pos + L' - 1)   does P[pos..w] occur?  bw[w] >= L'
//   extend   comp(P[pos]), comp(P[pos+1]), ...                       fw[pos] and cnt[pos] (forward_search_step :336-338)
//   next     P[e], P[e-1], ..., P[pos+1]                             bw[e], capped at e - pos: the next left end
// The step is the same operation in all three phases -- only the base and the position bookkeeping differ -- so lanes in
// different phases share every instruction; the wave-uniform loops of shrink_interval and lf_step2 are entered by all lanes.
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"

#include <cstdio>

namespace movi {

namespace {
enum : uint32_t { kPhWindow = 0, kPhExtend = 1, kPhNext = 2, kPhDone = 3 };
}

// a.comp: byte c = code of the complement of the base of code c (0xFF: not in the alphabet); a.min_len = L' >= 1.
// IdxT: the row-index type of the kept copy of the extend phase's last non-empty interval (uint32_t when DevIndex::idx32).
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void mem_kernel(DevIndex ix, MemArgs a, const uint8_t *__restrict__ bases,
                                                 const uint64_t *__restrict__ offs, uint64_t n_reads, MemOut *__restrict__ mems,
                                                 uint32_t *__restrict__ n_mems, uint8_t *__restrict__ err, DevStats *stats,
                                                 const uint32_t *__restrict__ order) {
    __shared__ uint8_t s_code[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();

    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = t < n_reads;
    const uint64_t rid = (valid && order) ? order[t] : t;
    const uint64_t beg = valid ? offs[rid] : 0;
    const uint32_t m = valid ? (uint32_t)(offs[rid + 1] - beg) : 0u;
    const uint8_t *R = bases + beg;
    MemOut *O = mems + beg;                              // MEM j of the read: O[j], j < m - L' + 1
    const uint32_t Lp = a.min_len, K = ix.ftab_k;
    auto comp = [&](uint32_t c) { return c == 0xFFu ? 0xFFu : (uint32_t)((a.comp >> (8u * c)) & 0xFFu); };

    uint32_t ph = (valid && m >= Lp) ? kPhWindow : kPhDone;
    uint32_t pos = 0;                 // the left end under test
    uint32_t e = 0;                   // end (exclusive) of the last MEM: the next phase walks back from it
    uint32_t j = 0, lim = 0, l = 0;   // next base of the phase, bases it may consume, bases consumed (interval non-empty after each)
    int32_t dir = -1;
    uint32_t nm = 0, failed = 0, ff_total = 0, scan_total = 0, lane_steps = 0, wave_steps = 0;
    uint64_t rs = 0, re = 0;
    uint32_t os = 0, oe = 0;
    uint2 rws = make_uint2(0, 0), rwe = make_uint2(0, 0);
    IdxT prs = 0, pre = 0;            // the interval before the last step (extend: reported if that step came out empty)
    uint32_t pos_ = 0, poe = 0;
    auto enter = [&](uint32_t p) {    // phase p from the current pos / e
        ph = p;
        l = 0;
        if (p == kPhWindow) { j = pos + Lp - 1; dir = -1; lim = Lp; }
        else if (p == kPhExtend) { j = pos; dir = 1; lim = m - pos; }
        else if (p == kPhNext) { j = e; dir = -1; lim = e - pos; }
    };
    if (ph == kPhWindow) enter(kPhWindow);

    while (wave_any(ph != kPhDone)) {
        const bool live = ph != kPhDone;
        wave_steps += 1;
        lane_steps += (uint32_t)live;
        const uint32_t b = live ? (ph == kPhExtend ? comp(s_code[R[j]]) : (uint32_t)s_code[R[j]]) : 0xFFu;
        bool stepped = false;
        // ---- a phase's first K bases by one lookup in the interval table (DevIndex::ftab), when they are all legal, stay
        // inside the phase's range, and the entry is valid (a cleared entry is not "absent": counter overflow clears it too)
        if (K != 0u && live && l == 0 && K <= lim) {
            uint32_t kidx = 0, bad = 0;
            for (uint32_t i = 0; i < K; ++i) {          // K is wave-uniform
                const uint32_t c0 = s_code[R[(int64_t)j + (int64_t)dir * (int64_t)i]];
                const uint32_t cc = (ph == kPhExtend ? comp(c0) : c0) - ix.sep;
                bad |= (uint32_t)(cc > 3u);
                kidx |= (cc & 3u) << (2u * i);
            }
            uint4 e4 = make_uint4(0, 0, 0, 0);
            if (!bad) e4 = ix.ftab[kidx];
            if (e4.w >> 31) {
                rs = (uint64_t)e4.x | ((uint64_t)(e4.z & 15u) << 32);
                re = (uint64_t)e4.y | ((uint64_t)((e4.z >> 4) & 15u) << 32);
                os = (e4.z >> 8) & 0xFFFu;
                oe = e4.z >> 20;
                ff_total += e4.w & 0x7FFFu;
                scan_total += (e4.w >> 15) & 0xFFFFu;
                rws = load_row<MODE>(ix.rows, rs);
                rwe = load_row<MODE>(ix.rows, re);
                l = K;
                j = (uint32_t)((int64_t)j + (int64_t)dir * (int64_t)K);
                stepped = true;
            }
        }
        // ---- one step: initialize_backward_search on a phase's first base, else update_interval + two LF moves
        const bool init = live && !stepped && l == 0 && b != 0xFFu;
        const bool ext = live && !stepped && l > 0 && b != 0xFFu;
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
        if (ext) { prs = (IdxT)rs; pre = (IdxT)re; pos_ = os; poe = oe; }
        if (ix.r >= 8) shrink_interval<MODE>(ix, ext && rs <= re, b, rs, os, rws, re, oe, rwe, scan_total);
        else shrink_interval_rows<MODE>(ix, ext && rs <= re, b, rs, os, rws, re, oe, rwe, scan_total);
        bool ne = ext && ((rs < re) || (rs == re && os <= oe));
        const uint32_t e12 = lf_step2<MODE>(ix, ne, rs, os, rws, re, oe, rwe, ff_total);
        if (e12) { failed = e12; ph = kPhDone; ne = false; }
        if (ne && !((rs < re) || (rs == re && os <= oe))) ne = false;
        if (ne || ne_init) { l += 1; j = (uint32_t)((int64_t)j + dir); }
        const bool grown = stepped || ne || ne_init;
        // ---- the phase ends at its first empty step or when its range is used up
        if (live && !failed && (!grown || l == lim)) {
            if (ph == kPhWindow) {
                if (l >= Lp) enter(kPhExtend);
                else {                                   // window P[pos..w] absent: skip past the failing base w - l
                    pos = pos + Lp - l;
                    if (pos + Lp <= m) enter(kPhWindow); else ph = kPhDone;
                }
            } else if (ph == kPhExtend) {
                if (l < Lp) {                            // fw[pos] < L' (a text not closed under rc)
                    pos += 1;
                    if (pos + Lp <= m) enter(kPhWindow); else ph = kPhDone;
                } else {
                    // cnt[pos]: MoveInterval::count of the last non-empty interval (include/move_intervals.hpp:47-58)
                    uint64_t cs = rs, ce = re;
                    uint32_t xs = os, xe = oe;
                    if (ext && !grown) { cs = prs; ce = pre; xs = pos_; xe = poe; }   // (an illegal base left the interval as it was)
                    uint64_t cnt;
                    if (cs == ce) cnt = (uint64_t)xe - xs + 1;
                    else cnt = (row_start<MODE>(ix, ce) + xe) - (row_start<MODE>(ix, cs) + xs) + 1;
                    e = pos + l;
                    MemOut o;
                    o.start = pos; o.end = e; o.count = cnt;
                    O[nm] = o;
                    nm += 1;
                    if (e == m) ph = kPhDone; else enter(kPhNext);
                }
            } else {                                     // next left end: max(pos + 1, e - bw[e] + 1), bw[e] capped at e - pos
                pos = (l == lim) ? pos + 1 : e - l + 1;
                // P[pos..e] occurs: when it spans a whole window, the window's test is known to pass
                if (e + 1 >= pos + Lp) enter(kPhExtend);
                else if (pos + Lp <= m) enter(kPhWindow);
                else ph = kPhDone;
            }
        }
    }
    if (valid) {
        n_mems[rid] = failed ? 0u : nm;
        if (err) err[rid] = (uint8_t)failed;
    }
    const uint32_t ffw = wave_sum(ff_total), scw = wave_sum(scan_total), erw = wave_sum(failed ? 1u : 0u), lsw = wave_sum(lane_steps);
    if ((threadIdx.x & 63) == 0 && stats) {
        if (ffw) atomicAdd(&stats->fast_forwards, (unsigned long long)ffw);
        if (scw) atomicAdd(&stats->scans, (unsigned long long)scw);
        if (erw) atomicAdd(&stats->errors, (unsigned long long)erw);
        atomicAdd(&stats->lane_steps, (unsigned long long)lsw);
        atomicAdd(&stats->wave_steps, (unsigned long long)wave_steps);
    }
}

hipError_t launch_mem(int mode, const DevIndex &ix, const MemArgs &a, const uint8_t *d_bases, const uint64_t *d_offsets,
                      uint64_t n_reads, MemOut *d_mems, uint32_t *d_n_mems, uint8_t *d_err, DevStats *d_stats,
                      const uint32_t *d_order, hipStream_t stream, LaunchInfo *info) {
    if (n_reads == 0) return hipSuccess;
    if (mode != 6 && mode != 3) return hipErrorInvalidValue;
    const uint64_t blocks = (n_reads + 63) / 64;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    char nm[96];
    snprintf(nm, sizeof(nm), "mem_kernel<%d, %s>", mode, ix.idx32 ? "unsigned int" : "unsigned long");
    note_walk_launch(nm);
    if (info) {
        *info = LaunchInfo();
        snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
        info->variant = 0; info->block_threads = 64; info->idx64 = ix.idx32 ? 0 : 1;
    }
    const dim3 grid((unsigned)blocks), block(64);
    if (mode == 6 && ix.idx32)
        hipLaunchKernelGGL((mem_kernel<6, uint32_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_mems, d_n_mems, d_err, d_stats, d_order);
    else if (mode == 6)
        hipLaunchKernelGGL((mem_kernel<6, uint64_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_mems, d_n_mems, d_err, d_stats, d_order);
    else if (ix.idx32)
        hipLaunchKernelGGL((mem_kernel<3, uint32_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_mems, d_n_mems, d_err, d_stats, d_order);
    else
        hipLaunchKernelGGL((mem_kernel<3, uint64_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_mems, d_n_mems, d_err, d_stats, d_order);
    return hipGetLastError();
}

// ---- compaction of the host path: n_mems -> exclusive prefix (one block), then the MEMs of every read to their place

constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void mem_scan_kernel(const uint32_t *__restrict__ n, uint64_t cnt, uint64_t *__restrict__ first) {
    __shared__ uint64_t part[kScanThreads];
    const uint64_t per = (cnt + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = (uint64_t)threadIdx.x * per, hi = lo + per < cnt ? lo + per : cnt;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += n[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {        // inclusive Hillis-Steele scan of the per-thread sums
        const uint64_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0ull;
    for (uint64_t i = lo; i < hi; ++i) { first[i] = run; run += n[i]; }
    if (threadIdx.x == kScanThreads - 1) first[cnt] = part[kScanThreads - 1];
}

__global__ __launch_bounds__(256) void mem_gather_kernel(const MemOut *__restrict__ mems, const uint64_t *__restrict__ offs,
                                                         const uint32_t *__restrict__ n, const uint64_t *__restrict__ first,
                                                         uint64_t n_reads, MemOut *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const MemOut *src = mems + offs[i];
    MemOut *dst = out + first[i];
    for (uint32_t k = 0; k < n[i]; ++k) dst[k] = src[k];
}

hipError_t launch_mem_compact(const MemOut *d_mems, const uint64_t *d_offsets, const uint32_t *d_n_mems, uint64_t n_reads,
                              uint64_t *d_first, MemOut *d_out, hipStream_t stream, bool scan_only) {
    if (!scan_only) {
        const uint64_t blocks = (n_reads + 255) / 256;
        if (blocks == 0) return hipSuccess;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(mem_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_mems, d_offsets, d_n_mems, d_first, n_reads, d_out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(mem_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_n_mems, n_reads, d_first);
    return hipGetLastError();
}

}  // namespace movi
