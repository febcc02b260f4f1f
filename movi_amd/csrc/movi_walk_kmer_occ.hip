// movi_walk_kmer_occ.hip -- k-mer occurrences: for every k-mer of every read, how often it occurs in the indexed text (the `count` of
// movi_count_device for that k-mer as a read of its own, 0 where it does not occur whole).  The contract is stated in
// include/movi_hip.h (movi_kmer_occ_device).  Not the reference's --kmer-count (src/sequitur.cpp:14-255), which stays refused.
//
// Three kernels on the caller's stream, and the slots of d_occ are all they share:
//   kmer_occ_mark_kernel     one lane per read: a *pending mark* (kOccPending) into the slot of every k-mer whose k bases are legal,
//                            0 into the read's other slots (a k-mer with an illegal base, the last k - 1 slots);
//   kmer_occ_kernel          the searches.  Blocks of one wavefront; a lane owns the slots lane, lane + stride, ... of all n_bases slots
//                            (locate_kernel's lists, movi_walk_sa.hip) and takes up its next slot in the iteration after a search
//                            ends, so the wavefronts stay full although a search that dies early is over in one step and a found
//                            k-mer takes 1 + (k - K) of them.  A slot that holds no mark costs one iteration; a marked slot g is a
//                            backward search over bases[g + k - 1] down to bases[g]: search_step (movi_search.hpp) with lim = k --
//                            the interval table's lookup first where K <= k --, which ends dead (0) or at l == k (the interval's
//                            count, MoveInterval::count).  No read ids anywhere: the marks carry everything;
//   kmer_occ_reduce_kernel   one wavefront per read: found, sum and the error code from the read's slots.
// A k-mer whose search hits one of the reference's LF throws becomes an error slot (kOccErr | code; MOVI_OCC_IS_ERROR).
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"

namespace movi {

namespace {

constexpr uint64_t kOccPending = 1ull << 62;             // bit 63 clear, above every count (a text has fewer than 2^40 positions)
constexpr uint64_t kOccErr = ~0xFFull;                   // | kErr*

// Slot beg + p of a read of m bases: pending iff P[p .. p + k) lies inside the read (and inside the n_slots slots of the call) and
// is all legal -- a running count of consecutive legal bases, left to right: the k-mer that ENDS at base q starts at q - k + 1.
__global__ __launch_bounds__(64) void kmer_occ_mark_kernel(DevIndex ix, uint32_t k, const uint8_t *__restrict__ bases,
                                                           const uint64_t *__restrict__ offs, uint64_t n_reads, uint64_t n_slots,
                                                           uint64_t *__restrict__ occ) {
    __shared__ uint8_t s_code[256];
    const ReadLane rl = read_lane(ix, s_code, offs, n_reads, nullptr);
    if (!rl.valid) return;
    const uint64_t beg = rl.beg, end = beg + rl.m;
    if (beg >= n_slots) return;
    if (end > n_slots) {                                   // n_bases != offsets[n_reads]: the read gets no k-mer (the reduction says why)
        for (uint64_t g = beg; g < n_slots; ++g) occ[g] = 0;
        return;
    }
    const uint32_t m = rl.m;
    uint32_t legal = 0;
    for (uint32_t q = 0; q < m; ++q) {
        const uint32_t cc = (uint32_t)s_code[bases[beg + q]] - ix.sep;
        legal = cc <= 3u ? legal + 1u : 0u;
        if (q + 1u >= k) occ[beg + (q + 1u - k)] = legal >= k ? kOccPending : 0ull;
    }
    for (uint32_t p = m >= k ? m - k + 1u : 0u; p < m; ++p) occ[beg + p] = 0;      // the last k - 1 slots hold no k-mer
}

}  // namespace

// IdxT: the type the lane's interval rows are kept in between iterations (uint32_t when DevIndex::idx32).
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void kmer_occ_kernel(DevIndex ix, uint32_t k, const uint8_t *__restrict__ bases, uint64_t n_slots,
                                                      uint64_t *__restrict__ occ, DevStats *stats) {
    __shared__ uint8_t s_code[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 64u;
    uint64_t g = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    uint32_t state = g < n_slots ? 1u : 0u;               // 0 = list done, 1 = take up slot g, 2 = searching
    uint32_t l = 0;                                       // bases of the k-mer taken (the interval is non-empty after each)
    uint32_t ff_total = 0, scan_total = 0, errs = 0;
    uint64_t lane_steps = 0, wave_steps = 0;
    IdxT krs = 0, kre = 0;
    uint32_t os = 0, oe = 0;
    uint2 rws = make_uint2(0, 0), rwe = make_uint2(0, 0);
    while (wave_any(state != 0u)) {
        wave_steps += 1;
        if (state == 1u) {                                // the lane's next slot
            // (a mark outside [0, n_slots - k] is none of the mark kernel's: never searched, so no base outside the batch is read)
            if (occ[g] == kOccPending && k <= n_slots && g <= n_slots - k) { l = 0; state = 2u; }
            else { g += stride; state = g < n_slots ? 1u : 0u; }
        }
        const bool live = state == 2u;                    // (a lane that took up a slot above steps in this same iteration)
        lane_steps += live ? 1u : 0u;
        // ---- one step leftwards on the k-mer's next base: bases[g + k - 1 - l - i], i < k - l
        uint64_t rs = krs, re = kre;
        const uint8_t *R = bases + g + (k - 1u - l);
        auto base_at = [&](uint32_t i) { return (uint32_t)s_code[*(R - i)]; };
        auto keep = [](uint64_t, uint64_t, uint32_t, uint32_t) {};
        const SearchStep st = search_step<MODE>(ix, live, k, l, base_at, keep, rs, os, rws, re, oe, rwe, ff_total, scan_total);
        krs = (IdxT)rs; kre = (IdxT)re;
        if (live && (st.err != 0u || st.taken == 0u || l == k)) {
            uint64_t v = 0;
            if (st.err) { v = kOccErr | st.err; errs += 1; }
            else if (st.taken != 0u) {                    // MoveInterval::count (include/move_intervals.hpp:47-58)
                if (rs == re) v = (uint64_t)oe - os + 1;
                else if (re - rs < (1ull << kPrefixShift)) {          // inside a checkpoint block's reach: the rows between the ends
                    v = (uint64_t)row_n<MODE>(rws) - os + oe + 1;
                    for (uint64_t j = rs + 1; j < re; ++j) v += row_n<MODE>(load_row<MODE>(ix.rows, j));
                } else v = (row_start<MODE>(ix, re) + oe) - (row_start<MODE>(ix, rs) + os) + 1;
            }
            occ[g] = v;
            g += stride;
            state = g < n_slots ? 1u : 0u;
        }
    }
    const uint32_t scw = wave_sum(scan_total), erw = wave_sum(errs);
    unsigned long long ffw = ff_total, lsw = lane_steps;    // summed in 64 bits: a lane's list holds many searches
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        ffw += __shfl_xor(ffw, s, 64);
        lsw += __shfl_xor(lsw, s, 64);
    }
    if ((threadIdx.x & 63) == 0 && stats) {
        if (ffw) atomicAdd(&stats->fast_forwards, ffw);
        if (scw) atomicAdd(&stats->scans, (unsigned long long)scw);
        if (erw) atomicAdd(&stats->errors, (unsigned long long)erw);
        atomicAdd(&stats->lane_steps, lsw);
        atomicAdd(&stats->wave_steps, (unsigned long long)wave_steps);
    }
}

namespace {

// One wavefront per read (four to a block).  A read with an error slot reports that slot's code -- the first one's -- and found = sum = 0;
// a read that reaches past the call's slots (n_bases != offsets[n_reads]) reports 0xFF.
__global__ __launch_bounds__(256) void kmer_occ_reduce_kernel(const uint64_t *__restrict__ occ, const uint64_t *__restrict__ offs,
                                                              uint64_t n_reads, uint64_t n_slots, uint32_t *__restrict__ found,
                                                              uint64_t *__restrict__ sum, uint8_t *__restrict__ err) {
    const uint64_t rid = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (rid >= n_reads) return;                           // (wave-uniform)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t beg = offs[rid], end = offs[rid + 1];
    const bool outside = end > n_slots || beg > end;
    unsigned long long s = 0;
    uint32_t f = 0;
    unsigned long long first_bad = ~0ull;                 // position | code of the read's first error slot
    if (!outside)
        for (uint64_t g = beg + lane; g < end; g += 64u) {
            const uint64_t v = occ[g];
            if (v >> 63) { if (first_bad == ~0ull) first_bad = ((g - beg) << 8) | (v & 0xFFu); }
            else { s += v; f += v != 0u ? 1u : 0u; }
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s += __shfl_xor(s, d, 64);
        f += __shfl_xor(f, d, 64);
        const unsigned long long o = __shfl_xor(first_bad, d, 64);
        first_bad = o < first_bad ? o : first_bad;
    }
    if (lane != 0u) return;
    const uint32_t code = outside ? 0xFFu : (first_bad == ~0ull ? 0u : (uint32_t)(first_bad & 0xFFu));
    if (found) found[rid] = code ? 0u : f;
    if (sum) sum[rid] = code ? 0ull : s;
    if (err) err[rid] = (uint8_t)code;
}

template <int MODE, typename IdxT>
void launch_occ_t(unsigned blocks, hipStream_t stream, const DevIndex &ix, uint32_t k, const uint8_t *d_bases, uint64_t n_slots,
                  uint64_t *d_occ, DevStats *d_stats) {
    hipLaunchKernelGGL((kmer_occ_kernel<MODE, IdxT>), dim3(blocks), dim3(64), 0, stream, ix, k, d_bases, n_slots, d_occ, d_stats);
}

}  // namespace

hipError_t launch_kmer_occ(int mode, const DevIndex &ix, uint32_t k, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t n_bases, uint64_t *d_occ, uint32_t *d_found, uint64_t *d_sum, uint8_t *d_err, DevStats *d_stats,
                           int num_cus, hipStream_t stream, LaunchInfo *info) {
    if (n_reads == 0) return hipSuccess;
    if ((mode != 6 && mode != 3) || k == 0u) return hipErrorInvalidValue;
    if ((n_reads + 63) / 64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    char nm[96];
    snprintf(nm, sizeof(nm), "kmer_occ_kernel<%d, %s>", mode, ix.idx32 ? "unsigned int" : "unsigned long");
    note_walk_launch(nm);
    if (info) {
        *info = LaunchInfo();
        snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
        info->variant = 0; info->block_threads = 64; info->idx64 = ix.idx32 ? 0 : 1;
        info->waves_per_cu = kKmerOccWaves;
    }
    if (n_bases != 0) {
        hipLaunchKernelGGL(kmer_occ_mark_kernel, dim3((unsigned)((n_reads + 63) / 64)), dim3(64), 0, stream, ix, k, d_bases, d_offsets, n_reads,
                           n_bases, d_occ);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        // one-wavefront blocks; at most kKmerOccWaves per CU, so that a lane's list holds many k-mers wherever there are many
        const uint64_t want = (n_bases + 63) / 64, cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * kKmerOccWaves;
        const unsigned blocks = (unsigned)(want < cap ? want : cap);
        if (mode == 6) {
            if (ix.idx32) launch_occ_t<6, uint32_t>(blocks, stream, ix, k, d_bases, n_bases, d_occ, d_stats);
            else launch_occ_t<6, uint64_t>(blocks, stream, ix, k, d_bases, n_bases, d_occ, d_stats);
        } else {
            if (ix.idx32) launch_occ_t<3, uint32_t>(blocks, stream, ix, k, d_bases, n_bases, d_occ, d_stats);
            else launch_occ_t<3, uint64_t>(blocks, stream, ix, k, d_bases, n_bases, d_occ, d_stats);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (d_found || d_sum || d_err) {
        hipLaunchKernelGGL(kmer_occ_reduce_kernel, dim3((unsigned)((n_reads + 3) / 4)), dim3(256), 0, stream, d_occ, d_offsets, n_reads, n_bases,
                           d_found, d_sum, d_err);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t preload_kmer_occ(int mode, bool idx32) {
    hipFuncAttributes at;
    const void *f = mode == 6 ? (idx32 ? (const void *)kmer_occ_kernel<6, uint32_t> : (const void *)kmer_occ_kernel<6, uint64_t>)
                              : (idx32 ? (const void *)kmer_occ_kernel<3, uint32_t> : (const void *)kmer_occ_kernel<3, uint64_t>);
    return hipFuncGetAttributes(&at, f);
}

}  // namespace movi
