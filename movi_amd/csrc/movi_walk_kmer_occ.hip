// movi_walk_kmer_occ.hip -- k-mer occurrences: for every k-mer of every read, how often it occurs in the indexed text (the `count` of
// movi_count_device for that k-mer as a read of its own, 0 where it does not occur whole).  The contract is stated in
// include/movi_hip.h (movi_kmer_occ_device).  Not the reference's --kmer-count (src/sequitur.cpp:14-255), which stays refused.
//
// Three kernels on the caller's stream, and the slots of d_occ are all they share:
//   kmer_occ_mark_kernel     one lane per read: a *pending mark* (kOccPending) into the slot of every k-mer whose k bases are legal,
//                            0 into the read's other slots (a k-mer with an illegal base, the last k - 1 slots);
//   kmer_occ_kernel          the searches.  Blocks of one wavefront; a lane owns the slots lane, lane + stride, ... of all n_bases slots
//                            and takes up its next slot in the iteration after a search ends (search_lists, movi_search.hpp), so
//                            the wavefronts stay full although a search that dies early is over in one step and a found k-mer
//                            takes 1 + (k - K) of them.  A slot that holds no mark costs one iteration; a marked slot g is a
//                            backward search over bases[g + k - 1] down to bases[g] with lim = k -- the interval table's lookup
//                            first where K <= k --, which ends dead (0) or at l == k (the interval's count, interval_count).  No
//                            read ids anywhere: the marks carry everything;
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

template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void kmer_occ_kernel(DevIndex ix, uint32_t k, const uint8_t *__restrict__ bases, uint64_t n_slots,
                                                      uint64_t *__restrict__ occ, DevStats *stats) {
    search_lists<MODE, IdxT>(ix, n_slots, stats,
        [&](uint64_t g, const uint8_t *&last, uint32_t &lim) {
            // (a mark outside [0, n_slots - k] is none of the mark kernel's: never searched, so no base outside the batch is read)
            if (!(occ[g] == kOccPending && k <= n_slots && g <= n_slots - k)) return false;
            last = bases + g + (k - 1u);
            lim = k;
            return true;
        },
        [&](uint64_t g, const SearchStep &st, uint64_t rs, uint32_t os, uint2 rws, uint64_t re, uint32_t oe) {
            uint64_t v = 0;
            if (st.err) v = kOccErr | st.err;
            else if (st.taken != 0u) v = interval_count<MODE>(ix, rs, os, rws, re, oe);
            occ[g] = v;
            return st.err == 0u;
        });
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

struct KmerOccFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &kmer_occ_kernel<MODE, IdxT>; }
};

}  // namespace

hipError_t launch_kmer_occ(int mode, const DevIndex &ix, uint32_t k, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t n_bases, uint64_t *d_occ, uint32_t *d_found, uint64_t *d_sum, uint8_t *d_err, DevStats *d_stats,
                           int num_cus, hipStream_t stream, LaunchInfo *info) {
    if (n_reads == 0) return hipSuccess;
    if ((mode != 6 && mode != 3) || k == 0u) return hipErrorInvalidValue;
    if ((n_reads + 63) / 64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (n_bases != 0) {
        hipLaunchKernelGGL(kmer_occ_mark_kernel, dim3((unsigned)((n_reads + 63) / 64)), dim3(64), 0, stream, ix, k, d_bases, d_offsets, n_reads,
                           n_bases, d_occ);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipError_t e = launch_lane_lists<KmerOccFamily>("kmer_occ_kernel", 0, mode, ix, n_bases, kKmerOccWaves, num_cus, stream, info, k, d_bases,
                                                    n_bases, d_occ, d_stats);
    if (e != hipSuccess) return e;
    if (d_found || d_sum || d_err) {
        hipLaunchKernelGGL(kmer_occ_reduce_kernel, dim3((unsigned)((n_reads + 3) / 4)), dim3(256), 0, stream, d_occ, d_offsets, n_reads, n_bases,
                           d_found, d_sum, d_err);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t preload_kmer_occ(int mode, bool idx32) { return preload_family<KmerOccFamily>(mode, idx32); }

}  // namespace movi
