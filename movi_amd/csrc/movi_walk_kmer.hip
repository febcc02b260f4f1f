// movi_walk_kmer.hip -- k-mer presence: MoveStructure::query_all_kmers / query_kmers_from, src/sequitur.cpp:257-421 (the non-count
// branch), over initialize_backward_search / backward_search, src/move_structure_search.cpp:169-293.  The contract -- the
// per-read array bw, the greedy loop over it, where it deviates from the reference -- is stated in include/movi_hip.h
// (movi_kmer_device).
//
// One lane per read, blocks of one wavefront, as mem_kernel (movi_walk_mem.hip).  Every iteration every lane with work takes
// ONE backward-search step on the base its phase asks for:
//   search   P[e], P[e-1], ... to the search's death or the read's left end      bw[e]: a run if >= k, else e is a dead end
//   look     P[a], P[a-1], ..., P[e-k+1]          (e - step <= a < e)            does the left part of e's window occur?
// The two phases differ only in where they start and how many bases they may take, so all lanes share every instruction.
//
// Which ends are skipped (every skip is of ends proven dead, so none changes the answer):
//   * a search or a look that dies ON an illegal base x kills every end in [x, x + k - 1]: e = x - 1;
//   * a look from a that dies before it has taken its k - (e - a) bases found an absent substring inside the window of every
//     end in [a, e]: e = a - 1 (the reference's look-ahead, sequitur.cpp:339-370, valid for any split point a);
//   * a search that dies short of k kills e alone: e -= 1.
// The reference looks ahead from e - k/3 before every search.  Here a look is taken only with a *hint*: the position x where
// the last search or look died, while x is still inside e's window -- P[x .. something] is absent, so a look that starts at or
// right of x and runs left is likely to die too --, and it starts at a = max(x, e - step), never left of the hint (a look
// from left of x would pass and be wasted).  After a look that passes, e is searched without another look.  Around one
// substituted base the k dead ends cost about three short looks instead of k searches of up to k - 1 steps each.  The split
// `step` comes from the host ("kmer_lookahead"; kmer_look_step, movi_abi.hip: by k and the text's length, none for short k).
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"

#include <cstdio>

namespace movi {

namespace {
enum : uint32_t { kPhSearch = 0, kPhLook = 1, kPhDone = 2 };
}

// a.k >= 1; a.step = the look-ahead's split (0 = no look-ahead).  IdxT: the type the lane's interval rows are kept in between
// iterations (uint32_t when DevIndex::idx32).
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void kmer_kernel(DevIndex ix, KmerArgs a, const uint8_t *__restrict__ bases,
                                                  const uint64_t *__restrict__ offs, uint64_t n_reads, KmerRun *__restrict__ runs,
                                                  uint32_t *__restrict__ n_runs, uint32_t *__restrict__ found,
                                                  uint8_t *__restrict__ err, DevStats *stats, const uint32_t *__restrict__ order) {
    __shared__ uint8_t s_code[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();

    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = t < n_reads;
    const uint64_t rid = (valid && order) ? order[t] : t;
    const uint64_t beg = valid ? offs[rid] : 0;
    const uint32_t m = valid ? (uint32_t)(offs[rid + 1] - beg) : 0u;
    const uint8_t *R = bases + beg;
    KmerRun *O = runs + beg;                             // run j of the read: O[j], j < m - k + 1
    const uint32_t k = a.k, step = a.step, K = ix.ftab_k;

    // Positions are kept one up, so that "none" and "left of the read" are 0: E = e + 1 (the end under test, exclusive),
    // X = x + 1 (the hint; 0 = none), J = j + 1 (the next base of the phase).
    uint32_t E = m, X = 0, J = 0;
    uint32_t lim = 0, l = 0;          // bases the phase may take, bases taken (interval non-empty after each)
    uint32_t ph = kPhDone;
    bool tried = false;               // a look from this E has passed: search it
    uint32_t nr = 0, nf = 0, failed = 0, ff_total = 0, scan_total = 0, lane_steps = 0, wave_steps = 0;
    IdxT krs = 0, kre = 0;
    uint32_t os = 0, oe = 0;
    uint2 rws = make_uint2(0, 0), rwe = make_uint2(0, 0);
    auto enter = [&]() {              // the next phase from E, X, tried
        l = 0;
        if (E < k) { ph = kPhDone; return; }
        if (step != 0u && !tried && X != 0u && X <= E && X + k > E) {   // the hint lies in e's window
            const uint32_t A = (E - step > X) ? E - step : X;           // (E >= k > step)
            if (A < E) { ph = kPhLook; J = A; lim = k - (E - A); return; }
        }
        ph = kPhSearch; J = E; lim = E; tried = false;
    };
    if (valid) enter();

    while (wave_any(ph != kPhDone)) {
        const bool live = ph != kPhDone;
        wave_steps += 1;
        lane_steps += (uint32_t)live;
        uint64_t rs = krs, re = kre;
        const uint32_t b = live ? (uint32_t)s_code[R[J - 1u]] : 0xFFu;
        bool stepped = false;
        // ---- a phase's first K bases by one lookup in the interval table (DevIndex::ftab), when they are all legal, stay
        // inside the phase's range, and the entry is valid (a cleared entry is not "absent": counter overflow clears it too)
        if (K != 0u && live && l == 0 && K <= lim) {
            uint32_t kidx = 0, bad = 0;
            for (uint32_t i = 0; i < K; ++i) {          // K is wave-uniform; J - 1 - i >= J - lim >= 0
                const uint32_t cc = (uint32_t)s_code[R[J - 1u - i]] - ix.sep;
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
                J -= K;
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
        if (ix.r >= 8) shrink_interval<MODE>(ix, ext && rs <= re, b, rs, os, rws, re, oe, rwe, scan_total);
        else shrink_interval_rows<MODE>(ix, ext && rs <= re, b, rs, os, rws, re, oe, rwe, scan_total);
        bool ne = ext && ((rs < re) || (rs == re && os <= oe));
        const uint32_t e12 = lf_step2<MODE>(ix, ne, rs, os, rws, re, oe, rwe, ff_total);
        if (e12) { failed = e12; ph = kPhDone; ne = false; }
        if (ne && !((rs < re) || (rs == re && os <= oe))) ne = false;
        if (ne || ne_init) { l += 1; J -= 1; }
        krs = (IdxT)rs; kre = (IdxT)re;
        const bool grown = stepped || ne || ne_init;
        // ---- the phase ends at its first empty step or when its range is used up.  A phase that died did so on base J - 1:
        // P[J-1 .. start of the phase] does not occur, or P[J-1] is illegal
        if (live && !failed && (!grown || l == lim)) {
            const bool died = !grown;
            const bool barrier = died && b == 0xFFu;
            if (ph == kPhLook) {
                if (!died) tried = true;                 // the left part of e's window occurs: nothing learnt, search e
                else if (barrier) { E = J - 1u; X = 0; }
                else { E = J + l - 1u; X = J; }          // every end from the look's start a = J + l - 1 up to e is dead: e = a - 1
            } else {
                if (l >= k) {                            // bw[e] = l: the k-mers starting at L, ..., L + l - k, L = e - l + 1
                    KmerRun o;
                    o.start = E - l; o.count = l - k + 1u;
                    O[nr] = o;
                    nr += 1;
                    nf += o.count;
                    if (barrier) { E = J - 1u; X = 0; }
                    else { E = E - l + k - 1u; X = E >= k ? J : 0u; }   // e = L + k - 2; the search died on L - 1 (or L = 0: over)
                } else if (barrier) { E = J - 1u; X = 0; }
                else { E -= 1u; X = J; }
            }
            enter();
        }
    }
    if (valid) {
        n_runs[rid] = failed ? 0u : nr;
        if (found) found[rid] = failed ? 0u : nf;
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

hipError_t launch_kmer(int mode, const DevIndex &ix, const KmerArgs &a, const uint8_t *d_bases, const uint64_t *d_offsets,
                       uint64_t n_reads, KmerRun *d_runs, uint32_t *d_n_runs, uint32_t *d_found, uint8_t *d_err,
                       DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info) {
    if (n_reads == 0) return hipSuccess;
    if ((mode != 6 && mode != 3) || a.k == 0u) return hipErrorInvalidValue;
    const uint64_t blocks = (n_reads + 63) / 64;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    char nm[96];
    snprintf(nm, sizeof(nm), "kmer_kernel<%d, %s>", mode, ix.idx32 ? "unsigned int" : "unsigned long");
    note_walk_launch(nm);
    if (info) {
        *info = LaunchInfo();
        snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
        info->variant = a.step ? 1 : 0; info->block_threads = 64; info->idx64 = ix.idx32 ? 0 : 1;
    }
    const dim3 grid((unsigned)blocks), block(64);
    if (mode == 6 && ix.idx32)
        hipLaunchKernelGGL((kmer_kernel<6, uint32_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_runs, d_n_runs, d_found, d_err, d_stats, d_order);
    else if (mode == 6)
        hipLaunchKernelGGL((kmer_kernel<6, uint64_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_runs, d_n_runs, d_found, d_err, d_stats, d_order);
    else if (ix.idx32)
        hipLaunchKernelGGL((kmer_kernel<3, uint32_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_runs, d_n_runs, d_found, d_err, d_stats, d_order);
    else
        hipLaunchKernelGGL((kmer_kernel<3, uint64_t>), grid, block, 0, stream, ix, a, d_bases, d_offsets, n_reads, d_runs, d_n_runs, d_found, d_err, d_stats, d_order);
    return hipGetLastError();
}

// ---- the host path's compaction: every read's runs from runs[offs[i] ..] to out[first[i] ..] (first: launch_mem_compact's scan)

__global__ __launch_bounds__(256) void kmer_gather_kernel(const KmerRun *__restrict__ runs, const uint64_t *__restrict__ offs,
                                                          const uint32_t *__restrict__ n, const uint64_t *__restrict__ first,
                                                          uint64_t n_reads, KmerRun *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const KmerRun *src = runs + offs[i];
    KmerRun *dst = out + first[i];
    for (uint32_t j = 0; j < n[i]; ++j) dst[j] = src[j];
}

hipError_t launch_kmer_gather(const KmerRun *d_runs, const uint64_t *d_offsets, const uint32_t *d_n_runs, uint64_t n_reads,
                              const uint64_t *d_first, KmerRun *d_out, hipStream_t stream) {
    const uint64_t blocks = (n_reads + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmer_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_runs, d_offsets, d_n_runs, d_first, n_reads, d_out);
    return hipGetLastError();
}

}  // namespace movi
