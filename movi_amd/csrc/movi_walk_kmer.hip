// movi_walk_kmer.hip -- k-mer presence: MoveStructure::query_all_kmers / query_kmers_from, src/sequitur.cpp:257-421 (the non-count
// branch), over initialize_backward_search / backward_search, src/move_structure_search.cpp:169-293.  The contract -- the
// per-read array bw, the greedy loop over it, where it deviates from the reference -- is stated in include/movi_hip.h
// (movi_kmer_device).
//
// One lane per read, blocks of one wavefront, as mem_kernel (movi_walk_mem.hip).  Every iteration every lane with work takes
// ONE backward-search step on the base its phase asks for:
//   search   P[e], P[e-1], ... to the search's death or the read's left end      bw[e]: a run if >= k, else e is a dead end
//   look     P[a], P[a-1], ..., P[e-k+1]          (e - step <= a < e)            does the left part of e's window occur?
// The two phases differ only in where they start and how many bases they may take, so all lanes share every instruction.  The step
// is search_step (movi_search.hpp, shared with the MEM kernel), and so are the prologue, the counters' way out and the launch; this
// file's own are the phases (enter, the phase-end block) and the interval's rows kept as IdxT between iterations.
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
    const ReadLane rl = read_lane(ix, s_code, offs, n_reads, order);
    const bool valid = rl.valid;
    const uint64_t rid = rl.rid, beg = rl.beg;
    const uint32_t m = rl.m;
    const uint8_t *R = bases + beg;
    KmerRun *O = runs + beg;                             // run j of the read: O[j], j < m - k + 1
    const uint32_t k = a.k, step = a.step;

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
        // ---- one step on the phase's next base: both phases read leftwards (J - 1 - i >= J - lim >= 0)
        uint64_t rs = krs, re = kre;
        auto base_at = [&](uint32_t i) { return (uint32_t)s_code[R[J - 1u - i]]; };
        auto keep = [](uint64_t, uint64_t, uint32_t, uint32_t) {};
        const SearchStep st = search_step<MODE>(ix, live, lim, l, base_at, keep, rs, os, rws, re, oe, rwe, ff_total, scan_total);
        if (st.err) { failed = st.err; ph = kPhDone; }
        J -= st.taken;
        krs = (IdxT)rs; kre = (IdxT)re;
        const uint32_t b = st.b;
        const bool grown = st.taken != 0u;
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
    flush_lane_stats(stats, ff_total, scan_total, failed, lane_steps, wave_steps);
}

namespace {
struct KmerFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &kmer_kernel<MODE, IdxT>; }
};
}

hipError_t launch_kmer(int mode, const DevIndex &ix, const KmerArgs &a, const uint8_t *d_bases, const uint64_t *d_offsets,
                       uint64_t n_reads, KmerRun *d_runs, uint32_t *d_n_runs, uint32_t *d_found, uint8_t *d_err,
                       DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info) {
    if (n_reads != 0 && a.k == 0u) return hipErrorInvalidValue;
    return launch_lane_per_read<KmerFamily>("kmer_kernel", a.step ? 1 : 0, mode, ix, n_reads, stream, info, a, d_bases, d_offsets, n_reads, d_runs,
                                            d_n_runs, d_found, d_err, d_stats, d_order);
}

}  // namespace movi
