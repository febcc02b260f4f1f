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
// The step is the same operation in all three phases -- search_step (movi_search.hpp, shared with the k-mer kernel); only the base
// and the position bookkeeping differ -- so lanes in different phases share every instruction.  What is this file's own: the phases
// (enter, the phase-end block) and the kept copy of the interval before the step.  Prologue, counters and launch: movi_search.hpp.
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"

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
    const ReadLane rl = read_lane(ix, s_code, offs, n_reads, order);
    const bool valid = rl.valid;
    const uint64_t rid = rl.rid, beg = rl.beg;
    const uint32_t m = rl.m;
    const uint8_t *R = bases + beg;
    MemOut *O = mems + beg;                              // MEM j of the read: O[j], j < m - L' + 1
    const uint32_t Lp = a.min_len;
    auto comp = [&](uint32_t c) { return c == 0xFFu ? 0xFFu : (uint32_t)((a.comp >> (8u * c)) & 0xFFu); };

    uint32_t ph = (valid && m >= Lp) ? kPhWindow : kPhDone;
    uint32_t pos = 0;                 // the left end under test
    uint32_t e = 0;                   // end (exclusive) of the last MEM: the next phase walks back from it
    uint32_t j = 0, lim = 0, l = 0;   // next base of the phase, bases it may consume, bases consumed (interval non-empty after each)
    uint32_t nm = 0, failed = 0, ff_total = 0, scan_total = 0, lane_steps = 0, wave_steps = 0;
    uint64_t rs = 0, re = 0;
    uint32_t os = 0, oe = 0;
    uint2 rws = make_uint2(0, 0), rwe = make_uint2(0, 0);
    IdxT prs = 0, pre = 0;            // the interval before the last step (extend: reported if that step came out empty)
    uint32_t pos_ = 0, poe = 0;
    auto enter = [&](uint32_t p) {    // phase p from the current pos / e
        ph = p;
        l = 0;
        if (p == kPhWindow) { j = pos + Lp - 1; lim = Lp; }
        else if (p == kPhExtend) { j = pos; lim = m - pos; }
        else if (p == kPhNext) { j = e; lim = e - pos; }
    };
    if (ph == kPhWindow) enter(kPhWindow);

    while (wave_any(ph != kPhDone)) {
        const bool live = ph != kPhDone;
        wave_steps += 1;
        lane_steps += (uint32_t)live;
        // ---- one step on the phase's next base: window and next read leftwards, extend reads the complement rightwards
        const bool fwd = ph == kPhExtend;
        auto base_at = [&](uint32_t i) {
            const uint32_t c = s_code[R[fwd ? j + i : j - i]];
            return fwd ? comp(c) : c;
        };
        auto keep = [&](uint64_t s0, uint64_t e0, uint32_t so, uint32_t eo) { prs = (IdxT)s0; pre = (IdxT)e0; pos_ = so; poe = eo; };
        const SearchStep st = search_step<MODE>(ix, live, lim, l, base_at, keep, rs, os, rws, re, oe, rwe, ff_total, scan_total);
        if (st.err) { failed = st.err; ph = kPhDone; }
        j = fwd ? j + st.taken : j - st.taken;
        const bool ext = st.ext, grown = st.taken != 0u;
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
    flush_lane_stats(stats, ff_total, scan_total, failed, lane_steps, wave_steps);
}

namespace {
struct MemFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &mem_kernel<MODE, IdxT>; }
};
}

hipError_t launch_mem(int mode, const DevIndex &ix, const MemArgs &a, const uint8_t *d_bases, const uint64_t *d_offsets,
                      uint64_t n_reads, MemOut *d_mems, uint32_t *d_n_mems, uint8_t *d_err, DevStats *d_stats,
                      const uint32_t *d_order, hipStream_t stream, LaunchInfo *info) {
    return launch_lane_per_read<MemFamily>("mem_kernel", 0, mode, ix, n_reads, stream, info, a, d_bases, d_offsets, n_reads, d_mems, d_n_mems,
                                           d_err, d_stats, d_order);
}

}  // namespace movi
