// movi_walk.hpp -- the PML walk: pml_kernel_flatp, the lane state machine every PML query runs on, and the dispatch
// from a launch's run-time choices to its instantiation.  Included by the movi_walk_*.hip translation units only.
#pragma once
#include "movi_device.hpp"

namespace movi {

// The walk ("flat state machine + row window, software-pipelined, window-parallel advance": what rounds 2 - 4 called
// variant 14): every lane runs the reference's per-base automaton (LF_move -> fast_forward -> match / reposition scan) for its
// own read, one row-window gather per iteration, with
//   * the 4-row WINDOW around the row it needs fetched instead of the row (32 B of one cache line, one L2 request) and every
//     fast-forward / scan step that stays inside it resolved in closed form (window_advance);
//   * the next window's address computed from the row alone (all selects) and its load issued BEFORE the step's
//     bookkeeping (PML packing and stores, bins, counters, base decode), which then runs under the gather's latency; the
//     load is unpredicated and branch-free (the table's last window is pulled back to rows [r-4, r); finished lanes re-read
//     window 0) -- with a predicated two-path fetch hipcc parked a `s_waitcnt vmcnt(0)` right behind the load and the
//     overlap was gone;
//   * STG = 0 only: read chunks double-buffered, 16 bases per fetch (the chunk load is always an L2 miss: its line was
//     evicted long ago), PMLs out as paired 16-byte stores.
// Removed in round 5 (measured, never a default; the code is in the history at commit ceb31ea): the hop-by-hop advance
// (HA >= 0: up to HA dependent in-window hops instead of the closed form; -2.5 % on long reads, -5.5 % on the 8 GB table,
// profiles/r02_window_parallel.txt), the row-at-a-time state machine without a window (pml_kernel_flat, "variant 7"), and
// LANE REFILL (REFILL = 1, "variant 13": a persistent grid whose idle lanes take the next reads of a per-wavefront pool fed
// from one global ticket counter; SIMT efficiency 0.72 -> 0.87 on c2 and no faster in rounds 2 and 4 -- fuller wavefronts
// issue more gathers per iteration and the fabric serves them no faster: profiles/r04_lane_refill.txt).
// SEG (segment-parallel long reads, movi_kernels.hpp): 0 = a lane walks a read; 1 = a lane walks one SEGMENT of a read
// from the state every read starts in (K1: its "read" is the segment -- bases at seg_in, PMLs to seg_out --, it leaves a
// checkpoint of its state and counters every 32 bases and its final state, reports an invariant violation in its
// segment's flag instead of err[] / zero-filling, and adds nothing to the global fast-forward / scan counters: which
// part of its work belongs to the read's real walk is only known after K2); 2 = whole reads again, but only those in
// seg.read_fail (K3).
// AHD (look-ahead rows, DevIndex::rows2; staged kernels only): the window comes from the table's second copy, together
// with the look-ahead entries of its four rows (the other half of the same 128-byte line).  When the step's emitted base is followed by a base that
// matches at the LF target j = id(row) without a fast-forward -- known from the entry: c(j), n(j) against the offset --
// the walk emits that PML as well and goes straight on to id(j): two bases for one gather.  Everything else (a
// mismatch, a fast-forward at j, the read's end, an invalid entry) takes the one-base step it always took.
// (Fetching only the entry of the row the window was fetched FOR -- 8 bytes instead of 32 -- misses the steps that end on a
// neighbour after a fast-forward or scan: 68.5 against 74.4 Gbases/s on c2, 54.1 against 62.8 on the random table.)
// (Round 4 built the same with entries that look TWO rows ahead -- "chain rows", 16 bytes per row, up to three bases per gather:
// bit-exact, lane iterations per base 0.68 -> 0.56 on c2 as tools/iter_model.c predicts, and 10 % SLOWER there, 38 % slower on a
// 113 M-row real BWT: twice the bytes, six loads and 18 % more instructions per iteration.  Measured with PMC
// (profiles/r04_chain_rows.txt) and removed again; the code is in the history: commit b8d3f4e.)
// FAST-FORWARD SKIP (DevIndex::ff_skip; look-ahead and deep rows; a wave-uniform run-time value, no instantiation of its own): the test
// that decides whether the next base rides along, offset < n(j), fails in two ways.  Where it fails because the offset is at or beyond
// n(j), the reference's next action is decided whatever that base is -- LF_move lands on j, fast_forward passes j -- so the gather goes
// to the window of j + 1 with that fast-forward taken.  Where j is its window's last row the old iteration learnt only "next window":
// c2 lane iterations per base 0.5426 -> 0.5068, fabric lines -4.1 %, 88.0 -> 89.8 Gbases/s for 22 more VALU per iteration
// (profiles/ff_skip.txt).
// PSH = 1 (round 4: "pair-shared gathers"; staged kernels, plain and look-ahead rows): the two lanes of a pair (2i, 2i + 1) fetch
// their windows TOGETHER -- one load instruction brings the even lane's window (each lane one 16-byte half), the next the odd
// lane's, and one exchange across the pair (DPP quad_perm) hands every lane the half it is missing.  Same loads per lane,
// same bytes -- but the two lanes' requests for adjacent bytes of a page are ONE address translation and ONE 32-byte access,
// where a lane's two 16-byte loads are two of each: tools/tlb_bench (profiles/r04_pair_shared_gather_microbench.txt), 32-byte
// window per chain step: 8 GB table 27.3 -> 49.4 G/s (the 8-byte gather rate), 2 GB 44.3 -> 54.8, 134 MB 52.0 -> 59.5.
// AHD = 3 (CHAIN ROWS; pml_kernel_chain below, a kernel of its own name over the same body; movi_chain_fields.hpp has the layout): rows of 32
// bytes that carry what the walk reads at j1 = id(row), j2 and j3, the ids up to j4 and n(j4) -- up to FOUR bases per gather.  The window
// stays half a cache line, two rows in the same four 16-byte loads, and its closed form has two rows where the deep rows' has three: no
// divide by three, two-way selects.  Round 4's rows of the same size looked two rows ahead through whole-line windows and six loads, and
// wrote PMLs through the packer at cap 9 (profiles/r04_chain_rows.txt); these look three ahead and skip the fast-forward behind every
// depth, the last ride's included (n(j4)).  Plain PML of whole reads on 32-bit row indexes, masks or the register packer out.
template <int MODE, typename IdxT, int CLS, int SEP, int SEG, int STG, int AHD, int PSH, int RING>
__global__ __launch_bounds__(256) void pml_kernel_flatp(DevIndex ix, const uint8_t *__restrict__ bases,
                                                       const uint64_t *__restrict__ offs, uint64_t n_reads,
                                                       uint16_t *__restrict__ out, uint8_t *__restrict__ err,
                                                       DevStats *stats, const uint32_t *__restrict__ order,
                                                       ClsArgs cls, SegArgs seg) {
    static_assert(AHD != 3, "the chain rows' walk is pml_kernel_chain");
#include "movi_walk_body.inc"
}
// The walk on the chain rows (AHD = 3 above; DevIndex::rows3 = the chain rows of this launch): staged reads of whole reads, 32-bit row
// indexes; RING 0 = PMLs through the register packer, 2 = reset masks (with the fused expansion and parked lanes, as ever).
template <int SEP, int RING>
__global__ __launch_bounds__(256) void pml_kernel_chain(DevIndex ix, const uint8_t *__restrict__ bases,
                                                       const uint64_t *__restrict__ offs, uint64_t n_reads,
                                                       uint16_t *__restrict__ out, uint8_t *__restrict__ err,
                                                       DevStats *stats, const uint32_t *__restrict__ order) {
    constexpr int MODE = 6, CLS = 0, SEG = 0, STG = 1, AHD = 3, PSH = 0;
    using IdxT = uint32_t;
    const ClsArgs cls{};
    const SegArgs seg{};
#include "movi_walk_body.inc"
}

// ---- from a launch's run-time choices (WalkLaunch, movi_kernels.hpp) to its instantiation.  Every translation unit that
// includes this header instantiates the kernels of ONE (IdxT, SEG class): movi_walk_u32.hip / _u64.hip (whole reads),
// movi_walkseg_u32.hip / _u64.hip (segments and re-walked reads), so that they compile side by side.
template <typename IdxT, int SEG, int CLS, int SEP, int STG, int AHD, int PSH, int RING>
static hipError_t walk_go(const WalkLaunch &L, LaunchInfo *info) {
    auto kern = pml_kernel_flatp<6, IdxT, CLS, SEP, SEG, STG, AHD, PSH, RING>;
    if (L.dyn_lds > 65536) {                               // every kernel that is handed more than 64 KiB of dynamic LDS must opt in first
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.dyn_lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(kern, L.grid, L.block, L.dyn_lds, L.stream, L.ix, L.bases, L.offs, L.n, L.out, L.err, L.stats, L.order, L.cls, L.seg);
    char name[96];                                         // the name as rocprofv3 prints it: every template argument, none dropped
    snprintf(name, sizeof(name), "pml_kernel_flatp<6, %s, %d, %d, %d, %d, %d, %d, %d>", sizeof(IdxT) == 4 ? "unsigned int" : "unsigned long",
             CLS, SEP, SEG, STG, AHD, PSH, RING);
    if (info) snprintf(info->kernel, sizeof(info->kernel), "%s", name);
    note_walk_launch(name);
    return hipGetLastError();
}
template <typename IdxT, int SEG, int CLS, int SEP>
static hipError_t walk_pick(const WalkLaunch &L, LaunchInfo *info) {
    if (!L.stg) return walk_go<IdxT, SEG, CLS, SEP, 0, 0, 0, 0>(L, info);
    if (L.ahd == 2) {                                      // deep rows: 32-bit row indexes, no pair-shared gathers (launch_pml sees to both)
        if constexpr (sizeof(IdxT) == 4) {
            if (L.ring == 2) {
                if constexpr (SEG == 0 && CLS == 0) return walk_go<IdxT, 0, 0, SEP, 1, 2, 0, 2>(L, info);
                else return hipErrorInvalidValue;
            }
            return L.ring ? walk_go<IdxT, SEG, CLS, SEP, 1, 2, 0, 1>(L, info) : walk_go<IdxT, SEG, CLS, SEP, 1, 2, 0, 0>(L, info);
        } else {
            return hipErrorInvalidValue;
        }
    }
    if (L.ring == 2) {                                     // reset masks out (plain PML of whole reads: launch_pml sees to it)
        if constexpr (SEG == 0 && CLS == 0) {
            switch ((L.ahd ? 2 : 0) | (L.psh ? 1 : 0)) {
            case 0: return walk_go<IdxT, 0, 0, SEP, 1, 0, 0, 2>(L, info);
            case 1: return walk_go<IdxT, 0, 0, SEP, 1, 0, 1, 2>(L, info);
            case 2: return walk_go<IdxT, 0, 0, SEP, 1, 1, 0, 2>(L, info);
            default: return walk_go<IdxT, 0, 0, SEP, 1, 1, 1, 2>(L, info);
            }
        } else {
            return hipErrorInvalidValue;
        }
    }
    switch ((L.ahd ? 4 : 0) | (L.psh ? 2 : 0) | (L.ring ? 1 : 0)) {
    case 0: return walk_go<IdxT, SEG, CLS, SEP, 1, 0, 0, 0>(L, info);
    case 1: return walk_go<IdxT, SEG, CLS, SEP, 1, 0, 0, 1>(L, info);
    case 2: return walk_go<IdxT, SEG, CLS, SEP, 1, 0, 1, 0>(L, info);
    case 3: return walk_go<IdxT, SEG, CLS, SEP, 1, 0, 1, 1>(L, info);
    case 4: return walk_go<IdxT, SEG, CLS, SEP, 1, 1, 0, 0>(L, info);
    case 5: return walk_go<IdxT, SEG, CLS, SEP, 1, 1, 0, 1>(L, info);
    case 6: return walk_go<IdxT, SEG, CLS, SEP, 1, 1, 1, 0>(L, info);
    default: return walk_go<IdxT, SEG, CLS, SEP, 1, 1, 1, 1>(L, info);
    }
}
template <typename IdxT, int SEG>
static hipError_t walk_dispatch(const WalkLaunch &L, LaunchInfo *info) {
    if (SEG != 0 || L.cls_mode == 0) return L.sep ? walk_pick<IdxT, SEG, 0, 1>(L, info) : walk_pick<IdxT, SEG, 0, 0>(L, info);
    if (SEG == 0 && L.cls_mode == 1) return L.sep ? walk_pick<IdxT, 0, 1, 1>(L, info) : walk_pick<IdxT, 0, 1, 0>(L, info);
    if (SEG == 0) return L.sep ? walk_pick<IdxT, 0, 2, 1>(L, info) : walk_pick<IdxT, 0, 2, 0>(L, info);
    return hipErrorInvalidValue;
}

}  // namespace movi
