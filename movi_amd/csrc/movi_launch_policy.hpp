// movi_launch_policy.hpp -- the launch policy of the PML / ZML / count queries: which kernel, which block, how much dynamic LDS and what it holds.
// For a PML call also the ROUTE its results take out of the walk (plan_pml: the vector, reset masks, the vector through masks), decided once:
// the C ABI's one PML helper asks, sizes the scratch the route needs and hands the plan to launch_pml, which acts on it and derives nothing.
// Plain C++ over plain values (no HIP type, no runtime call): movi_kernels.hip acts on these plans, tests/test_launch_policy_cpu.py prints them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace movi {

constexpr int kCountCapWaves = 16;   // the count kernel's cap on cache-resident tables (plan_count)
constexpr int kCapWaves = 7;   // resident wavefronts per CU of the lane state machine on big batches (round 2: 9, optimum 8-10; round 3, with the reads staged in LDS and the top-of-walk table: 6-8, profiles/r03_occupancy_sweep.txt)
constexpr int kCapWavesAhead = 9;    // ... when the walk runs on the look-ahead rows: fewer lines per base, more walks in flight pay (profiles/r03_ahead_rows_ab.txt)
constexpr int kCapWavesDeep = 13;    // ... on the deep rows: fewer lines per base again and more instructions per iteration (c2, cap 9 / 11 / 13 / 14 / 16: vector out 71.8 / 75.7 / 78.4 / 78.7 / 77.9, reset masks out 87.3 / 89.9 / 89.4 / 89.5 / 87.8 Gbases/s: profiles/r06_deep_rows.txt)
constexpr int kCapWavesChain = 13;   // ... on the chain rows: the deep rows' cap (a sweep of 11 / 13 / 14 on c2 is in profiles/chain_rows.txt)
constexpr uint32_t kChainHintW = 4;  // width of a reposition hint in the chain rows (movi_chain_fields.hpp)
constexpr uint32_t kOutRingBytes = 4096;          // pml_kernel_flatp<..., RING = 1>: the ring in the block's dynamic LDS its PMLs leave through (32 per lane)
constexpr uint64_t kOutRingReadLen = 1024;        // ... on by itself for batches whose mean read length is at least this (plan_pml)
constexpr size_t kZmlStageBytes = 10240;          // zml_kernel_flat: dynamic LDS per one-wavefront block for its staged reads (160 bases per lane; 16 wavefronts per CU)
constexpr uint64_t kDeepReadLen = 1024;           // plan_pml: batches whose mean read length is below this walk on the deep rows (where the handle holds them)
constexpr uint64_t kPairLoadBytes = 2ull << 30;   // walked tables of this size and more: pair-shared gathers (plan_pml)
constexpr int kParkLanesAuto = 0;                 // parked lanes: what "park_lanes" -1 picks where plan_pml's rule holds; 0 = off -- on c2 every threshold from 2 to 16 is slower than none (84.8 / 81.0 / 75.7 Gbases/s at 2 / 8 / 16 against 88.1: profiles/park_lanes.txt)
constexpr uint64_t kParkMinRounds = 2;            // ... and only for batches of at least this many rounds of resident wavefronts (unmeasured: with kParkLanesAuto 0 the rule picks nothing; it is where a non-zero default would start from)
constexpr int kFfSkipDeep = 1;                    // fast-forward skip (DevIndex::ff_skip): what "ff_skip" -1 picks on the deep rows -- c2 88.0 -> 89.8 Gbases/s, c2mid 70.6 -> 73.4, every run above the parent's fastest (profiles/ff_skip.txt)
constexpr int kFfSkipAhead = 0;                   // ... and on the look-ahead rows: off in this commit -- forced on it gains 3.9 % on c2synth, 0.5 % on c3 and 4.7 % on c4, every run above the parent's; the whole GPU suite has been run with 0 only, so 1 goes in together with a suite run (same file, section 5)

struct LaunchCfg {
    int block_threads = 0;   // 0 = auto: 64 for the PML and count kernels and the ZML state machine (finest dispatch grain), 256 for the base-synchronous ZML kernel
    // -1 auto; 0 first kernel (plain I/O; serves --logs), 1 base-synchronous packed I/O, 14 = the lane state machine over
    // row windows, software-pipelined (what auto picks).  (7 / 10 / 13 -- the row-at-a-time state machine, the hop-by-hop
    // advance, lane refill -- were A/B variants that never earned a default; removed in round 5.)
    int pml_variant = -1;
    int zml_variant = -1;  // -1 auto; 0 base-synchronous kernel, 1 lane state machine
    int count_variant = -1; // -1 auto (plan_count); 0 count_kernel_v0 (base-synchronous), 1 the lane state machine (zml_kernel_flat<..., CNT = 1>)
    int num_cus = 256;
    int waves_per_cu = 0;  // 0 = auto (the state machine on big batches: kCapWaves; else no cap); else cap resident waves per CU by padding the block's LDS allocation
    int seg_len = 2048;    // PML: batches whose mean read length is >= 2 x seg_len are walked segment-parallel (0 = never) ...
    int seg_probe = 1;     // ... if a probe of the batch finds that walks started mid-read fall into step quickly (0 = always: tests;
                           // 2 = no probe and no read-back at all, the caller's seg_verdict decides: the launch stays asynchronous)
    int seg_verdict = 0;   // seg_probe == 2: 1 = cut eligible batches, 0 = one lane per read
    int stage_reads = 1;   // every lane keeps the next stretch of its read in the block's LDS (rolling for long reads); 0 = off: A/B
    int inwin = 1;         // repositions inside the window resolved in the same iteration (0 = off: A/B)
    int out_ring = -1;     // PMLs out through a ring in LDS: -1 = batches of long reads (plan_pml), 0 / 1 = never / wherever it fits (A/B)
    int classify_fused = -1; // movi_pml_classify_*: -1 auto, 1 = vector + bins fused into the walk, 0 = the walk, then classify_kernel over the vectors
    int pair_loads = -1;   // the lanes of a pair fetch their row windows together (pml_kernel_flatp<..., PSH = 1>): -1 auto (tables of 2 GB and more), 0 never, 1 always
    int hints = 1;         // 1: mismatches whose scan leaves the row window jump by the reposition hints of the look-ahead rows (DevIndex::hints); 0 = off: A/B
    int zml_ahead = 0;     // 1: zml_kernel_flat<6, T, 0, 1> on the look-ahead rows where they exist (a third fewer iterations, no faster: opt-in)
    int fused_expand = 1;  // 1: a mask walk whose caller wants the vector expands its wavefronts' reads itself (DevIndex::expand_out); 0 = pml_expand_* kernels behind the walk: A/B
    int kmer_lookahead = -1; // kmer_kernel: -1 = hinted look-ahead with a split chosen by k and the text's length (kmer_look_step), 0 = every end searched from its own base, n >= 2 = split k / n (A/B)
    int park_lanes = -1;   // parked lanes of the mask walk (DevIndex::park_at): -1 = plan_pml's rule, 0 never, 1 .. 63 = a wavefront stops at that many walking lanes, wherever the walk can park (A/B)
    int ff_skip = -1;      // fast-forward skip of the PML walk on the look-ahead / deep rows (DevIndex::ff_skip): -1 = ff_skip_on's rule, 0 never, 1 always (A/B)
    int deep = -1;         // the PML walk on the deep rows (DevIndex::rows3) where the handle holds them: -1 = batches of short reads (mean length < kDeepReadLen), 0 never, 1 always
};

// What the policy reads of the index (DevIndex, movi_kernels.hpp).
struct TableFacts {
    uint64_t r = 0;
    bool idx32 = false, sep = false;
    bool rows2 = false, rows3 = false, hints = false;   // the look-ahead rows / the deep rows / reposition hints exist
    bool rows2_count = false;                           // the count query walks on the look-ahead rows too
    bool rows4 = false;                                 // the chain rows exist (pml_kernel_chain: four bases per gather)
};

// Occupancy cap: enforced by the dispatcher through the block's LDS allocation (160 KiB per CU); blocks beyond the cap queue and start
// as resident ones retire.  The dynamic LDS that lets exactly `blocks_per_cu` blocks (raised to `floor`) share a CU, every block's
// static LDS and the allocation granule counted as 1 KiB; at most `ceiling` (default: none); 0 (no padding) from 32 blocks on and for none.
inline size_t cap_lds(int blocks_per_cu, int floor, size_t ceiling = ~(size_t)0) {
    const int bpc = std::max(blocks_per_cu, floor);
    if (bpc <= 0 || bpc >= 32) return 0;
    return std::min<size_t>(ceiling, ((163840u / (unsigned)bpc) & ~1023u) - 1024u);
}

// ------------------------------------------------------------------------------------------------------------------- PML
// What a PML call asks of the policy: what the caller wants back, and the facts that sit in its pointers and in the handle's options.
enum class PmlWant {
    kVector,              // the u16 vector
    kMasks,               // reset masks are the result
    kVectorLendsMasks,    // the vector; the caller lends mask words as scratch: through masks where the walk writes them itself
};
struct PmlAsk {
    PmlWant want = PmlWant::kVector;
    int cm = 0;                      // 0 = PML vector only, 1 = vector + classification bins, 2 = bins only
    bool logging = false, have_seg_ws = false, ordered = false;
    bool out_aligned = true;         // the vector starts on a 16-byte boundary (the fused expansion's stores)
    int via_mask = 1;                // kVectorLendsMasks ("pml_via_mask"): 1 = wherever the walk writes masks itself, -1 = only for batches of short reads (mean length < kOutRingReadLen: long reads keep the LDS ring)
    bool park_queue = false;         // a park queue is lent ...
    uint64_t park_cap = 0;           // ... of this many records
};

// The walk of one PML call, apart from the segment plan's own decisions (plan_pml_seg): kernel, block, dynamic LDS, rows.
struct PmlPlan {
    int v = 14, bt = 64, wpc = 0;
    bool seg_eligible = false;       // a batch of long reads: the segment plan gets the first say (it may decline)
    size_t dyn_lds = 0;
    uint32_t stage_lds = 0;
    bool use_ring = false, use_ahead = false, use_pair = false;
    bool use_deep = false;           // the walk runs on the deep rows (DevIndex::rows3: three bases per gather)
    int park_lanes = 0;              // > 0: a mask walk of this plan parks a wavefront's last lanes for a second launch (plan_pml: where a queue is lent and, for the vector, the expansion is fused)
    bool use_chain = false;          // the walk runs on the chain rows (pml_kernel_chain: 32-byte rows, four bases per gather); use_deep is false then
};

// Where the results of one PML call leave the walk, and everything launch_pml needs to act on it: decided once, by plan_pml.
enum class PmlRouteKind {
    kVector,              // the u16 vector straight from the walk (register packer or LDS ring; fused bins ride here)
    kMaskNative,          // reset masks straight from the walk (pml_kernel_flatp<..., RING = 2>)
    kMaskFromTmp,         // the walk cannot write masks: its vector goes to `tmp` and launch_pml_to_mask packs it
    kVectorFused,         // the mask walk's wavefronts expand their own reads into the vector (DevIndex::expand_out)
    kVectorExpand,        // a native mask walk, launch_pml_expand behind it
};
struct PmlRoute {
    PmlPlan plan;
    PmlRouteKind kind = PmlRouteKind::kVector;
    bool valid = true;               // false: the call asks for what no kernel gives (masks with bins or logs, logs with bins)
    bool seg_first = false;          // the segment plan gets the first say; it writes a vector (masks: into `tmp`, packed behind it); if it declines: `kind`
    bool needs_tmp = false;          // masks as the result by way of a vector: the caller provides n_bases u16 of scratch
    int park_lanes = 0;              // the walk parks at this many lanes (0: no second launch) -- the queue fits ...
    uint64_t park_grid = 0;          // ... the blocks of the second launch
    uint32_t hint_w = 0;             // DevIndex::hint_w
    bool ff_skip = false;            // DevIndex::ff_skip
    int ahd = 0, psh = 0, ring = 0;  // the walk kernel's template selectors (WalkLaunch)
    bool through_masks() const { return kind != PmlRouteKind::kVector; }                                       // the walk (or the packer behind it) writes mask words
    bool lent_masks() const { return kind == PmlRouteKind::kVectorFused || kind == PmlRouteKind::kVectorExpand; }   // ... the caller's scratch
};

// Reads staged through LDS (pml_kernel_flatp<..., STG = 1>): the block's dynamic LDS holds the next stage_lds bases of each
// of its 64 reads.  A capped launch has that LDS anyway (`pad_lds`, the cap's padding: 21 KiB = 336 bases per lane at the default cap
// of 7 wavefronts per CU, 16 KiB = 256 at 9); an uncapped one (a batch of at most ~18 wavefronts per CU, one round) gets what
// its wavefronts per CU leave of the 160 KiB, so that the round stays one round.  Long reads roll through the same
// stretch (stage_from in the kernel).
// PMLs out through a ring in LDS (the kernel has the numbers): launches of long reads -- few wavefronts, each
// one's own instruction stream most of an iteration -- where the block's LDS holds the ring beside 96 staged bases.
// -> dyn_lds, stage_lds (bases per lane: a multiple of 16, 96 .. 1024; 0 = the launch does not stage) and use_ring of P
inline void stage_budget(PmlPlan &P, size_t pad_lds, bool uncapped, bool stage_ok, bool ring_wanted, uint64_t blocks, int num_cus) {
    P.dyn_lds = pad_lds;
    if (stage_ok && uncapped) {
        const uint64_t wn = (blocks + (uint64_t)num_cus - 1) / (uint64_t)num_cus;      // wavefronts per CU of this launch
        // (room for a quarter more: the dispatcher does not deal the blocks out evenly, and a CU that may hold no more than the
        // average leaves its surplus queued -- 150 k reads, 9.2 wavefronts per CU: 41.2 Gbases/s with room for 10, 45.8 for 12)
        const uint64_t room = wn + std::max<uint64_t>(2, wn / 4);
        if (wn <= 18) P.dyn_lds = std::min<size_t>(21504 + (ring_wanted ? kOutRingBytes : 0u), cap_lds((int)room, 0));
    }
    const size_t ring_b = (ring_wanted && P.dyn_lds >= kOutRingBytes + 96u * 64u) ? kOutRingBytes : 0;
    const uint32_t stage_cap = (uint32_t)std::min<size_t>(1024, ((P.dyn_lds - ring_b) / 64) & ~(size_t)15);
    P.stage_lds = (stage_ok && stage_cap >= 96) ? stage_cap : 0u;
    P.use_ring = ring_b != 0 && P.stage_lds != 0u;
}

// pair-shared gathers by themselves: tables beyond the reach of the per-CU TLBs ("pair_loads" 1 / 0 forces them on / off)
inline bool pair_wanted(const LaunchCfg &cfg, uint64_t walked_bytes) {
    return cfg.pair_loads > 0 || (cfg.pair_loads < 0 && walked_bytes >= kPairLoadBytes);
}

// Fast-forward skip (DevIndex::ff_skip), decided by the layout a launch walks on: the rule needs entries, so never on the plain rows.
inline bool ff_skip_on(const LaunchCfg &cfg, bool use_deep, bool use_ahead) {
    if (!use_deep && !use_ahead) return false;
    return cfg.ff_skip > 0 || (cfg.ff_skip < 0 && (use_deep ? kFfSkipDeep : kFfSkipAhead) != 0);
}

// The walk of a call (a.cm, a.logging, a.have_seg_ws, a.ordered) that writes reset masks (want_mask) or the vector: plan_pml's core.
inline PmlPlan plan_pml_walk(const TableFacts &ix, const LaunchCfg &cfg, uint64_t n_reads, uint64_t n_bases, const PmlAsk &a, bool want_mask) {
    const int cm = a.cm;
    const bool logging = a.logging, have_seg_ws = a.have_seg_ws, ordered = a.ordered;
    PmlPlan P;
    // Variants: 0 first correct kernel (serves --logs), 1 base-synchronous packed I/O (tables of fewer than 8 rows, batches of
    // fewer than 16 bases; A/B), 14 = the lane state machine over row windows (pml_kernel_flatp, movi_walk.hpp; the default).
    // (2-13 were experiments -- branchy / row-at-a-time state machines, 2/4-row neighbour windows, the unpipelined window
    // kernel, hop-by-hop advances, lane refill -- measured slower or no faster and removed; numbers in DESIGN.md section 3.)
    // Auto selection (measured on MI355X, profiles/r02_*): the state machine in blocks of ONE wavefront, and -- when there are
    // more reads than ~18 waves per CU -- at most kCapWaves wavefronts resident per CU.  Why a cap: between two
    // iterations of a lane its cache lines (the row window's neighbours, its read, its output) must survive in the
    // 4 MiB L2 of its XCD; with all 32 wave slots of a CU walking, 8 MiB of lines are in flight per XCD and neighbour
    // rows are refetched from the fabric.  1 M x 150 bp, Gbases/s, uncapped / capped at 8-10 waves per CU /
    // variant 1 (base-synchronous: its neighbour loads follow the gather at once, so it wants all the occupancy it can
    // get): pangenome 14 M rows 43.2 / 48.2 / 46.4; random tables of 10 M rows 40.0 / 47.5 / 43.6, 60 M 35.7 / 40.8 /
    // 36.3, 250 M (2 GB) 29.1 / 32.8 / 29.2, 500 M 27.9 / 30.3 / 27.7, 1 B (8 GB) 27.4 / 27.7 / 28.3.
    int v = cfg.pml_variant;
    // (batches of up to ~18 waves per CU run in ONE round, uncapped: with the cap, 224 k reads = 13.7 waves per CU run as
    // a full round of 9 and a half-empty one -- 38.3 against 39.2 Gbases/s; 300 k reads: 38.2 against 41.2; from 400 k
    // reads on the cap wins: 43.9 against 41.7.  profiles/r02_occupancy_cap_sweeps.txt)
    const bool big_batch = n_reads > (uint64_t)cfg.num_cus * 64u * 18u;
    if (v < 0) v = 14;
    if (v == 14 && (ix.r < 8 || n_bases < 16)) v = 1;                        // the clamped window needs >= 4 rows (r >= 8: two windows), the
                                                                             // 16-base fetches >= 16 bytes of bases
    if (cm != 0 && v == 0) v = 1;                                            // the first kernel carries no fused bins
    if (logging) v = 0;                                                      // per-base logs: the first kernel keeps them
    P.v = v;
    // Batches of long reads: segment-parallel (plain PML through the default kernel only).  One lane per read leaves the
    // GPU short of walks -- 100 k reads are 6 wavefronts per CU, and a single 1 Mbp read holds its lane for 2 s --;
    // cut into segments the same batch fills it like a batch of short reads.
    P.seg_eligible = have_seg_ws && !logging && cfg.seg_len >= 32 && !ordered && v == 14 && cfg.block_threads <= 64 &&
                     n_bases / n_reads >= 2ull * (uint64_t)cfg.seg_len && n_reads + n_bases / (uint64_t)cfg.seg_len < 0x7FFFFFF0ull;
    const int bt = cfg.block_threads > 0 ? cfg.block_threads : 64;           // one wavefront per block: finest dispatch grain
    P.bt = bt;
    const uint64_t blocks = (n_reads + bt - 1) / bt;
    int wpc = cfg.waves_per_cu;
    if (wpc < 0) wpc = 0;
    const bool stage_ok = cfg.stage_reads != 0 && bt == 64 && v == 14;                  // the staged kernels: one-wavefront blocks of the default walk
    // ... on the deep rows where the handle holds them and the batch is one of short reads: three bases per gather pay where reads follow the
    // text (c2: fabric lines per base 0.584 -> 0.477, 80.3 -> 89.6 Gbases/s with reset masks out); 10 kbp reads with 8 % substitutions spend
    // their iterations on repositions, which three-row windows serve worse than four-row ones (59.3 -> 44.4): profiles/r06_deep_rows.txt
    const bool deep_ok = stage_ok && ix.rows3 && ix.idx32 && (cfg.deep > 0 || (cfg.deep < 0 && n_bases / n_reads < kDeepReadLen));
    // ... on the chain rows where the handle holds them: the same batches of short reads, plain queries (no bins) through the register packer
    // or as reset masks (the kernel has no LDS ring); "deep" 0 keeps a launch off both copies
    const bool chain_ok = stage_ok && ix.rows4 && ix.idx32 && cm == 0 && cfg.deep != 0 && n_bases / n_reads < kDeepReadLen;
    const bool ahead_ok = stage_ok && (ix.rows2 || deep_ok || chain_ok);                // ... or on the look-ahead rows
    if (cfg.waves_per_cu == 0 && v == 14 && big_batch)
        wpc = chain_ok ? kCapWavesChain : (deep_ok ? kCapWavesDeep : (ahead_ok ? kCapWavesAhead : kCapWaves));     // the auto policy above
    P.wpc = wpc;
    // cfg.stage_reads: 1 = whenever it fits (default), 0 = never.
    // cfg.out_ring: -1 = batches of long reads, 0 / 1 = never / wherever it fits (A/B).  (Reset masks out: no PML leaves, no ring.)
    const bool ring_wanted = stage_ok && !want_mask && (cfg.out_ring > 0 || (cfg.out_ring < 0 && n_bases / n_reads >= kOutRingReadLen));
    // (`uncapped`: no cap was asked for or picked -- a cap of 32 wavefronts and more pads nothing and leaves the launch unstaged)
    stage_budget(P, wpc > 0 ? cap_lds(wpc / (bt / 64), 1) : 0, wpc == 0, stage_ok, ring_wanted, blocks, cfg.num_cus);
    P.use_chain = chain_ok && P.stage_lds != 0u && !P.use_ring;
    P.use_deep = deep_ok && P.stage_lds != 0u && !P.use_chain;
    P.use_ahead = (ix.rows2 || P.use_deep || P.use_chain) && stage_ok && P.stage_lds != 0u;
    // pair-shared gathers (pml_kernel_flatp<..., PSH = 1>): the staged default walk on the plain or the look-ahead rows
    // Where: on tables beyond the reach of the per-CU TLBs (~2 GB), where a lane's two (four) 16-byte loads are as many
    // translation requests and the L2 TLB's request rate bounds the walk -- real BWT of 226 M rows on the look-ahead rows (3.6 GB
    // copy) 39.4 -> 50.8 Gbases/s, the random 1 B-row table 32.6 -> 34.7 on its plain rows and 21.4 -> 44.2 on the look-ahead
    // copy (16 GB); below that the exchange costs about what the merged accesses give (random 25 / 50 / 100 M rows +4 / +5 / -2 %,
    // real 113 M rows +1.5 %, c2 -2.5 %, c3 -9 %: profiles/r04_pair_shared_gathers.txt).  "pair_loads" 1 / 0 forces it.
    P.use_pair = pair_wanted(cfg, ix.r * (P.use_ahead ? 16ull : 8ull)) && P.stage_lds != 0u && v == 14 && !P.use_deep && !P.use_chain;
    // Parked lanes (DevIndex::park_at): only where the walk writes reset masks itself -- the staged default walk, whole reads, no bins.
    // By itself ("park_lanes" -1) only for batches of kParkMinRounds rounds of wavefronts and more (a capped launch: `rounds` of wpc
    // wavefronts per CU) and of short reads: long reads roll through their staged stretch and a resumed lane would stage again mid-read
    // for every one of them.  "park_lanes" N forces it wherever the walk can park.
    if (want_mask && cm == 0 && !logging && v == 14 && P.stage_lds != 0u && n_reads <= 0xFFFFFFFFull) {   // (a record holds the read in 32 bits)
        const uint64_t per_round = (uint64_t)cfg.num_cus * (uint64_t)(wpc > 0 ? wpc : 32);
        const bool auto_on = blocks >= kParkMinRounds * per_round && n_bases / n_reads < kOutRingReadLen;
        P.park_lanes = cfg.park_lanes > 0 ? std::min(cfg.park_lanes, 63) : ((cfg.park_lanes < 0 && auto_on) ? kParkLanesAuto : 0);
    }
    return P;
}

// The plan of one PML call: the walk (plan_pml_walk) and the route its results take.
// The walk writes reset masks itself where it is the staged default walk (one-wavefront blocks of variant 14) of a plain query -- no bins,
// no logs.  Masks as the result come from there, or by way of a vector in `tmp` (the segment plan, the base-synchronous kernels, unstaged
// launches).  A caller who wants the VECTOR and lends mask words gets it through masks only where the walk writes them itself and the
// segment plan has no say -- the walk writes one bit per base (a ninth fewer vector instructions per iteration than the u16 packer, a
// third of the write traffic): c2 on the deep rows 78.4 -> 86.7 Gbases/s, the random 10 M-row table 62.4 -> 64.8, the 1 B-row table
// 42.3 -> 46.0 (profiles/r06_mask_path.txt) -- and, by the default policy (via_mask -1), the batch is one of short reads: long reads
// keep the ring in LDS, which is as good there (c3 16.76 against 16.66 ms).  Everywhere else such a call is planned again as the plain
// vector (the LDS ring is wanted again) and the lent words stay unused.
inline PmlRoute plan_pml(const TableFacts &ix, const LaunchCfg &cfg, uint64_t n_reads, uint64_t n_bases, const PmlAsk &a) {
    PmlRoute R;
    if (n_reads == 0) { R.valid = false; return R; }   // (an empty call has no route; the mean read length below divides by n_reads)
    const bool plain_query = a.cm == 0 && !a.logging;
    R.valid = !(a.want == PmlWant::kMasks && !plain_query) && !(a.logging && a.cm != 0);
    const bool lends = a.want == PmlWant::kVectorLendsMasks;
    PmlPlan &P = R.plan;
    P = plan_pml_walk(ix, cfg, n_reads, n_bases, a, a.want != PmlWant::kVector);
    auto writes_masks = [&] { return P.v == 14 && P.stage_lds != 0u; };
    bool masks = a.want == PmlWant::kMasks;
    if (lends) {
        masks = plain_query && !P.seg_eligible && writes_masks() && (a.via_mask > 0 || n_bases / n_reads < kOutRingReadLen);
        if (!masks) P = plan_pml_walk(ix, cfg, n_reads, n_bases, a, false);
    }
    const bool native = masks && writes_masks();
    // the vector from the mask walk itself: one-wavefront blocks whose 64 reads are one contiguous, 16-byte aligned stretch of it
    const bool fused = native && lends && P.bt == 64 && !a.ordered && a.out_aligned && cfg.fused_expand != 0;
    R.kind = !masks ? PmlRouteKind::kVector : !native ? PmlRouteKind::kMaskFromTmp : !lends ? PmlRouteKind::kMaskNative
             : fused ? PmlRouteKind::kVectorFused : PmlRouteKind::kVectorExpand;
    R.seg_first = P.seg_eligible;
    R.needs_tmp = masks && (P.seg_eligible || !native);
    // Parked lanes (DevIndex::park_at; the walk's park_lanes): where the walk writes the masks itself -- for the vector only on the fused
    // route, whose resumed lanes expand their own reads -- and the caller lent a queue with room for every lane of the second launch's
    // grid, whatever the counter says: park_lanes per wavefront, whole blocks (no read-back needed); slots are 32-bit.
    const uint64_t bt = (uint64_t)P.bt, waves = (n_reads + bt - 1) / bt * (bt / 64);
    const int park = (native && (!lends || fused) && a.park_queue) ? P.park_lanes : 0;
    const uint64_t park_grid_lanes = (waves * (uint64_t)(park > 0 ? park : 0) + bt - 1) / bt * bt;
    if (park > 0 && park_grid_lanes <= a.park_cap && park_grid_lanes <= 0x7FFFFFFFull) {
        R.park_lanes = park;
        R.park_grid = park_grid_lanes / bt;
    }
    R.hint_w = P.use_chain ? (cfg.hints != 0 ? kChainHintW : 0u) : P.use_deep ? (cfg.hints != 0 ? 2u : 0u) : ((cfg.hints != 0 && ix.hints && ix.rows2) ? 3u : 0u);
    R.ff_skip = P.v == 14 && ff_skip_on(cfg, P.use_deep || P.use_chain, P.use_ahead);
    R.ahd = P.use_chain ? 3 : (P.use_deep ? 2 : (P.use_ahead ? 1 : 0));
    R.psh = P.use_pair ? 1 : 0;
    R.ring = native ? 2 : (P.use_ring ? 1 : 0);
    return R;
}

// The segment length of one call: cfg.seg_len, or shorter (down to 512) when the batch is so small that even then the
// segments would not fill the GPU: `waves` wavefronts of segments per CU are aimed at.  The ZML parse is latency-bound
// and wants many (24: 25 k x 10 kbp 13.4 -> 17.2 Gbases/s, 5 k 1.0 uncut -> 6.9, 1 %-error reads 7.7 uncut -> 15.1); the
// PML walk pays more per boundary than it gains from lanes beyond ~8 per CU (with 24: 5 k x 10 kbp 7.5 -> 18.2, but
// 200 x 1 Mbp 27.5 -> 20.5 and 1 %-error reads 25.3 -> 20.4).  A full batch (100 k x 10 kbp) keeps cfg.seg_len.
constexpr uint64_t kSegWavesPml = 8, kSegWavesZml = 24;
inline uint32_t call_seg_len(const LaunchCfg &cfg, uint64_t n_bases, uint64_t waves) {
    const uint64_t want = (n_bases / ((uint64_t)cfg.num_cus * 64ull * waves)) & ~31ull;
    const uint64_t lo = cfg.seg_len < 512 ? (uint64_t)cfg.seg_len : 512ull;
    return (uint32_t)(want < lo ? lo : (want > (uint64_t)cfg.seg_len ? (uint64_t)cfg.seg_len : want));
}
// a batch of this many wavefronts of reads per CU and more fills the GPU as it is and is cut only if it is ragged (launch_pml_segmented, launch_zml_segmented)
constexpr uint64_t kSegRaggedWavesPml = 4, kSegRaggedWavesZml = 8;

// One launch of the PML segment plan's walk kernel in blocks of one wavefront: K1 over `lanes` = max_seg, K3 over `lanes` = n_reads.
// Segments and re-walked reads stage their bases through LDS, walk on the look-ahead rows and are capped like any other launch
// (v, bt, wpc and seg_eligible of the plan are not this function's to say: the default walk, 64, reported as 0).
inline PmlPlan plan_pml_seg(const TableFacts &ix, const LaunchCfg &cfg, uint64_t lanes, bool big_batch_cap) {
    PmlPlan P;
    const bool stage_ok = cfg.stage_reads != 0;
    const bool deep_ok = ix.rows3 && ix.idx32 && cfg.deep > 0 && stage_ok;   // the deep rows only on request ("deep" 1): segments are long reads
    int wpc = cfg.waves_per_cu;
    if (wpc < 0) wpc = 0;
    // (which caps: kCapWavesAhead also on the deep rows -- kCapWavesDeep was tuned on short reads and is never picked here)
    if (cfg.waves_per_cu == 0 && big_batch_cap && lanes > (uint64_t)cfg.num_cus * 64u * 18u)
        wpc = ((ix.rows2 || deep_ok) && stage_ok) ? kCapWavesAhead : kCapWaves;
    const size_t pad = cap_lds(wpc, 0);
    // (`uncapped`: nothing was padded -- unlike plan_pml, a cap of 32 wavefronts and more leaves the launch staged)
    // (ring rule: segments are long reads, so "out_ring" -1 means the ring wherever the block has room for it -- no look at the lengths)
    stage_budget(P, pad, pad == 0, stage_ok, cfg.out_ring != 0 && stage_ok, (lanes + 63) / 64, cfg.num_cus);
    P.use_deep = deep_ok && P.stage_lds != 0u;
    P.use_ahead = (ix.rows2 || deep_ok) && P.stage_lds != 0u;
    // (pair-shared gathers on tables beyond the TLBs' reach: plan_pml's rule, by the rows the handle holds rather than the rows walked)
    P.use_pair = P.stage_lds != 0u && !deep_ok && pair_wanted(cfg, ix.r * (ix.rows2 ? 16ull : 8ull));
    return P;
}

// ----------------------------------------------------------------------------------------------------------- ZML / count
// Batches of long reads: the segment plan gets the first say (every A/B option off, resident layouts 6 and 3)
inline bool zml_seg_eligible(const LaunchCfg &cfg, int mode, uint64_t n_reads, uint64_t n_bases, bool have_seg_ws, bool ordered) {
    return have_seg_ws && cfg.seg_len >= 32 && !ordered && cfg.zml_variant < 0 && cfg.block_threads == 0 && cfg.waves_per_cu <= 0 &&
           n_bases / n_reads >= 2ull * (uint64_t)cfg.seg_len && n_reads + n_bases / (uint64_t)cfg.seg_len < 0x7FFFFFF0ull &&
           (mode == 6 || mode == 3);
}
// K1 of the segmented ZML plan: the lane state machine where the plain query would use it (tables up to 3 GB; the clamped windows
// need >= 4 rows, the 16-base fetches 16 bytes), else the base-synchronous kernel
inline bool zml_seg_k1_flat(uint64_t r, uint64_t n_bases) { return r <= (3ull << 30) / 8 && r >= 8 && n_bases >= 16; }

// reads staged through LDS (round 6; the state machine in blocks of one wavefront): the cap's padding, or kZmlStageBytes of their own
inline uint32_t zml_stage(size_t &dyn_lds) {
    if (dyn_lds < kZmlStageBytes) dyn_lds = kZmlStageBytes;
    return (uint32_t)std::min<size_t>(1024, (dyn_lds / 64) & ~(size_t)15);
}

struct ZmlPlan {
    int v = 0;                       // ZML: 0 = base-synchronous kernel, 1 = lane state machine; count: 0 = count_kernel_v0, 1 = the state machine
    int bt = 64, wpc = 0;
    bool valid = true;               // false: the options ask for a kernel that cannot run here
    bool pair = false, ahead = false;
    size_t dyn_lds = 0;
    uint32_t stage_lds = 0;
};
inline ZmlPlan plan_zml(const TableFacts &ix, const LaunchCfg &cfg, int mode, uint64_t n_bases) {
    // 0 = base-synchronous kernel, 1 = lane state machine.  Measured (profiles/r02_zml_state_machine.txt), Gbases/s,
    // kernel 0 / 1: 100 k x 10 kbp 12.1 / 19.1 (pangenome), 12.2 / 18.2 (random 10 M rows); 1 M x 150 bp 36.8 / 39.2 and
    // 34.1 / 36.8; random tables of 120 M rows 24.6 / 28.3, 250 M (2 GB) 23.4 / 26.6, 500 M (4 GB) 21.3 / 16.6, 1 B (8 GB)
    // 17.0 / 13.8.  The state machine fetches two 4-row windows (four 16-byte loads, i.e. ~8 TLB lookups) per iteration:
    // beyond the ~1.7 GB reach of a CU's TLB that costs more than the base-synchronous kernel's dependent trips, so auto
    // picks it for tables up to 3 GB.  (Its first form walked the windows with eight sequential hops and was no faster
    // than kernel 0 anywhere: 12.4 on the long reads, 32.6 on the short ones; the closed-form window walk made it.)
    // Round 4: with the two windows fetched by PAIRS of lanes (zml_kernel_flat<..., PSH = 1>: half the translation requests) the
    // state machine serves the tables beyond 3 GB too: 1 B rows 16.8 (kernel 0) / 13.9 (kernel 1) -> 25.0 Gbases/s; below 2 GB the
    // exchange costs more than it gives (c2: 38.2 -> 36.6), so there the lanes keep their own loads (profiles/r04_zml_ahead.txt;
    // "pair_loads" 0: the old policy, 1: pairs everywhere).
    // (`ahead` and `pair` are settled BEFORE the kernel is picked: a caller who asks for the look-ahead rows forgoes the pairs, and
    // beyond 3 GB the unpaired state machine is the slowest of the three -- 13.9 against kernel 0's 16.8 Gbases/s at 1 B rows)
    ZmlPlan P;
    int v = cfg.zml_variant;
    const bool want_ahead = cfg.zml_ahead != 0 && mode == 6 && ix.rows2;
    const bool can_pair = !want_ahead && pair_wanted(cfg, ix.r * 8ull);
    if (v < 0) v = (ix.r <= (3ull << 30) / 8 || can_pair) ? 1 : 0;
    if (v == 1 && (ix.r < 8 || n_bases < 16)) v = 0;     // the clamped windows need >= 4 rows, the 16-base fetches 16 bytes
    P.v = v;
    P.bt = cfg.block_threads > 0 ? cfg.block_threads : (v == 1 ? 64 : 256);
    P.wpc = cfg.waves_per_cu > 0 ? cfg.waves_per_cu : 0;
    P.valid = mode == 6 || mode == 3;
    // The state machine on the look-ahead rows (round 4; "zml_ahead" 1, where the copy exists): a base both of whose LF moves
    // land without a fast-forward is complete without the target rows.  Lane iterations per base on c2 1.45 -> 0.98 -- and 37.3
    // instead of 38.2 Gbases/s (eight 16-byte loads per iteration instead of four, SIMT 0.72 -> 0.64; random 10 M-row table 35.9 ->
    // 35.0: profiles/r04_zml_ahead.txt), so it is an option, not the default.
    P.ahead = want_ahead && v == 1;
    P.pair = v == 1 && can_pair;
    if (P.wpc > 0) P.dyn_lds = cap_lds(P.wpc / (P.bt / 64), 3);   // occupancy cap by LDS padding, as in plan_pml (<= 64 KiB here)
    if (v == 1 && P.bt == 64 && cfg.stage_reads != 0) P.stage_lds = zml_stage(P.dyn_lds);
    return P;
}

inline ZmlPlan plan_count(const TableFacts &ix, const LaunchCfg &cfg, int mode, uint64_t n_reads, uint64_t n_bases) {
    // Blocks of one wavefront; on a cache-resident table (up to the 256 MiB of the Infinity Cache) and a batch of more than
    // ~24 wavefronts of reads per CU at most kCountCapWaves wavefronts resident per CU -- the same L2-retention effect as in
    // plan_pml: the search's neighbour rows (interval shrink, fast-forwards) must survive between a lane's steps.
    // profiles/r03_count_ftab.txt: pangenome 61.2 -> 67.5 Gbases/s (cap 15 - 16; 14: 66.2, 17: 64.2, 20: 62.5), random 80 MB
    // table 52.4 -> 54.6; HBM-resident tables lose with any cap (1.6 GB: 47.3 uncapped, 43.2 at 16) or are indifferent (8 GB).
    ZmlPlan P;
    P.bt = cfg.block_threads > 0 ? cfg.block_threads : 64;
    P.wpc = cfg.waves_per_cu > 0 ? cfg.waves_per_cu : 0;
    // Round 5 -- the search as a LANE STATE MACHINE over row windows (zml_kernel_flat<..., CNT = 1>; by pairs of lanes on plain rows of
    // 2 GB and more) wherever it can run: tables of 8 rows and more, batches of 16 bases and more, one-wavefront blocks.  Gbases/s of
    // read bases, count_kernel_v0 -> the state machine (profiles/r05_c5_count_pmc.txt): the 1 B-row blocked-thresholds table of BASELINE
    // config 5 37.2 -> 56.4 - 56.9 (without the pairs 32.3), random 200 M rows 46.6 -> 68.0, the c2 pangenome 71.4 (on its look-ahead
    // rows) -> 84.0 (on the plain rows).  cfg.count_variant: -1 = this policy, 0 = count_kernel_v0 (A/B; tiny tables and batches), 1 = the
    // state machine or nothing.
    const bool flat_ok = (mode == 6 || mode == 3) && ix.r >= 8 && n_bases >= 16 && P.bt == 64;
    if (flat_ok && cfg.count_variant != 0) {
        P.v = 1;
        P.pair = pair_wanted(cfg, ix.r * 8ull);
        // ("zml_ahead" 1, round 6: the search on the look-ahead rows where the handle holds them -- a base both of whose LF moves land without a
        // fast-forward is complete without the target rows; measured: profiles/r06_zml_count.txt)
        P.ahead = cfg.zml_ahead != 0 && mode == 6 && ix.rows2 && !P.pair;
        if (P.wpc > 0) P.dyn_lds = cap_lds(P.wpc, 3);     // "waves_per_cu": occupancy cap by LDS padding (<= 64 KiB here), as plan_zml
        if (cfg.stage_reads != 0) P.stage_lds = zml_stage(P.dyn_lds);
        return P;
    }
    P.v = 0;
    P.valid = cfg.count_variant <= 0 && (mode == 6 || mode == 3);
    P.ahead = mode == 6 && ix.rows2 && ix.rows2_count;   // the search walks on the look-ahead rows where they pay
    if (cfg.waves_per_cu == 0 && ix.r * (P.ahead ? 16ull : 8ull) <= (256ull << 20) &&   // (the bytes of the table the search walks on)
        n_reads > (uint64_t)cfg.num_cus * 64ull * 24ull) P.wpc = kCountCapWaves;
    if (P.wpc > 0) P.dyn_lds = cap_lds(P.wpc / (P.bt / 64), 1, 65536 - 1024);
    return P;
}

}  // namespace movi
