// movi_kernels.hpp -- device-side index view shared by the kernels and the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "movi_launch_policy.hpp"   // LaunchCfg, the kCap* / k*ReadLen / k*Bytes constants, the launch plans
#include "movi_deep_fields.hpp"     // the deep rows' two field maps (plain C++: host tests compile it too)
#include "movi_chain_fields.hpp"    // the chain rows' field map, likewise
#include "movi_buffers.hpp"         // the owning types (host side only); their two memory policies are below

namespace movi {

constexpr int kPrefixShift = 5;   // one BWT-position checkpoint every 32 rows (count path)

// What every kernel needs of the index, passed by value as a kernel argument
// (lives in the kernarg segment: scalar loads, no per-lane traffic).
struct DevIndex {
    const uint8_t *rows;          // r * row_bytes, packed exactly as in index.movi (mode 7: widened to 4 B per row)
    const uint32_t *id_blocks;    // mode 8: [alphabet][n_blocks]
    const uint8_t *code_of;       // 256 bytes: ASCII -> code 0..3 (1..4 with separators), 0xFF = illegal
    const uint64_t *row_start_ckpt; // BWT position of row 32*j (count path), r/32+1 entries
    uint64_t r;
    uint64_t end_bwt_idx;
    uint64_t n_blocks;
    uint64_t block_size;
    uint32_t block_shift;         // log2(block_size) when it is a power of two (always, in practice), else 0xFFFFFFFF
    uint32_t sigma;               // alphabet size: 4 (ACGT; fewer for reduced test alphabets) or 5 ('%' + ACGT)
    uint64_t end_thr[4];          // end_bwt_idx_thresholds, by DNA character
    uint64_t first_runs[6], first_offsets[6], last_runs[6], last_offsets[6];
    // `movi build --separators` indexes (MoveStructure::use_separator, src/move_structure.cpp:547-552): code 0 is
    // the separator '%', DNA codes are 1..4, and the rows OF the separator keep explicit thresholds in a side
    // table (separators_thresholds[separators_thresholds_map[idx]], src/move_structure_query.cpp:540-541) --
    // here sorted by row: sep_rows[k] <-> sep_vals[k] = 4 x u16 packed as (v0 | v1 << 16, v2 | v3 << 16)
    uint32_t sep;                 // 0 / 1
    uint32_t n_sep;
    const uint64_t *sep_rows;
    const uint2 *sep_vals;
    // sampled-thresholds (mode 7): tally_ids[character][checkpoint], widened from the file's 40-bit entries
    const uint64_t *tally;
    uint64_t tally_len;
    uint64_t tally_cp;            // rows between checkpoints (movi build --checkpoint, default 20)
    // 1: row indexes fit 32 bits (r < 2^32 - 1) -> the kernels' uint32_t instantiations; the "idx64" option clears it so
    // that tests can run the 64-bit instantiations (tables beyond 4 G rows) on small indexes
    uint32_t idx32;
    // Top-of-walk table ("kmer_k" option; 0 = none): every walk starts in the same state (row r-1), so its state after
    // the last K bases of the read depends on those K bases alone.  kmer[code of the K-mer] = that state (after the LF
    // towards base K, before its fast-forward), which of the K bases matched (their PMLs follow from that) and the
    // fast-forwards / scan rows the K steps took: one 16-byte lookup instead of K dependent row gathers.  The reference's
    // analogue is the ftab of its k-mer queries (src/move_structure_search.cpp:66-167, 203-259), there for intervals.
    // The same idea for the count query (the reference's own ftab, src/move_structure_search.cpp:66-167, 203-259): the
    // backward-search interval after the last K bases of a read is a function of those K bases.  ftab[code of the K-mer]:
    // x = run_start[31:0]; y = run_end[31:0]; z = run_start[35:32] | run_end[35:32] << 4 | offset_start << 8 | offset_end << 20
    // (12 bits each); w = fast-forwards (15 bits) | scan rows << 15 (16 bits) | valid << 31.  valid = 0: the interval of this K-mer
    // is empty before K bases are consumed (or a step throws): such reads take the ordinary search from their last base.
    uint32_t ftab_k;
    // set per launch, PML walk on the look-ahead or deep rows ("ff_skip"): 1 = FAST-FORWARD SKIP -- an LF whose entry says that the offset
    // arrives at or beyond n(j) (the chain breaks by a fast-forward, whatever the next base is) gathers the window of j + 1 with that
    // fast-forward already taken, instead of j's: where j is its window's last row the old iteration learnt only "next window".
    // 0 = every LF gathers its target's window.  Same vectors, error bytes and counters either way; fewer lane and wavefront steps.
    uint32_t ff_skip;
    const uint4 *ftab;
    uint32_t stage_lds;           // set per launch by launch_pml: bytes of dynamic LDS per lane for read staging (0 = none; 336 at cap 7)
    uint32_t mask_phase;          // set per launch, reset-mask output (pml_kernel_flatp<..., RING = 2>): the low 5 bits of the position of the batch's first base in the caller's whole read set (0 for a whole call)
    uint32_t inwin;               // set per launch: 1 = a reposition whose target is one of the window's rows is resolved in the same iteration
    uint32_t kmer_k;
    const uint4 *kmer;            // 4^K entries: x = row[31:0]; y = row[35:32] | off << 4 (12 bits) | match mask << 16 (K bits) |
                                  // valid << 31; z = fast-forwards; w = scan rows.  valid = 0: one of the K steps hit one of the
                                  // reference's throws -- such reads take the ordinary walk and report it
    // Look-ahead rows ("ahead_rows" option; nullptr = none): a second copy of the table in which every row carries, in the
    // SAME 128-byte line, what the row its LF points to looks like -- so that a step whose next base matches there without a
    // fast-forward (the common case on real reads) is taken without fetching that row: two bases per gather.  The count query's
    // two interval ends use the same entries (count_kernel_v0<6, 1>).
    // Layout: line L = rows 8L .. 8L+7 (64 bytes) followed by their 8 look-ahead entries (64 bytes); one more line at
    // byte rows2_tail holds rows r-4 .. r-1 and their entries (the walk's last, pulled-back window).  Entry of row i, with
    // j = id(i), j2 = id(j): x = j2[31:0]; y = n(j) (11 bits) | offset(j) << 11 (11 bits) | c(j) << 22 (3 bits) |
    // j2[35:32] << 25 | valid << 31.  valid = 0 when j or j2 is not a row (corrupt table): such steps are taken one by one.
    const uint8_t *rows2;
    uint64_t rows2_tail;
    // 1: the count query walks on them too.  It gains where walks that follow the text mostly arrive at their LF target
    // without a fast-forward (pangenome BWTs: 0.83 of the positions, +20 %) and loses where they do not (uniformly random
    // run sequences: 0.51, -12 %: the copy's lines hold half as many rows for the interval shrink) -- decided from that
    // ratio, which the builder tallies, when the copy is built by itself; a caller who asks for the copy gets it for both.
    uint32_t rows2_count;
    // Round 5 -- REPOSITION HINTS in the look-ahead copy of a table with fewer than 2^32 - 1 rows (hints = 1).  There the four
    // high id bits of a row (y[31:28]) and of its entry (y[28:25]) are zero and two entry bits (y[30:29]) were free: ten spare
    // bits per row.  Nine of them hold, for each of the row's three threshold slots k (= alphamap_3[c(row)][a], the same slot
    // that holds the threshold bit of read base a): how many rows BEYOND THE EDGE OF THE ROW'S WINDOW, in the direction the
    // threshold bit gives (0 = down, 1 = up: get_thresholds is n or 0 and offset < n, src/move_structure.cpp:295-309), the
    // nearest run of base a lies -- 1 .. 7, or 0 for "inside the window, further than 7 rows, nowhere, or this is the '$' row
    // (whose direction depends on the offset)".  A mismatch whose scan (reposition_up / _down, src/move_structure_query.cpp:188-232)
    // would leave the window then gathers the TARGET's window in its next iteration instead of walking there window by window.
    // hint of slot k = (h >> 3 k) & 7 with h = row.y >> 28 | (entry.y >> 25 & 0x3F) << 4.
    // In this form ids in rows2 are 32 bits wide: x alone (a row whose id is not a row reads x = 0xFFFFFFFF), and every
    // reader of rows2 masks the hint bits off (tab_row / tab_entry / the walk kernel).
    uint32_t hints;
    // set per launch: width of a hint field the walk looks at -- 3 = use the hints (on the deep rows: the width they were built with, deep_hint_bits), 0 = ignore them ("repo_hints" 0: A/B)
    uint32_t hint_w;
    // Round 6 -- DEEP ROWS ("deep_rows" option; nullptr = none; tables of fewer than 2^28 - 1 rows): a copy of the table in which every row
    // carries what the walk reads at its LF target j = id(i) AND at j2 = id(j) -- up to three bases per gather -- packed to 21.33 bytes
    // per row (round 4's chain rows held the same in 32 bytes per row and fell out of the Infinity Cache: profiles/r04_chain_rows.txt).
    // Window q = rows 3q .. 3q + 2 = 64 bytes at byte 64 q (two windows per 128-byte line, six rows per line); 16 dwords: row s at
    // dwords 5s .. 5s + 4, its ten extra bits at [10s + 9 : 10s] of dword 15.  What the five dwords and the ten bits hold is written
    // down, packed and unpacked in movi_deep_fields.hpp, in two FIELD MAPS that differ in three numbers only:
    //   wide ids   (28-bit ids, 0x0FFFFFFF = not a row; three 2-bit hints, reach 3):  every eligible table; the only map from 2^26 rows on
    //   narrow ids (26-bit ids, 0x03FFFFFF = not a row; three 4-bit hints, reach 15): tables of at most 2^26 - 1 rows ("deep_hint_bits" 4)
    // hints: one field per threshold slot k: rows beyond the edge of the row's three-row window at which the nearest run of the slot's
    // base lies in the direction the threshold bit gives, 1 .. reach; 0 = inside the window, further, nowhere, or the '$' row.  Scans
    // that run past reach 3 are 3.7 % of c2's lane iterations, on the reads that set their wavefronts' length (profiles/deep_hints.txt).
    // The rows of the last window beyond r - 1 are padding (c = 7, n = 0, never reached).
    const uint8_t *rows3;
    // the field map rows3 was built in (DeepMap; wave-uniform in the walk): mask of an id = the id that is no row, width of an id,
    // shift of j3 in dword 4, width of a hint as built (the launchers copy it to hint_w, or 0 with "repo_hints" 0)
    uint32_t deep_id_mask, deep_id_bits, deep_j3_shift, deep_hint_bits;
    // set per launch, reset-mask output (RING = 2) in blocks of one wavefront: non-null = every wavefront, when its 64 walks are over, turns
    // its reads' mask words into their u16 PML vectors here (through a tile in the LDS its reads were staged in: pml_kernel_flatp's tail)
    // -- the vector output at the mask walk's instruction count, the expansion hidden under the other wavefronts' gathers
    uint16_t *expand_out;
    // set per launch, reset-mask output (RING = 2) -- PARKED LANES: a wavefront's iteration count is its slowest lane's (c2: the mean read
    // takes 81 lane iterations, the mean wavefront 123), so a wavefront leaves its loop when at most `park_at` of its lanes still walk
    // (0 = off: when none does), parks their state -- one record each, slots reserved by one atomicAdd on *park_count -- and retires its
    // other reads.  A second launch of the same kernel behind the first on the same stream (`resume` = 1, park_at = 0) takes the records
    // 64 to a wavefront and finishes those reads.  Stream order is the only synchronisation; launch_pml sizes the queue and both grids.
    uint32_t park_at;
    uint32_t resume;
    uint4 *park_q;                // two uint4 per record: (read, k, row[31:0], row[63:32]), (offset, match length, partial mask word, fast-forward run | state << 30)
    unsigned long long *park_count;   // the queue's head: records written by the first launch (zeroed on the stream in front of it: park_reset_kernel)
};
constexpr size_t kParkRecBytes = 32, kParkHeadBytes = 32;   // the queue: a head that holds the counter, then the records

// Device counters of one query call.
struct DevStats {
    unsigned long long fast_forwards;
    unsigned long long scans;
    unsigned long long repositions;
    unsigned long long errors;
    // SIMT efficiency of the lane state machines: iterations in which a lane had work / 64 x wave iterations
    unsigned long long lane_steps;
    unsigned long long wave_steps;
    unsigned long long pad0_;
    unsigned long long segments;      // segment-parallel PML: segments walked, reads walked again
    unsigned long long rewalked;
    unsigned long long pad_;
};

constexpr uint32_t kTallySlots = 512;             // pairs of u64 counters a builder's tally is spread over (d_tally: 2 * kTallySlots u64, zeroed)

// What a launch_* call actually launched (movi_last_launch): the policy lives in the launchers, so they say what they picked.
struct LaunchInfo {
    char kernel[96] = {0};   // the dominant kernel's name as rocprofv3 prints it (template arguments included)
    int variant = -1;        // PML: 0, 1, 14; ZML: 0, 1; count: 0
    int block_threads = 0;
    int waves_per_cu = 0;    // resident-wavefront cap applied (0 = none)
    int segmented = 0;       // 1 = the segment-parallel plan ran (K1 + stitch + finalize around the named kernel)
    int idx64 = 0;           // 1 = the 64-bit row-index instantiation
    int ahead = 0;           // 1 = the walk ran on the look-ahead rows (two bases per gather where the next base matches), 2 = on the deep rows (three), 3 = on the chain rows (four)
    int staged = 0;          // > 0: every lane keeps the next `staged` bases of its read in LDS (pml_kernel_flatp<..., STG = 1>)
    int park_lanes = 0;      // > 0: the mask walk parked a wavefront's last `park_lanes` lanes and a second launch of the named kernel resumed them
    int ff_skip = 0;         // 1 = the PML walk ran with the fast-forward skip (DevIndex::ff_skip)
};

// Classifier::classify bins (src/classifier.cpp:99-143) fused into the PML kernels: per read the number of
// bins whose maximum is >= thr / < thr and the sum of the bin maxima.
struct ClsArgs {
    uint32_t bin_width = 0;                // 0 = no classification
    uint32_t thr = 0;
    uint32_t *above = nullptr;
    uint32_t *below = nullptr;
    uint64_t *sum_max = nullptr;
    // `movi query --logs` (src/read_processor.cpp:99-121,586-596, src/utils.cpp:268-289): per base, in emission order, the
    // fast-forwards of the LF that led to the NEXT base (entry k = LF into base k + 1; the last entry repeats the one before
    // it, as the reference's strand does when it writes the read out) and the rows the base's reposition scanned.
    // u16, truncated like MoveQuery's vectors.  Non-null: the first, base-synchronous kernel runs (pml_kernel<6, 0>).
    uint16_t *log_ff = nullptr;
    uint16_t *log_scan = nullptr;
};

// ---- segment-parallel long reads (PML) -------------------------------------------------------------------------
// A long read is cut into segments of about seg_len bases, every segment walked by its own lane from the state every
// read starts in (K1); then one lane per segment BOUNDARY continues the walk of the segment before across the
// boundary until it is in step -- same row, offset and match length at one of the checkpoints the speculative lane
// left every 32 bases -- with what that lane did (K2): from there on the two walks are the same walk.  A read all of
// whose boundaries fell into step is exact; any other is walked again from end to end (K3).  tests/studies/sync_study.py: on
// 10 kbp reads with 8 % / 1 % / 0.1 % substitutions a walk started mid-read is in step after a median of 11 / 80 / 607
// bases (maximum 107 / 665 / 4540).
struct SegCkpt { uint64_t idx; uint32_t off, ml, ff, scan, repo, pad_; };   // state after a base (before the LF to the next) + the segment's counters so far
struct SegFin { uint64_t idx; uint32_t off, ml; };                           // state after a segment's last base
struct SegTot { uint32_t ff, scan, repo, flag; };                            // a segment's counters; flag = kErr* of the speculative walk
struct SegArgs {
    const uint64_t *seg_in = nullptr;     // per segment: byte offset of its bases ...
    const uint64_t *seg_out = nullptr;    //   ... element offset of its first PML (emission order) ...
    const uint32_t *seg_len = nullptr;    //   ... and its length
    const uint64_t *n_seg = nullptr;      // device: number of segments
    SegCkpt *ckpt = nullptr;              // [(seg_out + k) >> 5] for every k of a segment with k % 32 == 31
    SegFin *fin = nullptr;
    SegTot *tot = nullptr;
    const uint8_t *read_fail = nullptr;   // K3: reads to walk again
    const uint32_t *go = nullptr;         // device: 1 = walk the segments; 0 = the probe advised against it: every read goes to K3
};

// The same for ZML (launch_zml_segmented): the state is the backward-search interval, its `open` flag and the match length.
struct ZSegCkpt { uint64_t rs, re; uint32_t os, oe, ml, open, ff, scan; };
struct ZSegFin { uint64_t rs, re; uint32_t os, oe, ml, open; };
struct ZSegArgs {
    const uint64_t *seg_in = nullptr;
    const uint64_t *seg_out = nullptr;
    const uint32_t *seg_len = nullptr;
    const uint64_t *n_seg = nullptr;
    ZSegCkpt *ckpt = nullptr;
    ZSegFin *fin = nullptr;
    SegTot *tot = nullptr;
    const uint8_t *read_fail = nullptr;
};

// What every launch of a query kernel over a batch carries.
struct BatchLaunch {
    dim3 grid, block;
    size_t dyn_lds = 0;
    hipStream_t stream = nullptr;
    DevIndex ix;
    const uint8_t *bases = nullptr;
    const uint64_t *offs = nullptr;
    uint64_t n = 0;                       // reads (SEG 0 / 2) or an upper bound of the segments (SEG 1: the kernel reads the count)
    uint16_t *out = nullptr;
    uint8_t *err = nullptr;
    DevStats *stats = nullptr;
    const uint32_t *order = nullptr;
};
// One launch of the walk kernel (pml_kernel_flatp, movi_walk.hpp): its arguments plus the run-time choices that pick the
// instantiation.  The launchers (launch_pml, launch_pml_segmented) fill it; the movi_walk*_u32 / _u64 translation units turn
// it into a launch and name the kernel (every template argument) in `info`.
struct WalkLaunch : BatchLaunch {
    ClsArgs cls;
    SegArgs seg;
    int cls_mode = 0;                     // 0 = PML vector, 1 = vector + classification bins, 2 = bins only
    int sep = 0, stg = 0, ahd = 0, psh = 0, ring = 0;   // separators index / reads staged through LDS / look-ahead rows / pair-shared gathers / PMLs out through the LDS ring (1) or as reset masks (2: `out` holds 32-bit words)
};
// One launch of a ZML / count kernel, likewise.  launch_zml, launch_zml_segmented and launch_count fill it; zml_dispatch (movi_kernels.hip)
// turns it into a launch and names the kernel in `info`.
struct ZmlLaunch : BatchLaunch {
    ZSegArgs seg_args;
    uint64_t *matched = nullptr, *count = nullptr;   // the count query's results (`out` is the ZML parse's)
    int mode = 6;                         // resident layout: 6 = regular-thresholds rows, 3 = regular rows (threshold-less types: 12-bit lengths)
    int flat = 0;                         // 1 = the lane state machine (zml_kernel_flat), 0 = base-synchronous (zml_kernel; cnt: count_kernel_v0)
    int idx32 = 0, seg = 0, ahead = 0, pair = 0, cnt = 0;   // 32-bit row indexes / 1 = segments (K1), 2 = re-walked reads (K3) / look-ahead rows / pair-shared gathers / the count query
};
// Diagnostic: when switched on (movi_launch_log), every launch of the walk kernel notes its name -- the K1 / K3 launches of the
// segment plan included, which LaunchInfo (the dominant kernel only) does not show.
void note_walk_launch(const char *kernel_name);
size_t take_launch_log(char *buf, size_t cap);   // switches the log on; returns the bytes the names (one per line) take; clears it
hipError_t launch_walk_u32(const WalkLaunch &L, LaunchInfo *info);
hipError_t launch_walk_u64(const WalkLaunch &L, LaunchInfo *info);
hipError_t launch_walkseg_u32(int seg, const WalkLaunch &L, LaunchInfo *info);   // seg: 1 = segments (K1), 2 = re-walked reads (K3)
hipError_t launch_walkseg_u64(int seg, const WalkLaunch &L, LaunchInfo *info);
hipError_t preload_walk_u32();            // load the translation unit's code object now (movi_index_prepare)
hipError_t preload_walk_u64();
hipError_t preload_walkseg_u32();
hipError_t preload_walkseg_u64();

// The library's memory policies (movi_buffers.hpp) and the owning types on them.  Errors of a free are dropped: it runs in destructors
// and on cleanup paths, whose caller is about to read an earlier message.
struct DeviceMem {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void *p) { (void)hipHostFree(p); }
};
using DevBuf = GrowBuf<DeviceMem>;
using PinnedBuf = GrowBuf<PinnedMem>;
using GraphDevBuf = GraphSafeBuf<DeviceMem>;
template <class T> using DevPtr = OwnedPtr<T, DeviceMem>;
template <class T> hipError_t dev_alloc(DevPtr<T> &p, size_t bytes) { return alloc_owned(p, bytes); }

// Device workspace of the segmented path, owned by whoever owns the stream (the handle; a pipeline slot): grow-only.
using SegWorkspace = DevBuf;

// Reset masks instead of the PML vector (round 6; movi_pml_mask_device): PML[k] = reset(k) ? 0 : PML[k - 1] + 1, so one bit per base
// says everything the u16 vector does.  words: bit k % 32 of word ((offsets[i] + phase) >> 5) + i + k / 32 = 1 iff step k of read i
// reset match_len (its PML is 0); phase = the low five bits of the batch's first base's position in the caller's whole read set
// (sub-batches of one call then concatenate word for word).  The default walk writes them natively (pml_kernel_flatp<..., RING = 2>);
// every other path (segment-parallel long reads, the base-synchronous kernels) writes its vector to tmp_pml (n_bases u16, which the
// caller provides whenever the call's route says needs_tmp) and pml_to_mask_kernel packs it.
// The mask buffers of one PML call.  Which of them the call uses is the route's to say (PmlRoute, movi_launch_policy.hpp): `words` are the
// result (kMaskNative, kMaskFromTmp) or scratch the caller lent for the vector (kVectorFused: the mask walk expands its wavefronts' reads
// itself; kVectorExpand: the pml_expand_* kernels do it behind the walk) and stay unused on the plain vector route.
struct MaskArgs {
    uint32_t *words = nullptr;
    uint32_t phase = 0;
    uint16_t *tmp_pml = nullptr;
    // parked lanes (DevIndex::park_at): device scratch of kParkHeadBytes + park_cap records of kParkRecBytes; null = the walk parks nothing
    void *park_q = nullptr;
    uint64_t park_cap = 0;
};
uint64_t pml_mask_words(uint64_t n_reads, uint64_t n_bases, uint32_t phase);          // words a batch's masks take (gap words included)
TableFacts facts(const DevIndex &ix, bool chain_rows = false);   // what the launch policy reads of the index (chain_rows: the handle holds them)
// u16 vector <-> masks, streaming (one lane per read; a wavefront per read from a mean length of 2048 bases)
hipError_t launch_pml_expand(const uint32_t *d_words, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint32_t phase,
                             uint16_t *d_out, hipStream_t stream);
// n 8-byte words from page-locked host memory (or anywhere the device can read) to the device by a kernel on `stream`: small blocks that
// must not queue behind bulk transfers on the copy engine (run_pipelined's per-chunk offsets)
hipError_t launch_copy_words(uint64_t *d_dst, const uint64_t *src, uint64_t n, hipStream_t stream);
// Reads packed two bits per base (include/movi_hip.h) -> one byte per base (movi_walk_pack.hip): d_out[j] = base first_base + j, whose code is
// bits 2 * ((first_base + j) & 3) of d_packed[(first_base + j) >> 2]; exception i then puts d_exc_byte[i] at d_out[d_exc_pos[i] - exc_origin]
// (positions outside [exc_origin, exc_origin + n_bases) are left alone).  Two kernels on `stream`, nothing else: allocates nothing, capturable.
hipError_t launch_unpack_reads(const uint8_t *d_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *d_exc_pos,
                               const uint8_t *d_exc_byte, uint64_t n_exc, uint64_t exc_origin, uint8_t *d_out, hipStream_t stream);
hipError_t launch_stats_reset(DevStats *d_stats, hipStream_t stream);   // a call's counters zeroed by a kernel (calls under a stream capture: movi_kernels.hip says why)
hipError_t preload_pack();                // load the translation unit's code object now (movi_index_prepare)
hipError_t launch_pml_to_mask(const uint16_t *d_pml, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint32_t phase,
                              uint32_t *d_words, hipStream_t stream);

// One PML call as launch_pml takes it, beside the plan (plan_pml) that says what to do with it.
struct PmlCall {
    int mode = 6;                         // the resident row layout (the query kernels exist for 6 only)
    const DevIndex *ix = nullptr;
    const LaunchCfg *cfg = nullptr;
    const uint8_t *bases = nullptr;
    const uint64_t *offs = nullptr;
    uint64_t n_reads = 0, n_bases = 0;
    uint16_t *out = nullptr;              // the u16 vector; null: verdict bins only (cls.bin_width != 0), or reset masks are the result
    uint8_t *err = nullptr;
    DevStats *stats = nullptr;
    const uint32_t *order = nullptr;
    hipStream_t stream = nullptr;
    ClsArgs cls;
    SegWorkspace *seg_ws = nullptr;       // non-null allows the segment-parallel path for batches of long reads (cfg.seg_len)
    int ragged_hint = -1;                 // 1 / 0 = the caller knows that the longest read is / is not more than 1.5 x the mean, -1 = it does not (device offsets only)
    int *seg_verdict = nullptr;
    LaunchInfo *info = nullptr;
    MaskArgs mask;
    const uint8_t *chain_rows = nullptr;  // the handle's chain rows (null: it holds none): what a route with ahd == 3 walks on
    int cls_mode() const { return cls.bin_width == 0 ? 0 : (out ? 1 : 2); }   // 0 = PML vector only, 1 = vector + classification bins, 2 = bins only
    bool logging() const { return cls.log_ff != nullptr || cls.log_scan != nullptr; }
};
// What the call asks of the policy: `want` and "pml_via_mask" from the caller, the rest read off the call's pointers.
PmlAsk pml_ask(const PmlCall &c, PmlWant want, int via_mask);
// Validates, runs the route's pre-step (the park queue's reset), the walk (or the segment plan where it has the first say) and the
// route's post-step (masks packed from the vector in tmp, or the vector expanded from the masks).
hipError_t launch_pml(const PmlCall &c, const PmlRoute &route);

hipError_t launch_count(int mode, const DevIndex &ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                        uint64_t n_reads, uint64_t *d_matched, uint64_t *d_count, uint8_t *d_err,
                        DevStats *d_stats, const uint32_t *d_order, const LaunchCfg &cfg, hipStream_t stream,
                        LaunchInfo *info = nullptr, uint64_t n_bases = 0);   // n_bases: the batch's size if the caller knows it (the state machine needs >= 16)

hipError_t launch_zml(int mode, const DevIndex &ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                      uint64_t n_reads, uint64_t n_bases, uint16_t *d_out, uint8_t *d_err, DevStats *d_stats,
                      const uint32_t *d_order, const LaunchCfg &cfg, hipStream_t stream,
                      SegWorkspace *seg_ws = nullptr, int ragged_hint = -1, int *seg_verdict = nullptr,
                      LaunchInfo *info = nullptr);

// d_err (optional): reads flagged there report no bins (0, 0, 0), like the fused kernels.
// n_bases (optional): the batch's size, if the caller knows it -- batches of long reads (mean >= 1024) take a wavefront per read.
hipError_t launch_classify(const uint16_t *d_pml, const uint64_t *d_offsets, uint64_t n_reads, uint32_t bin_width,
                           uint32_t thr, uint32_t *d_above, uint32_t *d_below, uint64_t *d_sum, hipStream_t stream,
                           const uint8_t *d_err = nullptr, uint64_t n_bases = 0);

// Mode 7: ix = a mode-7 view (widened rows + tally table); writes r mode-6 rows (8 bytes each) with the ids recovered by get_id.
hipError_t expand_sampled_rows(int mode, const DevIndex &ix, void *d_rows6, hipStream_t stream);   // mode 7 or 5
// Modes 8 / 2: ix = a blocked view (raw 6-byte rows + id_blocks); writes r 8-byte rows (regular-thresholds / regular
// layout) with the ids get_id reconstructs.
hipError_t expand_blocked_rows(int mode, const DevIndex &ix, void *d_rows6, hipStream_t stream);

// Mode 7: 3-byte file rows -> one dword per row (d_wide: r * 4 bytes + 16 of slack).
hipError_t widen_rows(const uint8_t *d_packed, uint64_t r, uint32_t *d_wide, hipStream_t stream);

// Fills the 4^K entries of the top-of-walk table (DevIndex::kmer) by walking every K-mer from the start state with the
// plain base-synchronous automaton.  ix.kmer / ix.kmer_k of `ix` are ignored; K in [1, 12]; thresholds types (kmode 6) only.
hipError_t build_kmer_table(const DevIndex &ix, uint32_t K, uint4 *d_table, hipStream_t stream);
// Look-ahead rows (DevIndex::rows2): ahead_rows_bytes(r) bytes at d_rows2, written by one kernel (a gather of id(id(i))
// per row); *tail = DevIndex::rows2_tail.  Thresholds types (kmode 6: the PML walk's rows), r >= 8.
uint64_t ahead_rows_bytes(uint64_t r);
// Deep rows (DevIndex::rows3): deep_rows_bytes(r) bytes at d_rows3 (zeroed by the call), one kernel (three dependent gathers per row).
// Thresholds types (kmode 6), 8 <= r < 2^28 - 1.
uint64_t deep_rows_bytes(uint64_t r);
bool deep_rows_eligible(uint64_t r);
hipError_t build_deep_rows(int kmode, const DevIndex &ix, int hint_bits, uint8_t *d_rows3, hipStream_t stream);   // hint_bits: 2 or 4 (deep_map_for)
// Chain rows (pml_kernel_chain; "chain_rows" option): chain_rows_bytes(r) bytes at d_rows4, every byte written by one kernel (four dependent
// gathers per row).  Thresholds types (kmode 6), 8 <= r < 2^28 - 1.  The kernels' view of the index has no field for them: a launch that
// walks on them hands the table over in PmlCall::chain_rows and launch_pml puts it where that kernel reads its rows (DevIndex::rows3).
uint64_t chain_rows_bytes(uint64_t r);
bool chain_rows_eligible(uint64_t r);
hipError_t build_chain_rows(int kmode, const DevIndex &ix, uint8_t *d_rows4, hipStream_t stream);
hipError_t launch_walk_chain(const WalkLaunch &L, LaunchInfo *info);   // pml_kernel_chain<SEP, RING> (movi_walk_chain.hip): L.sep, L.ring 0 / 2
hipError_t preload_walk_chain();
bool ahead_rows_hinted(uint64_t r);    // the copy of a table of r rows carries reposition hints and 32-bit ids (DevIndex::hints)
hipError_t build_ahead_rows(int kmode, const DevIndex &ix, uint8_t *d_rows2, uint64_t *tail, hipStream_t stream,
                            unsigned long long *d_tally = nullptr);   // d_tally: 2 * kTallySlots zeroed u64 (tally_add spreads the atomics by block; the caller sums the pairs), optional
// sum of d_tally[2 s] / sum of d_tally[2 s + 1] over the kTallySlots pairs (2 * kTallySlots zeroed u64) = share of the BWT positions of every stride-th row that reach their LF
// target without a fast-forward (no_ff_share_kernel): the launch policy's statistic, without building the copy
hipError_t tally_no_ff_share(int kmode, const DevIndex &ix, uint64_t stride, unsigned long long *d_tally, hipStream_t stream);

// Fills the 4^K entries of the count query's interval table (DevIndex::ftab); mode = resident layout (6 or 3).
hipError_t build_ftab(int mode, const DevIndex &ix, uint32_t K, uint4 *d_table, hipStream_t stream);

// MEM finding (movi_walk_mem.hip; MoveStructure::query_mems, src/mem_finder.cpp:7-145).  MemOut is movi_mem_t.
struct MemOut { uint32_t start, end; uint64_t count; };
struct MemArgs {
    uint64_t comp;       // byte c: code of the complement of the base of code c, 0xFF = not in the alphabet
    uint32_t min_len;    // L' = max(L, 1)
    uint32_t pad_;
};
hipError_t launch_mem(int mode, const DevIndex &ix, const MemArgs &a, const uint8_t *d_bases, const uint64_t *d_offsets,
                      uint64_t n_reads, MemOut *d_mems, uint32_t *d_n_mems, uint8_t *d_err, DevStats *d_stats,
                      const uint32_t *d_order, hipStream_t stream, LaunchInfo *info);

// k-mer presence (movi_walk_kmer.hip; MoveStructure::query_all_kmers, src/sequitur.cpp:322-421).  KmerRun is movi_kmer_run_t.
struct KmerRun { uint32_t start, count; };
struct KmerArgs {
    uint32_t k;          // >= 1
    uint32_t step;       // the look-ahead's split: a look starts at most this far left of the end under test (0 = no look-ahead)
};
hipError_t launch_kmer(int mode, const DevIndex &ix, const KmerArgs &a, const uint8_t *d_bases, const uint64_t *d_offsets,
                       uint64_t n_reads, KmerRun *d_runs, uint32_t *d_n_runs, uint32_t *d_found, uint8_t *d_err,
                       DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info);

// k-mer occurrences (movi_walk_kmer_occ.hip): d_occ[offsets[i] + p] = occurrences of the k-mer at p of read i, over all n_bases slots;
// d_found / d_sum / d_err per read, each optional.  Mark, search (search_lists, movi_search.hpp) and reduction, three kernels on
// `stream`; no scratch.
constexpr int kKmerOccWaves = 16;    // kmer_occ_kernel: one-wavefront blocks per CU a launch fills at most (a lane then owns a list of slots)
hipError_t launch_kmer_occ(int mode, const DevIndex &ix, uint32_t k, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t n_bases, uint64_t *d_occ, uint32_t *d_found, uint64_t *d_sum, uint8_t *d_err, DevStats *d_stats,
                           int num_cus, hipStream_t stream, LaunchInfo *info);
hipError_t preload_kmer_occ(int mode, bool idx32);   // load the translation unit's code object now (movi_index_prepare)

// Locate (movi_walk_sa.hip; MoveStructure::get_SA_entries, src/move_structure.cpp:35-48; the layouts and the walk, locate_walk, are
// stated in movi_sa.hpp, the lanes' item lists in movi_lists.hpp).
constexpr int kLocateWaves = 16;     // locate_kernel, hits_walk_kernel, color_walk_kernel: one-wavefront blocks per CU a launch fills at most (a lane then owns a list of items)
struct LocArgs {
    const uint4 *rows = nullptr;        // the locate rows: 16 bytes per row
    const uint64_t *samples = nullptr;  // n / rate + 1 entries (not read in successor mode)
    uint64_t n = 0;                     // BWT length: no walk is longer
    uint64_t n_entries = 0;             // sample indexes are below this
    uint32_t rate = 0;
    uint32_t succ = 0;                  // 1 = successor mode: one LF step first; out = the sample's index, aux = the distance
    uint64_t *aux = nullptr;
};
uint64_t locate_rows_bytes(uint64_t r);
// d_loc: locate_rows_bytes(r) bytes; *n_total (host, optional) = the sum of the row lengths.  Allocates its scan's scratch and waits.
hipError_t build_locate_rows(int mode, const DevIndex &ix, uint64_t rate, uint4 *d_loc, uint64_t *n_total, hipStream_t stream);
hipError_t locate_rows_all_p(const uint4 *d_loc, uint64_t first, uint64_t cnt, uint64_t rate, uint64_t *d_all_p, hipStream_t stream);
// In place: d_pos[i] = a packed position in, its suffix-array entry out (successor mode: see LocArgs).
hipError_t launch_locate(int mode, const DevIndex &ix, const LocArgs &a, uint64_t *d_pos, uint64_t n_items, DevStats *d_stats,
                         int num_cus, hipStream_t stream, LaunchInfo *info);
// The PML walk that records its positions (mode-6 rows): d_pml optional, d_pos[offsets[i] + k] = position after base len - 1 - k.
hipError_t launch_sa_pos(const DevIndex &ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint16_t *d_pml,
                         uint64_t *d_pos, uint8_t *d_err, DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info);
// d_samples: loc.n / loc.rate + 1 entries.  *bad (host) = findings that one cycle over all samples cannot produce (0 = the array is
// complete).  Allocates its scratch and waits.
hipError_t build_sampled_sa(int mode, const DevIndex &ix, const LocArgs &loc, uint64_t *d_samples, DevStats *d_stats, int num_cus,
                            hipStream_t stream, uint32_t *bad, LaunchInfo *info);
hipError_t preload_sa(int mode, bool idx32);   // load the translation unit's code object now (movi_index_prepare)
// Locate count and MEM hits (movi_walk_hits.hip): per match item (read, start, end) the occurrences of P[start .. end) in the text --
// d_occ[i] --, the exclusive prefix sum of min(occ, max_occ) -- d_first[0 .. n_items] --, and the text positions of those hits in BWT
// order in d_positions[d_first[i] .. d_first[i + 1]) as far as they lie below positions_cap.  Interval search (search_lists,
// movi_search.hpp), scan, expansion and locate walk (locate_walk, movi_sa.hpp) on `stream`; the intervals, the scan's input and its temporary storage live in d_work (hits_work_layout).  stages: 3 = the
// whole call; 1 / 2 = stop after the scan / the expansion (a measurement hook: the steps timed apart).
struct HitsItem { uint32_t read, start, end; };          // movi_match_t
constexpr int kHitsWaves = 16;                           // hits_interval_kernel: one-wavefront blocks per CU a launch fills at most
constexpr uint64_t kHitsMaxItems = 0x7FFFFFFFull;        // n_items + 1 values go through one 32-bit-indexed device scan
constexpr uint64_t kHitsIntervalBytes = 24;
struct HitsWorkLayout { uint64_t intervals, listed, scan_temp, total; };   // byte offsets into d_work, and its size
// (the scan's temporary storage: a few words of look-back state per block of at least 256 values -- bounded here by half a byte per
// value plus 32 KiB, several times what hipCUB asks for; the launcher checks hipCUB's own figure against it)
inline HitsWorkLayout hits_work_layout(uint64_t n_items) {
    auto up = [](uint64_t v) { return (v + 255u) & ~255ull; };
    HitsWorkLayout w;
    w.intervals = 0;
    w.listed = up(n_items * kHitsIntervalBytes);
    w.scan_temp = w.listed + up((n_items + 1) * 8);
    w.total = w.scan_temp + up(n_items / 2 + (32u << 10));
    return w;
}
hipError_t launch_locate_matches(int mode, const DevIndex &ix, const LocArgs &loc, const uint8_t *d_bases, const uint64_t *d_offsets,
                                 uint64_t n_reads, const HitsItem *d_items, uint64_t n_items, uint32_t max_occ, uint64_t *d_occ,
                                 uint64_t *d_first, uint64_t *d_positions, uint64_t positions_cap, uint8_t *d_item_err, void *d_work,
                                 uint64_t work_bytes, int stages, DevStats *d_stats, int num_cus, hipStream_t stream, LaunchInfo *info);
hipError_t preload_hits(int mode, bool idx32);   // load the translation unit's code object now (movi_index_prepare)
// d_pos[m] = the packed position of BWT position m * loc.rate, m < n_samples (what build_sampled_sa starts its list from).
hipError_t launch_sample_positions(int mode, const DevIndex &ix, const LocArgs &loc, uint64_t n_samples, uint64_t *d_pos, hipStream_t stream);

// Movi Color (movi_walk_color.hip; the tables and the key are stated in movi_color.hpp).
struct ColorTables {
    const uint16_t *flat = nullptr;     // every distinct set: size, then its sorted members
    const uint64_t *inds = nullptr;     // r offsets into flat
    uint64_t flat_size = 0;
    uint32_t num_species = 0;
};
// One read's result of the multi-class scoring (movi_mc_read_t): ReadProcessor::process_char, src/read_processor.cpp:122-186.
struct McRead { uint16_t best, second; uint32_t colors_count, sum_ml, best_count, second_count, reserved_; };
// Lane slots [t0, t1) of a batch of n_reads reads.  d_counts: num_species u32 per read, zeroed by the caller; indexed by read
// (by_read) or by slot - t0 (the handle's scratch).  d_pml optional.
hipError_t launch_color(const DevIndex &ix, const ColorTables &ct, uint32_t min_len, const uint8_t *d_bases, const uint64_t *d_offsets,
                        uint64_t t0, uint64_t t1, uint16_t *d_pml, McRead *d_out, uint32_t *d_counts, bool by_read, uint8_t *d_err,
                        DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info);
hipError_t preload_color(int mode, bool idx32);
// The builder: the (row, document) pairs of every BWT position, sorted and unique, in a buffer of the call's own (*d_keys, to be
// hipFree'd by the caller; *n_keys pairs).  loc: the attached sampled suffix array.  h_doc_ends / h_doc_ids: n_docs strictly
// increasing end offsets and the documents' numbers.  chunk_keys: at most this many BWT positions per chunk (0 = what the device's
// free memory allows).  *bad (host) = findings that a consistent table and array cannot produce.  seconds[0] / [1]: walks / sorts.
hipError_t build_color_keys(int mode, const DevIndex &ix, const LocArgs &loc, const uint64_t *h_doc_ends, const uint16_t *h_doc_ids,
                            uint32_t n_docs, uint64_t chunk_keys, int num_cus, hipStream_t stream, uint64_t **d_keys, uint64_t *n_keys,
                            uint32_t *bad, uint32_t *n_chunks, double *seconds, LaunchInfo *info, uint64_t *key_cap = nullptr);
// (on hipErrorOutOfMemory *n_keys = the unique keys held when the next stretch did not fit and *key_cap = the budget, in keys)

// Compaction of per-read results of variable length (the host path of both): d_first[0..n] = exclusive prefix of the counts d_n
// (d_first[n] = their total); then read i's d_n[i] elements of elem_bytes (8 or 16) from d_src[d_offsets[i]..] to d_out[d_first[i]..].
hipError_t launch_count_scan(const uint32_t *d_n, uint64_t n_reads, uint64_t *d_first, hipStream_t stream);
hipError_t launch_gather(const void *d_src, size_t elem_bytes, const uint64_t *d_offsets, const uint32_t *d_n, uint64_t n_reads,
                         const uint64_t *d_first, void *d_out, hipStream_t stream);

// Fills ckpt[j] = BWT position of row (j << kPrefixShift), j = 0 .. ceil(r/32).
hipError_t build_row_start_ckpt(int mode, const uint8_t *d_rows, uint64_t r, uint64_t *d_ckpt,
                                hipStream_t stream);

}  // namespace movi
