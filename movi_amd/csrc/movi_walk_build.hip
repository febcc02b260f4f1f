// movi_walk_build.hip -- index.movi from a run-length BWT, on the GPU: what MoveStructure::build() derives from the run heads, the run
// lengths and the thresholds of pfp-thresholds (src/move_structure_build.cpp:17-72 with --preprocessed: :240-324 row boundaries,
// :74-121 + :449-692 LF of the row heads -> id / offset, :694-731 base intervals, :807-935 thresholds, :939-1074 blocked ids,
// :486-496 / :571-596 / :677-682 tally ids; src/move_structure_io.cpp:435-469 the file).  The contract is in include/movi_hip.h
// (movi_build_from_rlbwt); the stages, as DESIGN.md "Build from a run-length BWT" lists them:
//   1  run starts            exclusive sum of the lengths (hipcub)
//   2  threshold split points radix sort + unique of the thresholds (hipcub), merged with the run starts by rank
//   3  rows                  pieces of MAX_RUN_LENGTH per segment, their sum (hipcub) = r, then a row-sized kernel
//   4  LF of the row heads   per-character sum of the lengths in row order            (slot scan: add, forward)
//   5  id and offset         a binary search over all_p per row, in the apply phase of stage 4's scan
//   6  thresholds            nearest row below with each other character             (slot scan: rightmost defined, reverse)
//   7  blocked / tally ids   latest id per character at the block boundaries / check points (slot scan: rightmost defined, forward)
//   8  pack, copy down, assemble the image on the host
// Stages 4, 6 and 7 are ONE hand-written scan over the rows (scan_rows below) whose state is a 64-bit slot per character.
// (Named into the movi_walk*.hip family, though it walks nothing: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library
// from that glob, and movi_abi.hip calls into this file.)
#include "movi_build.hpp"

#include "../../include/movi_hip.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace movi {

namespace {

// ------------------------------------------------------------------------------------------------ searches
// Fixed trip counts (`steps` = the bit length of the array's size): wave-uniform loops, as the control-flow note in movi_device.hpp
// asks; an iteration past the end of the search is a no-op and loads nothing.
__host__ __device__ inline int search_steps(uint64_t n) {
    int s = 0;
    while (n) { s++; n >>= 1; }
    return s;
}
// the number of a[0 .. n) that are <= x (UPPER) or < x (!UPPER); a is ascending
template <bool UPPER>
__device__ __forceinline__ uint64_t bound_u64(const uint64_t *__restrict__ a, uint64_t n, uint64_t x, int steps) {
    uint64_t lo = 0, len = n;
    for (int s = 0; s < steps; ++s) {
        const uint64_t half = len >> 1, mid = lo + half;
        const uint64_t v = len ? a[mid] : 0;
        const bool right = len != 0 && (UPPER ? v <= x : v < x);
        lo = right ? mid + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------------ the slot scan
// A scan over the rows whose state is one 64-bit slot per character (at most five: '%' + ACGT).  A row contributes one value to one
// slot, or nothing; the operator joins slots pairwise.  Three phases, each streaming the rows once: every block reduces its tile of
// kScanTile rows to one state (scan_reduce_kernel), one block scans the tiles' states (scan_sums_kernel), every block scans its tile
// again from its prefix and hands every row the state BEFORE it (scan_apply_kernel).  REV runs it from the last row to the first.
// A thread owns kScanItems neighbouring rows, so a wavefront's loads cover whole lines.
constexpr int kSlots = 5;
constexpr uint64_t kUndef = ~0ull;                       // no value yet (thresholds and ids are below 2^40)
constexpr int kScanThreads = 256, kScanItems = 8;
constexpr uint64_t kScanTile = (uint64_t)kScanThreads * kScanItems;

struct Slots { uint64_t v[kSlots]; };
struct Item { uint32_t slot; uint64_t val; };            // slot >= kSlots: the row contributes nothing

struct OpAdd {                                           // sums
    static constexpr uint64_t kIdentity = 0;
    static __device__ __forceinline__ uint64_t join(uint64_t a, uint64_t b) { return a + b; }
};
struct OpLast {                                          // the rightmost defined value wins
    static constexpr uint64_t kIdentity = kUndef;
    static __device__ __forceinline__ uint64_t join(uint64_t a, uint64_t b) { return b != kUndef ? b : a; }
};

// (slots are picked by compare-and-select over the unrolled five, never by a run-time index: the state stays in registers)
template <class Op>
__device__ __forceinline__ Slots slots_identity() {
    Slots s;
#pragma unroll
    for (int a = 0; a < kSlots; a++) s.v[a] = Op::kIdentity;
    return s;
}
template <class Op>
__device__ __forceinline__ void slots_join(Slots &a, const Slots &b) {       // a = a then b
#pragma unroll
    for (int k = 0; k < kSlots; k++) a.v[k] = Op::join(a.v[k], b.v[k]);
}
template <class Op>
__device__ __forceinline__ void slots_fold(Slots &s, const Item &it) {
#pragma unroll
    for (int a = 0; a < kSlots; a++) s.v[a] = it.slot == (uint32_t)a ? Op::join(s.v[a], it.val) : s.v[a];
}
__device__ __forceinline__ uint64_t slots_get(const Slots &s, uint32_t slot) {
    uint64_t x = 0;
#pragma unroll
    for (int a = 0; a < kSlots; a++) x = slot == (uint32_t)a ? s.v[a] : x;
    return x;
}

// Inclusive scan of one state per thread through the LDS (double-buffered, log2(256) rounds); returns the state of the threads
// before this one and the block's total.  Every thread of the block makes the call.
template <class Op>
__device__ __forceinline__ Slots block_scan(const Slots &mine, Slots (*sh)[kScanThreads], Slots &total) {
    const int t = threadIdx.x;
    sh[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kScanThreads; d <<= 1) {
        Slots x = sh[cur][t];
        if (t >= d) {
            Slots y = sh[cur][t - d];
            slots_join<Op>(y, x);
            x = y;
        }
        sh[cur ^ 1][t] = x;
        __syncthreads();
        cur ^= 1;
    }
    total = sh[cur][kScanThreads - 1];
    Slots before = slots_identity<Op>();
    if (t > 0) before = sh[cur][t - 1];
    return before;
}

template <class Op, bool REV, class F>
__device__ __forceinline__ Slots tile_reduce(const F &f, uint64_t r) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    Slots s = slots_identity<Op>();
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        const uint64_t k = base + j;
        if (k < r) slots_fold<Op>(s, f.item(REV ? r - 1 - k : k));
    }
    return s;
}

template <class Op, bool REV, class F>
__global__ __launch_bounds__(kScanThreads) void scan_reduce_kernel(F f, uint64_t r, Slots *__restrict__ sums) {
    __shared__ Slots sh[2][kScanThreads];
    Slots total;
    (void)block_scan<Op>(tile_reduce<Op, REV>(f, r), sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[b] becomes the state of the tiles before b; one block, a thread owns `chunk` neighbouring tiles
template <class Op>
__global__ __launch_bounds__(kScanThreads) void scan_sums_kernel(Slots *__restrict__ sums, uint64_t nb) {
    __shared__ Slots sh[2][kScanThreads];
    const uint64_t chunk = (nb + kScanThreads - 1) / kScanThreads, lo = (uint64_t)threadIdx.x * chunk;
    Slots s = slots_identity<Op>();
    for (uint64_t c = 0; c < chunk; c++)
        if (lo + c < nb) slots_join<Op>(s, sums[lo + c]);
    Slots total;
    Slots run = block_scan<Op>(s, sh, total);
    for (uint64_t c = 0; c < chunk; c++)
        if (lo + c < nb) {
            const Slots x = sums[lo + c];
            sums[lo + c] = run;
            slots_join<Op>(run, x);
        }
}

template <class Op, bool REV, class F>
__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(F f, uint64_t r, const Slots *__restrict__ sums) {
    __shared__ Slots sh[2][kScanThreads];
    Slots total;
    const Slots before = block_scan<Op>(tile_reduce<Op, REV>(f, r), sh, total);
    Slots state = sums[blockIdx.x];
    slots_join<Op>(state, before);
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    for (int j = 0; j < kScanItems; j++) {
        const uint64_t k = base + j;
        if (k < r) {
            const uint64_t i = REV ? r - 1 - k : k;
            f.apply(i, state);
            slots_fold<Op>(state, f.item(i));
        }
    }
}

uint64_t scan_tiles(uint64_t r) { return (r + kScanTile - 1) / kScanTile; }

// d_sums: scan_tiles(r) states
template <class Op, bool REV, class F>
hipError_t scan_rows(const F &f, uint64_t r, Slots *d_sums, hipStream_t stream) {
    const unsigned nb = (unsigned)scan_tiles(r);
    hipLaunchKernelGGL((scan_reduce_kernel<Op, REV, F>), dim3(nb), dim3(kScanThreads), 0, stream, f, r, d_sums);
    hipLaunchKernelGGL((scan_sums_kernel<Op>), dim3(1), dim3(kScanThreads), 0, stream, d_sums, (uint64_t)nb);
    hipLaunchKernelGGL((scan_apply_kernel<Op, REV, F>), dim3(nb), dim3(kScanThreads), 0, stream, f, r, (const Slots *)d_sums);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ stage 2: the split points
// U[0 .. *nu): the distinct thresholds, ascending.  One is kept when it is below n and no run starts there; lb = the run starts
// below it, so a kept one lies in run lb - 1.
__global__ __launch_bounds__(256) void split_keep_kernel(const uint64_t *__restrict__ U, const uint64_t *__restrict__ nu,
                                                         const uint64_t *__restrict__ run_start, uint64_t R, uint64_t n, int steps,
                                                         uint32_t *__restrict__ keep, uint32_t *__restrict__ lb_out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > R) return;
    uint32_t k = 0, lbv = 0;
    if (j < R && j < *nu) {
        const uint64_t x = U[j];
        const uint64_t lb = bound_u64<false>(run_start, R, x, steps);
        k = (x < n && (lb == R || run_start[lb] != x)) ? 1u : 0u;
        lbv = (uint32_t)lb;
    }
    keep[j] = k;                                         // (keep[R] = 0: the sum's last item)
    if (j < R) lb_out[j] = lbv;
}

// The run starts and the kept split points merged by rank into the segment starts; seg_run = the run a segment lies in.
// kpos = the exclusive sum of keep, R + 1 items.
__global__ __launch_bounds__(256) void split_merge_kernel(const uint64_t *__restrict__ U, const uint64_t *__restrict__ nu,
                                                          const uint64_t *__restrict__ run_start, uint64_t R, uint64_t n, int steps,
                                                          const uint32_t *__restrict__ keep, const uint32_t *__restrict__ lb,
                                                          const uint32_t *__restrict__ kpos, uint64_t *__restrict__ seg_start,
                                                          uint32_t *__restrict__ seg_run, uint64_t *__restrict__ nseg) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= R) return;
    if (keep[j]) {
        const uint64_t s = (uint64_t)kpos[j] + lb[j];
        seg_start[s] = U[j];
        seg_run[s] = lb[j] - 1u;
    }
    const uint64_t below = bound_u64<false>(U, *nu < R ? *nu : R, run_start[j], steps);   // (below <= R: kpos has R + 1 items)
    const uint64_t s = j + kpos[below];
    seg_start[s] = run_start[j];
    seg_run[s] = (uint32_t)j;
    if (j == 0) {
        const uint64_t total = R + kpos[R];
        seg_start[total] = n;
        *nseg = total;
    }
}

// ------------------------------------------------------------------------------------------------ stage 3: the rows
__global__ __launch_bounds__(256) void pieces_kernel(const uint64_t *__restrict__ seg_start, uint64_t nseg, uint32_t maxrun,
                                                     uint64_t *__restrict__ pieces) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg) pieces[s] = (seg_start[s + 1] - seg_start[s] + maxrun - 1) / maxrun;
    else if (s == nseg) pieces[s] = 0;                   // the sum's last item: first_row[nseg] = r
}

struct RowArrays {
    uint64_t *all_p;       // r + 1: the BWT position of every row's first character, then n
    uint16_t *lens;
    uint8_t *code;
    uint32_t *row_run;     // the original run a row lies in
    uint64_t *end;         // end_bwt_idx: the terminator's row
};

__global__ __launch_bounds__(256) void rows_kernel(const uint64_t *__restrict__ first_row, const uint64_t *__restrict__ seg_start,
                                                   const uint32_t *__restrict__ seg_run, uint64_t nseg, const uint8_t *__restrict__ heads,
                                                   const uint8_t *__restrict__ code_of, uint32_t maxrun, uint64_t r, uint64_t n, int steps,
                                                   RowArrays o) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r) return;
    const uint64_t s = bound_u64<true>(first_row, nseg, i, steps) - 1;          // first_row[0] = 0 <= i
    const uint64_t p = seg_start[s] + (i - first_row[s]) * maxrun, rest = seg_start[s + 1] - p;
    const uint32_t run = seg_run ? seg_run[s] : (uint32_t)s;
    const uint8_t h = heads[run];
    o.all_p[i] = p;
    o.lens[i] = (uint16_t)(rest < maxrun ? rest : maxrun);
    o.code[i] = code_of[h];
    o.row_run[i] = run;
    if (h == 0) *o.end = i;                              // one row: the terminator's run has length 1
    if (i == 0) o.all_p[r] = n;
}

// ------------------------------------------------------------------------------------------------ stages 4 + 5: LF, id, offset
// find_run_heads_information (:74-121) + LF_heads (src/move_structure.cpp:515-523): lf = C[a] + the characters a in the rows before;
// build_move_rows (:449-692): id = the last row that starts at or before lf.  A binary search per row (the merge -- lf ascends within
// a character -- is the follow-up).
struct LfScan {
    RowArrays rows;
    uint64_t r;
    uint64_t C[kSlots];
    int steps;
    uint64_t *pp_id;
    uint16_t *off;
    __device__ __forceinline__ Item item(uint64_t i) const {
        return Item{i == *rows.end ? (uint32_t)kSlots : (uint32_t)rows.code[i], rows.lens[i]};
    }
    __device__ __forceinline__ void apply(uint64_t i, const Slots &before) const {
        const uint32_t a = rows.code[i];
        uint64_t c = 0;
#pragma unroll
        for (int k = 0; k < kSlots; k++) c = a == (uint32_t)k ? C[k] : c;
        const uint64_t lf = i == *rows.end ? 0 : c + slots_get(before, a);
        const uint64_t id = bound_u64<true>(rows.all_p, r, lf, steps) - 1;      // all_p[0] = 0 <= lf
        pp_id[i] = id;
        off[i] = (uint16_t)(lf - rows.all_p[id]);
    }
};

// find_base_interval_data (:694-731): a handful of look-ups, one thread.  out: first_runs | first_offsets | last_runs | last_offsets,
// kSlots + 1 each.
__global__ void base_intervals_kernel(RowArrays rows, uint64_t r, uint32_t sigma, Slots counts, int steps, uint64_t *__restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t *fr = out, *fo = out + (kSlots + 1), *lr = out + 2 * (kSlots + 1), *lo = out + 3 * (kSlots + 1);
    fr[0] = fo[0] = lr[0] = lo[0] = 0;
    uint64_t cc = 1;
    for (uint32_t a = 0; a < sigma; a++) {
        if (lo[a] + 1 >= rows.lens[lr[a]]) { fr[a + 1] = lr[a] + 1; fo[a + 1] = 0; }
        else { fr[a + 1] = lr[a]; fo[a + 1] = lo[a] + 1; }
        cc += slots_get(counts, a);
        const uint64_t k = bound_u64<false>(rows.all_p, r, cc, steps);         // rows starting before cc: >= 1
        lr[a + 1] = k - 1;
        lo[a + 1] = cc - rows.all_p[k - 1] - 1;
    }
}

// ------------------------------------------------------------------------------------------------ stage 6: thresholds
// compute_thresholds (:807-935), the reference's descending loop as a reverse scan: for row i and every other character j, cur = the
// threshold of the nearest row below i whose code is j (n when there is none); the terminator's row counts as a row of code 0 with its
// own run's threshold (:823).  The reference counts its index into the thresholds down where `code changes or a neighbour is the
// terminator's row`; on input that passed rlbwt_check that is the run a row lies in: row_run is used.  Row 0 is not visited (:903-929).
constexpr uint32_t kAlphamap3 =                           // src/utils.cpp:5-8, two bits per entry, entry (a, b) at bit 2 * (4 a + b)
    (3u << 0) | (0u << 2) | (1u << 4) | (2u << 6) | (0u << 8) | (3u << 10) | (1u << 12) | (2u << 14) |
    (0u << 16) | (1u << 18) | (3u << 20) | (2u << 22) | (0u << 24) | (1u << 26) | (2u << 28) | (3u << 30);

struct ThrScan {
    RowArrays rows;
    const uint64_t *thr;         // per original run
    uint64_t n;
    uint32_t sigma, sep;
    uint8_t *tbits;              // per row: the three threshold bits
    uint64_t *end_thr;           // [4]
    const uint32_t *sep_rank;    // separators: the rows of code 0 before this one; m of them in all
    uint64_t m;
    uint16_t *sep_thr;           // [m][4], in descending row order (the order the reference appends them in)
    uint64_t *sep_map;           // [m][2]: row, entry; ascending rows
    uint32_t *inside;            // findings: a threshold strictly inside a row
    __device__ __forceinline__ Item item(uint64_t i) const { return Item{(uint32_t)rows.code[i], thr[rows.row_run[i]]}; }
    __device__ __forceinline__ void apply(uint64_t i, const Slots &below) const {
        const uint32_t rc = rows.code[i];
        const bool sep_row = sep != 0u && rc == 0u, end_row = i == *rows.end;
        uint64_t entry = 0;
        if (sep_row) {
            entry = m - 1 - sep_rank[i];
            sep_map[2 * (uint64_t)sep_rank[i]] = i;
            sep_map[2 * (uint64_t)sep_rank[i] + 1] = entry;
        }
        uint32_t bits = 0;
        if (i != 0) {
            const uint64_t p = rows.all_p[i], len = rows.lens[i];
#pragma unroll
            for (uint32_t j = 0; j < (uint32_t)kSlots; j++) {
                if (j >= sigma || j == rc || (sep != 0u && j == 0u)) continue;   // :849-852: no threshold is kept FOR the separator
                const uint64_t cur = below.v[j] == kUndef ? n : below.v[j];
                const uint64_t val = cur >= p + len ? len : (cur <= p ? 0 : cur - p);
                if (end_row) end_thr[j - sep] = val;                             // set_threshold_for_one_character :776-779
                else if (sep_row) sep_thr[entry * 4 + (j - 1u)] = (uint16_t)val; // :781-784
                else if (val != 0 && val != len) atomicAdd(inside, 1u);           // :869-871: rows are split at the thresholds
                else bits |= (val ? 1u : 0u) << ((kAlphamap3 >> (2u * (4u * (rc - sep) + (j - sep)))) & 3u);
            }
        }
        tbits[i] = (uint8_t)bits;
    }
};

// ------------------------------------------------------------------------------------------------ stage 7: ids of the compact types
// compute_blocked_ids (:939-1074): per block and character the last adjusted id (id - first_runs[c + 1]) strictly before the block,
// 0 when there is none; a row keeps its distance from that.
struct BlockScan {
    RowArrays rows;
    const uint64_t *pp_id, *first_runs;
    uint32_t sigma;
    uint64_t block_size, n_blocks;
    uint32_t *id_blocks;         // [sigma][n_blocks]
    __device__ __forceinline__ Item item(uint64_t i) const {
        const uint32_t c = rows.code[i];
        return Item{i == *rows.end ? (uint32_t)kSlots : c, pp_id[i] - first_runs[c + 1]};
    }
    __device__ __forceinline__ void apply(uint64_t i, const Slots &before) const {
        if (i % block_size != 0) return;
#pragma unroll
        for (uint32_t a = 0; a < (uint32_t)kSlots; a++)
            if (a < sigma) id_blocks[a * n_blocks + i / block_size] = before.v[a] == kUndef ? 0u : (uint32_t)before.v[a];
    }
};

__global__ __launch_bounds__(256) void blocked_ids_kernel(RowArrays rows, uint64_t r, const uint64_t *__restrict__ pp_id,
                                                          const uint64_t *__restrict__ first_runs, uint64_t block_size, uint64_t n_blocks,
                                                          const uint32_t *__restrict__ id_blocks, uint32_t *__restrict__ blocked,
                                                          unsigned long long *__restrict__ max_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long b = 0;
    if (i < r && i != *rows.end) {
        const uint32_t c = rows.code[i];
        b = pp_id[i] - first_runs[c + 1] - id_blocks[c * n_blocks + i / block_size];
    }
    if (i < r) blocked[i] = (uint32_t)b;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(b, s, 64);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0 && b) atomicMax(max_out, b);
}

// The tally table (:486-496, :571-596, :677-682): at every `ck`-th row the id of the latest run of each character, that row included;
// a character not seen yet gets the id of its first run, which is first_runs[c + 1] (that run's LF is C[c]); one extra last entry
// holds the final ids.
struct TallyScan {
    RowArrays rows;
    const uint64_t *pp_id, *first_runs;
    uint32_t sigma;
    uint64_t r, ck, n_tally;
    uint64_t *tally;             // [sigma][n_tally]
    __device__ __forceinline__ Item item(uint64_t i) const {
        return Item{i == *rows.end ? (uint32_t)kSlots : (uint32_t)rows.code[i], pp_id[i]};
    }
    __device__ __forceinline__ void apply(uint64_t i, const Slots &before) const {
        const bool at_ck = i % ck == 0, last = i == r - 1;
        if (!at_ck && !last) return;
        Slots now = before;
        slots_fold<OpLast>(now, item(i));
#pragma unroll
        for (uint32_t a = 0; a < (uint32_t)kSlots; a++) {
            if (a >= sigma) continue;
            const uint64_t v = now.v[a] == kUndef ? first_runs[a + 1] : now.v[a];
            if (at_ck) tally[a * n_tally + i / ck] = v;
            if (last) tally[a * n_tally + n_tally - 1] = v;
        }
    }
};

// ------------------------------------------------------------------------------------------------ stage 8: the packed rows
// include/move_row.hpp:128-142 with the masks of include/move_row_configs.hpp (:21-136); tools/build_index.cpp packs the same.
template <int MODE>
__global__ __launch_bounds__(256) void pack_kernel(RowArrays rows, uint64_t r, const uint64_t *__restrict__ pp_id, const uint16_t *__restrict__ off,
                                                   const uint8_t *__restrict__ tbits, const uint32_t *__restrict__ blocked, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r) return;
    const uint32_t n = rows.lens[i], o = off[i], c = rows.code[i], t = tbits ? tbits[i] : 0u;
    if (MODE == 6 || MODE == 3) {                          // mode 3: 12-bit n / offset, no threshold bits (t == 0)
        const uint64_t d = pp_id[i];
        uint16_t *w = reinterpret_cast<uint16_t *>(out) + i * 4;
        w[0] = (uint16_t)(d & 0xFFFFu);
        w[1] = (uint16_t)((d >> 16) & 0xFFFFu);
        w[2] = (uint16_t)(n | (((t >> 1) & 1u) << 11) | (((t >> 2) & 1u) << 12) | (c << 13));
        w[3] = (uint16_t)(o | ((t & 1u) << 11) | ((uint32_t)(d >> 32) << 12));
    } else if (MODE == 8 || MODE == 2) {
        const uint32_t b = blocked[i];
        uint16_t *w = reinterpret_cast<uint16_t *>(out) + i * 3;
        w[0] = (uint16_t)(b & 0xFFFFu);
        if (MODE == 8) {
            w[1] = (uint16_t)(n | ((b >> 16) << 10));
            w[2] = (uint16_t)(o | (c << 10) | ((t & 1u) << 13) | (((t >> 1) & 1u) << 14) | (((t >> 2) & 1u) << 15));
        } else {                                           // 24-bit id, MoveRow::set_id src/move_row.cpp:213-225
            w[1] = (uint16_t)(n | (((b >> 16) & 0x3Fu) << 10));
            w[2] = (uint16_t)(o | (c << 10) | ((b >> 22) << 14));
        }
    } else {
        uint8_t *w = out + i * 3;
        w[0] = (uint8_t)(n & 0xFFu);
        w[1] = (uint8_t)(o & 0xFFu);
        w[2] = MODE == 7 ? (uint8_t)((o >> 8) | ((n >> 8) << 1) | (c << 2) | ((t & 7u) << 5))
                         : (uint8_t)((o >> 8) | ((n >> 8) << 2) | (c << 4));
    }
}

struct IsCode0 {
    __host__ __device__ __forceinline__ uint32_t operator()(const uint8_t &c) const { return c == 0 ? 1u : 0u; }
};

// ------------------------------------------------------------------------------------------------ the host side
// Device memory of one build: freed on every return path; counts what is held for the profile.
struct DevPool {
    std::vector<std::pair<void *, size_t>> held;
    uint64_t now = 0, peak = 0;
    hipError_t err = hipSuccess;
    ~DevPool() { for (auto &p : held) (void)hipFree(p.first); }
    template <typename T>
    T *get(uint64_t count) {
        if (err != hipSuccess) return nullptr;
        void *p = nullptr;
        const size_t bytes = (size_t)(count ? count : 1) * sizeof(T);
        err = hipMalloc(&p, bytes);
        if (err != hipSuccess) return nullptr;
        held.emplace_back(p, bytes);
        now += bytes;
        peak = now > peak ? now : peak;
        return static_cast<T *>(p);
    }
    void release(void *p) {
        for (size_t k = 0; k < held.size(); k++)
            if (held[k].first == p) {
                (void)hipFree(p);
                now -= held[k].second;
                held.erase(held.begin() + (long)k);
                return;
            }
    }
};

void put64(std::vector<uint8_t> &o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

int hip_fail(hipError_t e, const char *what, std::string &why) {
    why = std::string(what) + ": " + hipGetErrorString(e) + " (hipError " + std::to_string((int)e) + ")";
    (void)hipGetLastError();
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? MOVI_ERR_NO_DEVICE : MOVI_ERR_HIP;
}

#define BUILD_TRY(expr, what)                                       \
    do {                                                            \
        hipError_t e_ = (expr);                                     \
        if (e_ == hipSuccess) e_ = pool.err;                        \
        if (e_ != hipSuccess) return hip_fail(e_, what, why);       \
    } while (0)

}  // namespace

int build_from_rlbwt(uint32_t mode, const uint8_t *h_heads, const uint64_t *h_lens, const uint64_t *h_thr, uint64_t original_r,
                     const RlbwtInfo &info, void **h_image, size_t *image_bytes, std::string &why) {
    const uint64_t R = original_r, n = info.n;
    const uint32_t maxrun = build_max_run(mode), sigma = info.sigma, sep = info.sep;
    const bool with_thr = build_mode_thresholds(mode), blocked_mode = mode == 8 || mode == 2, tally_mode = mode == 7 || mode == 5;
    // MOVI_BUILD_PROFILE=1: wait after every stage and print the stages' seconds and the peak device bytes (profiles/build_rlbwt.txt)
    const bool profile = std::getenv("MOVI_BUILD_PROFILE") && std::string(std::getenv("MOVI_BUILD_PROFILE")) == "1";
    hipStream_t stream = nullptr;
    DevPool pool;
    double stage_s[8] = {0};
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](int k) -> hipError_t {
        if (!profile) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        const auto t = std::chrono::steady_clock::now();
        stage_s[k] += std::chrono::duration<double>(t - t_last).count();
        t_last = t;
        return e;
    };
    void *d_temp = nullptr;
    size_t temp_cap = 0;
    auto temp = [&](size_t bytes) -> void * {             // hipcub's scratch: grown, never shrunk
        if (bytes > temp_cap) {
            if (d_temp) pool.release(d_temp);
            d_temp = pool.get<uint8_t>(bytes);
            temp_cap = d_temp ? bytes : 0;
        }
        return d_temp;
    };
    size_t tb = 0;

    // ---- stage 1: upload; run starts = the exclusive sum of the lengths, R + 1 items (the last is n)
    uint8_t *d_heads = pool.get<uint8_t>(R);
    uint8_t *d_code_of = pool.get<uint8_t>(256);
    uint64_t *d_lens = pool.get<uint64_t>(R + 1);
    uint64_t *d_run_start = pool.get<uint64_t>(R + 1);
    uint64_t *d_thr = with_thr ? pool.get<uint64_t>(R) : nullptr;
    BUILD_TRY(pool.err, "allocating the run arrays");
    BUILD_TRY(hipMemcpyAsync(d_heads, h_heads, R, hipMemcpyHostToDevice, stream), "copying the run heads");
    BUILD_TRY(hipMemcpyAsync(d_code_of, info.code_of, 256, hipMemcpyHostToDevice, stream), "copying the alphabet map");
    BUILD_TRY(hipMemcpyAsync(d_lens, h_lens, R * 8, hipMemcpyHostToDevice, stream), "copying the run lengths");
    BUILD_TRY(hipMemsetAsync(d_lens + R, 0, 8, stream), "clearing");
    if (with_thr) BUILD_TRY(hipMemcpyAsync(d_thr, h_thr, R * 8, hipMemcpyHostToDevice, stream), "copying the thresholds");
    BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_lens, d_run_start, (int)(R + 1), stream), "sizing the run-start sum");
    BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(temp(tb), tb, d_lens, d_run_start, (int)(R + 1), stream), "summing the run lengths");
    pool.release(d_lens);                                  // (stream order: the free waits for the sum)
    BUILD_TRY(lap(0), "stage 1");

    // ---- stage 2: segments = the runs cut at the thresholds
    uint64_t nseg = R;
    uint64_t *d_seg_start = d_run_start;
    uint32_t *d_seg_run = nullptr;
    if (with_thr) {
        const int n_bits = search_steps(n), steps_R = search_steps(R);
        uint64_t *d_sorted = pool.get<uint64_t>(R), *d_uniq = pool.get<uint64_t>(R), *d_counts = pool.get<uint64_t>(2);
        uint32_t *d_keep = pool.get<uint32_t>(R + 1), *d_kpos = pool.get<uint32_t>(R + 1), *d_lb = pool.get<uint32_t>(R);
        d_seg_start = pool.get<uint64_t>(2 * R + 1);
        d_seg_run = pool.get<uint32_t>(2 * R);
        BUILD_TRY(pool.err, "allocating the split points");
        BUILD_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, d_thr, d_sorted, (int)R, 0, n_bits, stream), "sizing the threshold sort");
        BUILD_TRY(hipcub::DeviceRadixSort::SortKeys(temp(tb), tb, d_thr, d_sorted, (int)R, 0, n_bits, stream), "sorting the thresholds");
        BUILD_TRY(hipcub::DeviceSelect::Unique(nullptr, tb, d_sorted, d_uniq, d_counts, (int)R, stream), "sizing the unique step");
        BUILD_TRY(hipcub::DeviceSelect::Unique(temp(tb), tb, d_sorted, d_uniq, d_counts, (int)R, stream), "dropping equal thresholds");
        hipLaunchKernelGGL(split_keep_kernel, dim3(blocks_of(R + 1)), dim3(256), 0, stream, d_uniq, d_counts, d_run_start, R, n, steps_R, d_keep, d_lb);
        BUILD_TRY(hipGetLastError(), "split_keep_kernel");
        BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_keep, d_kpos, (int)(R + 1), stream), "sizing the split-point sum");
        BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(temp(tb), tb, d_keep, d_kpos, (int)(R + 1), stream), "ranking the split points");
        hipLaunchKernelGGL(split_merge_kernel, dim3(blocks_of(R)), dim3(256), 0, stream, d_uniq, d_counts, d_run_start, R, n, steps_R, d_keep, d_lb,
                           d_kpos, d_seg_start, d_seg_run, d_counts + 1);
        BUILD_TRY(hipGetLastError(), "split_merge_kernel");
        BUILD_TRY(hipMemcpyAsync(&nseg, d_counts + 1, 8, hipMemcpyDeviceToHost, stream), "reading the segment count");
        BUILD_TRY(hipStreamSynchronize(stream), "the split points");
        for (void *p : {(void *)d_sorted, (void *)d_uniq, (void *)d_counts, (void *)d_keep, (void *)d_kpos, (void *)d_lb, (void *)d_run_start})
            pool.release(p);
        if (nseg < R || nseg > 2 * R) { why = "internal error: " + std::to_string(nseg) + " segments from " + std::to_string(R) + " runs"; return MOVI_ERR_INVARIANT; }
        if (nseg > kBuildMaxItems) {
            why = std::to_string(nseg) + " runs after the split at the thresholds: the builder's device scans are 32-bit indexed, at most 2^31 - 2 are served";
            return MOVI_ERR_ARG;
        }
    }
    BUILD_TRY(lap(1), "stage 2");

    // ---- stage 3: rows.  r is read back before the row-sized allocations.  (The host waits for a value four times in a build: the
    // segment count above, r, the count of separator rows in stage 6, the largest blocked id once per round in stage 7.)
    uint64_t r = 0;
    uint64_t *d_pieces = pool.get<uint64_t>(nseg + 1), *d_first_row = pool.get<uint64_t>(nseg + 1);
    BUILD_TRY(pool.err, "allocating the segments");
    hipLaunchKernelGGL(pieces_kernel, dim3(blocks_of(nseg + 1)), dim3(256), 0, stream, d_seg_start, nseg, maxrun, d_pieces);
    BUILD_TRY(hipGetLastError(), "pieces_kernel");
    BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_pieces, d_first_row, (int)(nseg + 1), stream), "sizing the row sum");
    BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(temp(tb), tb, d_pieces, d_first_row, (int)(nseg + 1), stream), "counting the rows");
    BUILD_TRY(hipMemcpyAsync(&r, d_first_row + nseg, 8, hipMemcpyDeviceToHost, stream), "reading the row count");
    BUILD_TRY(hipStreamSynchronize(stream), "the row count");
    pool.release(d_pieces);
    if (d_temp) { pool.release(d_temp); d_temp = nullptr; temp_cap = 0; }
    if (r < nseg) { why = "internal error: " + std::to_string(r) + " rows from " + std::to_string(nseg) + " segments"; return MOVI_ERR_INVARIANT; }
    if (r > kBuildMaxItems) {
        why = std::to_string(r) + " rows: the builder's device scans are 32-bit indexed, at most 2^31 - 2 rows are served";
        return MOVI_ERR_ARG;
    }
    const int steps_r = search_steps(r);
    RowArrays rows;
    rows.all_p = pool.get<uint64_t>(r + 1);
    rows.lens = pool.get<uint16_t>(r);
    rows.code = pool.get<uint8_t>(r);
    rows.row_run = pool.get<uint32_t>(r);
    uint64_t *d_small = pool.get<uint64_t>(40);            // end | end_thr[4] | base intervals [4][6] | blocked max | findings (u32)
    BUILD_TRY(pool.err, "allocating the rows");
    rows.end = d_small;
    uint64_t *d_end_thr = d_small + 1, *d_base = d_small + 5;
    unsigned long long *d_max = reinterpret_cast<unsigned long long *>(d_small + 29);
    uint32_t *d_inside = reinterpret_cast<uint32_t *>(d_small + 30);
    BUILD_TRY(hipMemsetAsync(d_small, 0, 40 * 8, stream), "clearing");
    hipLaunchKernelGGL(rows_kernel, dim3(blocks_of(r)), dim3(256), 0, stream, d_first_row, d_seg_start, d_seg_run, nseg, d_heads, d_code_of, maxrun, r,
                       n, search_steps(nseg), rows);
    BUILD_TRY(hipGetLastError(), "rows_kernel");
    pool.release(d_first_row);
    pool.release(d_seg_start);
    if (d_seg_run) pool.release(d_seg_run);
    pool.release(d_heads);
    BUILD_TRY(lap(2), "stage 3");

    // ---- stages 4 + 5
    Slots *d_sums = pool.get<Slots>(scan_tiles(r));
    uint64_t *d_pp_id = pool.get<uint64_t>(r);
    uint16_t *d_off = pool.get<uint16_t>(r);
    BUILD_TRY(pool.err, "allocating the ids");
    {
        LfScan f;
        f.rows = rows; f.r = r; f.steps = steps_r; f.pp_id = d_pp_id; f.off = d_off;
        uint64_t c = 1;
        for (uint32_t a = 0; a < (uint32_t)kSlots; a++) { f.C[a] = c; c += a < sigma ? info.counts[a] : 0; }
        BUILD_TRY((scan_rows<OpAdd, false>(f, r, d_sums, stream)), "the LF scan");
        Slots counts;
        for (int a = 0; a < kSlots; a++) counts.v[a] = (uint32_t)a < sigma ? info.counts[a] : 0;
        hipLaunchKernelGGL(base_intervals_kernel, dim3(1), dim3(64), 0, stream, rows, r, sigma, counts, steps_r, d_base);
        BUILD_TRY(hipGetLastError(), "base_intervals_kernel");
    }
    BUILD_TRY(lap(3), "stages 4 and 5");

    // ---- stage 6
    uint8_t *d_tbits = nullptr;
    uint16_t *d_sep_thr = nullptr;
    uint64_t *d_sep_map = nullptr;
    uint64_t m = 0;
    if (with_thr) {
        d_tbits = pool.get<uint8_t>(r);
        uint32_t *d_sep_rank = nullptr;
        if (sep) {                                         // the rows of code 0 ('%' and the terminator's), ranked
            d_sep_rank = pool.get<uint32_t>(r + 1);
            BUILD_TRY(pool.err, "allocating the separator ranks");
            hipcub::TransformInputIterator<uint32_t, IsCode0, const uint8_t *> flags(rows.code, IsCode0());
            // (r items and the total from the last rank + the last flag: the code array has no slot to spare)
            BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flags, d_sep_rank, (int)r, stream), "sizing the separator ranks");
            BUILD_TRY(hipcub::DeviceScan::ExclusiveSum(temp(tb), tb, flags, d_sep_rank, (int)r, stream), "ranking the separator rows");
            uint32_t last_rank = 0;
            uint8_t last_code = 0;
            BUILD_TRY(hipMemcpyAsync(&last_rank, d_sep_rank + (r - 1), 4, hipMemcpyDeviceToHost, stream), "reading the separator count");
            BUILD_TRY(hipMemcpyAsync(&last_code, rows.code + (r - 1), 1, hipMemcpyDeviceToHost, stream), "reading the separator count");
            BUILD_TRY(hipStreamSynchronize(stream), "the separator count");
            m = (uint64_t)last_rank + (last_code == 0 ? 1u : 0u);
            d_sep_thr = pool.get<uint16_t>(m * 4);
            d_sep_map = pool.get<uint64_t>(m * 2);
            BUILD_TRY(pool.err, "allocating the separator thresholds");
            if (m) BUILD_TRY(hipMemsetAsync(d_sep_thr, 0, m * 8, stream), "clearing");
        }
        BUILD_TRY(pool.err, "allocating the threshold bits");
        ThrScan f;
        f.rows = rows; f.thr = d_thr; f.n = n; f.sigma = sigma; f.sep = sep; f.tbits = d_tbits; f.end_thr = d_end_thr;
        f.sep_rank = d_sep_rank; f.m = m; f.sep_thr = d_sep_thr; f.sep_map = d_sep_map; f.inside = d_inside;
        BUILD_TRY((scan_rows<OpLast, true>(f, r, d_sums, stream)), "the threshold scan");
        if (d_sep_rank) pool.release(d_sep_rank);
        pool.release(d_thr);
    }
    pool.release(rows.row_run);
    BUILD_TRY(lap(4), "stage 6");

    // ---- stage 7
    uint32_t *d_blocked = nullptr, *d_id_blocks = nullptr;
    uint64_t block_size = mode == 2 ? 1ull << 22 : 1ull << 20, n_blocks = 0;       // move_row_configs.hpp:73 / :102
    // MAX_ALLOWED_BLOCKED_ID, :74 / :103: what the row's id field holds.  The reference sets it anew in every round (:956; the halving at
    // :1051 is lost with the round), so a smaller block is held to the same bound.  (Were the bound halved with the block size, as
    // tools/build_index.cpp restates it, no round after a failed one could pass: a block that exceeds 4 b - 1
    // holds a half that exceeds 2 b - 1.  The two rules give the same bytes on every table the halved rule finishes on: those that need
    // no halving.)
    const uint64_t max_allowed = mode == 2 ? (1ull << 24) - 1 : (1ull << 22) - 1;
    if (blocked_mode) {
        d_blocked = pool.get<uint32_t>(r);
        for (;;) {                                         // halve the block size until the largest distance fits: one scan,
            n_blocks = (r + block_size - 1) / block_size;  // one kernel and one max per round
            d_id_blocks = pool.get<uint32_t>(sigma * n_blocks);
            BUILD_TRY(pool.err, "allocating the id blocks");
            BUILD_TRY(hipMemsetAsync(d_max, 0, 8, stream), "clearing");
            BlockScan f;
            f.rows = rows; f.pp_id = d_pp_id; f.first_runs = d_base; f.sigma = sigma; f.block_size = block_size; f.n_blocks = n_blocks;
            f.id_blocks = d_id_blocks;
            BUILD_TRY((scan_rows<OpLast, false>(f, r, d_sums, stream)), "the id-block scan");
            hipLaunchKernelGGL(blocked_ids_kernel, dim3(blocks_of(r)), dim3(256), 0, stream, rows, r, d_pp_id, d_base, block_size, n_blocks,
                               d_id_blocks, d_blocked, d_max);
            BUILD_TRY(hipGetLastError(), "blocked_ids_kernel");
            unsigned long long mx = 0;
            BUILD_TRY(hipMemcpyAsync(&mx, d_max, 8, hipMemcpyDeviceToHost, stream), "reading the largest blocked id");
            BUILD_TRY(hipStreamSynchronize(stream), "the blocked ids");
            if (mx <= max_allowed) break;
            pool.release(d_id_blocks);
            block_size /= 2;
            if (block_size == 0) { why = "internal error: no block size holds the blocked ids"; return MOVI_ERR_INVARIANT; }
        }
    }
    const uint64_t tally_ck = 20, n_tally = r / tally_ck + 2;                      // movi_options.hpp:257
    uint64_t *d_tally = nullptr;
    if (tally_mode) {
        d_tally = pool.get<uint64_t>(sigma * n_tally);
        BUILD_TRY(pool.err, "allocating the tally table");
        BUILD_TRY(hipMemsetAsync(d_tally, 0, sigma * n_tally * 8, stream), "clearing");   // (r a multiple of 20: entry r / 20 stays 0)
        TallyScan f;
        f.rows = rows; f.pp_id = d_pp_id; f.first_runs = d_base; f.sigma = sigma; f.r = r; f.ck = tally_ck; f.n_tally = n_tally; f.tally = d_tally;
        BUILD_TRY((scan_rows<OpLast, false>(f, r, d_sums, stream)), "the tally scan");
    }
    BUILD_TRY(lap(5), "stage 7");

    // ---- stage 8: pack; the image: header and tables from the host, the rows straight from the device
    const uint64_t row_bytes = (mode == 6 || mode == 3) ? 8 : (blocked_mode ? 6 : 3);
    uint8_t *d_packed = pool.get<uint8_t>(r * row_bytes);
    BUILD_TRY(pool.err, "allocating the packed rows");
    const dim3 grid(blocks_of(r)), block(256);
    switch (mode) {
        case 6: hipLaunchKernelGGL(pack_kernel<6>, grid, block, 0, stream, rows, r, d_pp_id, d_off, d_tbits, d_blocked, d_packed); break;
        case 3: hipLaunchKernelGGL(pack_kernel<3>, grid, block, 0, stream, rows, r, d_pp_id, d_off, d_tbits, d_blocked, d_packed); break;
        case 8: hipLaunchKernelGGL(pack_kernel<8>, grid, block, 0, stream, rows, r, d_pp_id, d_off, d_tbits, d_blocked, d_packed); break;
        case 2: hipLaunchKernelGGL(pack_kernel<2>, grid, block, 0, stream, rows, r, d_pp_id, d_off, d_tbits, d_blocked, d_packed); break;
        case 7: hipLaunchKernelGGL(pack_kernel<7>, grid, block, 0, stream, rows, r, d_pp_id, d_off, d_tbits, d_blocked, d_packed); break;
        default: hipLaunchKernelGGL(pack_kernel<5>, grid, block, 0, stream, rows, r, d_pp_id, d_off, d_tbits, d_blocked, d_packed); break;
    }
    BUILD_TRY(hipGetLastError(), "pack_kernel");
    uint64_t small[40];
    BUILD_TRY(hipMemcpyAsync(small, d_small, sizeof(small), hipMemcpyDeviceToHost, stream), "reading the derived scalars");
    std::vector<uint32_t> id_blocks(blocked_mode ? sigma * n_blocks : 0);
    std::vector<uint64_t> tally(tally_mode ? sigma * n_tally : 0), sep_map(m * 2);
    std::vector<uint16_t> sep_thr(m * 4);
    if (!id_blocks.empty()) BUILD_TRY(hipMemcpyAsync(id_blocks.data(), d_id_blocks, id_blocks.size() * 4, hipMemcpyDeviceToHost, stream), "reading the id blocks");
    if (!tally.empty()) BUILD_TRY(hipMemcpyAsync(tally.data(), d_tally, tally.size() * 8, hipMemcpyDeviceToHost, stream), "reading the tally table");
    if (m) {
        BUILD_TRY(hipMemcpyAsync(sep_thr.data(), d_sep_thr, m * 8, hipMemcpyDeviceToHost, stream), "reading the separator thresholds");
        BUILD_TRY(hipMemcpyAsync(sep_map.data(), d_sep_map, m * 16, hipMemcpyDeviceToHost, stream), "reading the separator map");
    }
    BUILD_TRY(hipStreamSynchronize(stream), "the packed rows");
    uint32_t inside = 0;
    memcpy(&inside, &small[30], 4);
    if (inside) {
        why = "internal error: " + std::to_string(inside) + " threshold(s) strictly inside a row -- the rows are split at every threshold";
        return MOVI_ERR_INVARIANT;
    }
    const uint64_t end_bwt_idx = small[0];

    // serialize, src/move_structure_io.cpp:435-469 (v2 header include/utils.hpp:32-61; its padding bytes are zero here)
    std::vector<uint8_t> head, tail;
    head.resize(48, 0);
    const uint32_t magic = 0x4D4F5649u;
    memcpy(&head[0], &magic, 4);
    head[4] = 2; head[7] = (uint8_t)mode;
    const uint64_t hdr[4] = {n, r, R, end_bwt_idx};
    memcpy(&head[16], hdr, 32);
    for (int i = 0; i < 4; i++) put64(head, small[1 + i]);                          // end_bwt_idx_thresholds
    for (int i = 0; i < 8; i++) put64(head, 0);
    put64(head, 256);
    for (int c = 0; c < 256; c++) {
        uint64_t am = 256;
        for (uint32_t a = 0; a < sigma; a++) if (info.alphabet[a] == c) am = a;
        put64(head, c == 0 ? 256 : am);
    }
    put64(head, sigma);
    for (uint32_t a = 0; a < sigma; a++) head.push_back(info.alphabet[a]);
    head.push_back(0); head.push_back(0); head.push_back(0);                       // u16 nt_splitting, bool constant
    if (tally_mode) {                                                              // write_tally_table, io.cpp:328-336
        for (int b = 0; b < 4; b++) tail.push_back((uint8_t)((uint32_t)tally_ck >> (8 * b)));
        put64(tail, n_tally);
        for (uint64_t v : tally) for (int b = 0; b < 5; b++) tail.push_back((uint8_t)(v >> (8 * b)));   // MoveTally: u32 low | u8 high
    }
    for (int i = 0; i < 3; i++) put64(tail, 0);                                    // overflow tables (empty)
    put64(tail, sigma);
    for (uint32_t a = 0; a < sigma; a++) put64(tail, info.counts[a]);
    put64(tail, sigma + 1);
    const uint64_t *base = small + 5;                                              // first_runs | first_offsets | last_runs | last_offsets
    for (int t : {2, 3, 0, 1})
        for (uint32_t a = 0; a <= sigma; a++) put64(tail, base[t * (kSlots + 1) + a]);
    if (blocked_mode) {
        put64(tail, n_blocks);
        const uint8_t *p = reinterpret_cast<const uint8_t *>(id_blocks.data());
        tail.insert(tail.end(), p, p + id_blocks.size() * 4);
        put64(tail, block_size);
    }
    if (sep && with_thr) {                                                         // write_separators_thresholds, io.cpp:399-413
        put64(tail, m);
        const uint8_t *p = reinterpret_cast<const uint8_t *>(sep_thr.data());
        tail.insert(tail.end(), p, p + m * 8);
        put64(tail, m);
        for (uint64_t v : sep_map) put64(tail, v);
    }
    const size_t total = head.size() + (size_t)(r * row_bytes) + tail.size();
    void *img = nullptr;
    BUILD_TRY(hipHostMalloc(&img, total, hipHostMallocDefault), "allocating the image");
    uint8_t *out = static_cast<uint8_t *>(img);
    memcpy(out, head.data(), head.size());
    memcpy(out + head.size() + r * row_bytes, tail.data(), tail.size());
    hipError_t e = hipMemcpyAsync(out + head.size(), d_packed, r * row_bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipHostFree(img); return hip_fail(e, "copying the rows down", why); }
    (void)lap(6);
    if (profile)
        fprintf(stderr, "[movi build profile] original_r %llu r %llu n %llu | upload+run starts %.6f s, split points %.6f s, rows %.6f s, LF+id/offset %.6f s, "
                        "thresholds %.6f s, compact ids %.6f s, pack+copy down+image %.6f s | peak device bytes %llu (%.1f per row)\n",
                (unsigned long long)R, (unsigned long long)r, (unsigned long long)n, stage_s[0], stage_s[1], stage_s[2], stage_s[3], stage_s[4], stage_s[5],
                stage_s[6], (unsigned long long)pool.peak, (double)pool.peak / (double)r);
    *h_image = img;
    *image_bytes = total;
    return MOVI_OK;
}

}  // namespace movi
