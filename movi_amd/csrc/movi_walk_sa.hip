// movi_walk_sa.hip -- locate: suffix-array entries from a sampled suffix array.
//   locate_kernel      MoveStructure::get_SA_entries (src/move_structure.cpp:35-48): from a BWT position, LF steps until a position that is a
//                      multiple of the sample rate; the answer is that sample + the steps taken.  In "successor" mode the same walk, one
//                      LF step taken first, links every sampled position to the next one down the text: the builder's list.
//   sa_pos_kernel      the PML walk (MoveStructure::query_pml, src/move_structure_query.cpp:266-361) that also records where it stands
//                      after every base -- the positions get_SA_entries is called on (:354-357).
//   build_sampled_sa   find_sampled_SA_entries (src/move_structure_build.cpp:1174-1212) without its n sequential LF steps: the list of
//                      the sampled positions, ranked by pointer jumping.
// The contract is stated in include/movi_hip.h (movi_locate_device, movi_sa_entries_device, movi_ssa_build); the locate rows and the
// packed positions in movi_sa.hpp.
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"
#include "movi_sa.hpp"

#include <hipcub/hipcub.hpp>

namespace movi {

// ------------------------------------------------------------------------------------------------ locate
// locate_walk (movi_sa.hpp) over the n_items positions of `pos`, the count known to the host.
//   a.succ == 0   pos[item] = samples[s] + distance, NOT reduced modulo n: a walk that passes text position 0 stops at BWT position 0
//                 (sample 0 = n - 1) and returns entry + n, as the reference does;
//   a.succ == 1   one LF step first; pos[item] = s, a.aux[item] = distance (0 where the walk failed).
// An item that is kPosNone stays; one that is not a position of the table, or whose walk breaks an invariant of the table (the
// reference's throws; more than n steps), becomes kPosNone and is counted in DevStats::errors.
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void locate_kernel(DevIndex ix, LocArgs a, uint64_t *__restrict__ pos, uint64_t n_items, DevStats *stats) {
    locate_walk<MODE, IdxT>(ix, a, pos, n_items, stats,
        [&](uint64_t item, uint64_t s, uint64_t dist) {
            if (s >= a.n_entries) { pos[item] = kPosNone; return false; }
            if (a.succ) { pos[item] = s; a.aux[item] = dist; }
            else pos[item] = a.samples[s] + dist;
            return true;
        },
        [&](uint64_t item) {
            pos[item] = kPosNone;
            if (a.succ) a.aux[item] = 0;
        });
}

namespace {
struct LocateFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &locate_kernel<MODE, IdxT>; }
};
}  // namespace

hipError_t launch_locate(int mode, const DevIndex &ix, const LocArgs &a, uint64_t *d_pos, uint64_t n_items, DevStats *d_stats,
                         int num_cus, hipStream_t stream, LaunchInfo *info) {
    if (n_items == 0) return hipSuccess;
    if ((mode != 6 && mode != 3) || a.rate == 0u || !a.rows) return hipErrorInvalidValue;
    return launch_lane_lists<LocateFamily>("locate_kernel", a.succ ? 1 : 0, mode, ix, n_items, kLocateWaves, num_cus, stream, info, a, d_pos,
                                           n_items, d_stats);
}

// ------------------------------------------------------------------------------------------------ the position walk
// One lane per read, base-synchronous: pml_kernel<6, 0>'s automaton (walk_base), which besides the u16 PML writes the packed position
// the walk stands at AFTER process_char and BEFORE the LF step of every base -- illegal bases included: the state is unchanged there and
// the reference still records an entry.  Emission order: slot offs[i] + k belongs to base len - 1 - k.  No top-of-walk table, which
// would skip the first states.  A read that hits one of the reference's throws reports kPosNone in every slot, all-zero PMLs and its code.
// (About 1 % of a locate at rate 100: kept simple.)
template <typename IdxT>
__global__ __launch_bounds__(64) void sa_pos_kernel(DevIndex ix, const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offs,
                                                    uint64_t n_reads, uint16_t *__restrict__ pml, uint64_t *__restrict__ pos,
                                                    uint8_t *__restrict__ err, DevStats *stats, const uint32_t *__restrict__ order) {
    __shared__ uint8_t s_code[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = t < n_reads;
    const uint64_t rid = (valid && order) ? order[t] : t;
    const uint64_t beg = valid ? offs[rid] : 0;
    const uint64_t len = valid ? offs[rid + 1] - beg : 0;
    const uint8_t *R = bases + beg;
    const EndThr ethr = end_thresholds(ix);
    uint32_t ff_total = 0, scan_total = 0, repo_total = 0, failed = 0;
    IdxT kidx = (IdxT)(ix.r - 1);                            // ReadProcessor::reset_process, src/read_processor.cpp:69-70
    uint2 row = load_row<6>(ix.rows, ix.r - 1);
    uint32_t off = row_n<6>(row) - 1, ml = 0;
    for (uint64_t k = 0; wave_any(k < len && failed == 0u); ++k) {
        const bool live = k < len && failed == 0u;
        const uint32_t a = live ? (uint32_t)s_code[R[len - 1 - k]] : 0xFFu;
        uint64_t idx = kidx;
        const uint32_t e = walk_base<6>(ix, ethr, live, k != 0, a, idx, off, row, ml, ff_total, scan_total, repo_total);
        kidx = (IdxT)idx;
        if (e) failed = e;
        else if (live) {
            if (pml) pml[beg + k] = (uint16_t)(ml > 65535u ? 65535u : ml);
            pos[beg + k] = pos_pack(idx, off);
        }
    }
    if (failed) {
        for (uint64_t k = 0; k < len; ++k) {
            if (pml) pml[beg + k] = 0;
            pos[beg + k] = kPosNone;
        }
    }
    if (valid && err) err[rid] = (uint8_t)failed;
    const uint32_t ffw = wave_sum(ff_total), scw = wave_sum(scan_total), rpw = wave_sum(repo_total), erw = wave_sum(failed ? 1u : 0u);
    if ((threadIdx.x & 63) == 0 && stats) {
        if (ffw) atomicAdd(&stats->fast_forwards, (unsigned long long)ffw);
        if (scw) atomicAdd(&stats->scans, (unsigned long long)scw);
        if (rpw) atomicAdd(&stats->repositions, (unsigned long long)rpw);
        if (erw) atomicAdd(&stats->errors, (unsigned long long)erw);
    }
}

hipError_t launch_sa_pos(const DevIndex &ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint16_t *d_pml,
                         uint64_t *d_pos, uint8_t *d_err, DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info) {
    if (n_reads == 0) return hipSuccess;
    const uint64_t blocks = (n_reads + 63) / 64;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    char nm[96];
    snprintf(nm, sizeof(nm), "sa_pos_kernel<%s>", ix.idx32 ? "unsigned int" : "unsigned long");
    note_walk_launch(nm);
    if (info) {
        *info = LaunchInfo();
        snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
        info->variant = 0; info->block_threads = 64; info->idx64 = ix.idx32 ? 0 : 1;
    }
    if (ix.idx32)
        hipLaunchKernelGGL(sa_pos_kernel<uint32_t>, dim3((unsigned)blocks), dim3(64), 0, stream, ix, d_bases, d_offsets, n_reads, d_pml, d_pos,
                           d_err, d_stats, d_order);
    else
        hipLaunchKernelGGL(sa_pos_kernel<uint64_t>, dim3((unsigned)blocks), dim3(64), 0, stream, ix, d_bases, d_offsets, n_reads, d_pml, d_pos,
                           d_err, d_stats, d_order);
    return hipGetLastError();
}

hipError_t preload_sa(int mode, bool idx32) {
    hipFuncAttributes at;
    hipError_t e = preload_family<LocateFamily>(mode, idx32);
    if (e == hipSuccess && mode == 6)
        e = hipFuncGetAttributes(&at, idx32 ? (const void *)sa_pos_kernel<uint32_t> : (const void *)sa_pos_kernel<uint64_t>);
    return e;
}

// ------------------------------------------------------------------------------------------------ the locate rows
namespace {

template <int MODE>
__global__ __launch_bounds__(256) void row_len_kernel(const uint8_t *__restrict__ rows, uint64_t r, uint64_t *__restrict__ lens) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < r) lens[i] = row_n<MODE>(load_row<MODE>(rows, i));
}

__global__ __launch_bounds__(256) void loc_rows_kernel(const uint8_t *__restrict__ rows, uint64_t r, const uint64_t *__restrict__ all_p,
                                                       uint64_t rate, uint4 *__restrict__ loc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < r) loc[i] = loc_make(load_row<6>(rows, i), all_p[i], rate);      // (the 8 bytes as they are: modes 6 and 3 alike)
}

// all_p back out of the locate rows (movi_ssa_save)
__global__ __launch_bounds__(256) void loc_all_p_kernel(const uint4 *__restrict__ loc, uint64_t first, uint64_t cnt, uint64_t rate,
                                                        uint64_t *__restrict__ all_p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) { const uint4 v = loc[first + i]; all_p[i] = loc_quot(v) * rate + loc_rem(v); }
}

// P[m] = the packed position of BWT position m * rate, m < n_samples: every row writes the multiples of rate it holds
template <int MODE>
__global__ __launch_bounds__(256) void sample_pos_kernel(const uint4 *__restrict__ loc, uint64_t r, uint32_t rate, uint64_t n_samples,
                                                         uint64_t *__restrict__ P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r) return;
    const uint4 v = loc[i];
    const uint32_t n = row_n<MODE>(loc_row(v)), rem = loc_rem(v);
    uint64_t m = loc_quot(v) + (rem ? 1u : 0u);
    for (uint32_t o = rem ? rate - rem : 0u; o < n; o += rate, ++m)
        if (m < n_samples) P[m] = pos_pack(i, o);
}

// ---- ranking the list of the samples.  next[j] / dist[j]: the sample that follows j down the text and how far.  LF is one cycle over the
// n BWT positions, so the samples form one cycle through sample 0 (= n - 1, the text's last position); it is cut in front of sample 0 --
// the node whose successor is 0 becomes the tail, a self-loop of length 0 -- and pointer jumping over (next, dist, hops), double-buffered,
// gives every node its distance and its number of hops to the tail.  bad[0] counts what a single cycle over all samples cannot produce.
struct ListNode { uint64_t next, dist, hops; };

__global__ __launch_bounds__(256) void list_init_kernel(const uint64_t *__restrict__ next, const uint64_t *__restrict__ dist, uint64_t m,
                                                        ListNode *__restrict__ out, unsigned long long *__restrict__ tail, uint32_t *__restrict__ bad) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    ListNode nd{next[j], dist[j], 1};
    if (nd.next >= m) { atomicAdd(bad, 1u); nd.next = j; nd.dist = 0; nd.hops = 0; }     // (kPosNone of a failed walk lands here too)
    else if (nd.next == 0) {
        tail[0] = j;                                       // exactly one, or tail[1] says otherwise
        tail[2] = nd.dist;                                 // the cut edge's length: the cycle's lengths must add up to n
        atomicAdd(&tail[1], 1ull);
        nd.next = j; nd.dist = 0; nd.hops = 0;
    }
    out[j] = nd;
}

__global__ __launch_bounds__(256) void list_jump_kernel(const ListNode *__restrict__ in, uint64_t m, ListNode *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const ListNode a = in[j], b = in[a.next];
    out[j] = ListNode{b.next, a.dist + b.dist, a.hops + b.hops};
}

// sample[j] = n - 1 - (distance from sample 0 to j); the hops to the tail must be a permutation of 0 .. m - 1
__global__ __launch_bounds__(256) void list_final_kernel(const ListNode *__restrict__ in, uint64_t m, uint64_t n, const unsigned long long *__restrict__ tail,
                                                         uint32_t *__restrict__ seen, uint64_t *__restrict__ samples, uint32_t *__restrict__ bad) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const ListNode nd = in[j], head = in[0];
    const bool ok = tail[1] == 1ull && nd.next == tail[0] && nd.hops < m && nd.dist <= head.dist && head.dist + tail[2] == n;
    if (!ok || atomicAdd(&seen[nd.hops], 1u) != 0u) { atomicAdd(bad, 1u); return; }
    samples[j] = n - 1 - (head.dist - nd.dist);
}

unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

uint64_t locate_rows_bytes(uint64_t r) { return r * 16; }

hipError_t build_locate_rows(int mode, const DevIndex &ix, uint64_t rate, uint4 *d_loc, uint64_t *n_total, hipStream_t stream) {
    if ((mode != 6 && mode != 3) || rate == 0 || rate > (1ull << kLocRemBits) || ix.r > 0x7FFFFFFFull * 256) return hipErrorInvalidValue;
    const uint64_t r = ix.r;
    DevPtr<uint64_t> len, allp;
    DevPtr<void> temp;
    size_t temp_bytes = 0;
    hipError_t e = dev_alloc(len, (r + 1) * 8);
    if (e == hipSuccess) e = dev_alloc(allp, (r + 1) * 8);
    uint64_t *d_len = len.get(), *d_allp = allp.get();
    if (e == hipSuccess) e = hipMemsetAsync(d_len + r, 0, 8, stream);
    if (e == hipSuccess) {
        if (mode == 6) hipLaunchKernelGGL(row_len_kernel<6>, dim3(blocks_of(r)), dim3(256), 0, stream, ix.rows, r, d_len);
        else hipLaunchKernelGGL(row_len_kernel<3>, dim3(blocks_of(r)), dim3(256), 0, stream, ix.rows, r, d_len);
        e = hipGetLastError();
    }
    if (e == hipSuccess && r + 1 > 0x7FFFFFFFull) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, d_len, d_allp, (int)(r + 1), stream);
    if (e == hipSuccess) e = dev_alloc(temp, temp_bytes ? temp_bytes : 8);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(temp.get(), temp_bytes, d_len, d_allp, (int)(r + 1), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(loc_rows_kernel, dim3(blocks_of(r)), dim3(256), 0, stream, ix.rows, r, d_allp, rate, d_loc);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_total) e = hipMemcpyAsync(n_total, d_allp + r, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
}

hipError_t locate_rows_all_p(const uint4 *d_loc, uint64_t first, uint64_t cnt, uint64_t rate, uint64_t *d_all_p, hipStream_t stream) {
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(loc_all_p_kernel, dim3(blocks_of(cnt)), dim3(256), 0, stream, d_loc, first, cnt, rate, d_all_p);
    return hipGetLastError();
}

hipError_t launch_sample_positions(int mode, const DevIndex &ix, const LocArgs &loc, uint64_t n_samples, uint64_t *d_pos, hipStream_t stream) {
    if ((mode != 6 && mode != 3) || loc.rate == 0u || !loc.rows || ix.r > 0x7FFFFFFFull * 256) return hipErrorInvalidValue;
    if (mode == 6) hipLaunchKernelGGL(sample_pos_kernel<6>, dim3(blocks_of(ix.r)), dim3(256), 0, stream, loc.rows, ix.r, loc.rate, n_samples, d_pos);
    else hipLaunchKernelGGL(sample_pos_kernel<3>, dim3(blocks_of(ix.r)), dim3(256), 0, stream, loc.rows, ix.r, loc.rate, n_samples, d_pos);
    return hipGetLastError();
}

hipError_t build_sampled_sa(int mode, const DevIndex &ix, const LocArgs &loc, uint64_t *d_samples, DevStats *d_stats, int num_cus,
                            hipStream_t stream, uint32_t *bad_out, LaunchInfo *info) {
    const uint64_t n = loc.n, rate = loc.rate, m = (n + rate - 1) / rate, entries = n / rate + 1;
    *bad_out = 0;
    if (m == 0 || m > 0x7FFFFFFFull * 256) return hipErrorInvalidValue;
    DevPtr<uint64_t> next, dist;
    DevPtr<ListNode> la, lb;
    DevPtr<unsigned long long> tail;                       // tail node, tails found, the cut edge's length | then bad (u32)
    DevPtr<uint32_t> seen;
    hipError_t e = dev_alloc(next, m * 8);
    if (e == hipSuccess) e = dev_alloc(dist, m * 8);
    if (e == hipSuccess) e = dev_alloc(la, m * sizeof(ListNode));
    if (e == hipSuccess) e = dev_alloc(lb, m * sizeof(ListNode));
    if (e == hipSuccess) e = dev_alloc(tail, 32);
    if (e == hipSuccess) e = dev_alloc(seen, m * 4);
    uint64_t *d_next = next.get(), *d_dist = dist.get();
    ListNode *d_a = la.get(), *d_b = lb.get();
    unsigned long long *d_tail = tail.get();
    uint32_t *d_seen = seen.get();
    uint32_t *d_bad = d_tail ? reinterpret_cast<uint32_t *>(d_tail + 3) : nullptr;
    if (e == hipSuccess) e = hipMemsetAsync(d_tail, 0, 32, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_seen, 0, m * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_next, 0xFF, m * 8, stream);        // a sample no row holds stays kPosNone: counted by the walk
    if (e == hipSuccess) e = hipMemsetAsync(d_dist, 0, m * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_samples, 0, entries * 8, stream);  // (where rate divides n the last entry addresses no position: 0)
    if (e == hipSuccess) {
        if (mode == 6) hipLaunchKernelGGL(sample_pos_kernel<6>, dim3(blocks_of(ix.r)), dim3(256), 0, stream, loc.rows, ix.r, loc.rate, m, d_next);
        else hipLaunchKernelGGL(sample_pos_kernel<3>, dim3(blocks_of(ix.r)), dim3(256), 0, stream, loc.rows, ix.r, loc.rate, m, d_next);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        LocArgs a = loc;
        a.succ = 1;
        a.aux = d_dist;
        a.samples = nullptr;
        a.n_entries = m;
        e = launch_locate(mode, ix, a, d_next, m, d_stats, num_cus, stream, info);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(list_init_kernel, dim3(blocks_of(m)), dim3(256), 0, stream, d_next, d_dist, m, d_a, d_tail, d_bad);
        e = hipGetLastError();
    }
    for (uint64_t span = 1; e == hipSuccess && span < m; span <<= 1) {           // ceil(log2(m)) rounds
        hipLaunchKernelGGL(list_jump_kernel, dim3(blocks_of(m)), dim3(256), 0, stream, d_a, m, d_b);
        e = hipGetLastError();
        std::swap(d_a, d_b);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(list_final_kernel, dim3(blocks_of(m)), dim3(256), 0, stream, d_a, m, n, d_tail, d_seen, d_samples, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad_out, d_bad, 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
}

}  // namespace movi
