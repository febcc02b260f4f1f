// movi_lists.hpp -- a lane's strided list of items: what the list-owning kernels share (locate_kernel, hits_walk_kernel,
// hits_interval_kernel, kmer_occ_kernel, color_walk_kernel).  Blocks are one wavefront wide; a lane owns the items lane, lane + stride,
// ... (stride = the launch's lanes) and takes up its next item in the iteration after one ends: no cross-lane traffic, and all lanes
// stay busy until the lists run out although the items' lengths differ widely.  The launch is launch_lane_lists (movi_search.hpp).
#pragma once
#include "movi_device.hpp"

namespace movi {

struct LaneList {
    uint64_t item, stride, n;
    uint32_t state;                                       // 0 = list done, 1 = take up `item`, 2 = busy on it
    __device__ __forceinline__ explicit LaneList(uint64_t n_items)
        : item((uint64_t)blockIdx.x * 64u + threadIdx.x), stride((uint64_t)gridDim.x * 64u), n(n_items), state(item < n_items ? 1u : 0u) {}
    __device__ __forceinline__ bool any() const { return wave_any(state != 0u); }     // the loop's condition: wave-uniform
    __device__ __forceinline__ void next() {              // `item` is over: on to the lane's next one, or done
        item += stride;
        state = item < n ? 1u : 0u;
    }
};

// The lane's counters to DevStats (may be null), one atomic per wavefront and counter; errs = items of the lane that failed.  The
// fast-forwards and the steps are summed in 64 bits: a lane's list holds many items, and 64 lanes of long walks pass 2^32.
__device__ __forceinline__ void flush_list_stats(DevStats *stats, uint32_t ff_total, uint32_t scan_total, uint32_t errs, uint64_t lane_steps,
                                                 uint64_t wave_steps) {
    const uint32_t scw = wave_sum(scan_total), erw = wave_sum(errs);
    unsigned long long ffw = ff_total, lsw = lane_steps;
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

}  // namespace movi
