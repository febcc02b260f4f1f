// movi_walk_text.hip -- run heads, run lengths and thresholds from a text, on the GPU: what the reference's external pipeline
// (prepare_ref + pfp-thresholds, src/movi_launcher.cpp:190-242) and the host constructor (tools/build_index.cpp: SA-IS, Kasai,
// leftmost-minimum thresholds) hand to MoveStructure::build().  The contract is in include/movi_hip.h (movi_rlbwt_from_text); the
// stages, as DESIGN.md "Build from a text" lists them:
//   1  suffix array   prefix doubling: a radix sort (hipcub) of one 64-bit key per suffix and round -- the first round's key is the
//                     suffix's first 8 characters, a later one (rank[i], rank[i + h]) --, boundary flags and their sum = the new
//                     ranks, a scatter = the inverse; until all N ranks differ.  Every round sorts all N suffixes (no filter for
//                     the ones that are unique already: DESIGN.md section 8).
//   2  BWT and runs   bwt[t] = text[sa[t] - 1]; the run starts by a select (hipcub), the heads by a gather
//   3  LCP            Kasai's algorithm, a lane per `chunk` neighbouring text positions (lcp_kernel)
//   4  thresholds     the leftmost (minimum, position) of the LCP per run, then per character of the alphabet one segmented-minimum
//                     scan over the runs (hipcub) that restarts after every run of that character
//   5  verify         (option) the suffix array against the text and its inverse, the LCP at 4096 sampled positions
// Positions, ranks and LCP values are 32 bits: N = n + 1 <= 2^32 - 2^20 + 1 (movi_text.hpp).
// (Named into the movi_walk*.hip family for the reason movi_walk_build.hip gives.)
#include "movi_text.hpp"

#include "../../include/movi_hip.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <vector>

namespace movi {

namespace {

unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }
int bit_length(uint64_t n) {
    int s = 0;
    while (n) { s++; n >>= 1; }
    return s;
}

// the 8 bytes at text position p, first character in the low byte; w = the padded text as words (text_padded_bytes)
__device__ __forceinline__ uint64_t window8(const uint64_t *__restrict__ w, uint64_t p) {
    const uint64_t lo = w[p >> 3], hi = w[(p >> 3) + 1];
    const uint32_t s = (uint32_t)(p & 7u) * 8u;
    return s ? (lo >> s) | (hi << (64u - s)) : lo;
}

// ------------------------------------------------------------------------------------------------ stage 1: the suffix array
// The first round's key: 8 characters, the first one in the top byte.  The zeros behind the terminator order a suffix that ends
// within the window before every longer one, and no two suffixes share a key that holds the terminator.
__global__ __launch_bounds__(256) void first_keys_kernel(const uint64_t *__restrict__ w, uint64_t N, uint64_t *__restrict__ keys,
                                                         uint32_t *__restrict__ sa) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    keys[i] = __builtin_bswap64(window8(w, i));
    sa[i] = (uint32_t)i;
}

// A later round's key for the suffix at sa[t]: its rank, then the rank + 1 of the suffix h further on (0 past the end), nb bits each.
__global__ __launch_bounds__(256) void rank_keys_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ rank, uint64_t h, uint64_t N,
                                                        int nb, uint64_t *__restrict__ keys) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const uint64_t i = sa[t];
    const uint64_t second = i + h < N ? (uint64_t)rank[i + h] + 1 : 0;
    keys[t] = ((uint64_t)rank[i] << nb) | second;
}

struct KeyChanged {                                      // 1 where a new group of equal keys starts (not at t = 0: ranks count from 0)
    const uint64_t *keys;
    __host__ __device__ __forceinline__ uint32_t operator()(const uint64_t &t) const { return t != 0 && keys[t] != keys[t - 1] ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void scatter_ranks_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ dense, uint64_t N,
                                                            uint32_t *__restrict__ rank) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) rank[sa[t]] = dense[t];                   // sa is a permutation of 0 .. N - 1 in every round: the sort moves the values only
}

// ------------------------------------------------------------------------------------------------ stage 2: BWT and runs
__global__ __launch_bounds__(256) void bwt_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa, uint64_t N, uint8_t *__restrict__ bwt) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const uint32_t p = sa[t];
    bwt[t] = p ? text[p - 1] : (uint8_t)0;
}

struct IsRunHead {
    const uint8_t *bwt;
    __host__ __device__ __forceinline__ bool operator()(const uint64_t &t) const { return t == 0 || bwt[t] != bwt[t - 1]; }
};

__global__ __launch_bounds__(256) void heads_kernel(const uint8_t *__restrict__ bwt, uint32_t *__restrict__ run_start, uint64_t R, uint64_t N,
                                                    uint8_t *__restrict__ heads) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < R) heads[k] = bwt[run_start[k]];
    else if (k == R) run_start[R] = (uint32_t)N;         // (N < 2^32)
}

// ------------------------------------------------------------------------------------------------ stage 3: LCP
// Kasai's algorithm cut into chunks of the text: a lane owns `chunk` neighbouring positions, starts the first at h = 0 and carries
// h - 1 to the next.  Position i: r = isa[i], j = sa[r - 1], h grows while the windows at i + h and j + h are equal, lcp[r] = h.
// The two suffixes differ at the latest where the shorter one's terminator stands (the text holds no other 0), so no window starts
// past position N - 1; the bound below holds a damaged array to that too.  Per lane at most chunk + the longest repeat / 8 trips.
// One-wavefront blocks and a wave-uniform loop, predicated per lane (the control-flow note of movi_device.hpp).
__global__ __launch_bounds__(64) void lcp_kernel(const uint64_t *__restrict__ w, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ isa,
                                                 uint64_t N, uint32_t chunk, uint32_t *__restrict__ lcp) {
    const uint64_t lane = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    uint64_t i = lane * chunk;
    const uint64_t end = i + chunk < N ? i + chunk : N;
    uint32_t state = i < N ? 1u : 0u;                    // 0 = done, 1 = take up position i, 2 = comparing
    uint64_t h = 0, j = 0;
    uint32_t r = 0;
    while (__ballot(state != 0u) != 0ull) {
        if (state == 1u) {
            r = isa[i];
            if (r == 0u || r >= N) {                     // the smallest suffix has no neighbour above
                if (r == 0u) lcp[0] = 0u;
                h = 0;
                i += 1;
                state = i < end ? 1u : 0u;
            } else {
                j = sa[r - 1u];
                state = 2u;
            }
        }
        if (state == 2u) {
            const bool inside = i + h < N && j + h < N;
            const uint64_t x = inside ? window8(w, i + h) ^ window8(w, j + h) : 1ull;
            if (x == 0ull) {
                h += 8;
            } else {
                h += (uint64_t)((__ffsll((unsigned long long)x) - 1) >> 3);
                lcp[r] = (uint32_t)h;
                h = h ? h - 1 : 0;
                i += 1;
                state = i < end ? 1u : 0u;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ stage 4: thresholds
// A (value, position) pair as one integer: the smaller integer is the smaller LCP value and, among equals, the leftmost position.
constexpr uint64_t kNoMin = ~0ull;                       // (no LCP value is 2^32 - 1)
constexpr uint32_t kLongRun = 256;
__device__ __forceinline__ uint64_t lcp_at(const uint32_t *__restrict__ lcp, uint64_t t) { return ((uint64_t)lcp[t] << 32) | t; }

// The minimum over every run: a lane per run; a run longer than kLongRun goes on a list for long_run_min_kernel.
__global__ __launch_bounds__(256) void run_min_kernel(const uint32_t *__restrict__ lcp, const uint32_t *__restrict__ run_start, uint64_t R,
                                                      uint64_t *__restrict__ run_min, uint32_t *__restrict__ long_runs, uint32_t long_cap,
                                                      uint32_t *__restrict__ n_long) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= R) return;
    const uint64_t s = run_start[k], e = run_start[k + 1];
    uint64_t m = kNoMin;
    if (e - s > kLongRun) {
        const uint32_t q = atomicAdd(n_long, 1u);
        if (q < long_cap) long_runs[q] = (uint32_t)k;    // (cap = N / kLongRun + 1 holds them all)
    } else {
        for (uint64_t t = s; t < e; t++) {
            const uint64_t v = lcp_at(lcp, t);
            m = v < m ? v : m;
        }
    }
    run_min[k] = m;
}
__global__ __launch_bounds__(64) void long_run_min_kernel(const uint32_t *__restrict__ lcp, const uint32_t *__restrict__ run_start,
                                                          const uint32_t *__restrict__ long_runs, const uint32_t *__restrict__ n_long,
                                                          uint32_t long_cap, uint64_t *__restrict__ run_min) {
    const uint32_t count = *n_long < long_cap ? *n_long : long_cap;
    for (uint32_t q = blockIdx.x; q < count; q += gridDim.x) {           // a wavefront per run
        const uint32_t k = long_runs[q];
        const uint64_t s = run_start[k], e = run_start[k + 1];
        unsigned long long m = kNoMin;
        for (uint64_t t = s + threadIdx.x; t < e; t += 64u) {
            const uint64_t v = lcp_at(lcp, t);
            m = v < m ? v : m;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(m, d, 64);
            m = o < m ? o : m;
        }
        if (threadIdx.x == 0) run_min[k] = m;
    }
}

// The scan for character c.  A run contributes its minimum, a run of c restarts; the state BEFORE run k is then the minimum over
// the runs since the last run of c, and whether there was one.  thr[k] = the position in min(that state, the LCP at run k's first
// position) -- lcp[e + 1 .. s] of pfp-thresholds' .thr_pos, tools/build_index.cpp:186-203 --, 0 where c has not occurred before.
struct Seg { uint64_t key, restart; };
struct SegJoin {                                         // a, then b
    __host__ __device__ __forceinline__ Seg operator()(const Seg &a, const Seg &b) const {
        return b.restart ? b : Seg{a.key < b.key ? a.key : b.key, a.restart};
    }
};
struct SegOfRun {
    const uint8_t *heads;
    const uint64_t *run_min;
    uint8_t c;
    __host__ __device__ __forceinline__ Seg operator()(const uint64_t &k) const { return heads[k] == c ? Seg{kNoMin, 1ull} : Seg{run_min[k], 0ull}; }
};
// Where the scan's states go: nowhere but into the thresholds of c's runs (the states themselves, 16 bytes per run, are never held).
struct ThrSink {
    const uint8_t *heads;
    const uint32_t *run_start, *lcp;
    uint32_t *thr;
    uint8_t c;
    __device__ __forceinline__ void put(uint64_t k, const Seg &before) const {
        if (heads[k] != c) return;
        const uint64_t head = lcp_at(lcp, run_start[k]), m = before.key < head ? before.key : head;
        thr[k] = before.restart ? (uint32_t)m : 0u;
    }
};
struct ThrRef {
    ThrSink sink;
    uint64_t k;
    __device__ __forceinline__ const ThrRef &operator=(const Seg &s) const { sink.put(k, s); return *this; }
};
struct ThrOut {
    using iterator_category = std::random_access_iterator_tag;
    using value_type = Seg;
    using difference_type = ptrdiff_t;
    using pointer = Seg *;
    using reference = ThrRef;
    ThrSink sink;
    uint64_t k;
    __host__ __device__ __forceinline__ ThrRef operator*() const { return ThrRef{sink, k}; }
    __host__ __device__ __forceinline__ ThrRef operator[](ptrdiff_t d) const { return ThrRef{sink, k + (uint64_t)d}; }
    __host__ __device__ __forceinline__ ThrOut operator+(ptrdiff_t d) const { return ThrOut{sink, k + (uint64_t)d}; }
    __host__ __device__ __forceinline__ ThrOut operator-(ptrdiff_t d) const { return ThrOut{sink, k - (uint64_t)d}; }
    __host__ __device__ __forceinline__ ThrOut &operator+=(ptrdiff_t d) { k += (uint64_t)d; return *this; }
    __host__ __device__ __forceinline__ ThrOut &operator++() { k += 1; return *this; }
    __host__ __device__ __forceinline__ ThrOut operator++(int) { ThrOut o = *this; k += 1; return o; }
};

// ------------------------------------------------------------------------------------------------ stage 5: verify
// bad[0]: sa is no permutation of 0 .. N - 1, or isa is not its inverse; bad[1]: two neighbouring suffixes out of order -- by their
// first characters, or, those being equal, by the ranks of the suffixes one further on (with [0] clean that is the whole order, by
// induction over the text from its end); bad[2]: the LCP at a sampled position is not what a direct comparison gives.
__global__ __launch_bounds__(256) void verify_sa_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ isa,
                                                        uint64_t N, uint32_t *__restrict__ seen, uint32_t *__restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const uint64_t a = sa[t];
    if (a >= N) { atomicAdd(&bad[0], 1u); return; }
    const uint32_t bit = 1u << (a & 31u);
    if ((atomicOr(&seen[a >> 5], bit) & bit) || isa[a] != t) atomicAdd(&bad[0], 1u);
    if (t == 0) return;
    const uint64_t b = sa[t - 1];
    if (b >= N) return;                                  // (counted by its own thread)
    const uint8_t ca = text[a], cb = text[b];
    bool ok = cb <= ca;
    if (cb == ca) ok = a + 1 < N && b + 1 < N && isa[b + 1] < isa[a + 1];
    if (!ok) atomicAdd(&bad[1], 1u);
}

constexpr uint32_t kVerifySamples = 4096;
__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(64) void verify_lcp_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ lcp,
                                                        uint64_t N, uint64_t seed, uint32_t *__restrict__ bad) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= kVerifySamples || N < 2) return;
    const uint64_t r = 1 + mix64(seed + (uint64_t)q * 0x9E3779B97F4A7C15ull) % (N - 1);
    const uint64_t i = sa[r], j = sa[r - 1];
    uint64_t h = 0;
    while (i + h < N && j + h < N && text[i + h] == text[j + h]) h++;       // a byte at a time: this is the check, not the pass
    if (i >= N || j >= N || i == j || h != lcp[r]) atomicAdd(&bad[2], 1u);
}

// ------------------------------------------------------------------------------------------------ the host side
// Device memory of one build: freed on every return path; counts what is held.
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

// Page-locked host arrays of one call: handed to the caller only when everything succeeded.
struct HostOut {
    void *p[3] = {nullptr, nullptr, nullptr};
    ~HostOut() { for (void *q : p) if (q) (void)hipHostFree(q); }
};

int hip_fail(hipError_t e, const char *what, std::string &why) {
    why = std::string(what) + ": " + hipGetErrorString(e) + " (hipError " + std::to_string((int)e) + ")";
    (void)hipGetLastError();
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? MOVI_ERR_NO_DEVICE : MOVI_ERR_HIP;
}

#define TEXT_TRY(expr, what)                                        \
    do {                                                            \
        hipError_t e_ = (expr);                                     \
        if (e_ == hipSuccess) e_ = pool.err;                        \
        if (e_ != hipSuccess) return hip_fail(e_, what, why);       \
    } while (0)

}  // namespace

int rlbwt_from_text(const uint8_t *h_text, uint64_t n, bool with_thr, uint32_t lcp_chunk, bool verify, uint64_t max_device_bytes,
                    uint8_t **h_heads, uint64_t **h_lens, uint64_t **h_thr, uint64_t *original_r, TextBuildStats &stats, std::string &why) {
    const uint64_t N = n + 1;
    const int nb = bit_length(N);
    stats = TextBuildStats();
    stats.n_positions = N;
    hipStream_t stream = nullptr;

    // ---- the plan against the memory, before the first allocation
    const uint64_t need = text_device_bytes(N);
    uint64_t avail = max_device_bytes;
    if (!avail) {
        size_t free_b = 0, total_b = 0;
        const hipError_t e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess) return hip_fail(e, "asking for the free device memory", why);
        avail = free_b;
    }
    if (need > avail) {
        why = "the build of " + std::to_string(N) + " BWT positions needs " + std::to_string(need) + " device bytes, " + std::to_string(avail) +
              (max_device_bytes ? " are allowed (max_device_bytes)" : " are free on the device");
        return MOVI_ERR_ARG;
    }

    DevPool pool;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](int k) -> hipError_t {
        const hipError_t e = hipStreamSynchronize(stream);
        const auto t = std::chrono::steady_clock::now();
        stats.seconds[k] += std::chrono::duration<double>(t - t_last).count();
        t_last = t;
        return e;
    };
    const uint64_t scratch_cap = text_scratch_bytes(N);
    uint8_t *d_scratch = nullptr;
    size_t tb = 0;
    bool scratch_short = false;
    auto scratch = [&](size_t bytes) -> void * {          // hipcub's scratch: one allocation of the planned size
        if (bytes > scratch_cap) { scratch_short = true; tb = 0; return nullptr; }   // (hipcub then only sizes again: nothing runs)
        return d_scratch;
    };
#define SCRATCH_CHECK(what)                                                                                                       \
    if (scratch_short) {                                                                                                          \
        why = std::string("internal error: ") + what + " asks for more scratch than the plan grants (" + std::to_string(scratch_cap) + " bytes)"; \
        return MOVI_ERR_INVARIANT;                                                                                                \
    }

    // ---- upload
    const uint64_t padded = text_padded_bytes(N);
    uint8_t *d_text = pool.get<uint8_t>(padded);
    uint32_t *d_rank = pool.get<uint32_t>(N);
    uint64_t *d_keys[2] = {pool.get<uint64_t>(N + 2), pool.get<uint64_t>(N + 2)};
    uint32_t *d_vals[2] = {pool.get<uint32_t>(N), pool.get<uint32_t>(N)};
    d_scratch = pool.get<uint8_t>(scratch_cap);
    uint64_t *d_small = pool.get<uint64_t>(8);            // run count | long-run count (u32) | verify findings (3 x u32)
    TEXT_TRY(pool.err, "allocating the sort buffers");
    const uint64_t *d_words = reinterpret_cast<const uint64_t *>(d_text);
    TEXT_TRY(hipMemcpyAsync(d_text, h_text, n, hipMemcpyHostToDevice, stream), "copying the text");
    TEXT_TRY(hipMemsetAsync(d_text + n, 0, padded - n, stream), "clearing");
    TEXT_TRY(hipMemsetAsync(d_small, 0, 64, stream), "clearing");
    TEXT_TRY(lap(0), "the upload");

    // ---- stage 1: prefix doubling
    hipcub::DoubleBuffer<uint64_t> keys(d_keys[0], d_keys[1]);
    hipcub::DoubleBuffer<uint32_t> vals(d_vals[0], d_vals[1]);
    hipLaunchKernelGGL(first_keys_kernel, dim3(blocks_of(N)), dim3(256), 0, stream, d_words, N, keys.Current(), vals.Current());
    TEXT_TRY(hipGetLastError(), "first_keys_kernel");
    for (uint64_t h = 8;; h *= 2) {
        const int end_bit = stats.rounds == 0 ? 64 : 2 * nb;
        TEXT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, vals, N, 0, end_bit, stream), "sizing the suffix sort");
        TEXT_TRY(hipcub::DeviceRadixSort::SortPairs(scratch(tb), tb, keys, vals, N, 0, end_bit, stream), "sorting the suffixes");
        SCRATCH_CHECK("the suffix sort");
        stats.rounds += 1;
        uint32_t *d_dense = reinterpret_cast<uint32_t *>(keys.Alternate());
        hipcub::TransformInputIterator<uint32_t, KeyChanged, hipcub::CountingInputIterator<uint64_t>> flags(hipcub::CountingInputIterator<uint64_t>(0),
                                                                                                           KeyChanged{keys.Current()});
        TEXT_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, flags, d_dense, N, stream), "sizing the rank sum");
        TEXT_TRY(hipcub::DeviceScan::InclusiveSum(scratch(tb), tb, flags, d_dense, N, stream), "numbering the groups");
        SCRATCH_CHECK("the rank sum");
        hipLaunchKernelGGL(scatter_ranks_kernel, dim3(blocks_of(N)), dim3(256), 0, stream, vals.Current(), d_dense, N, d_rank);
        TEXT_TRY(hipGetLastError(), "scatter_ranks_kernel");
        uint32_t last = 0;
        TEXT_TRY(hipMemcpyAsync(&last, d_dense + (N - 1), 4, hipMemcpyDeviceToHost, stream), "reading the group count");
        TEXT_TRY(hipStreamSynchronize(stream), "a doubling round");
        if ((uint64_t)last == N - 1) break;                // all ranks differ: vals.Current() is the suffix array, d_rank its inverse
        if (h >= 2 * N || (uint64_t)last >= N) {
            why = "internal error: " + std::to_string((uint64_t)last + 1) + " groups of " + std::to_string(N) + " suffixes after comparing " +
                  std::to_string(h) + " characters";
            return MOVI_ERR_INVARIANT;
        }
        hipLaunchKernelGGL(rank_keys_kernel, dim3(blocks_of(N)), dim3(256), 0, stream, vals.Current(), d_rank, h, N, nb, keys.Current());
        TEXT_TRY(hipGetLastError(), "rank_keys_kernel");
    }
    const uint32_t *d_sa = vals.Current(), *d_isa = d_rank;
    TEXT_TRY(lap(1), "the suffix sort");

    // ---- stage 2: BWT and runs.  The key buffers are free now: A = LCP (N x u32) | run starts (R + 1 x u32);
    // B = BWT (N) | run heads (R) | thresholds (R x u32, from the next multiple of 8)
    uint8_t *buf_a = reinterpret_cast<uint8_t *>(keys.Current()), *buf_b = reinterpret_cast<uint8_t *>(keys.Alternate());
    uint32_t *d_lcp = reinterpret_cast<uint32_t *>(buf_a), *d_run_start = d_lcp + N;
    uint8_t *d_bwt = buf_b, *d_heads = buf_b + N;
    uint32_t *d_thr = reinterpret_cast<uint32_t *>(buf_b + ((2 * N + 7) & ~7ull));
    hipLaunchKernelGGL(bwt_kernel, dim3(blocks_of(N)), dim3(256), 0, stream, d_text, d_sa, N, d_bwt);
    TEXT_TRY(hipGetLastError(), "bwt_kernel");
    uint64_t R = 0;
    {
        hipcub::CountingInputIterator<uint64_t> positions(0);
        TEXT_TRY(hipcub::DeviceSelect::If(nullptr, tb, positions, d_run_start, d_small, (int64_t)N, IsRunHead{d_bwt}, stream), "sizing the run select");
        TEXT_TRY(hipcub::DeviceSelect::If(scratch(tb), tb, positions, d_run_start, d_small, (int64_t)N, IsRunHead{d_bwt}, stream), "selecting the run starts");
        SCRATCH_CHECK("the run select");
        TEXT_TRY(hipMemcpyAsync(&R, d_small, 8, hipMemcpyDeviceToHost, stream), "reading the run count");
        TEXT_TRY(hipStreamSynchronize(stream), "the run starts");
    }
    if (R == 0 || R > N) { why = "internal error: " + std::to_string(R) + " runs in " + std::to_string(N) + " BWT positions"; return MOVI_ERR_INVARIANT; }
    hipLaunchKernelGGL(heads_kernel, dim3(blocks_of(R + 1)), dim3(256), 0, stream, d_bwt, d_run_start, R, N, d_heads);
    TEXT_TRY(hipGetLastError(), "heads_kernel");
    stats.original_r = R;
    TEXT_TRY(lap(2), "the runs");

    // ---- stage 3: LCP
    if (with_thr) {
        const uint32_t chunk = lcp_chunk ? lcp_chunk : text_default_lcp_chunk(N);
        const uint64_t lanes = (N + chunk - 1) / chunk;
        hipLaunchKernelGGL(lcp_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, stream, d_words, d_sa, d_isa, N, chunk, d_lcp);
        TEXT_TRY(hipGetLastError(), "lcp_kernel");
        TEXT_TRY(lap(3), "the LCP pass");
    }

    // ---- stage 5 (before the text goes): verify
    uint32_t *d_bad = reinterpret_cast<uint32_t *>(d_small + 2);
    if (verify) {
        uint32_t *d_seen = pool.get<uint32_t>(N / 32 + 2);
        TEXT_TRY(pool.err, "allocating the verifier's bitmap");
        TEXT_TRY(hipMemsetAsync(d_seen, 0, (N / 32 + 2) * 4, stream), "clearing");
        hipLaunchKernelGGL(verify_sa_kernel, dim3(blocks_of(N)), dim3(256), 0, stream, d_text, d_sa, d_isa, N, d_seen, d_bad);
        TEXT_TRY(hipGetLastError(), "verify_sa_kernel");
        if (with_thr) {
            hipLaunchKernelGGL(verify_lcp_kernel, dim3(kVerifySamples / 64), dim3(64), 0, stream, d_text, d_sa, d_lcp, N, 0x6D6F7669ull ^ N, d_bad);
            TEXT_TRY(hipGetLastError(), "verify_lcp_kernel");
        }
        uint32_t bad[3] = {0, 0, 0};
        TEXT_TRY(hipMemcpyAsync(bad, d_bad, 12, hipMemcpyDeviceToHost, stream), "reading the verifier's findings");
        TEXT_TRY(hipStreamSynchronize(stream), "the verifier");
        pool.release(d_seen);
        if (bad[0] || bad[1] || bad[2]) {
            why = "verify: the suffix array is " + std::string(bad[0] ? "not a permutation with its inverse (" + std::to_string(bad[0]) + " findings)" : "a permutation") +
                  ", " + std::to_string(bad[1]) + " neighbouring pair(s) out of order, " + std::to_string(bad[2]) + " of " +
                  std::to_string(kVerifySamples) + " sampled LCP values wrong";
            return MOVI_ERR_INVARIANT;
        }
        stats.verified = 1;
        TEXT_TRY(lap(5), "the verifier");
    }
    stats.device_bytes = pool.peak;
    pool.release(d_text);
    pool.release(d_rank);
    pool.release(d_vals[0]);
    pool.release(d_vals[1]);

    // ---- the run heads come down first: they say which characters there are
    HostOut out;
    TEXT_TRY(hipHostMalloc(&out.p[0], R, hipHostMallocDefault), "allocating the run heads");
    TEXT_TRY(hipHostMalloc(&out.p[1], R * 8, hipHostMallocDefault), "allocating the run lengths");
    uint8_t *heads = static_cast<uint8_t *>(out.p[0]);
    uint64_t *lens = static_cast<uint64_t *>(out.p[1]), *thr = nullptr;
    std::vector<uint32_t> down(R + 1);
    TEXT_TRY(hipMemcpyAsync(heads, d_heads, R, hipMemcpyDeviceToHost, stream), "reading the run heads");
    TEXT_TRY(hipMemcpyAsync(down.data(), d_run_start, (R + 1) * 4, hipMemcpyDeviceToHost, stream), "reading the run starts");
    TEXT_TRY(hipStreamSynchronize(stream), "the runs");
    for (uint64_t k = 0; k < R; k++) lens[k] = (uint64_t)down[k + 1] - down[k];
    TEXT_TRY(lap(2), "the runs");

    // ---- stage 4: thresholds
    if (with_thr) {
        bool present[256] = {false};
        for (uint64_t k = 0; k < R; k++) present[heads[k]] = true;
        const uint32_t long_cap = (uint32_t)(N / kLongRun + 1);
        uint64_t *d_run_min = pool.get<uint64_t>(R);
        uint32_t *d_long = pool.get<uint32_t>(long_cap), *d_n_long = reinterpret_cast<uint32_t *>(d_small + 1);
        TEXT_TRY(pool.err, "allocating the run minima");
        hipLaunchKernelGGL(run_min_kernel, dim3(blocks_of(R)), dim3(256), 0, stream, d_lcp, d_run_start, R, d_run_min, d_long, long_cap, d_n_long);
        TEXT_TRY(hipGetLastError(), "run_min_kernel");
        hipLaunchKernelGGL(long_run_min_kernel, dim3(1024), dim3(64), 0, stream, d_lcp, d_run_start, d_long, d_n_long, long_cap, d_run_min);
        TEXT_TRY(hipGetLastError(), "long_run_min_kernel");
        for (int c = 0; c < 256; c++) {
            if (!present[c]) continue;
            hipcub::TransformInputIterator<Seg, SegOfRun, hipcub::CountingInputIterator<uint64_t>> in(hipcub::CountingInputIterator<uint64_t>(0),
                                                                                                      SegOfRun{d_heads, d_run_min, (uint8_t)c});
            const ThrOut sink{ThrSink{d_heads, d_run_start, d_lcp, d_thr, (uint8_t)c}, 0};
            TEXT_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, tb, in, sink, SegJoin(), Seg{kNoMin, 0ull}, R, stream), "sizing the threshold scan");
            TEXT_TRY(hipcub::DeviceScan::ExclusiveScan(scratch(tb), tb, in, sink, SegJoin(), Seg{kNoMin, 0ull}, R, stream), "the threshold scan");
            SCRATCH_CHECK("the threshold scan");
        }
        TEXT_TRY(hipHostMalloc(&out.p[2], R * 8, hipHostMallocDefault), "allocating the thresholds");
        thr = static_cast<uint64_t *>(out.p[2]);
        TEXT_TRY(hipMemcpyAsync(down.data(), d_thr, R * 4, hipMemcpyDeviceToHost, stream), "reading the thresholds");
        TEXT_TRY(hipStreamSynchronize(stream), "the thresholds");
        for (uint64_t k = 0; k < R; k++) thr[k] = down[k];
        stats.device_bytes = pool.peak > stats.device_bytes ? pool.peak : stats.device_bytes;
        TEXT_TRY(lap(4), "the thresholds");
    }
    *h_heads = heads;
    *h_lens = lens;
    *h_thr = thr;
    *original_r = R;
    out.p[0] = out.p[1] = out.p[2] = nullptr;
    return MOVI_OK;
}

}  // namespace movi
