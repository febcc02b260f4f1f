// movi_walk_color.hip -- Movi Color, default colour mode (flat colour table, one document set per run).
//   color_walk_kernel  build_doc_pats (src/move_structure_color.cpp:4-24) without its n sequential LF steps: every sampled BWT position
//                      walks down the text to the previous sample and writes, for every position it passes, the key
//                      (row << 16) | document -- the document by the reference's rule, :14-19.
//   build_color_keys   build_doc_sets' per-run sets (:27-55): the keys sorted and made unique on the device, chunk by chunk.  (Giving
//                      equal sets one number in first-appearance order, :57-63, and flat_and_serialize_colors_vectors,
//                      src/move_structure_io.cpp:513-548, run on the host: movi_abi.hip.)
//   color_kernel       the PML walk with the multi-class scoring of ReadProcessor::process_char (src/read_processor.cpp:122-186) fused in
//                      where the reference has it: after the LF step, before the base is compared.
// The contract is stated in include/movi_hip.h (movi_color_build, movi_multi_classify_device); the tables in movi_color.hpp.
// (Named into the movi_walk*.hip family: the sanitizer build of tests/fuzz/fuzz_parse.sh compiles the library from that glob.)
#include "movi_search.hpp"
#include "movi_color.hpp"

#include <chrono>
#include <vector>

#include <hipcub/hipcub.hpp>

namespace movi {

// ------------------------------------------------------------------------------------------------ the builder's walk
// The samples sorted by their text position cut the text into stretches: item i (sample tj[i], text position tv[i]) owns the positions
// tv[i], tv[i] - 1, ..., tv[i - 1] + 1 -- len = tv[i] - tv[i - 1] of them, tv[-1] = -1 -- and must then stand on sample tj[i - 1] (the
// lowest one walks through text position 0 to BWT position 0, sample 0).  A chunk of items is a stretch of the text, so its keys are
// indexed by text position and every slot has exactly one writer.  The lanes own lists of items (LaneList, movi_lists.hpp) and step by
// loc_lf_step, as locate_walk's do.  bad[0] counts what a consistent table and array cannot produce: a walk that meets a sample too early, too late
// or meets the wrong one, a position outside the table, a BWT position passed twice (the bitmap `visited`).
struct ColWalkArgs {
    const uint64_t *P;         // packed position of every sample
    const uint64_t *tv, *tj;   // the samples by text position: value, index
    uint64_t i0, tlo, n_keys;  // the chunk: its first item, the text position of keys[0], its keys
    const uint64_t *doc_ends;  // strictly increasing
    const uint16_t *doc_ids;
    uint32_t n_docs, doc_bits;
    uint64_t *keys;
    uint32_t *visited, *bad;
};

template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void color_walk_kernel(DevIndex ix, LocArgs a, ColWalkArgs c, uint64_t n_items, DevStats *stats) {
    LaneList ls(n_items);
    IdxT kidx = 0;
    uint32_t off = 0, ff_total = 0, errs = 0, doc = 0;
    uint64_t dist = 0, len = 0, t = 0, expect = 0, doc_lo = 0, lane_steps = 0, wave_steps = 0;
    uint4 v = make_uint4(0, 0, 0, 0);
    const uint32_t rate = a.rate;
    while (ls.any()) {
        wave_steps += 1;
        if (ls.state == 1u) {                             // the lane's next item
            const uint64_t i = c.i0 + ls.item, j = c.tj[i];
            t = c.tv[i];
            len = i ? t - c.tv[i - 1] : t + 1;
            expect = i ? c.tj[i - 1] : 0;
            const uint64_t p = j < a.n_entries ? c.P[j] : kPosNone;
            const uint64_t row = p >> kPosOffBits;
            if (p != kPosNone && row < ix.r && len != 0 && t < a.n && t - c.tlo < c.n_keys && len - 1 <= t - c.tlo) {
                kidx = (IdxT)row;
                off = (uint32_t)p & ((1u << kPosOffBits) - 1u);
                v = loc_load(a.rows, row);
                dist = 0;
                uint32_t lo = 0, hi = c.n_docs - 1;       // the first document that ends beyond t; the last one takes what lies past every end
                for (uint32_t s = 0; s < c.doc_bits; ++s) {
                    const uint32_t mid = (lo + hi) >> 1;
                    const bool up = lo < hi && c.doc_ends[mid] <= t;
                    const bool dn = lo < hi && !up;
                    lo = up ? mid + 1 : lo;
                    hi = dn ? mid : hi;
                }
                doc = lo;
                doc_lo = doc ? c.doc_ends[doc - 1] : 0;
                ls.state = 2u;
            } else {
                errs += 1;
                ls.next();
            }
        }
        if (ls.state == 2u) {
            const uint32_t tp = loc_rem(v) + off;         // < 2^24 + 2^12
            const bool hit = (tp % rate == 0u) && dist != 0;
            if (hit || dist >= len) {                     // the walk is over: on the expected sample after len steps, or an error
                if (!(hit && dist == len && loc_quot(v) + tp / rate == expect)) errs += 1;
                ls.next();
            }
        }
        const bool walk = ls.state == 2u;                 // (a lane that took up an item above steps in this same iteration)
        uint64_t idx = kidx;
        const uint64_t bwt = loc_quot(v) * rate + loc_rem(v) + off, row_now = kidx, tt = t - dist;
        const uint32_t e = loc_lf_step<MODE>(a.rows, ix.r, walk, idx, off, v, ff_total, [&]() {
            if (walk) {                                   // the position's key, under the gather of the next row
                if (tt < doc_lo) { doc -= 1; doc_lo = doc ? c.doc_ends[doc - 1] : 0; }    // src/move_structure_color.cpp:15-17
                const uint64_t slot = tt - c.tlo;
                if (slot < c.n_keys && bwt < a.n) {
                    c.keys[slot] = (row_now << kColorKeyDocBits) | (uint64_t)c.doc_ids[doc];
                    const uint32_t bit = 1u << (bwt & 31u);
                    if (atomicOr(&c.visited[bwt >> 5], bit) & bit) errs += 1;
                } else errs += 1;
                lane_steps += 1;
                dist += 1;
            }
        });
        kidx = (IdxT)idx;
        if (walk && e != 0u) {                            // a corrupt table: an error, not a hang
            errs += 1;
            ls.next();
        }
    }
    if (errs) atomicAdd(c.bad, errs);
    flush_list_stats(stats, ff_total, 0u, 0u, lane_steps, wave_steps);
}

namespace {

__global__ __launch_bounds__(256) void iota_kernel(uint64_t *out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

unsigned blocks256(uint64_t n) { return (unsigned)((n + 255) / 256); }

struct ColorWalkFamily {
    template <int MODE, typename IdxT> static auto kernel() { return &color_walk_kernel<MODE, IdxT>; }
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

constexpr uint64_t kMaxKeys = 1ull << 30;               // hipcub's item counts are ints

}  // namespace

hipError_t build_color_keys(int mode, const DevIndex &ix, const LocArgs &loc, const uint64_t *h_doc_ends, const uint16_t *h_doc_ids,
                            uint32_t n_docs, uint64_t chunk_keys, int num_cus, hipStream_t stream, uint64_t **d_keys_out, uint64_t *n_keys_out,
                            uint32_t *bad_out, uint32_t *n_chunks, double *seconds, LaunchInfo *info, uint64_t *key_cap) {
    const uint64_t n = loc.n, rate = loc.rate, m = (n + rate - 1) / rate;
    *d_keys_out = nullptr; *n_keys_out = 0; *bad_out = 0; *n_chunks = 0;
    seconds[0] = seconds[1] = 0.0;
    if ((mode != 6 && mode != 3) || m == 0 || m > 0x7FFFFFFFull || n_docs == 0 || ix.r >= (1ull << (64 - kColorKeyDocBits))) return hipErrorInvalidValue;
    DevPtr<uint64_t> P, sv, si, tvd, tj, ends, ka, kb;
    DevPtr<uint16_t> ids;
    DevPtr<uint32_t> visited, badc;                       // badc[0] = findings, badc[1] = hipcub's number of unique keys
    DevPtr<void> temp;
    size_t temp_bytes = 0;
    std::vector<uint64_t> tv(m);
    const uint64_t vis_words = (n + 31) / 32;
    hipError_t e = dev_alloc(P, m * 8);
    if (e == hipSuccess) e = dev_alloc(sv, m * 8);
    if (e == hipSuccess) e = dev_alloc(si, m * 8);
    if (e == hipSuccess) e = dev_alloc(tvd, m * 8);
    if (e == hipSuccess) e = dev_alloc(tj, m * 8);
    if (e == hipSuccess) e = dev_alloc(ends, (size_t)n_docs * 8);
    if (e == hipSuccess) e = dev_alloc(ids, (size_t)n_docs * 2);
    if (e == hipSuccess) e = dev_alloc(visited, vis_words * 4);
    if (e == hipSuccess) e = dev_alloc(badc, 8);
    uint64_t *d_P = P.get(), *d_sv = sv.get(), *d_si = si.get(), *d_tv = tvd.get(), *d_tj = tj.get(), *d_ends = ends.get();
    uint16_t *d_ids = ids.get();
    uint32_t *d_visited = visited.get(), *d_bad = badc.get();
    if (e == hipSuccess) e = hipMemsetAsync(d_visited, 0, vis_words * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_P, 0xFF, m * 8, stream);           // a sample no row holds stays kPosNone: counted by the walk
    if (e == hipSuccess) e = hipMemcpyAsync(d_ends, h_doc_ends, (size_t)n_docs * 8, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ids, h_doc_ids, (size_t)n_docs * 2, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = launch_sample_positions(mode, ix, loc, m, d_P, stream);
    // the samples by text position
    if (e == hipSuccess) e = hipMemcpyAsync(d_sv, loc.samples, m * 8, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(iota_kernel, dim3(blocks256(m)), dim3(256), 0, stream, d_si, m);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, d_sv, d_tv, d_si, d_tj, (int)m, 0, 64, stream);
    if (e == hipSuccess) e = dev_alloc(temp, temp_bytes ? temp_bytes : 8);
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(temp.get(), temp_bytes, d_sv, d_tv, d_si, d_tj, (int)m, 0, 64, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tv.data(), d_tv, m * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    temp.reset();                                          // (freed here, not at the end: the key budget below is what is free now)
    sv.reset();
    si.reset();
    // the samples must be distinct text positions whose highest is n - 1 (sample 0): then the stretches add up to n
    bool shape = e == hipSuccess && tv[m - 1] == n - 1;
    for (uint64_t i = 1; shape && i < m; i++) shape = tv[i] > tv[i - 1];
    uint64_t longest = 0;
    for (uint64_t i = 0; shape && i < m; i++) longest = std::max(longest, i ? tv[i] - tv[i - 1] : tv[0] + 1);
    // two key buffers of 8 bytes per key (sorted + unique keys so far | the chunk's keys, and the sort's other side) and hipcub's scratch
    // (about as much again): free / 64 keys keep all of it within half of what is free
    uint64_t cap = 0;
    if (e == hipSuccess && shape) {
        size_t free_b = 0, total_b = 0;
        e = hipMemGetInfo(&free_b, &total_b);
        cap = std::min<uint64_t>(kMaxKeys, (uint64_t)free_b / 64);              // half of what is free
        cap = std::min<uint64_t>(cap, n + (chunk_keys ? std::min(chunk_keys, n) : n));   // (never more than everything at once)
        if (cap < longest) e = hipErrorOutOfMemory;
    }
    if (e == hipSuccess && shape) e = dev_alloc(ka, cap * 8);
    if (e == hipSuccess && shape) e = dev_alloc(kb, cap * 8);
    uint64_t *d_a = ka.get(), *d_b = kb.get();
    if (e == hipSuccess && shape) {
        size_t t1 = 0, t2 = 0;
        e = hipcub::DeviceRadixSort::SortKeys(nullptr, t1, d_a, d_b, (int)cap, 0, 64, stream);
        if (e == hipSuccess) e = hipcub::DeviceSelect::Unique(nullptr, t2, d_b, d_a, d_bad + 1, (int)cap, stream);
        temp_bytes = std::max(t1, t2);
        if (e == hipSuccess) e = dev_alloc(temp, temp_bytes ? temp_bytes : 8);
    }
    void *d_temp = temp.get();
    int key_bits = (int)kColorKeyDocBits;
    while (key_bits < 64 && (ix.r >> (key_bits - (int)kColorKeyDocBits)) != 0) key_bits++;
    uint32_t doc_bits = 1;
    while ((1u << doc_bits) < n_docs) doc_bits++;
    uint64_t acc = 0, i0 = 0;
    uint32_t chunks = 0, h_cnt[2] = {0, 0};
    while (e == hipSuccess && shape && i0 < m) {
        const uint64_t tlo = i0 ? tv[i0 - 1] + 1 : 0;
        const uint64_t room = std::min<uint64_t>(cap - acc, chunk_keys ? chunk_keys : cap);
        uint64_t i1 = i0 + 1;                                               // at least one item, however long its stretch
        while (i1 < m && tv[i1] - tlo + 1 <= room) i1++;
        const uint64_t n_keys = tv[i1 - 1] - tlo + 1;
        if (acc + n_keys > cap) { e = hipErrorOutOfMemory; break; }
        ColWalkArgs c{d_P, d_tv, d_tj, i0, tlo, n_keys, d_ends, d_ids, n_docs, doc_bits + 1, d_a + acc, d_visited, d_bad};
        auto tw = std::chrono::steady_clock::now();
        e = launch_lane_lists<ColorWalkFamily>("color_walk_kernel", 0, mode, ix, i1 - i0, kLocateWaves, num_cus, stream, info, loc, c, i1 - i0,
                                               (DevStats *)nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        seconds[0] += seconds_since(tw);
        auto ts = std::chrono::steady_clock::now();
        const uint64_t cnt = acc + n_keys;
        size_t tb = temp_bytes;
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortKeys(d_temp, tb, d_a, d_b, (int)cnt, 0, key_bits, stream);
        tb = temp_bytes;
        if (e == hipSuccess) e = hipcub::DeviceSelect::Unique(d_temp, tb, d_b, d_a, d_bad + 1, (int)cnt, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_bad, 8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        seconds[1] += seconds_since(ts);
        if (e == hipSuccess && h_cnt[0]) break;                              // findings: the keys are not to be trusted
        acc = h_cnt[1];
        i0 = i1;
        chunks += 1;
    }
    *bad_out = !shape ? 1u : h_cnt[0];
    *n_chunks = chunks;
    if (key_cap) *key_cap = cap;
    if (e == hipErrorOutOfMemory) *n_keys_out = acc;
    if (e != hipSuccess || *bad_out) return e;
    *d_keys_out = ka.release();                            // the caller's from here on
    *n_keys_out = acc;
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------ the query
// One lane per read, base-synchronous: walk_base's automaton (the one sa_pos_kernel runs), cut open between its LF step and its
// comparison, where process_char scores (src/read_processor.cpp:122-186): the match length carried over from the base before is
// tested against min_len BEFORE this base's character is looked at, and the set of the row the walk stands on after the LF step is
// counted member by member in stored order -- best / second-best change on a strictly greater count only, so the order of the bases
// and of the members decides ties, and a read is scored by its own lane from end to end.  The row the next LF step will fetch if this
// base matches is gathered before the scoring and used by that step unless the base repositioned.
// A read that hits one of the reference's throws reports its code, no document, zero counters and all-zero PMLs.
template <int MODE, typename IdxT>
__global__ __launch_bounds__(64) void color_kernel(DevIndex ix, ColorTables ct, uint32_t min_len, const uint8_t *__restrict__ bases,
                                                   const uint64_t *__restrict__ offs, uint64_t t0, uint64_t t1, uint16_t *__restrict__ pml,
                                                   McRead *__restrict__ out, uint32_t *__restrict__ counts, uint32_t by_read,
                                                   uint8_t *__restrict__ err, DevStats *stats, const uint32_t *__restrict__ order) {
    __shared__ uint8_t s_code[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_code[i] = ix.code_of[i];
    __syncthreads();
    const uint64_t t = t0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = t < t1;
    const uint64_t rid = (valid && order) ? order[t] : t;
    const uint64_t beg = valid ? offs[rid] : 0;
    const uint64_t len = valid ? offs[rid + 1] - beg : 0;
    const uint8_t *R = bases + beg;
    uint32_t *cnt = counts + (by_read ? rid : t - t0) * (uint64_t)ct.num_species;
    const EndThr ethr = end_thresholds(ix);
    uint32_t ff_total = 0, scan_total = 0, repo_total = 0, failed = 0;
    IdxT kidx = (IdxT)(ix.r - 1);                            // ReadProcessor::reset_process, src/read_processor.cpp:69-77
    uint2 row = load_row<MODE>(ix.rows, ix.r - 1), pre = row;
    uint32_t off = row_n<MODE>(row) - 1, ml = 0;
    uint32_t best = kDocNone, second = kDocNone, cbest = 0, csecond = 0, colors_count = 0, sum_ml = 0;
    bool have_pre = false;
    for (uint64_t k = 0; wave_any(k < len && failed == 0u); ++k) {
        bool live = k < len && failed == 0u;
        const uint32_t a = live ? (uint32_t)s_code[R[len - 1 - k]] : 0xFFu;
        uint64_t idx = kidx;
        uint32_t e = lf_step_pre<MODE>(ix, live && k != 0, idx, off, row, have_pre, pre, ff_total);      // process_char :100-116
        if (e) { failed = e; live = false; }
        have_pre = false;
        if (live) {                                          // the next step's row if this base matches: gathered under the scoring
            const uint64_t j = row_id<MODE>(row, idx, ix);
            if (j < ix.r) { pre = load_row<MODE>(ix.rows, j); have_pre = true; }
        }
        uint32_t m = 0, sz = 0;
        uint64_t at = 0;
        if (live && ml >= min_len) {                         // :123-147
            colors_count += 1;
            const uint64_t fi = ct.inds[idx];
            if (fi < ct.flat_size) {
                sz = ct.flat[fi];
                at = fi + 1;
                if (at + sz > ct.flat_size) sz = (uint32_t)(ct.flat_size - at);
            }
        }
        for (; wave_any(m < sz); ++m) {                      // :159-169
            if (m < sz) {
                const uint32_t doc = ct.flat[at + m];
                if (doc < ct.num_species) {
                    const uint32_t c = cnt[doc] + 1;
                    cnt[doc] = c;
                    if (doc == best) cbest = c;
                    else if (best == kDocNone || c > cbest) { second = best; csecond = cbest; best = doc; cbest = c; }
                    else if (second == kDocNone || c > csecond) { second = doc; csecond = c; }
                }
            }
        }
        const uint64_t before = idx;
        e = walk_base<MODE>(ix, ethr, live, false, a, idx, off, row, ml, ff_total, scan_total, repo_total);   // :188-229
        if (idx != before) have_pre = false;
        kidx = (IdxT)idx;
        if (e) failed = e;
        else if (live) {
            if (pml) pml[beg + k] = (uint16_t)(ml > 65535u ? 65535u : ml);
            sum_ml += ml;                                    // :237 (uint32_t there too)
        }
    }
    if (failed) {
        for (uint64_t k = 0; pml && k < len; ++k) pml[beg + k] = 0;
        for (uint32_t d = 0; d < ct.num_species; ++d) cnt[d] = 0;
        best = second = kDocNone;
        colors_count = sum_ml = 0;
    }
    if (valid) {
        out[rid] = McRead{(uint16_t)best, (uint16_t)second, colors_count, sum_ml, best == kDocNone ? 0u : cbest, second == kDocNone ? 0u : csecond, 0u};
        if (err) err[rid] = (uint8_t)failed;
    }
    const uint32_t ffw = wave_sum(ff_total), scw = wave_sum(scan_total), rpw = wave_sum(repo_total), erw = wave_sum(failed ? 1u : 0u);
    if ((threadIdx.x & 63) == 0 && stats) {
        if (ffw) atomicAdd(&stats->fast_forwards, (unsigned long long)ffw);
        if (scw) atomicAdd(&stats->scans, (unsigned long long)scw);
        if (rpw) atomicAdd(&stats->repositions, (unsigned long long)rpw);
        if (erw) atomicAdd(&stats->errors, (unsigned long long)erw);
    }
}

hipError_t launch_color(const DevIndex &ix, const ColorTables &ct, uint32_t min_len, const uint8_t *d_bases, const uint64_t *d_offsets,
                        uint64_t t0, uint64_t t1, uint16_t *d_pml, McRead *d_out, uint32_t *d_counts, bool by_read, uint8_t *d_err,
                        DevStats *d_stats, const uint32_t *d_order, hipStream_t stream, LaunchInfo *info) {
    if (t1 <= t0) return hipSuccess;
    const uint64_t blocks = (t1 - t0 + 63) / 64;
    if (blocks > 0x7FFFFFFFull || !ct.flat || !ct.inds || !d_counts || !d_out) return hipErrorInvalidValue;
    char nm[96];
    snprintf(nm, sizeof(nm), "color_kernel<6, %s>", ix.idx32 ? "unsigned int" : "unsigned long");
    note_walk_launch(nm);
    if (info) {
        *info = LaunchInfo();
        snprintf(info->kernel, sizeof(info->kernel), "%s", nm);
        info->variant = 0; info->block_threads = 64; info->idx64 = ix.idx32 ? 0 : 1;
    }
    if (ix.idx32)
        hipLaunchKernelGGL((color_kernel<6, uint32_t>), dim3((unsigned)blocks), dim3(64), 0, stream, ix, ct, min_len, d_bases, d_offsets, t0, t1,
                           d_pml, d_out, d_counts, by_read ? 1u : 0u, d_err, d_stats, d_order);
    else
        hipLaunchKernelGGL((color_kernel<6, uint64_t>), dim3((unsigned)blocks), dim3(64), 0, stream, ix, ct, min_len, d_bases, d_offsets, t0, t1,
                           d_pml, d_out, d_counts, by_read ? 1u : 0u, d_err, d_stats, d_order);
    return hipGetLastError();
}

hipError_t preload_color(int mode, bool idx32) {
    hipFuncAttributes at;
    if (mode != 6) return hipSuccess;
    return hipFuncGetAttributes(&at, idx32 ? (const void *)color_kernel<6, uint32_t> : (const void *)color_kernel<6, uint64_t>);
}

}  // namespace movi
