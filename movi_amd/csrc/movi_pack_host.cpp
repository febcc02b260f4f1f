// movi_pack_host.cpp -- two bits per base on the host: pack_reads / unpack_reads (movi_pack_host.hpp; the format is stated in
// include/movi_hip.h).  Pure host code; AVX2 behind a run-time check, the plain loop everywhere else.
#include "movi_pack_host.hpp"
#include "movi_expand_host.hpp"
#include "../../include/movi_hip.h"

#include <immintrin.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace movi {

namespace {

constexpr uint8_t kExc = 0x80;                 // not upper-case A / C / G / T: code 0 in the stream + an entry in the list
constexpr uint64_t kMinSliceBases = 1u << 16;  // a worker thread is not worth starting for less

struct Tables {
    uint8_t code[256];                         // byte -> 0..3, or kExc
    uint32_t four[256];                        // packed byte -> its four bases, first base in the low byte
    Tables() {
        for (int i = 0; i < 256; i++) code[i] = kExc;
        code['A'] = 0; code['C'] = 1; code['G'] = 2; code['T'] = 3;
        static const uint8_t acgt[4] = {'A', 'C', 'G', 'T'};
        for (int i = 0; i < 256; i++)
            four[i] = (uint32_t)acgt[i & 3] | (uint32_t)acgt[(i >> 2) & 3] << 8 | (uint32_t)acgt[(i >> 4) & 3] << 16 | (uint32_t)acgt[(i >> 6) & 3] << 24;
    }
};
const Tables kT;

// exceptions straight into the caller's arrays, counted past their capacity
struct CappedSink {
    uint64_t *pos;
    uint8_t *byte;
    uint64_t cap, n = 0;
    void add(uint64_t p, uint8_t b) {
        if (n < cap) { pos[n] = p; byte[n] = b; }
        ++n;
    }
};
// a worker's own list
struct VectorSink {
    std::vector<uint64_t> pos;
    std::vector<uint8_t> byte;
    void add(uint64_t p, uint8_t b) { pos.push_back(p); byte.push_back(b); }
};

bool have_avx2() {
    static const bool v = __builtin_cpu_supports("avx2");
    return v;
}

// 32 bases that are all A / C / G / T -> 8 packed bytes; false (nothing written) if one of them is not
__attribute__((target("avx2"))) inline bool pack32_avx2(const uint8_t *in, uint8_t *out) {
    const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(in));
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, _mm256_set1_epi8('A')), _mm256_cmpeq_epi8(v, _mm256_set1_epi8('C'))),
                                       _mm256_or_si256(_mm256_cmpeq_epi8(v, _mm256_set1_epi8('G')), _mm256_cmpeq_epi8(v, _mm256_set1_epi8('T'))));
    if (_mm256_movemask_epi8(ok) != -1) return false;
    // ((x >> 1) ^ (x >> 2)) & 3: 0x41 -> 0, 0x43 -> 1, 0x47 -> 2, 0x54 -> 3 (the bits a 16-bit shift drags in from the neighbour are masked off)
    const __m256i c = _mm256_and_si256(_mm256_xor_si256(_mm256_srli_epi16(v, 1), _mm256_srli_epi16(v, 2)), _mm256_set1_epi8(3));
    const __m256i p = _mm256_maddubs_epi16(c, _mm256_set1_epi16(0x0401));        // c0 + 4 c1 | c2 + 4 c3
    const __m256i q = _mm256_madd_epi16(p, _mm256_set1_epi32(0x00100001));       // (c0 + 4 c1) + 16 (c2 + 4 c3): one packed byte per dword
    const __m256i s = _mm256_shuffle_epi8(q, _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                                              0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1));
    const uint32_t lo = (uint32_t)_mm256_extract_epi32(s, 0), hi = (uint32_t)_mm256_extract_epi32(s, 4);
    memcpy(out, &lo, 4);
    memcpy(out + 4, &hi, 4);
    return true;
}

// Bases [j0, j1) of the call (relative to first_base).  first_base + j0 is a multiple of four unless j0 == 0, and so is
// first_base + j1 unless j1 is the call's end: a slice shares no byte with its neighbours.
template <typename Sink>
void pack_slice_plain(const uint8_t *in, uint64_t first_base, uint64_t j0, uint64_t j1, uint8_t *packed, Sink &sink, bool avx2) {
    uint64_t j = j0, b = first_base + j0;
    if ((b & 3) && j < j1) {                                  // the call's first byte: the bits of earlier bases stay
        uint8_t v = packed[b >> 2] & (uint8_t)((1u << (2 * (b & 3))) - 1u);
        const uint64_t at = b >> 2;
        for (; (b & 3) && j < j1; ++j, ++b) {
            const uint8_t l = kT.code[in[j]];
            if (l & kExc) sink.add(b, in[j]);
            v |= (uint8_t)((l & 3u) << (2 * (b & 3)));
        }
        packed[at] = v;
    }
    uint8_t *o = packed + (b >> 2);
    while (j + 4 <= j1) {
        if (avx2 && j + 32 <= j1 && pack32_avx2(in + j, o)) {
            j += 32; b += 32; o += 8;
            continue;
        }
        const uint64_t stop = (avx2 && j + 32 <= j1) ? j + 32 : j + 4;   // (a group of 32 with an exception in it: the plain loop)
        for (; j < stop; j += 4, b += 4, ++o) {
            const uint8_t l0 = kT.code[in[j]], l1 = kT.code[in[j + 1]], l2 = kT.code[in[j + 2]], l3 = kT.code[in[j + 3]];
            if ((l0 | l1 | l2 | l3) & kExc) {
                if (l0 & kExc) sink.add(b, in[j]);
                if (l1 & kExc) sink.add(b + 1, in[j + 1]);
                if (l2 & kExc) sink.add(b + 2, in[j + 2]);
                if (l3 & kExc) sink.add(b + 3, in[j + 3]);
            }
            *o = (uint8_t)((l0 & 3u) | (l1 & 3u) << 2 | (l2 & 3u) << 4 | (l3 & 3u) << 6);
        }
    }
    if (j < j1) {                                             // the call's last byte: unused bits are 0
        uint8_t v = 0;
        for (; j < j1; ++j, ++b) {
            const uint8_t l = kT.code[in[j]];
            if (l & kExc) sink.add(b, in[j]);
            v |= (uint8_t)((l & 3u) << (2 * (b & 3)));
        }
        *o = v;
    }
}

// slice k of `slices`: boundaries on multiples of four bases (absolute)
uint64_t slice_start(uint64_t first_base, uint64_t n_bases, uint64_t k, uint64_t slices) {
    if (k == 0) return 0;
    if (k >= slices) return n_bases;
    const uint64_t per = (n_bases + slices - 1) / slices;
    const uint64_t at = ((first_base + k * per + 3) & ~(uint64_t)3) - first_base;
    return at < n_bases ? at : n_bases;
}

int workers_for(uint64_t n_bases, int n_threads) {
    if (n_threads <= 0) n_threads = host_threads_default();
    const uint64_t most = n_bases / kMinSliceBases;
    if ((uint64_t)n_threads > most) n_threads = (int)most;
    return n_threads < 1 ? 1 : n_threads;
}

void unpack_slice(const uint8_t *packed, uint64_t first_base, uint64_t j0, uint64_t j1, const uint64_t *exc_pos, const uint8_t *exc_byte,
                  uint64_t n_exc, uint8_t *out) {
    uint64_t j = j0, b = first_base + j0;
    for (; (b & 3) && j < j1; ++j, ++b) out[j] = (uint8_t)(kT.four[packed[b >> 2]] >> (8 * (b & 3)));
    for (; j + 4 <= j1; j += 4, b += 4) memcpy(out + j, &kT.four[packed[b >> 2]], 4);
    for (; j < j1; ++j, ++b) out[j] = (uint8_t)(kT.four[packed[b >> 2]] >> (8 * (b & 3)));
    const uint64_t *lo = std::lower_bound(exc_pos, exc_pos + n_exc, first_base + j0);
    const uint64_t *hi = std::lower_bound(lo, exc_pos + n_exc, first_base + j1);
    for (const uint64_t *p = lo; p < hi; ++p) out[*p - first_base] = exc_byte[p - exc_pos];
}

}  // namespace

void pack_reads_scalar(const uint8_t *h_bases, uint64_t first_base, uint64_t n_bases, uint8_t *h_packed, uint64_t *h_exc_pos,
                       uint8_t *h_exc_byte, uint64_t exc_cap, uint64_t *n_exc) {
    CappedSink sink{h_exc_pos, h_exc_byte, exc_cap};
    pack_slice_plain(h_bases, first_base, 0, n_bases, h_packed, sink, false);
    *n_exc = sink.n;
}

bool pack_reads(const uint8_t *h_bases, uint64_t first_base, uint64_t n_bases, uint8_t *h_packed, uint64_t *h_exc_pos,
                uint8_t *h_exc_byte, uint64_t exc_cap, uint64_t *n_exc, int n_threads) {
    const int workers = workers_for(n_bases, n_threads);
    const bool avx2 = have_avx2();
    if (workers == 1) {
        CappedSink sink{h_exc_pos, h_exc_byte, exc_cap};
        pack_slice_plain(h_bases, first_base, 0, n_bases, h_packed, sink, avx2);
        *n_exc = sink.n;
        return sink.n <= exc_cap;
    }
    std::vector<VectorSink> sinks((size_t)workers);
    std::vector<std::thread> pool;
    for (int k = 1; k < workers; k++)
        pool.emplace_back([&, k] {
            pack_slice_plain(h_bases, first_base, slice_start(first_base, n_bases, (uint64_t)k, (uint64_t)workers),
                             slice_start(first_base, n_bases, (uint64_t)k + 1, (uint64_t)workers), h_packed, sinks[(size_t)k], avx2);
        });
    pack_slice_plain(h_bases, first_base, 0, slice_start(first_base, n_bases, 1, (uint64_t)workers), h_packed, sinks[0], avx2);
    for (auto &t : pool) t.join();
    // every worker's exceptions are ascending and the slices are in order: concatenated they are the call's list
    uint64_t n = 0;
    for (const VectorSink &s : sinks) {
        const uint64_t room = n < exc_cap ? exc_cap - n : 0, take = std::min<uint64_t>(room, s.pos.size());
        if (take) {
            memcpy(h_exc_pos + n, s.pos.data(), (size_t)take * 8);
            memcpy(h_exc_byte + n, s.byte.data(), (size_t)take);
        }
        n += s.pos.size();
    }
    *n_exc = n;
    return n <= exc_cap;
}

void unpack_reads(const uint8_t *h_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *h_exc_pos,
                  const uint8_t *h_exc_byte, uint64_t n_exc, uint8_t *h_bases_out, int n_threads) {
    const int workers = workers_for(n_bases, n_threads);
    std::vector<std::thread> pool;
    for (int k = 1; k < workers; k++)
        pool.emplace_back([&, k] {
            unpack_slice(h_packed, first_base, slice_start(first_base, n_bases, (uint64_t)k, (uint64_t)workers),
                         slice_start(first_base, n_bases, (uint64_t)k + 1, (uint64_t)workers), h_exc_pos, h_exc_byte, n_exc, h_bases_out);
        });
    unpack_slice(h_packed, first_base, 0, slice_start(first_base, n_bases, 1, (uint64_t)workers), h_exc_pos, h_exc_byte, n_exc, h_bases_out);
    for (auto &t : pool) t.join();
}

}  // namespace movi

// ---- the C entry points (include/movi_hip.h): pure host code, no device is touched

using namespace movi;

static bool range_overflows(uint64_t first_base, uint64_t n_bases) { return first_base + n_bases < first_base || first_base + n_bases + 3 < 3; }

extern "C" int movi_reads_pack_host(const uint8_t *h_bases, uint64_t first_base, uint64_t n_bases, uint8_t *h_packed, uint64_t *h_exc_pos,
                                    uint8_t *h_exc_byte, uint64_t exc_cap, uint64_t *n_exc, int n_threads) {
    if (n_exc) *n_exc = 0;
    if (!n_exc || (n_bases && (!h_bases || !h_packed)) || (exc_cap && (!h_exc_pos || !h_exc_byte))) return set_last_error(MOVI_ERR_ARG, "NULL host buffer");
    if (range_overflows(first_base, n_bases)) return set_last_error(MOVI_ERR_ARG, "first_base + n_bases overflows");
    if (!pack_reads(h_bases, first_base, n_bases, h_packed, h_exc_pos, h_exc_byte, exc_cap, n_exc, n_threads))
        return set_last_error(MOVI_ERR_ARG, (std::to_string(*n_exc) + " exceptions do not fit into exc_cap = " + std::to_string(exc_cap)).c_str());
    return MOVI_OK;
}

extern "C" int movi_reads_unpack_host(const uint8_t *h_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *h_exc_pos,
                                      const uint8_t *h_exc_byte, uint64_t n_exc, uint8_t *h_bases_out, int n_threads) {
    if ((n_bases && (!h_packed || !h_bases_out)) || (n_exc && (!h_exc_pos || !h_exc_byte))) return set_last_error(MOVI_ERR_ARG, "NULL host buffer");
    if (range_overflows(first_base, n_bases)) return set_last_error(MOVI_ERR_ARG, "first_base + n_bases overflows");
    if (!exceptions_in_order(h_exc_pos, n_exc, first_base, first_base + n_bases))
        return set_last_error(MOVI_ERR_ARG, "exception positions are not strictly ascending inside [first_base, first_base + n_bases)");
    unpack_reads(h_packed, first_base, n_bases, h_exc_pos, h_exc_byte, n_exc, h_bases_out, n_threads);
    return MOVI_OK;
}
