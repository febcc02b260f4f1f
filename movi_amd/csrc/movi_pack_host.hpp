// movi_pack_host.hpp -- reads packed two bits per base (the format of include/movi_hip.h, "2-bit packed reads") on the host:
// the packer a caller runs while it parses, and its exact inverse (what the tests hold the device's unpack kernels to).
// Pure C++ (no HIP): compiled by g++.
#pragma once
#include <stdint.h>

namespace movi {

// Base b (absolute, the numbering of offsets[]) lives in byte b >> 2 of the packed buffer at bits 2 * (b & 3); A = 0, C = 1,
// G = 2, T = 3.  Every other byte value is an exception: code 0 in the stream, (position, byte) in the sparse list.
inline uint64_t packed_bytes(uint64_t first_base, uint64_t n_bases) { return (first_base + n_bases + 3) >> 2; }

// h_bases[j] is base first_base + j.  Bits of the first byte that belong to bases before first_base are kept as they are (a
// caller appends batch after batch to one buffer); bits of the last byte past the range are written 0.  Exceptions: absolute
// positions, ascending, at most exc_cap of them are written; *n_exc = how many there are.  Returns false when they did not fit.
// n_threads workers on slices aligned to four bases (<= 0: host_threads_default(); short inputs stay on the calling thread).
bool pack_reads(const uint8_t *h_bases, uint64_t first_base, uint64_t n_bases, uint8_t *h_packed, uint64_t *h_exc_pos,
                uint8_t *h_exc_byte, uint64_t exc_cap, uint64_t *n_exc, int n_threads);
void pack_reads_scalar(const uint8_t *h_bases, uint64_t first_base, uint64_t n_bases, uint8_t *h_packed, uint64_t *h_exc_pos,
                       uint8_t *h_exc_byte, uint64_t exc_cap, uint64_t *n_exc);   // the plain loop (what the tests hold the vector code to)

// The inverse: h_bases_out[j] = base first_base + j.  The exceptions must be ascending and inside the range: the caller checks
// (exceptions_in_order).
void unpack_reads(const uint8_t *h_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *h_exc_pos,
                  const uint8_t *h_exc_byte, uint64_t n_exc, uint8_t *h_bases_out, int n_threads);
// strictly ascending and inside [lo, hi)
inline bool exceptions_in_order(const uint64_t *h_exc_pos, uint64_t n_exc, uint64_t lo, uint64_t hi) {
    if (n_exc == 0) return true;
    if (h_exc_pos[0] < lo || h_exc_pos[n_exc - 1] >= hi) return false;
    uint64_t bad = 0;
    for (uint64_t i = 1; i < n_exc; i++) bad |= (uint64_t)(h_exc_pos[i] <= h_exc_pos[i - 1]);
    return bad == 0;
}

// movi_reads_pack_host and movi_reads_unpack_host (include/movi_hip.h) are defined in movi_pack_host.cpp itself: nothing else of the
// library needs that file, so a build of the other translation units alone still links.  Their error messages reach movi_last_error
// through this hook, which movi_abi.hip defines (returns `code`).
int set_last_error(int code, const char *msg);

}  // namespace movi
