// movi_walk_pack.hip -- reads packed two bits per base (include/movi_hip.h, "2-bit packed reads") back to the byte per base that
// every walk kernel stages from: movi_reads_unpack_device, and the packed *_host entry points in front of a chunk's walk.
// Streams 1/4 byte in and 1 byte out per base; the walk behind it moves about 60 bytes of fabric lines per base.
#include "movi_kernels.hpp"

namespace movi {

constexpr int kUnpackThreads = 256;
constexpr uint32_t kAcgt = 0x54474341u;        // 'A' | 'C' << 8 | 'G' << 16 | 'T' << 24: byte c is the letter of code c

// eight bits of codes (four bases) -> four selector bytes 0..3, first base in the low byte
__device__ __forceinline__ uint32_t spread4(uint32_t x) {
    x = (x | (x << 12)) & 0x000F000Fu;
    return (x | (x << 6)) & 0x03030303u;
}
// ... -> their letters: a byte permute against the constant (selectors 0..3 pick from the second operand), no memory lookup
__device__ __forceinline__ uint32_t letters4(uint32_t x) { return __builtin_amdgcn_perm(0u, kAcgt, spread4(x & 0xFFu)); }

// One thread, 16 output bases: group g holds out[16 g - shift, 16 g - shift + 16), shift = the output pointer's low four
// bits, so every group that lies wholly inside [0, n) leaves in one aligned 16-byte store.  Its codes are 32 bits of the packed
// stream from bit 2 * ((first_base + j) & 3) of byte (first_base + j) >> 2: the (at most two) aligned dwords that hold them,
// funnel-shifted.  An aligned dword is only fetched if the group needs a byte of it, so no fetch leaves the aligned dwords the
// caller's packed bytes lie in.  The range's first and last partial groups take byte loads and byte stores inside [0, n).
__global__ __launch_bounds__(kUnpackThreads) void unpack_reads_kernel(const uint8_t *__restrict__ packed, uint64_t first_base, uint64_t n,
                                                                      uint8_t *__restrict__ out, uint32_t shift, uint64_t n_groups) {
    const uint64_t stride = (uint64_t)gridDim.x * kUnpackThreads;
    for (uint64_t g = (uint64_t)blockIdx.x * kUnpackThreads + threadIdx.x; g < n_groups; g += stride) {
        const uint64_t lo = g * 16 >= shift ? g * 16 - shift : 0;              // the group's bases inside the range: [lo, hi)
        const uint64_t end = g * 16 - shift + 16;                              // (g == 0: 16 - shift, no wrap)
        const uint64_t hi = end < n ? end : n;
        if (hi - lo == 16) {
            const uint64_t b = first_base + lo;
            const uint8_t *p = packed + (b >> 2);
            const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
            const uint32_t *w = reinterpret_cast<const uint32_t *>(p - mis);       // (pointer arithmetic, not integer: the loads stay global loads)
            const uint32_t sh = 8u * mis + 2u * (uint32_t)(b & 3);                 // 0 .. 30
            const uint32_t w0 = w[0], w1 = sh ? w[1] : 0u;
            const uint32_t c = __funnelshift_r(w0, w1, sh);
            uint4 v;
            v.x = letters4(c);
            v.y = letters4(c >> 8);
            v.z = letters4(c >> 16);
            v.w = letters4(c >> 24);
            *reinterpret_cast<uint4 *>(out + lo) = v;
        } else {
            for (uint64_t j = lo; j < hi; ++j) {
                const uint64_t b = first_base + j;
                out[j] = (uint8_t)(kAcgt >> (8u * ((packed[b >> 2] >> (2u * (uint32_t)(b & 3))) & 3u)));
            }
        }
    }
}

// One thread, one exception: behind the kernel above on the same stream.  A position outside the range is not written.
__global__ __launch_bounds__(kUnpackThreads) void unpack_exceptions_kernel(const uint64_t *__restrict__ exc_pos, const uint8_t *__restrict__ exc_byte,
                                                                           uint64_t n_exc, uint64_t origin, uint64_t n, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kUnpackThreads + threadIdx.x;
    if (i >= n_exc) return;
    const uint64_t j = exc_pos[i] - origin;
    if (j < n) out[j] = exc_byte[i];
}

hipError_t launch_unpack_reads(const uint8_t *d_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *d_exc_pos,
                               const uint8_t *d_exc_byte, uint64_t n_exc, uint64_t exc_origin, uint8_t *d_out, hipStream_t stream) {
    if (n_bases == 0) return hipSuccess;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    const uint64_t n_groups = (n_bases + shift + 15) / 16;
    uint64_t blocks = (n_groups + kUnpackThreads - 1) / kUnpackThreads;
    if (blocks > (1u << 20)) blocks = 1u << 20;                               // (the kernel strides)
    note_walk_launch("unpack_reads_kernel");
    hipLaunchKernelGGL(unpack_reads_kernel, dim3((unsigned)blocks), dim3(kUnpackThreads), 0, stream, d_packed, first_base, n_bases, d_out, shift,
                       n_groups);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_exc == 0) return e;
    const uint64_t eblocks = (n_exc + kUnpackThreads - 1) / kUnpackThreads;
    if (eblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    note_walk_launch("unpack_exceptions_kernel");
    hipLaunchKernelGGL(unpack_exceptions_kernel, dim3((unsigned)eblocks), dim3(kUnpackThreads), 0, stream, d_exc_pos, d_exc_byte, n_exc, exc_origin,
                       n_bases, d_out);
    return hipGetLastError();
}

hipError_t preload_pack() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&unpack_reads_kernel));
}

}  // namespace movi
