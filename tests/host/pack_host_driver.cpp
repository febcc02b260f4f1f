// pack_host_driver.cpp -- stand-alone driver of movi_amd/csrc/movi_pack_host.cpp for a sanitizer build (host code only, no GPU):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pack_host_driver tests/host/pack_host_driver.cpp \
//       movi_amd/csrc/movi_pack_host.cpp movi_amd/csrc/movi_expand_host.cpp -lpthread && ./pack_host_driver
// Round trips of tests/test_packed_reads_cpu.py in buffers of EXACTLY the stated sizes (heap allocations: a byte too far is a
// report): all 256 byte values, ACGT only, N at 0.1 %; every length 0 .. 70 and lengths that go to worker threads; first_base
// 0 .. 7; 1 and 4 threads; the vector loop against the plain one; exc_cap one too small.
#include "../../movi_amd/csrc/movi_pack_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace movi;

int movi::set_last_error(int code, const char *) { return code; }   // (the library's is in movi_abi.hip: not part of this build)

static int g_cases = 0;

#define REQUIRE(c)                                                                     \
    do {                                                                               \
        if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

static void one(const std::vector<uint8_t> &x, uint64_t first_base, int threads) {
    const uint64_t n = x.size(), nbytes = packed_bytes(first_base, n);
    // exactly-sized heap buffers; the bases from first_base on only (the packed buffer starts at base 0)
    uint8_t *in = static_cast<uint8_t *>(malloc(n ? n : 1));
    if (n) memcpy(in, x.data(), n);
    uint8_t *packed = static_cast<uint8_t *>(calloc(nbytes ? nbytes : 1, 1));
    uint8_t *packed_ref = static_cast<uint8_t *>(calloc(nbytes ? nbytes : 1, 1));
    uint64_t need = 0, got = 0;
    pack_reads_scalar(in, first_base, n, packed_ref, nullptr, nullptr, 0, &need);      // count
    uint64_t *pos = static_cast<uint64_t *>(malloc(need ? need * 8 : 1)), *pos_ref = static_cast<uint64_t *>(malloc(need ? need * 8 : 1));
    uint8_t *byte = static_cast<uint8_t *>(malloc(need ? need : 1)), *byte_ref = static_cast<uint8_t *>(malloc(need ? need : 1));
    pack_reads_scalar(in, first_base, n, packed_ref, pos_ref, byte_ref, need, &got);
    REQUIRE(got == need);
    REQUIRE(pack_reads(in, first_base, n, packed, pos, byte, need, &got, threads) && got == need);
    REQUIRE(memcmp(packed, packed_ref, nbytes) == 0);
    REQUIRE(need == 0 || (memcmp(pos, pos_ref, need * 8) == 0 && memcmp(byte, byte_ref, need) == 0));
    REQUIRE(exceptions_in_order(pos, need, first_base, first_base + n));
    uint8_t *back = static_cast<uint8_t *>(malloc(n ? n : 1));
    unpack_reads(packed, first_base, n, pos, byte, need, back, threads);
    REQUIRE(n == 0 || memcmp(back, in, n) == 0);
    if (need) {                                                                        // one too small: reported, nothing past the caps
        uint64_t *pos1 = static_cast<uint64_t *>(malloc(need > 1 ? (need - 1) * 8 : 1));
        uint8_t *byte1 = static_cast<uint8_t *>(malloc(need > 1 ? need - 1 : 1));
        REQUIRE(!pack_reads(in, first_base, n, packed, pos1, byte1, need - 1, &got, threads) && got == need);
        free(pos1);
        free(byte1);
    }
    free(in); free(packed); free(packed_ref); free(pos); free(pos_ref); free(byte); free(byte_ref); free(back);
    ++g_cases;
}

int main() {
    std::mt19937_64 rng(7);
    auto make = [&](int kind, uint64_t n) {
        std::vector<uint8_t> x(n);
        for (auto &c : x) {
            if (kind == 0) c = (uint8_t)(rng() & 0xFF);
            else c = (uint8_t)"ACGT"[rng() & 3];
            if (kind == 2 && rng() % 1000 == 0) c = 'N';
        }
        if (kind == 2 && n) x[rng() % n] = 'N';
        return x;
    };
    for (int threads : {1, 4})
        for (uint64_t first_base = 0; first_base < 8; first_base++) {
            for (uint64_t n = 0; n <= 70; n++)
                for (int kind = 0; kind < 3; kind++) one(make(kind, n), first_base, threads);
            for (int kind = 0; kind < 3; kind++) one(make(kind, 4 * 65536 + 77 + first_base), first_base, threads);
        }
    printf("pack_host_driver: %d cases ok\n", g_cases);
    return 0;
}
