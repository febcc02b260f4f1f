// rlbwt_check_driver.cpp -- TEST INFRASTRUCTURE: movi::rlbwt_check (movi_amd/csrc/movi_build.hpp) on tables given on stdin, for
// tests/test_rlbwt_check_cpu.py, which compiles it with -fsanitize=address,undefined.
//   stdin : R with_thr, then R lines "head length threshold" (head: the byte's value; all decimal, up to 2^64 - 1)
//   stdout: "ok n sigma sep end_run alphabet[0] counts[0] ... " or "refused WHICH WHY" (WHICH: heads, lens or thr)
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "../../movi_amd/csrc/movi_build.hpp"

int main() {
    uint64_t R = 0;
    int with_thr = 0;
    if (scanf("%" SCNu64 " %d", &R, &with_thr) != 2) return 2;
    std::vector<uint8_t> heads(R);
    std::vector<uint64_t> lens(R), thr(R);
    for (uint64_t k = 0; k < R; k++) {
        unsigned h = 0;
        if (scanf("%u %" SCNu64 " %" SCNu64, &h, &lens[k], &thr[k]) != 3 || h > 255) return 2;
        heads[k] = (uint8_t)h;
    }
    movi::RlbwtInfo info;
    movi::RlbwtArray which;
    std::string why;
    if (!movi::rlbwt_check(heads.data(), lens.data(), with_thr ? thr.data() : nullptr, R, info, which, why)) {
        printf("refused %s %s\n", which == movi::kRlbwtHeads ? "heads" : which == movi::kRlbwtLens ? "lens" : "thr", why.c_str());
        return 0;
    }
    printf("ok %" PRIu64 " %u %u %" PRIu64, info.n, info.sigma, info.sep, info.end_run);
    for (uint32_t a = 0; a < info.sigma; a++) printf(" %u %" PRIu64, (unsigned)info.alphabet[a], info.counts[a]);
    printf("\n");
    return 0;
}
