// Test driver of tests/test_kmer_occ_cpu.py: one line through the writer of `movi query --kmer-occ` (append_kmer_occ_line,
// movi_amd/host/output.cpp).  argv: id query_length k found sum [occ]... -- one value per base of the read, as the engine returns
// them (the writer prints the first max(0, query_length - k + 1)); the line goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../movi_amd/host/output.hpp"

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const uint64_t len = strtoull(argv[2], nullptr, 10);
    std::vector<uint64_t> occ;
    for (int i = 6; i < argc; i++) occ.push_back(strtoull(argv[i], nullptr, 10));
    if (occ.size() != len) return 2;
    std::string txt;
    movi_host::append_kmer_occ_line(txt, argv[1], len, (uint32_t)strtoul(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10),
                                    strtoull(argv[5], nullptr, 10), occ.data());
    fwrite(txt.data(), 1, txt.size(), stdout);
    return 0;
}
