// Test driver of tests/test_kmer_cpu.py: one k-mer line through the writer of `movi query --kmer` (append_kmer_line,
// movi_amd/host/output.cpp).  argv: id query_length k found [start count]...; the line goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../movi_amd/host/output.hpp"

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 5) % 2) return 2;
    std::vector<movi_kmer_run_t> runs;
    for (int i = 5; i + 1 < argc; i += 2)
        runs.push_back(movi_kmer_run_t{(uint32_t)strtoul(argv[i], nullptr, 10), (uint32_t)strtoul(argv[i + 1], nullptr, 10)});
    std::string txt;
    movi_host::append_kmer_line(txt, argv[1], strtoull(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10),
                                strtoull(argv[4], nullptr, 10), runs.data(), runs.size());
    fwrite(txt.data(), 1, txt.size(), stdout);
    return 0;
}
