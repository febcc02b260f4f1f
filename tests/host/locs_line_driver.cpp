// Test driver of tests/test_locate_matches_cpu.py: one line through the writers of `movi query --count --locate` and `--mem --locate`
// (append_count_locs_line, append_mem_locs_line, movi_amd/host/output.cpp).  argv: count id query_length matched occ [position]...
// or: mem id start end occ [position]... -- the positions given are the listed ones; the line goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../movi_amd/host/output.hpp"

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const uint64_t a = strtoull(argv[3], nullptr, 10), b = strtoull(argv[4], nullptr, 10), occ = strtoull(argv[5], nullptr, 10);
    std::vector<uint64_t> pos;
    for (int i = 6; i < argc; i++) pos.push_back(strtoull(argv[i], nullptr, 10));
    std::string txt;
    if (!strcmp(argv[1], "count")) movi_host::append_count_locs_line(txt, argv[2], a, b, occ, pos.data(), pos.size());
    else if (!strcmp(argv[1], "mem")) movi_host::append_mem_locs_line(txt, argv[2], a, b, occ, pos.data(), pos.size());
    else return 2;
    fwrite(txt.data(), 1, txt.size(), stdout);
    return 0;
}
