// Test driver of tests/test_sa_cpu.py: one record of <prefix>.sa_entries.bpf through the writer of `movi query --sa-entries`
// (append_sa_record, movi_amd/host/output.cpp).  argv: id [entry]...; the record goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../movi_amd/host/output.hpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<uint64_t> e;
    for (int i = 2; i < argc; i++) e.push_back(strtoull(argv[i], nullptr, 10));
    std::string rec;
    movi_host::append_sa_record(rec, argv[1], e.data(), e.size());
    fwrite(rec.data(), 1, rec.size(), stdout);
    return 0;
}
