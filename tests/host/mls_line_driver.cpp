// Test driver of tests/test_color_cpu.py: report lines of `movi query --multi-classify` through its writer (append_mls_line,
// movi_amd/host/output.cpp).  stdin, one read per line: id length best second colors_count sum_ml report_all min_diff_frac min_score_frac
// n_species, then n_species taxa, then n_species counters.  The lines go to stdout.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../movi_amd/host/output.hpp"

int main() {
    std::string id, out;
    uint64_t len;
    unsigned best, second, colors, sum, all, ns;
    float mdf, msf;
    while (std::cin >> id >> len >> best >> second >> colors >> sum >> all >> mdf >> msf >> ns) {
        std::vector<uint32_t> taxa(ns), cnt(ns);
        for (auto &t : taxa) std::cin >> t;
        for (auto &c : cnt) std::cin >> c;
        movi_mc_read_t r{};
        r.best = (uint16_t)best;
        r.second = (uint16_t)second;
        r.colors_count = colors;
        r.sum_ml = sum;
        r.best_count = best < ns ? cnt[best] : 0;
        r.second_count = second < ns ? cnt[second] : 0;
        movi_host::append_mls_line(out, id, len, r, cnt.data(), taxa, all != 0, mdf, msf);
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
