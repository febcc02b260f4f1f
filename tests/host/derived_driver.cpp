// Test driver of tests/test_derived_cpu.py: the rules of movi_amd/csrc/movi_derived.hpp on a scripted device, without a GPU.
// stdin: one case per line (lines that start with '#' are skipped):
//   kmode r dna total free mem_fails sample full fail_mask : step step ...
//   kmode, r, dna      the table's facts (dna: four letters besides the separator)
//   total, free        what the device's memory query answers, in bytes; mem_fails 1: the query itself fails
//   sample             the share a sample of the rows gives, or x: the sample fails
//   full               the share the builder of the look-ahead rows tallies over every row
//   fail_mask          builds that fail: 1 kmer, 2 ftab, 4 ahead, 8 deep, 16 ckpt
//   steps, run in order on one handle:
//     P                a PML query                      C       a count query (also what MEM and k-mer queries call)
//     Rp / Rc / Rpc    movi_index_prepare with those bits
//     S key value      movi_set_option: kmer_k, ftab_k, ahead_rows, deep_rows (the build-now options), deep_hint_bits, count_variant
//     F bytes          from here on the device answers this many free bytes
//     xN               the step before it runs N times in all
// stdout, one line per case:
//   the device calls in order, each as step:call (steps count from 1, a repeated step once per run) --
//     mem | sample | kmer K | ftab K | ckpt | ahead auto | ahead asked | deep B | drop T -- and what a step itself reports:
//     refused (a build-now option on an ineligible table), failed (its build failed, or the count tables' checkpoints)
//   | held  kmer ftab ahead deep ckpt (0 / 1 each)  rows2_count  the deep rows' hint width (0 = none held)
//   | policy  kmer_auto ftab_auto ahead_auto deep_auto deep_hint_bits ahead_retry_in count_declined_ahead ahead_tallied ahead_no_ff prepared
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../movi_amd/csrc/movi_derived.hpp"

using namespace movi;

static const char *const kNames[kDerivedTables] = {"kmer", "ftab", "ahead", "deep", "ckpt"};

struct FakeDev {
    explicit FakeDev(DerivedFacts &f) : facts(f) {}
    DerivedFacts &facts;
    uint64_t total = 0, free_b = 0;
    bool mem_fails = false, sample_fails = false;
    double sample = 0.0, full = 0.0;
    unsigned fail_mask = 0;
    int step = 0;
    bool rows2_count = false;
    int deep_width = 0;
    std::string trace;
    void say(const std::string &what) { trace += (trace.empty() ? "" : " ") + std::to_string(step) + ":" + what; }
    bool built(DerivedTable t) {
        if (fail_mask & (1u << t)) return false;
        facts.held[t] = true;
        return true;
    }
    bool mem_info(uint64_t &f, uint64_t &t) {
        say("mem");
        if (mem_fails) return false;
        f = free_b; t = total;
        return true;
    }
    bool sample_no_ff(double &share) {
        say("sample");
        if (sample_fails) return false;
        share = sample;
        return true;
    }
    bool build_kmer(uint32_t K) { say("kmer " + std::to_string(K)); return built(kTabKmer); }
    bool build_ftab(uint32_t K) { say("ftab " + std::to_string(K)); return built(kTabFtab); }
    bool build_ckpt() { say("ckpt"); return built(kTabCkpt); }
    bool build_deep(int hint_bits) {
        say("deep " + std::to_string(hint_bits));
        if (!built(kTabDeep)) return false;
        deep_width = hint_bits;
        return true;
    }
    bool build_ahead(bool by_itself, double &share, bool &serves_count) {
        say(by_itself ? "ahead auto" : "ahead asked");
        if (!built(kTabAhead)) return false;
        share = full;
        serves_count = rows2_count = ahead_serves_count(by_itself, full);
        return true;
    }
    void drop(DerivedTable t) {
        say(std::string("drop ") + kNames[t]);
        facts.held[t] = false;
        if (t == kTabAhead) rows2_count = false;
        if (t == kTabDeep) deep_width = 0;
    }
};

static bool run_step(const std::vector<std::string> &st, DerivedPolicy &p, DerivedFacts &f, FakeDev &dev) {
    const std::string &op = st[0];
    if (op == "P") {
        ensure_pml_tables(p, f, dev, false);
    } else if (op == "C") {
        if (!ensure_count_tables(p, f, dev, false)) dev.say("failed");
    } else if (op[0] == 'R') {
        on_prepare(p);
        if (op.find('p') != std::string::npos) ensure_pml_tables(p, f, dev, true);
        if (op.find('c') != std::string::npos && !ensure_count_tables(p, f, dev, true)) { dev.say("failed"); return true; }
        on_prepared(p);
    } else if (op == "F") {
        dev.free_b = strtoull(st[1].c_str(), nullptr, 10);
    } else if (op == "S") {
        const long long v = atoll(st[2].c_str());
        if (st[1] == "deep_hint_bits") { p.deep_hint_bits = (int)v; return true; }
        if (st[1] == "count_variant") { f.count_variant = (int)v; return true; }
        const DerivedTable t = st[1] == "kmer_k" ? kTabKmer : st[1] == "ftab_k" ? kTabFtab : st[1] == "ahead_rows" ? kTabAhead : st[1] == "deep_rows" ? kTabDeep : kDerivedTables;
        if (t == kDerivedTables) return false;
        const TableRequest got = request_table(p, f, dev, t, (uint32_t)v);
        if (got == TableRequest::kIneligible) dev.say("refused");
        if (got == TableRequest::kBuildFailed) dev.say("failed");
    } else {
        return false;
    }
    return true;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        std::vector<std::string> w;
        for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) w.push_back(t);
        if (w.size() < 11 || w[9] != ":") { fprintf(stderr, "bad case\n"); return 2; }
        DerivedPolicy p;
        DerivedFacts f;
        f.kmode = atoi(w[0].c_str());
        f.r = strtoull(w[1].c_str(), nullptr, 10);
        f.dna = w[2] != "0";
        f.ahead_bytes = ((f.r + 7) / 8 + 1) * 128;               // ahead_rows_bytes, movi_kernels.hip
        f.deep_bytes = ((f.r + 2) / 3) * 64;                     // deep_rows_bytes
        FakeDev dev(f);
        dev.total = strtoull(w[3].c_str(), nullptr, 10);
        dev.free_b = strtoull(w[4].c_str(), nullptr, 10);
        dev.mem_fails = w[5] != "0";
        dev.sample_fails = w[6] == "x";
        dev.sample = dev.sample_fails ? 0.0 : strtod(w[6].c_str(), nullptr);
        dev.full = strtod(w[7].c_str(), nullptr);
        dev.fail_mask = (unsigned)atoi(w[8].c_str());
        std::vector<std::string> prev;
        for (size_t i = 10; i < w.size();) {
            std::vector<std::string> st;
            int times = 1;
            if (w[i][0] == 'x' && !prev.empty()) { st = prev; times = atoi(w[i].c_str() + 1) - 1; i += 1; }
            else {
                const size_t n = w[i] == "S" ? 3 : w[i] == "F" ? 2 : 1;
                if (i + n > w.size()) { fprintf(stderr, "bad step\n"); return 2; }
                st.assign(w.begin() + (long)i, w.begin() + (long)(i + n));
                i += n;
            }
            for (int k = 0; k < times; k++) {
                dev.step += 1;
                if (!run_step(st, p, f, dev)) { fprintf(stderr, "bad step: %s\n", st[0].c_str()); return 2; }
            }
            prev = st;
        }
        printf("%s | held %d %d %d %d %d %d %d | policy %d %d %d %d %d %d %d %d %.4f %d\n", dev.trace.empty() ? "-" : dev.trace.c_str(),
               (int)f.held[kTabKmer], (int)f.held[kTabFtab], (int)f.held[kTabAhead], (int)f.held[kTabDeep], (int)f.held[kTabCkpt],
               (int)dev.rows2_count, dev.deep_width, p.kmer_auto, p.ftab_auto, p.ahead_auto, p.deep_auto, p.deep_hint_bits, p.ahead_retry_in,
               (int)p.count_declined_ahead, (int)p.ahead_tallied, p.ahead_no_ff, (int)p.prepared);
    }
    return 0;
}
