// Test driver of tests/test_chain_fields_cpu.py: the chain rows' field map (movi_amd/csrc/movi_chain_fields.hpp) without a GPU.
//   roundtrip SEED N   every field at its extremes (all combinations of {0, 1, max - 1, max} per group) and N random rows through
//                      chain_pack / chain_unpack and the walk's readers; prints "ok <rows checked>"
//   fields             stdin: r end_row, then r lines "id n off c thr": prints, per row i < padded r, the unpacked fields of
//                      chain_fields_of: j1 j2 j3 j4 | c n off thr | cj1 nj1 offj1 | cj2 nj2 offj2 | cj3 nj3 offj3 | nj4
//   hints REACH        stdin: r, the r letter codes, then r lines of three up bits: prints per row the three hints of chain_hint_of
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../movi_amd/csrc/movi_chain_fields.hpp"

static bool same(const ChainFields &a, const ChainFields &b) {
    for (int t = 0; t < 4; ++t) if (a.j[t] != b.j[t]) return false;
    for (int t = 0; t < 3; ++t) if (a.cj[t] != b.cj[t] || a.nj[t] != b.nj[t] || a.offj[t] != b.offj[t]) return false;
    return a.thr == b.thr && a.n == b.n && a.off == b.off && a.c == b.c && a.nj4 == b.nj4 && a.hints == b.hints;
}

static int check(const ChainFields &f) {
    uint32_t d[8];
    chain_pack(f, d);
    ChainFields want = f;
    for (int t = 0; t < 4; ++t) want.j[t] = f.j[t] < kChainIdMask ? f.j[t] : kChainIdMask;   // any id that is no 28-bit row index: "not a row"
    const ChainFields g = chain_unpack(d);
    if (!same(g, want)) return 1;
    // the walk's readers, dword by dword
    if (chain_get_id(d[0]) != want.j[0] || chain_get_id(d[2]) != want.j[1] || chain_get_id(d[4]) != want.j[2] || chain_get_id(d[6]) != want.j[3]) return 2;
    for (uint32_t k = 0; k < 3; ++k) {
        if (chain_get_thr(d[0], k) != ((f.thr >> k) & 1u)) return 3;
        if (chain_get_hint(d[2 + 2 * k]) != ((f.hints >> (4 * k)) & 15u)) return 4;
    }
    if (chain_get_n(d[1]) != f.n || chain_get_off(d[1]) != f.off || chain_get_c(d[1]) != f.c) return 5;
    if (chain_get_cj1(d[1]) != f.cj[0] || chain_get_cj2(d[1]) != f.cj[1] || chain_get_cj3(d[5]) != f.cj[2]) return 6;
    for (int t = 0; t < 3; ++t) if (chain_get_n(d[3 + 2 * t]) != f.nj[t] || chain_get_off(d[3 + 2 * t]) != f.offj[t]) return 7;
    if (chain_get_nj4(d[0], d[7]) != f.nj4) return 8;
    return 0;
}

static int roundtrip(uint64_t seed, long n_random) {
    const uint32_t ids[] = {0u, 1u, kChainIdMask - 1u, kChainIdMask, 0x10000005u, 0xFFFFFFFFu};      // (the last three: not a row; 2^28 + 5 cut to 28 bits would be row 5)
    const uint32_t e11[] = {0u, 1u, 0x7FEu, 0x7FFu};
    const uint32_t c3[] = {0u, 3u, 4u, 7u};
    long rows = 0;
    ChainFields f;
    // one group of fields at its extremes at a time, the others at a pattern that a wrong shift would disturb
    for (int group = 0; group < 6; ++group)
        for (uint32_t x : ids) for (uint32_t y : e11) for (uint32_t z : e11) for (uint32_t w : c3) for (uint32_t h : {0u, 1u, 14u, 15u}) {
            for (int t = 0; t < 4; ++t) f.j[t] = 0x05555555u;
            for (int t = 0; t < 3; ++t) { f.cj[t] = 5u; f.nj[t] = 0x2AAu; f.offj[t] = 0x555u; }
            f.thr = 5u; f.n = 0x555u; f.off = 0x2AAu; f.c = 2u; f.nj4 = 0x4D2u; f.hints = 0xA5Au;
            if (group < 4) f.j[group] = x; else f.j[0] = f.j[3] = x;
            if (group < 3) { f.nj[group] = y; f.offj[group] = z; f.cj[group] = w; f.hints = (f.hints & ~(15u << (4 * group))) | (h << (4 * group)); }
            else if (group == 3) { f.n = y; f.off = z; f.c = w; f.thr = h & 7u; }
            else if (group == 4) { f.nj4 = y; f.nj[2] = z; f.offj[2] = y; f.cj[2] = w; }
            else { f.nj4 = z; f.thr = w & 7u; f.hints = h | (h << 4) | (h << 8); f.cj[0] = w; f.cj[1] = 7u - w; }
            if (int e = check(f)) { printf("mismatch %d in group %d\n", e, group); return 1; }
            rows += 1;
        }
    std::mt19937_64 rng(seed);
    for (long i = 0; i < n_random; ++i) {
        for (int t = 0; t < 4; ++t) f.j[t] = (uint32_t)rng() >> ((rng() & 3u) == 0 ? 0 : 4);
        for (int t = 0; t < 3; ++t) { f.cj[t] = rng() & 7u; f.nj[t] = rng() & 0x7FFu; f.offj[t] = rng() & 0x7FFu; }
        f.thr = rng() & 7u; f.n = rng() & 0x7FFu; f.off = rng() & 0x7FFu; f.c = rng() & 7u; f.nj4 = rng() & 0x7FFu; f.hints = rng() & 0xFFFu;
        if (int e = check(f)) { printf("mismatch %d in random row %ld\n", e, i); return 1; }
        rows += 1;
    }
    printf("ok %ld\n", rows);
    return 0;
}

struct Row { uint64_t id; uint32_t n, off, c, thr; };

static int fields() {
    uint64_t r = 0, end_row = 0;
    if (scanf("%" SCNu64 " %" SCNu64, &r, &end_row) != 2) return 2;
    std::vector<Row> rows(r);
    for (auto &w : rows) if (scanf("%" SCNu64 " %u %u %u %u", &w.id, &w.n, &w.off, &w.c, &w.thr) != 5) return 2;
    auto row_of = [&rows](uint64_t t, uint64_t &id, uint32_t &n, uint32_t &off, uint32_t &c, uint32_t &thr) {
        const Row &w = rows.at(t);                       // (a read beyond the table throws: the rule must ask for rows only)
        id = w.id; n = w.n; off = w.off; c = w.c; thr = w.thr;
    };
    const uint64_t padded = (r + 1) / 2 * 2;
    if (chain_rows_bytes_of(r) != padded * kChainRowBytes) return 3;
    for (uint64_t i = 0; i < padded; ++i) {
        uint32_t d[8];
        chain_pack(chain_fields_of(row_of, r, end_row, i), d);
        const ChainFields f = chain_unpack(d);
        printf("%u %u %u %u | %u %u %u %u | %u %u %u | %u %u %u | %u %u %u | %u\n", f.j[0], f.j[1], f.j[2], f.j[3], f.c, f.n, f.off, f.thr,
               f.cj[0], f.nj[0], f.offj[0], f.cj[1], f.nj[1], f.offj[1], f.cj[2], f.nj[2], f.offj[2], f.nj4);
    }
    return 0;
}

static int hints(uint32_t reach) {
    uint64_t r = 0;
    if (scanf("%" SCNu64, &r) != 1) return 2;
    std::vector<uint32_t> codes(r), up(3 * r);
    for (auto &c : codes) if (scanf("%u", &c) != 1) return 2;
    for (auto &u : up) if (scanf("%u", &u) != 1) return 2;
    auto c_of = [&codes](uint64_t t) { return codes.at(t); };
    for (uint64_t i = 0; i < r; ++i) {
        uint32_t h[3] = {0, 0, 0};
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t c = codes[i], a = k < c ? k : k + 1u;
            if (c > 3u || a > 3u) continue;
            h[k] = chain_hint_of(c_of, r, i, a, up[3 * i + k] == 0, reach);
        }
        printf("%u %u %u\n", h[0], h[1], h[2]);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "roundtrip")) return roundtrip(strtoull(argv[2], nullptr, 10), atol(argv[3]));
    if (argc >= 2 && !strcmp(argv[1], "fields")) return fields();
    if (argc >= 3 && !strcmp(argv[1], "hints")) return hints((uint32_t)atoi(argv[2]));
    fprintf(stderr, "usage: chain_fields_driver roundtrip SEED N | fields | hints REACH\n");
    return 2;
}
