// Host driver of movi_amd/csrc/movi_deep_fields.hpp for tests/test_deep_fields_cpu.py (built with -fsanitize=address,undefined).
//   deep_fields_driver roundtrip <seed> <n>   pack / unpack of both field maps over extreme and random field values; prints "ok <cases>"
//   deep_fields_driver map                    stdin: lines "r want_bits" -> "id_bits id_mask hint_bits j3_shift"
//   deep_fields_driver hints <reach>          stdin: r, then r letter codes, then r lines of three up-bits -> per row "h0 h1 h2"
//                                             (deep_hint_of for the letter of each threshold slot; rows of code >= 4 take none)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../movi_amd/csrc/movi_deep_fields.hpp"

static uint64_t rng_state;
static uint32_t rnd() {                                     // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int check(const DeepMap &m, const DeepFields &f) {
    uint32_t d[5], x;
    deep_pack(m, f, d, x);
    if (x >> 10) return 1;                                  // ten extra bits, no more
    const DeepFields g = deep_unpack(m, d, x);
    const uint32_t hmask = (1u << (3u * m.hint_bits)) - 1u;
    auto id = [&](uint32_t v) { return v < m.id_mask ? v : m.id_mask; };
    if (g.j != id(f.j) || g.j2 != id(f.j2) || g.j3 != id(f.j3)) return 2;
    if (g.thr != (f.thr & 7u) || g.n != f.n || g.off != f.off || g.c != f.c || g.cj != f.cj || g.cj2 != f.cj2) return 3;
    if (g.nj != f.nj || g.offj != f.offj || g.nj2 != f.nj2 || g.offj2 != f.offj2) return 4;
    if (g.hints != (f.hints & hmask)) return 5;
    for (uint32_t k = 0; k < 3; ++k)                        // the walk's reader of one slot, at the built width and switched off
        if (deep_get_hint(deep_get_hints(d[2], d[4], m.id_bits), k, m.hint_bits) != ((f.hints >> (m.hint_bits * k)) & ((1u << m.hint_bits) - 1u)) ||
            deep_get_hint(deep_get_hints(d[2], d[4], m.id_bits), k, 0u) != 0u) return 6;
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "roundtrip")) {
        rng_state = strtoull(argv[2], nullptr, 10) | 1ull;
        const long n = atol(argv[3]);
        const DeepMap maps[2] = {deep_map_for(1000, 2), deep_map_for(1000, 4)};
        long cases = 0;
        for (const DeepMap &m : maps) {
            const uint32_t ids[] = {0u, 1u, m.id_mask - 1u, m.id_mask, m.id_mask + 1u, 0x0FFFFFFFu, 0xFFFFFFFFu};
            const uint32_t e11[] = {0u, 1u, 0x3FFu, 0x400u, 0x7FFu};
            for (uint32_t a : ids) for (uint32_t b : ids) for (uint32_t c : ids)
                for (uint32_t v : e11) for (uint32_t h : {0u, 0xFFFFFFFFu, 0x555u, 0xAAAu}) {
                    DeepFields f{a, b, c, h & 7u, v, 0x7FFu - v, 7u - (v & 7u), v & 7u, (v >> 3) & 7u, 0x7FFu - v, v, v, 0x7FFu - v, h};
                    const int rc = check(m, f);
                    if (rc) { printf("extreme case fails: rc %d map %u\n", rc, m.id_bits); return 1; }
                    ++cases;
                }
            for (long i = 0; i < n; ++i) {
                DeepFields f{rnd() >> (rnd() & 7u), rnd() >> (rnd() & 7u), rnd() >> (rnd() & 7u), rnd() & 7u, rnd() & 0x7FFu, rnd() & 0x7FFu,
                             rnd() & 7u, rnd() & 7u, rnd() & 7u, rnd() & 0x7FFu, rnd() & 0x7FFu, rnd() & 0x7FFu, rnd() & 0x7FFu, rnd()};
                const int rc = check(m, f);
                if (rc) { printf("random case %ld fails: rc %d map %u\n", i, rc, m.id_bits); return 1; }
                ++cases;
            }
        }
        printf("ok %ld\n", cases);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "map")) {
        unsigned long long r; int bits;
        while (scanf("%llu %d", &r, &bits) == 2) {
            const DeepMap m = deep_map_for(r, bits);
            printf("%u %u %u %u\n", m.id_bits, m.id_mask, m.hint_bits, m.j3_shift);
        }
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "hints")) {
        const uint32_t reach = (uint32_t)atoi(argv[2]);
        unsigned long long r;
        if (scanf("%llu", &r) != 1) return 2;
        std::vector<uint32_t> codes(r), up(3 * r);
        for (auto &c : codes) if (scanf("%u", &c) != 1) return 2;
        for (auto &u : up) if (scanf("%u", &u) != 1) return 2;
        auto c_of = [&](uint64_t t) { return codes[t]; };
        for (uint64_t i = 0; i < r; ++i) {
            uint32_t h[3] = {0, 0, 0};
            const uint32_t c = codes[i];
            for (uint32_t k = 0; k < 3 && c < 4; ++k) {
                const uint32_t a = k < c ? k : k + 1u;
                if (a > 3u) continue;
                h[k] = deep_hint_of(c_of, r, i, a, up[3 * i + k] == 0u, reach);
            }
            printf("%u %u %u\n", h[0], h[1], h[2]);
        }
        return 0;
    }
    fprintf(stderr, "usage: deep_fields_driver roundtrip <seed> <n> | map | hints <reach>\n");
    return 2;
}
