// Test driver of tests/test_host_plan_cpu.py: the plan of a *_host call (movi_amd/csrc/movi_host_plan.hpp), printed without a GPU.
// stdin: one case per line (lines that start with '#' are skipped), 22 integers:
//   query (0 PML/ZML, 1 logs, 2 sa-entries, 3 count/classify, 4 multi-classify, 5 MEM/k-mer)  zml  want_vector  want_words
//   reads_pinned  vector_pinned  small_bytes   host_overlap host_autopin host_masks host_mask_share pipe_chunk_bases seg_seen seg_len
//   pin_ok (page-locking for the call, where the plan tries it, succeeds)   packed (reads two bits per base)
//   n_reads off0 pattern a b seed      the offsets, made here (no bases are allocated): offsets[0] = off0, then read lengths by pattern --
//     0: a   1: a, b alternating   2: a, but b reads from n_reads / 3 on are empty   3: a, but read n_reads / 2 has b bases
//     4: a + x % (b - a + 1), x from a 64-bit LCG seeded with `seed`
// stdout, one line per case:
//   route overlapped pin_reads pin_vector demoted ahead quartered vector_down words_in_block small_bytes target min_reads
//   | number of chunks | the first three chunks and the last one, each: i first nr b0 nb masks phase [first packed byte, packed bytes] | fnv
// route: vector | masks | mixed (the settled route); demoted: a mixed call that became a masks call; ahead: the reads go up ahead of the
// loop; quartered: the first chunks are a quarter and a half; fnv: 64-bit FNV-1a over every chunk's fields.
// With the argument "chunks": every chunk of every case instead, one per line (first nr b0 nb masks phase), an empty line after each case.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../movi_amd/csrc/movi_host_plan.hpp"

using namespace movi;

static std::vector<uint64_t> make_offsets(uint64_t n, uint64_t off0, int pattern, uint64_t a, uint64_t b, uint64_t seed) {
    std::vector<uint64_t> o(n + 1);
    o[0] = off0;
    uint64_t x = seed;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t len = a;
        if (pattern == 1 && (i & 1)) len = b;
        if (pattern == 2 && i >= n / 3 && i < n / 3 + b) len = 0;
        if (pattern == 3 && i == n / 2) len = b;
        if (pattern == 4) { x = x * 6364136223846793005ull + 1442695040888963407ull; len = a + (x >> 33) % (b - a + 1); }
        o[i + 1] = o[i] + len;
    }
    return o;
}

int main(int argc, char **argv) {
    const bool every_chunk = argc > 1 && !strcmp(argv[1], "chunks");
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long f[22];
        int n = 0, pos = 0, adv = 0;
        while (n < 22 && sscanf(line + pos, "%lld%n", &f[n], &adv) == 1) { pos += adv; ++n; }
        if (n != 22) { fprintf(stderr, "bad case: %s", line); return 2; }
        const bool pin_ok = f[14] != 0, packed = f[15] != 0;
        const uint64_t n_reads = (uint64_t)f[16];
        const std::vector<uint64_t> offs = make_offsets(n_reads, (uint64_t)f[17], (int)f[18], (uint64_t)f[19], (uint64_t)f[20], (uint64_t)f[21]);
        HostFacts F;
        F.query = (HostQuery)f[0]; F.zml = f[1] != 0; F.want_vector = f[2] != 0; F.want_words = f[3] != 0;
        F.reads_pinned = f[4] != 0; F.vector_pinned = f[5] != 0; F.small_bytes = (size_t)f[6];
        F.total = offs[n_reads] - offs[0]; F.n_reads = n_reads;
        HostOptions O;
        O.host_overlap = (int)f[7]; O.host_autopin = (int)f[8]; O.host_masks = (int)f[9]; O.host_mask_share = (int)f[10];
        O.pipe_chunk_bases = (uint64_t)f[11]; O.seg_seen = f[12] != 0; O.seg_len = (int)f[13];
        HostCall call = plan_host_call(F, O);
        const HostRoute asked = call.route;
        call.settle(call.pin_reads && pin_ok);
        const std::vector<HostChunk> chunks = plan_chunks(call, offs.data(), n_reads);
        if (every_chunk) {
            for (const HostChunk &c : chunks)
                printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %u\n", c.first, c.nr, c.b0, c.nb, (int)c.masks, c.phase);
            printf("\n");
            continue;
        }
        static const char *const routes[] = {"vector", "masks", "mixed"};
        printf("%s %d %d %d %d %d %d %d %d %zu %" PRIu64 " %" PRIu64 " | %zu",
               routes[(int)call.route], (int)call.overlapped, (int)call.pin_reads, (int)call.pin_vector, (int)(asked != call.route),
               (int)call.upload_ahead(chunks.size()), (int)(call.rule.head[0] != 0), (int)call.vector_down, (int)call.words_in_block, call.small_bytes,
               call.rule.target, call.rule.min_reads, chunks.size());
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](uint64_t v) { for (int k = 0; k < 8; k++) { h ^= (v >> (8 * k)) & 0xFF; h *= 1099511628211ull; } };
        for (size_t i = 0; i < chunks.size(); i++) {
            const HostChunk &c = chunks[i];
            mix(c.first); mix(c.nr); mix(c.b0); mix(c.nb); mix(c.masks); mix(c.phase);
            if (i < 3 || i + 1 == chunks.size()) {
                printf(" | %zu %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %u", i, c.first, c.nr, c.b0, c.nb, (int)c.masks, c.phase);
                if (packed) printf(" %" PRIu64 " %zu", c.b0 >> 2, packed_span_bytes(c.b0, c.nb));
            }
        }
        printf(" | %016" PRIx64 "\n", h);
    }
    return 0;
}
