// build_index.cpp -- the bench and test tool around the CPU index constructor (movi_amd/host/constructor.hpp: SA-IS, Kasai LCP,
// per-run thresholds, move rows, `index.movi` bytes for modes 2 / 3 / 5 / 6 / 7 / 8).  What is the tool's own: a FASTA or a synthetic
// pangenome as the text -- linear time, so that a 64-genome pangenome with ~10 M runs and 640 Mbp of text is built in minutes --, reads
// drawn from that text, and the run-length BWT files beside the index.
//
// usage: build_index fasta <ref.fasta> <mode 2|3|5|6|7|8> <out_dir> [separators]     ("separators" = movi build --separators:
//            every record and reverse complement followed by %; sizes 948232 / 711854 B, tests/test_build.cpp:79,95)
//        build_index pangenome <ancestor_len> <n_genomes> <snp_rate> <seed> <mode> <out_dir> [n_reads read_len sub_rate]
//            [n_reads2 read_len2 sub_rate2]
//            (also writes <out_dir>/text.bin and reads.bin (and reads2.bin): fixed-length substrings of the text
//            with substitutions)
//        build_index reads <text.bin> <n_reads> <read_len> <sub_rate> <seed> <out_file>
//        build_index pangenome <ancestor_len> <n_genomes> <snp_rate> <seed> <mode> <out_dir> text-only     (writes text.bin only)
//        ... --emit-rlbwt PREFIX   (anywhere on a fasta / pangenome line: also writes PREFIX.bwt.heads, PREFIX.bwt.len and PREFIX.thr_pos,
//            the run-length BWT and the per-run thresholds as `movi rlbwt` and pfp-thresholds write them: the input of
//            `movi build --preprocessed`)
#include <cstdlib>
#include <iostream>

#include "../movi_amd/host/constructor.hpp"

using namespace movi_constructor;

static uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void write_file(const std::string &path, const std::vector<uint8_t> &data) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(data.data()), (std::streamsize)data.size());
    if (!f.good()) throw std::runtime_error("cannot write " + path);
}

// Fixed-length substrings of the text with substitutions (rate sub_rate) and 0.1 % 'N'.
static void draw_reads(const std::vector<uint8_t> &text, std::vector<uint8_t> &reads, uint64_t n_reads, uint64_t read_len,
                       double sub_rate, uint64_t sr) {
    for (uint64_t i = 0; i < n_reads; i++) {
        const uint64_t pos = splitmix64(sr) % (text.size() - read_len);
        memcpy(&reads[i * read_len], &text[pos], read_len);
        for (uint64_t k = 0; k < read_len; k++) {
            const double u = (double)(splitmix64(sr) >> 11) * (1.0 / 9007199254740992.0);
            if (u < 0.001) reads[i * read_len + k] = 'N';
            else if (u < 0.001 + sub_rate) reads[i * read_len + k] = "ACGT"[splitmix64(sr) & 3];
        }
    }
}

static int run(int argc, char **argv) {
    std::string emit_rlbwt;
    for (int i = 1; i + 1 < argc; i++)
        if (std::string(argv[i]) == "--emit-rlbwt") {                      // taken out of the line: the rest is positional
            emit_rlbwt = argv[i + 1];
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    if (argc < 2) { fprintf(stderr, "usage: see the header of tools/build_index.cpp\n"); return 1; }
    const std::string cmd = argv[1];
    std::vector<uint8_t> text;
    int mode = 6;
    std::string out_dir;
    uint64_t n_reads = 0, read_len = 0, seed = 1;
    double sub_rate = 0;
    if (cmd == "fasta" && argc >= 5) {
        mode = atoi(argv[3]);
        out_dir = argv[4];
        const bool separators = argc >= 6 && std::string(argv[5]) == "separators";   // movi build --separators
        if (!text_from_fasta(argv[2], separators, text)) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    } else if (cmd == "pangenome" && argc >= 8) {
        const uint64_t anc_len = strtoull(argv[2], nullptr, 10), n_genomes = strtoull(argv[3], nullptr, 10);
        const double snp = atof(argv[4]);
        seed = strtoull(argv[5], nullptr, 10);
        mode = atoi(argv[6]);
        out_dir = argv[7];
        if (argc >= 11) { n_reads = strtoull(argv[8], nullptr, 10); read_len = strtoull(argv[9], nullptr, 10); sub_rate = atof(argv[10]); }
        uint64_t st = seed * 0x9E3779B97F4A7C15ull + 7;
        std::string anc(anc_len, 'A');
        for (auto &c : anc) c = "ACGT"[splitmix64(st) & 3];
        // a shallow star phylogeny: every genome = ancestor + its own SNPs, plus SNPs shared by a random half
        for (uint64_t g = 0; g < n_genomes; g++) {
            std::string s = anc;
            uint64_t sg = seed * 1315423911ull + g * 2654435761ull;
            const uint64_t k = (uint64_t)(snp * anc_len);
            for (uint64_t i = 0; i < k; i++) {
                const uint64_t pos = splitmix64(sg) % anc_len;
                s[pos] = "ACGT"[splitmix64(sg) & 3];
            }
            uint64_t sh = seed * 77 + 5;                                   // shared variants: same stream for all genomes
            for (uint64_t i = 0; i < k; i++) {
                const uint64_t pos = splitmix64(sh) % anc_len;
                const char alt = "ACGT"[splitmix64(sh) & 3];
                const uint64_t carriers = splitmix64(sh);
                if ((carriers >> (g & 63)) & 1) s[pos] = alt;
            }
            append_clean(text, s);
        }
    } else if (cmd == "reads" && argc >= 8) {
        // build_index reads <text.bin> <n_reads> <read_len> <sub_rate> <seed> <out_file>
        std::ifstream in(argv[2], std::ios::binary);
        if (!in.good()) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        in.seekg(0, std::ios::end);
        text.resize((size_t)in.tellg());
        in.seekg(0);
        in.read(reinterpret_cast<char *>(text.data()), (std::streamsize)text.size());
        n_reads = strtoull(argv[3], nullptr, 10); read_len = strtoull(argv[4], nullptr, 10); sub_rate = atof(argv[5]);
        seed = strtoull(argv[6], nullptr, 10);
        std::vector<uint8_t> reads(n_reads * read_len);
        draw_reads(text, reads, n_reads, read_len, sub_rate, seed * 31 + 99);
        write_file(argv[7], reads);
        return 0;
    } else {
        fprintf(stderr, "usage: see the header of tools/build_index.cpp\n");
        return 1;
    }
    if (mode != 2 && mode != 3 && mode != 5 && mode != 6 && mode != 7 && mode != 8) { fprintf(stderr, "mode must be 2, 3, 5, 6, 7 or 8\n"); return 1; }
    mkdir(out_dir.c_str(), 0777);
    if (cmd == "pangenome" && argc == 9 && std::string(argv[8]) == "text-only") {   // only <out_dir>/text.bin (seconds): lets `reads` draw from a cached index's text
        write_file(out_dir + "/text.bin", text);
        return 0;
    }
    if (cmd == "pangenome") write_file(out_dir + "/text.bin", text);       // lets `reads` draw more reads later
    for (int set = 0; set < 2; set++) {                                    // optional second read set: argv[11..13] -> reads2.bin
        if (set == 1) {
            if (cmd != "pangenome" || argc < 14) break;
            n_reads = strtoull(argv[11], nullptr, 10); read_len = strtoull(argv[12], nullptr, 10); sub_rate = atof(argv[13]);
        }
        if (!n_reads) continue;
        std::vector<uint8_t> reads(n_reads * read_len);
        draw_reads(text, reads, n_reads, read_len, sub_rate, seed * 31 + 99 + set);
        write_file(out_dir + (set ? "/reads2.bin" : "/reads.bin"), reads);
    }
    const Rlbwt rl = rlbwt_from_text(text);
    if (!emit_rlbwt.empty()) write_rlbwt_files(emit_rlbwt, rl.heads.data(), rl.lens.data(), rl.thr.data(), rl.heads.size());
    write_file(out_dir + "/index.movi", image_from_rlbwt(rl, mode));
    return 0;
}

int main(int argc, char **argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
