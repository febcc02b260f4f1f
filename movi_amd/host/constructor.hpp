// constructor.hpp -- the in-memory CPU index constructor for modes 2 / 3 / 5 / 6 / 7 / 8, in two stages with the run-length BWT
// between them (rlbwt_from_text, image_from_rlbwt), and the files that go with it (read_rlbwt_files / write_rlbwt_files, write_index_dir).
// Plain C++17, header-only: `movi build` (build_cmd.cpp) and the bench / test tool (tools/build_index.cpp) include it.  Linear time,
// texts up to 2^31 characters; failures are std::runtime_error.  What is computed follows the reference (file:line of its tree):
//   src/prepare_ref.cpp:39-58            cleaning ("not upper-case ACGT -> 'A'"), reverse complement per record
//   pfp-thresholds (external, tag `movi`) BWT with terminator byte 0; threshold of a run = leftmost minimum LCP
//                                         between the end of the previous run of that character and the run start
//   src/move_structure_build.cpp:328-396 row boundaries: character change, threshold position, MAX_RUN_LENGTH
//   :74-121, :449-692                    LF of run heads -> (id, offset); :694-731 base intervals
//   :807-935                             threshold bits (incl. the '$'-row-is-an-'A'-row quirk, :823)
//   :939-1074                            blocked ids;  src/move_structure_io.cpp:435-469 file layout
// Checked byte-for-byte against tests/golden/index_*/index.movi (whose sizes are the reference's
// known answers 948119 / 711733, tests/test_build.cpp:37,53) in tests/test_build_tool.py.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <sys/stat.h>
#include <utility>
#include <vector>

namespace movi_constructor {

typedef int32_t sa_t;

// ------------------------------------------------------------------ SA-IS (induced sorting), own implementation
namespace sais {

template <typename T>
inline void get_counts(const T *s, sa_t *c, sa_t n, sa_t k) {
    for (sa_t i = 0; i < k; i++) c[i] = 0;
    for (sa_t i = 0; i < n; i++) c[s[i]]++;
}
inline void get_buckets(const sa_t *c, sa_t *b, sa_t k, bool end) {
    sa_t sum = 0;
    if (end) for (sa_t i = 0; i < k; i++) { sum += c[i]; b[i] = sum; }
    else for (sa_t i = 0; i < k; i++) { sum += c[i]; b[i] = sum - c[i]; }
}

template <typename T>
inline void induce(const std::vector<bool> &is_s, sa_t *sa, const T *s, sa_t *c, sa_t *b, sa_t n, sa_t k) {
    get_buckets(c, b, k, false);                      // L-type, left to right
    for (sa_t i = 0; i < n; i++) {
        sa_t j = sa[i] - 1;
        if (sa[i] > 0 && !is_s[j]) sa[b[s[j]]++] = j;
    }
    get_buckets(c, b, k, true);                       // S-type, right to left
    for (sa_t i = n - 1; i >= 0; i--) {
        sa_t j = sa[i] - 1;
        if (sa[i] > 0 && is_s[j]) sa[--b[s[j]]] = j;
    }
}

// s[n-1] must be the unique smallest symbol (sentinel).
template <typename T>
inline void build(const T *s, sa_t *sa, sa_t n, sa_t k) {
    std::vector<bool> is_s(n);
    is_s[n - 1] = true;
    for (sa_t i = n - 2; i >= 0; i--) is_s[i] = s[i] < s[i + 1] || (s[i] == s[i + 1] && is_s[i + 1]);
    auto is_lms = [&](sa_t i) { return i > 0 && is_s[i] && !is_s[i - 1]; };
    std::vector<sa_t> c(k), b(k);
    get_counts(s, c.data(), n, k);
    // stage 1: sort LMS substrings
    get_buckets(c.data(), b.data(), k, true);
    for (sa_t i = 0; i < n; i++) sa[i] = -1;
    for (sa_t i = 1; i < n; i++) if (is_lms(i)) sa[--b[s[i]]] = i;
    induce(is_s, sa, s, c.data(), b.data(), n, k);
    // compact sorted LMS substrings, name them
    sa_t n1 = 0;
    for (sa_t i = 0; i < n; i++) if (is_lms(sa[i])) sa[n1++] = sa[i];
    for (sa_t i = n1; i < n; i++) sa[i] = -1;
    sa_t name = 0, prev = -1;
    for (sa_t i = 0; i < n1; i++) {
        sa_t pos = sa[i];
        bool diff = false;
        if (prev < 0) diff = true;
        else {
            for (sa_t d = 0;; d++) {
                if (s[pos + d] != s[prev + d] || is_s[pos + d] != is_s[prev + d]) { diff = true; break; }
                if (d > 0 && (is_lms(pos + d) || is_lms(prev + d))) break;
            }
        }
        if (diff) { name++; prev = pos; }
        sa[n1 + pos / 2] = name - 1;
    }
    for (sa_t i = n - 1, j = n - 1; i >= n1; i--) if (sa[i] >= 0) sa[j--] = sa[i];
    // stage 2: solve the reduced problem
    sa_t *sa1 = sa, *s1 = sa + n - n1;
    if (name < n1) {
        build<sa_t>(s1, sa1, n1, name);
    } else {
        for (sa_t i = 0; i < n1; i++) sa1[s1[i]] = i;
    }
    // stage 3: induce the result
    get_buckets(c.data(), b.data(), k, true);
    for (sa_t i = 1, j = 0; i < n; i++) if (is_lms(i)) s1[j++] = i;
    for (sa_t i = 0; i < n1; i++) sa1[i] = s1[sa1[i]];
    for (sa_t i = n1; i < n; i++) sa[i] = -1;
    for (sa_t i = n1 - 1; i >= 0; i--) {
        sa_t j = sa[i];
        sa[i] = -1;
        sa[--b[s[j]]] = j;
    }
    induce(is_s, sa, s, c.data(), b.data(), n, k);
}

}  // namespace sais

// ------------------------------------------------------------------------------------------- FASTA -> text
inline void append_clean(std::vector<uint8_t> &text, const std::string &seq, bool separators = false) {
    // src/prepare_ref.cpp:39-58: the test uses the ORIGINAL byte, so lower case also becomes 'A';
    // with separators (:61-66) the record and its reverse complement are each followed by '%'
    const size_t a = text.size();
    for (char ch : seq) text.push_back((ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') ? (uint8_t)ch : (uint8_t)'A');
    const size_t b = text.size();
    if (separators) text.push_back('%');
    for (size_t i = b; i-- > a;) {
        uint8_t c = text[i];
        text.push_back(c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A');
    }
    if (separators) text.push_back('%');
}

// FASTA -> the indexed text (prepare_ref: every record forward + reverse complement, cleaned; with `separators` a '%'
// after every sequence).  Returns false when the file cannot be read.  doc_ends (optional): where every record's document ends in the
// text -- prepare_ref's doc_offsets for one FASTA (src/prepare_ref.cpp:37, :66, :73-76, :121-127): a document is a record with its reverse
// complement and its separators.
inline bool text_from_fasta(const std::string &path, bool separators, std::vector<uint8_t> &text, std::vector<uint64_t> *doc_ends = nullptr) {
    std::ifstream in(path);
    if (!in.good()) return false;
    std::string line, seq;
    bool have = false;
    while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n' || line.back() == ' ')) line.pop_back();
        if (!line.empty() && line[0] == '>') {
            if (have) { append_clean(text, seq, separators); if (doc_ends) doc_ends->push_back(text.size()); }
            seq.clear();
            have = true;
        } else if (have) seq += line;
    }
    if (have) { append_clean(text, seq, separators); if (doc_ends) doc_ends->push_back(text.size()); }
    return true;
}

// -------------------------------------------------------------------------------------- text -> run-length BWT
// The maximal runs of the BWT (terminator byte 0) and, per run, pfp-thresholds' threshold position.
struct Rlbwt {
    std::vector<uint8_t> heads;
    std::vector<uint64_t> lens, thr;
    uint64_t n = 0;                                                       // characters, terminator included
};

// The terminator is appended to `text` for the duration of the call.  Peak: text + sa + rank + lcp, 13 bytes per character.
inline Rlbwt rlbwt_from_text(std::vector<uint8_t> &text) {
    if ((uint64_t)text.size() + 1 >= (1ull << 31)) throw std::runtime_error("text too long for 32-bit suffix array");
    text.push_back(0);                                                    // terminator
    const sa_t n = (sa_t)text.size();
    std::vector<sa_t> sa(n);
    fprintf(stderr, "[build_index] n = %d, building the suffix array...\n", n);
    sais::build<uint8_t>(text.data(), sa.data(), n, 256);
    // LCP (Kasai): lcp[i] = lcp(suffix sa[i-1], suffix sa[i])
    fprintf(stderr, "[build_index] LCP...\n");
    std::vector<sa_t> rank(n), lcp(n, 0);
    for (sa_t i = 0; i < n; i++) rank[sa[i]] = i;
    {
        sa_t h = 0;
        for (sa_t i = 0; i < n; i++) {
            sa_t r = rank[i];
            if (r > 0) {
                sa_t j = sa[r - 1];
                while (i + h < n && j + h < n && text[i + h] == text[j + h]) h++;
                lcp[r] = h;
                if (h > 0) h--;
            } else h = 0;
        }
    }
    std::vector<sa_t>().swap(rank);
    std::vector<uint8_t> bwt(n);
    for (sa_t i = 0; i < n; i++) bwt[i] = sa[i] ? text[sa[i] - 1] : 0;
    std::vector<sa_t>().swap(sa);
    text.pop_back();
    // thresholds per run, and the runs themselves
    fprintf(stderr, "[build_index] thresholds + rows...\n");
    Rlbwt rl;
    rl.n = (uint64_t)n;
    const sa_t INF = 0x7fffffff;
    sa_t curmin[256], arg[256], run_start = 0;
    bool seen[256];
    for (int c = 0; c < 256; c++) { curmin[c] = INF; arg[c] = 0; seen[c] = false; }
    const int syms[6] = {0, '%', 'A', 'C', 'G', 'T'};
    for (sa_t i = 0; i < n; i++) {
        if (i > 0) for (int c : syms) if (lcp[i] < curmin[c]) { curmin[c] = lcp[i]; arg[c] = i; }
        const uint8_t c = bwt[i];
        if (i == 0 || bwt[i - 1] != c) {
            if (i > 0) rl.lens.push_back((uint64_t)(i - run_start));
            run_start = i;
            rl.heads.push_back(c);
            rl.thr.push_back(seen[c] ? (uint64_t)arg[c] : 0);
        }
        seen[c] = true;
        curmin[c] = INF;                                                  // the range restarts after this position
    }
    rl.lens.push_back((uint64_t)(n - run_start));
    return rl;
}

// ------------------------------------------------------------------------------- run-length BWT -> index.movi bytes
constexpr int alphamap_3[4][4] = {{3, 0, 1, 2}, {0, 3, 1, 2}, {0, 1, 3, 2}, {0, 1, 2, 3}};   // src/utils.cpp:5-8
constexpr uint64_t kTallyCheckpoint = 20;                                 // movi_options.hpp:257

inline void put64(std::vector<uint8_t> &o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

// What index.movi holds, filled in by the stages below in the order image_from_rlbwt calls them.
struct Table {
    int mode = 0, sep = 0;                                                // sep: five symbols led by '%' (MoveStructure::use_separator, src/move_structure.cpp:547-552)
    bool with_thresholds = false;
    uint64_t n = 0, r = 0, original_r = 0, end_bwt_idx = 0;
    uint64_t alphamap[256];
    std::vector<uint8_t> alphabet;
    std::vector<uint64_t> counts;
    size_t sigma = 0;
    std::vector<uint64_t> p, dest;                                        // rows: where each starts (p[r] = n), where its head goes,
    std::vector<uint8_t> code, tbits;                                     // its character's code, its threshold bits,
    std::vector<uint16_t> len, doff;                                      // its length and the offset in the destination row
    std::vector<uint64_t> first_runs, first_offsets, last_runs, last_offsets;
    uint64_t end_thr[4] = {0, 0, 0, 0};
    std::vector<std::array<uint16_t, 4>> sep_thr;
    std::vector<std::pair<uint64_t, uint64_t>> sep_map;
    std::vector<uint32_t> blocked, id_blocks;
    uint64_t n_blocks = 0, block_size = 0;
    std::vector<uint64_t> tally;
};

// build_alphabet, src/move_structure_build.cpp:428-447
inline void alphabet_of_runs(Table &t, const Rlbwt &rl) {
    uint64_t cnt_all[256] = {0};
    for (size_t k = 0; k < rl.heads.size(); k++) cnt_all[rl.heads[k]] += rl.lens[k];
    for (int c = 0; c < 256; c++) t.alphamap[c] = 256;
    for (int c = 1; c < 256; c++)
        if (cnt_all[c]) { t.alphamap[c] = t.alphabet.size(); t.alphabet.push_back((uint8_t)c); t.counts.push_back(cnt_all[c]); }
    t.sigma = t.alphabet.size();
    t.sep = (t.sigma == 5 && t.alphabet[0] == '%') ? 1 : 0;
    if (t.sigma < 1 || (t.sigma > 4 && !t.sep)) throw std::runtime_error("only DNA alphabets (<= 4 symbols, or '%' + ACGT) are in scope");
}

// Rows (:328-396) start where a run starts and, with thresholds, at every threshold position (fill_bits_by_thresholds :733-746); a
// piece between two such positions is then cut every MAX_RUN_LENGTH characters, counted from the piece's start.
inline void rows_of_runs(Table &t, const Rlbwt &rl) {
    const uint32_t maxrun = t.mode == 6 ? 2047 : (t.mode == 7 ? 511 : (t.mode == 3 ? 4095 : 1023));   // move_row_configs.hpp:51,101,135,117,31,72
    // The thresholds in ascending order.  Those of one character's runs ascend already (each lies behind that character's previous
    // run), so they are gathered per character and the lists merged: linear, where sorting them was slower than the rest of the stage.
    std::vector<uint64_t> cuts;
    size_t ci = 0;
    if (t.with_thresholds) {
        size_t first[257] = {0}, next[256];
        for (uint8_t h : rl.heads) first[h + 1]++;
        for (int c = 0; c < 256; c++) { first[c + 1] += first[c]; next[c] = first[c]; }
        cuts.resize(rl.thr.size());
        for (size_t k = 0; k < cuts.size(); k++) cuts[next[rl.heads[k]]++] = rl.thr[k];
        for (int c = 1; c < 256; c++) std::inplace_merge(cuts.begin(), cuts.begin() + first[c], cuts.begin() + first[c + 1]);
        if (!std::is_sorted(cuts.begin(), cuts.end())) std::sort(cuts.begin(), cuts.end());   // (arrays that are no text's)
    }
    uint64_t start = 0;
    for (size_t k = 0; k < rl.heads.size(); k++) {
        const uint64_t end = start + rl.lens[k];
        const uint8_t h = rl.heads[k];
        if (h == 0) t.end_bwt_idx = t.p.size();
        while (start < end) {
            while (ci < cuts.size() && cuts[ci] <= start) ci++;
            const uint64_t piece_end = ci < cuts.size() && cuts[ci] < end ? cuts[ci] : end;
            for (; start < piece_end; start += maxrun) {
                t.p.push_back(start);
                t.code.push_back(h == 0 ? 0 : (uint8_t)t.alphamap[h]);    // set_c: alphamap[0] == 256 shifts out
                t.len.push_back((uint16_t)std::min<uint64_t>(maxrun, piece_end - start));
            }
            start = piece_end;
        }
    }
    t.r = t.p.size();
    t.p.push_back(t.n);
}

// LF of run heads (LF_heads, src/move_structure.cpp:515-523); destinations are monotone per character
inline void lf_of_heads(Table &t) {
    t.dest.resize(t.r);
    t.doff.resize(t.r);
    uint64_t C[5], rk[5] = {0, 0, 0, 0, 0}, ptr[5] = {0, 0, 0, 0, 0};
    C[0] = 1;
    for (size_t a = 1; a < t.sigma; a++) C[a] = C[a - 1] + t.counts[a - 1];
    for (uint64_t i = 0; i < t.r; i++) {
        if (i == t.end_bwt_idx) { t.dest[i] = 0; t.doff[i] = 0; continue; }
        const int a = t.code[i];
        const uint64_t lf = C[a] + rk[a];
        rk[a] += t.len[i];
        uint64_t p = ptr[a];
        while (t.p[p + 1] <= lf) p++;
        ptr[a] = p;
        t.dest[i] = p;
        t.doff[i] = (uint16_t)(lf - t.p[p]);
    }
}

// base intervals (:694-731)
inline void base_intervals(Table &t) {
    t.first_runs.assign(1, 0); t.first_offsets.assign(1, 0); t.last_runs.assign(1, 0); t.last_offsets.assign(1, 0);
    uint64_t cc = 1;
    for (size_t a = 0; a < t.sigma; a++) {
        const uint64_t lr = t.last_runs.back(), lo = t.last_offsets.back();
        if (lo + 1 >= t.len[lr]) { t.first_runs.push_back(lr + 1); t.first_offsets.push_back(0); }
        else { t.first_runs.push_back(lr); t.first_offsets.push_back(lo + 1); }
        cc += t.counts[a];
        const uint64_t k = std::lower_bound(t.p.begin(), t.p.begin() + t.r, cc) - t.p.begin();   // rows starting before cc
        t.last_runs.push_back(k - 1);
        t.last_offsets.push_back(cc - t.p[k - 1] - 1);
    }
}

// threshold bits (:807-935).  With separators (:826-831, :836-858, :912-921) no threshold is kept FOR the
// separator; a row OF the separator (and the '$' row, whose character field decodes as one) gets an explicit
// 4-value entry in separators_thresholds, appended in descending row order, row 0 last.
inline void threshold_bits(Table &t, const std::vector<uint64_t> &thr) {
    t.tbits.assign(t.r, 0);
    if (!t.with_thresholds) return;                                       // no thresholds of any kind
    const int sep = t.sep;
    std::vector<uint64_t> at(t.sigma, t.n);
    uint64_t thr_i = t.original_r - 1;
    for (uint64_t i = t.r - 1; i > 0; --i) {
        const int rc = t.code[i];                                         // '$' row has c == 0 -> behaves as 'A' (:823)
        if (sep && rc == 0) {
            t.sep_thr.push_back({0, 0, 0, 0});
            t.sep_map.emplace_back(i, t.sep_thr.size() - 1);
        }
        for (size_t j = 0; j < t.sigma; j++) {
            if ((int)j == rc) {
                at[j] = thr[thr_i];
            } else {
                if (sep && j == 0) continue;                              // :849-852
                const uint64_t cur = at[j];
                int bit;
                uint64_t val;
                if (cur >= t.p[i] + t.len[i]) { val = t.len[i]; bit = 1; }
                else if (cur <= t.p[i]) { val = 0; bit = 0; }
                else { val = cur - t.p[i]; bit = -1; }                    // strictly inside the row (:869-871)
                if (i == t.end_bwt_idx) t.end_thr[j - sep] = val;
                else if (sep && rc == 0) t.sep_thr.back()[j - 1] = (uint16_t)val;
                else {
                    if (bit < 0) throw std::runtime_error("threshold strictly inside a row");
                    t.tbits[i] |= (uint8_t)(bit << alphamap_3[rc - sep][j - sep]);
                }
            }
        }
        if (t.code[i] != t.code[i - 1] || i == t.end_bwt_idx || i - 1 == t.end_bwt_idx) thr_i--;
    }
    if (sep && t.code[0] == 0) {                                          // :917-920
        t.sep_thr.push_back({0, 0, 0, 0});
        t.sep_map.emplace_back(0, t.sep_thr.size() - 1);
    }
    std::sort(t.sep_map.begin(), t.sep_map.end());                        // the reference walks an unordered_map; ascending rows here
}

// blocked ids (:939-1074), modes 8 and 2
inline void blocked_ids(Table &t) {
    t.block_size = t.mode == 2 ? 1ull << 22 : 1ull << 20;                 // move_row_configs.hpp:73 / :102
    uint64_t max_allowed = t.mode == 2 ? (1ull << 24) - 1 : (1ull << 22) - 1;   // :74 / :103
    t.blocked.resize(t.r);
    for (;;) {
        t.n_blocks = (t.r + t.block_size - 1) / t.block_size;
        t.id_blocks.assign(t.sigma * t.n_blocks, 0);
        uint64_t last[5] = {0, 0, 0, 0, 0};
        bool ok = true;
        for (uint64_t i = 0; i < t.r && ok; i++) {
            if (i % t.block_size == 0) for (size_t a = 0; a < t.sigma; a++) t.id_blocks[a * t.n_blocks + i / t.block_size] = (uint32_t)last[a];
            if (i == t.end_bwt_idx) { t.blocked[i] = 0; continue; }
            const int c = t.code[i];
            const uint64_t adj = t.dest[i] - t.first_runs[c + 1];
            const uint64_t b = adj - t.id_blocks[c * t.n_blocks + i / t.block_size];
            if (b > max_allowed) { ok = false; break; }
            t.blocked[i] = (uint32_t)b;
            last[c] = adj;
        }
        if (ok) return;
        t.block_size /= 2;
        max_allowed = ((max_allowed + 1) / 2) - 1;
    }
}

// sampled ids (modes 7 and 5; src/move_structure_build.cpp:486-496, :571-596, :677-682): every 20 rows the destination id
// of the latest run of each character; a character not seen yet gets the id of its first run once it shows up
inline void sampled_tally(Table &t) {
    const uint64_t n_tally = t.r / kTallyCheckpoint + 2;
    t.tally.assign(t.sigma * n_tally, 0);
    std::vector<uint64_t> cur(t.sigma, t.r);
    for (uint64_t i = 0; i < t.r; i++) {
        if (i != t.end_bwt_idx) {
            const int a = t.code[i];
            if (cur[a] == t.r) for (uint64_t k = 0; k <= i / kTallyCheckpoint; k++) t.tally[a * n_tally + k] = t.dest[i];
            cur[a] = t.dest[i];
        }
        if (i % kTallyCheckpoint == 0) for (size_t a = 0; a < t.sigma; a++) t.tally[a * n_tally + i / kTallyCheckpoint] = cur[a];
    }
    for (size_t a = 0; a < t.sigma; a++) t.tally[a * n_tally + n_tally - 1] = cur[a];
}

// Row i in the layout of the table's type (include/move_row.hpp, move_row_configs.hpp)
inline void put_row(std::vector<uint8_t> &o, const Table &t, uint64_t i) {
    const uint32_t len = t.len[i], doff = t.doff[i], code = t.code[i], tb = t.tbits[i], b = t.blocked.empty() ? 0 : t.blocked[i];
    const uint64_t d = t.dest[i];
    uint16_t w[4];
    size_t bytes = 6;
    if (t.mode == 6 || t.mode == 3) {                                     // mode 3: 12-bit n / offset, no threshold bits (tb == 0)
        w[0] = (uint16_t)(d & 0xFFFF);
        w[1] = (uint16_t)((d >> 16) & 0xFFFF);
        w[2] = (uint16_t)(len | (((tb >> 1) & 1) << 11) | (((tb >> 2) & 1) << 12) | (code << 13));
        w[3] = (uint16_t)(doff | ((tb & 1) << 11) | ((uint32_t)(d >> 32) << 12));
        bytes = 8;
    } else if (t.mode == 2) {                                             // blocked: 24-bit id, MoveRow::set_id src/move_row.cpp:213-225
        w[0] = (uint16_t)(b & 0xFFFF);
        w[1] = (uint16_t)(len | (((b >> 16) & 0x3F) << 10));
        w[2] = (uint16_t)(doff | (code << 10) | ((b >> 22) << 14));
    } else if (t.mode == 8) {
        w[0] = (uint16_t)(b & 0xFFFF);
        w[1] = (uint16_t)(len | ((b >> 16) << 10));
        w[2] = (uint16_t)(doff | (code << 10) | ((tb & 1) << 13) | (((tb >> 1) & 1) << 14) | (((tb >> 2) & 1) << 15));
    } else {                                                              // sampled: configs :107-118; with thresholds move_row.hpp:122-127, configs :120-136
        w[0] = (uint16_t)((len & 0xFF) | ((doff & 0xFF) << 8));
        w[1] = t.mode == 5 ? (uint16_t)((doff >> 8) | ((len >> 8) << 2) | (code << 4)) : (uint16_t)((doff >> 8) | ((len >> 8) << 1) | (code << 2) | ((tb & 7) << 5));
        bytes = 3;
    }
    const uint8_t *p = reinterpret_cast<const uint8_t *>(w);
    o.insert(o.end(), p, p + bytes);
}

// serialize (src/move_structure_io.cpp:435-469)
inline std::vector<uint8_t> serialise(const Table &t) {
    std::vector<uint8_t> o;
    o.reserve(2215 + t.r * 8 + 512 + t.id_blocks.size() * 4);
    o.resize(48, 0);
    const uint32_t magic = 0x4D4F5649u;
    memcpy(&o[0], &magic, 4);
    o[4] = 2; o[5] = 0; o[6] = 0; o[7] = (uint8_t)t.mode; o[8] = 0;
    const uint64_t hdr[4] = {t.n, t.r, t.original_r, t.end_bwt_idx};
    memcpy(&o[16], hdr, 32);
    for (int i = 0; i < 4; i++) put64(o, t.end_thr[i]);
    for (int i = 0; i < 8; i++) put64(o, 0);
    put64(o, 256);
    for (int c = 0; c < 256; c++) put64(o, t.alphamap[c]);
    put64(o, t.sigma);
    for (uint8_t a : t.alphabet) o.push_back(a);
    o.push_back(0); o.push_back(0); o.push_back(0);                       // u16 nt_splitting, bool constant
    for (uint64_t i = 0; i < t.r; i++) put_row(o, t, i);
    if (t.mode == 7 || t.mode == 5) {                                     // write_tally_table, io.cpp:328-336
        const uint32_t cp32 = (uint32_t)kTallyCheckpoint;
        for (int b = 0; b < 4; b++) o.push_back((uint8_t)(cp32 >> (8 * b)));
        put64(o, t.tally.size() / t.sigma);
        for (uint64_t v : t.tally) for (int b = 0; b < 5; b++) o.push_back((uint8_t)(v >> (8 * b)));   // MoveTally: u32 low | u8 high
    }
    for (int i = 0; i < 3; i++) put64(o, 0);
    put64(o, t.counts.size());
    for (uint64_t c : t.counts) put64(o, c);
    put64(o, t.last_runs.size());
    for (uint64_t v : t.last_runs) put64(o, v);
    for (uint64_t v : t.last_offsets) put64(o, v);
    for (uint64_t v : t.first_runs) put64(o, v);
    for (uint64_t v : t.first_offsets) put64(o, v);
    if (t.mode == 8 || t.mode == 2) {
        put64(o, t.n_blocks);
        const uint8_t *p = reinterpret_cast<const uint8_t *>(t.id_blocks.data());
        o.insert(o.end(), p, p + t.id_blocks.size() * 4);
        put64(o, t.block_size);
    }
    if (t.sep && t.with_thresholds) {                                     // write_separators_thresholds, io.cpp:399-413
        put64(o, t.sep_thr.size());
        for (const auto &s : t.sep_thr) for (int k = 0; k < 4; k++) { o.push_back((uint8_t)(s[k] & 0xFF)); o.push_back((uint8_t)(s[k] >> 8)); }
        put64(o, t.sep_map.size());
        for (const auto &kv : t.sep_map) { put64(o, kv.first); put64(o, kv.second); }
    }
    return o;
}

inline std::vector<uint8_t> image_from_rlbwt(const Rlbwt &rl, int mode) {
    Table t;
    t.mode = mode;
    t.with_thresholds = mode != 5 && mode != 3 && mode != 2;              // sampled / regular / blocked: USE_THRESHOLDS is off
    t.n = rl.n;
    t.original_r = rl.heads.size();
    alphabet_of_runs(t, rl);
    rows_of_runs(t, rl);
    lf_of_heads(t);
    base_intervals(t);
    threshold_bits(t, rl.thr);
    if (mode == 8 || mode == 2) blocked_ids(t);
    if (mode == 7 || mode == 5) sampled_tally(t);
    std::vector<uint8_t> o = serialise(t);
    fprintf(stderr, "[build_index] n = %d, original_r = %llu, r = %llu, n/r = %.2f, index %zu bytes\n", (int)t.n,
            (unsigned long long)t.original_r, (unsigned long long)t.r, (double)t.n / t.r, o.size());
    return o;
}

// ---------------------------------------------------------------------------------------------------- files
// `count` values as five little-endian bytes each (the .bwt.len and .thr_pos of `movi rlbwt` and pfp-thresholds), written in blocks
inline void write_five(std::ofstream &f, const uint64_t *values, uint64_t count) {
    std::vector<char> buf;
    buf.reserve(5u << 16);
    for (uint64_t k = 0; k < count; k++) {
        for (int b = 0; b < 5; b++) buf.push_back((char)(values[k] >> (8 * b)));
        if (buf.size() == (5u << 16) || k + 1 == count) { f.write(buf.data(), (std::streamsize)buf.size()); buf.clear(); }
    }
}

// PREFIX.bwt.heads, PREFIX.bwt.len and, unless thr is null, PREFIX.thr_pos: the input of `movi build --preprocessed`
inline void write_rlbwt_files(const std::string &prefix, const uint8_t *heads, const uint64_t *lens, const uint64_t *thr, uint64_t R) {
    std::ofstream hf(prefix + ".bwt.heads", std::ios::binary), lf(prefix + ".bwt.len", std::ios::binary);
    hf.write(reinterpret_cast<const char *>(heads), (std::streamsize)R);
    write_five(lf, lens, R);
    hf.close(); lf.close();
    bool ok = hf.good() && lf.good();
    if (thr) {
        std::ofstream tf(prefix + ".thr_pos", std::ios::binary);
        write_five(tf, thr, R);
        tf.close();
        ok = ok && tf.good();
    }
    if (!ok) throw std::runtime_error("cannot write " + prefix + ".bwt.heads / .bwt.len / .thr_pos");
}

// The five-byte little-endian values of a file the caller has found it can open, one per run, read in blocks.  `what` names them in a
// finding, `bad_size` opens the finding about a size that is no multiple of five and `bad_size_end` closes it.
inline std::vector<uint64_t> read_five(const std::string &path, uint64_t R, const std::string &heads_path, const char *what,
                                       const std::string &bad_size, const char *bad_size_end) {
    struct stat sb;
    const uint64_t bytes = stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode) ? (uint64_t)sb.st_size : 0;
    if (bytes % 5 != 0) throw std::runtime_error(bad_size + path + ": " + std::to_string(bytes) + " bytes is not a multiple of 5" + bad_size_end);
    if (bytes / 5 != R)
        throw std::runtime_error(path + " holds " + std::to_string(bytes / 5) + " " + what + " but " + heads_path + " holds " + std::to_string(R) + " run heads");
    std::ifstream f(path, std::ios::binary);
    std::vector<uint64_t> values(R, 0);
    std::vector<char> block(5u << 16);
    for (uint64_t k = 0; k < R;) {
        const uint64_t m = std::min<uint64_t>(R - k, 1u << 16);
        if (!f.read(block.data(), (std::streamsize)(5 * m))) throw std::runtime_error("cannot read " + path);
        for (uint64_t j = 0; j < m; j++) memcpy(&values[k++], &block[5 * j], 5);
    }
    return values;
}

// What write_rlbwt_files wrote, or an external BWT tool, `movi rlbwt` and pfp-thresholds: compute_length_from_bwt,
// src/move_structure_build.cpp:152-181, and with_thr read_thresholds, src/utils.cpp:150-200 (PREFIX.thr_pos is not opened otherwise).
// Sizes and counts are checked here, the contents by movi::rlbwt_check (csrc/movi_build.hpp).
inline Rlbwt read_rlbwt_files(const std::string &prefix, bool with_thr) {
    const std::string heads_path = prefix + ".bwt.heads", len_path = prefix + ".bwt.len", thr_path = prefix + ".thr_pos";
    Rlbwt rl;
    std::ifstream hf(heads_path, std::ios::binary);
    if (!hf.good()) throw std::runtime_error("[build] Failed to open the heads file: " + heads_path);
    rl.heads.assign(std::istreambuf_iterator<char>(hf), std::istreambuf_iterator<char>());
    const uint64_t R = rl.heads.size();
    if (R == 0) throw std::runtime_error(heads_path + ": holds no run");
    if (!std::ifstream(len_path).good()) throw std::runtime_error("[build] Failed to open the len file: " + len_path);
    rl.lens = read_five(len_path, R, heads_path, "lengths", "", " (one 5-byte length per run)");
    for (uint64_t len : rl.lens) rl.n += len;
    if (!with_thr) return rl;
    if (!std::ifstream(thr_path).good()) throw std::runtime_error("[read_thresholds] open() file " + thr_path + " failed");
    rl.thr = read_five(thr_path, R, heads_path, "thresholds", "[read_thresholds] invilid file ", "");
    // when the thresholds overflow 5 bytes the reference recovers the true values: a sudden drop to less than a tenth of the last
    // value, which was not small itself, is one more wrap (:172-196; unsigned arithmetic as there)
    const uint64_t kMax5 = 1ull << 40;
    uint64_t wraps = 0;
    for (uint64_t k = 0; k < R; k++) {
        const uint64_t v = rl.thr[k];
        if (k > 0 && v != 0 && v < (rl.thr[k - 1] - wraps * kMax5) / 10 && (rl.thr[k - 1] - wraps * kMax5) > kMax5 / 10) wraps += 1;
        rl.thr[k] = v + wraps * kMax5;
    }
    return rl;
}

// DIR/index.movi and, unless doc_ends is null, DIR/ref.fa.doc_offsets: one cumulative end per line, as prepare_ref writes them
inline void write_index_dir(const std::string &dir, const void *image, size_t bytes, const std::vector<uint64_t> *doc_ends) {
    mkdir(dir.c_str(), 0777);
    std::ofstream f(dir + "/index.movi", std::ios::binary);
    f.write(static_cast<const char *>(image), (std::streamsize)bytes);
    f.close();
    if (!f.good()) throw std::runtime_error("cannot write " + dir + "/index.movi");
    if (!doc_ends) return;
    std::ofstream d(dir + "/ref.fa.doc_offsets");
    for (uint64_t e : *doc_ends) d << e << "\n";
    d.close();
    if (!d.good()) throw std::runtime_error("cannot write " + dir + "/ref.fa.doc_offsets");
}

}  // namespace movi_constructor
