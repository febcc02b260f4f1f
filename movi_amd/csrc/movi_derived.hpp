// movi_derived.hpp -- which derived tables a handle holds: the top-of-walk table, the count query's interval table, the look-ahead rows,
// the deep rows and the row-start checkpoints.  What the first query builds by itself, what movi_index_prepare builds, what the four
// build-now options ("kmer_k", "ftab_k", "ahead_rows", "deep_rows") drop and build, and what is given up for good, tried again at once or
// asked again after 64 calls.  Plain C++ over plain values (no HIP type, no runtime call): the rules are straight-line functions over a
// small device interface `Dev`, which movi_abi.hip implements with the HIP sequences (DerivedDev) and tests/host/derived_driver.cpp with a
// scripted fake (tests/test_derived_cpu.py holds the rules to tests/golden/derived_table.txt, recorded from the code they replaced).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "movi_deep_fields.hpp"   // kDeepWideMaxRows
#include "movi_chain_fields.hpp"  // kChainMaxRows

namespace movi {

enum DerivedTable { kTabKmer = 0, kTabFtab, kTabAhead, kTabDeep, kTabCkpt, kTabChain, kDerivedTables };

// The policy's state, one per handle.
struct DerivedPolicy {
    int kmer_auto = 12;              // K of the table the first PML query builds by itself (0 = none: "kmer_k" 0)
    int ftab_auto = 12;              // K of the table the first count query builds by itself (0 = none)
    int ahead_auto = 1;              // 1: the first PML query builds them when the device has room for them (ahead_wanted)
    int deep_auto = 1;               // 1: the first PML query builds them for tables of at most kDeepAutoRows rows (instead of the look-ahead rows)
    int deep_hint_bits = -1;         // "deep_hint_bits": width of a reposition hint in the deep rows when they are next built: -1 = kDeepHintBitsDefault, 2 or 4
    int ahead_retry_in = 0;          // the copy was declined for lack of device memory: calls until the device is asked again (not every call)
    bool count_declined_ahead = false;   // the count query's auto-build found the copy not worth keeping (rows2_count == 0): do not build it per call
    bool ahead_tallied = false;
    double ahead_no_ff = 0.0;        // share of the table's positions that arrive at their LF target without a fast-forward (sampled, or tallied by the builder of the look-ahead rows)
    bool prepared = false;           // movi_index_prepare has run: query calls build and allocate nothing any more (a declined copy is retried by movi_index_prepare only)
    int chain_auto = 1;              // 1: the first PML query builds the chain rows beside the deep rows where ensure_chain_rows says so ("chain_rows" -1)
};

// What the rules read of the handle.  `held` is refreshed by the device interface after every build and every drop: the rules hold a
// reference and read it again after each call on `Dev`.
struct DerivedFacts {
    int kmode = 0;                   // row layout the kernels run on (6 = regular-thresholds, 3 = regular)
    uint64_t r = 0;
    bool dna = false;                // sigma - sep == 4
    int count_variant = -1;          // "count_variant": the look-ahead copy serves count_kernel_v0 only, i.e. 0
    uint64_t ahead_bytes = 0, deep_bytes = 0;   // what the two row copies of a table of r rows take (ahead_rows_bytes, deep_rows_bytes)
    bool held[kDerivedTables] = {false, false, false, false, false};
    uint64_t chain_bytes = 0;        // what the chain rows of a table of r rows take (chain_rows_bytes)
};

// Top-of-walk table (DevIndex::kmer): 16 << 2K bytes, filled by one kernel; the call waits for it -- chunks of the
// overlapped host path walk on other streams.
inline bool kmer_eligible(const DerivedFacts &f) { return f.kmode == 6 && f.dna && f.r >= 8; }

// Look-ahead rows (DevIndex::rows2): a second copy of the table, 16 bytes per row, built by itself by the first PML query
// wherever the device has room for it.  History of the rule: round 3 built it up to 100 M rows only -- on a uniformly random
// table, the worst case for it (the base after the LF fast-forwards more often than not), it was +14 % at 20 M rows, +8 % at
// 100 M, -9 % at 200 M and -37 % at 1 B, where the two extra 16-byte loads per step cost more translation requests than the
// skipped rows save (profiles/r03_ahead_rows_threshold.txt); round 4 first let the table's own statistic (share of positions
// that arrive at their LF target without a fast-forward: 0.83 / 0.75 on real BWTs, 0.51 on random ones) extend it to 256 M
// rows of real text (113 M rows: 42.3 -> 53.5 Gbases/s, profiles/r04_real_100M.txt).  The pair-shared gathers then removed
// the translation cost the size rule was about (launch_pml: on for walked tables of 2 GB and more): on the look-ahead rows
// the random table now runs 45.4 against 38.5 Gbases/s at 200 M rows, 43.4 / 36.3 at 350 M, 44.4 / 34.8 at 700 M and
// 42.0 - 44.2 / 34.6 at 1 B (without the pairs: 21.4), the real 226 M-row BWT 50.8 / 38.6
// (profiles/r04_pair_shared_gathers.txt) -- so the copy pays at every size measured, and only memory decides.
// The statistic still steers the count query (kAheadCountRatio below) and is reported (movi_index_info "ahead_no_ff").
inline bool ahead_eligible(const DerivedFacts &f) { return f.kmode == 6 && f.r >= 8 && (f.r >> 36) == 0; }
// by_itself: built by the size policy, not on request -- then the count query uses the copy only where the table's own
// statistic says it pays (DevIndex::rows2_count)
constexpr double kAheadCountRatio = 0.67;
inline bool ahead_serves_count(bool by_itself, double no_ff) { return !by_itself || no_ff >= kAheadCountRatio; }

// Deep rows (DevIndex::rows3; round 6): the PML walk's layout for tables of fewer than 2^28 - 1 rows -- 1.33 x the bytes of the look-ahead
// rows for three bases per gather instead of two.  Built by itself up to kDeepAutoRows rows (the copy then stays within reach of the
// Infinity Cache and the per-CU TLBs: profiles/r06_deep_rows.txt has the sizes measured), instead of the look-ahead rows, which the PML
// walk no longer needs then; "deep_rows" 1 / 0 builds / frees them at any eligible size.
constexpr uint64_t kDeepAutoRows = 48ull << 20;             // 50 M rows: a copy of 1 GiB
// Width of a reposition hint in the deep rows ("deep_hint_bits" -1).  4 = narrow ids, reach 15: the builder looks up to 15 rows past
// either edge of a window for each of a row's three slots instead of 3 (c2, 14 M rows: profiles/deep_hints.txt has the build time).
constexpr int kDeepHintBitsDefault = 4;
inline bool deep_rows_fit(uint64_t r) { return r >= 8 && r <= kDeepWideMaxRows; }   // (the builder's own check: deep_rows_eligible, movi_kernels.hpp)
inline bool deep_eligible(const DerivedFacts &f) { return f.kmode == 6 && deep_rows_fit(f.r); }
// The hint width the deep rows are built with now (4 bits need narrow ids: tables of 2^26 rows and more keep wide ids and 2 bits)
inline int deep_hint_width(const DerivedPolicy &p, const DerivedFacts &f) {
    return (int)deep_map_for(f.r, p.deep_hint_bits < 0 ? kDeepHintBitsDefault : p.deep_hint_bits).hint_bits;
}

// Chain rows (pml_kernel_chain): 32 bytes per row, up to four bases per gather in half-line windows of two rows.  1.5 x the bytes of the deep
// rows for 11 % fewer fabric lines per base where chains run deep (c2: tools/iter_model.c 0.447 -> 0.396 lines per base, lane iterations per
// base 0.4888 -> 0.4394 measured; the 450 MB table's line rate is 8 % lower than the 300 MB one's and the launch 2.2 % faster, every run above
// the deep rows' fastest: profiles/chain_rows.txt); where every other base fast-forwards the deeper chain is rarely ridden and the bigger
// table only costs cache reach (c2mid, modelled: 0.534 -> 0.514 lines for + 50 % bytes).  Built by itself BESIDE the deep rows -- long reads
// and segment plans keep walking there -- where the deep rows' own conditions hold and
//   * the table has at least kChainMinRows rows: 12 Mi rows are the deep rows that fill the 256 MiB Infinity Cache (64 bytes per three rows);
//     a smaller table's launch is not bound by fabric lines, and every index of the test suite but the two pangenomes lies below it;
//   * the tallied no-fast-forward share is at least kChainNoFfShare: c2 0.834, c2mid 0.732;
//   * the device has room for the rows and 2 GiB beside them.
// kChainMinRows = kChainNoTable would switch the auto-build off; "chain_rows" 1 builds the rows on any eligible index.
constexpr uint64_t kChainNoTable = ~0ull;
constexpr uint64_t kChainMinRows = 12ull << 20;
constexpr double kChainNoFfShare = 0.80;
inline bool chain_rows_fit(uint64_t r) { return r >= 8 && r <= kChainMaxRows; }
inline bool chain_eligible(const DerivedFacts &f) { return f.kmode == 6 && chain_rows_fit(f.r); }
// The auto-build (after ensure_pml_tables, whose tally it reads): a failed or declined build leaves the deep rows in charge.
template <class Dev>
void ensure_chain_rows(DerivedPolicy &p, const DerivedFacts &f, Dev &dev, bool from_prepare) {
    if (p.chain_auto <= 0 || f.held[kTabChain] || !chain_eligible(f) || !(from_prepare || !p.prepared)) return;
    if (!f.held[kTabDeep] || f.r > kDeepAutoRows) return;                  // beside the deep rows, where the policy builds those
    if (f.r < kChainMinRows || !p.ahead_tallied || p.ahead_no_ff < kChainNoFfShare) { p.chain_auto = 0; return; }
    uint64_t free_b = 0, total_b = 0;
    if (!dev.mem_info(free_b, total_b) || free_b < f.chain_bytes + (2ull << 30) || !dev.build_chain()) p.chain_auto = 0;
}
// The count query's interval table (DevIndex::ftab): any DNA index, thresholds or not.
inline bool ftab_eligible(const DerivedFacts &f) { return (f.kmode == 6 || f.kmode == 3) && f.dna; }

// The statistic over a sample of the table's rows, before anything is built.  A sample that fails leaves it untallied.
template <class Dev>
void sample_no_ff(DerivedPolicy &p, Dev &dev) {
    if (p.ahead_tallied) return;
    double share = 0.0;
    if (!dev.sample_no_ff(share)) return;
    p.ahead_no_ff = share;
    p.ahead_tallied = true;
}
// Should the first query build the look-ahead rows by itself?  Yes, if they leave room for the query's own buffers.
template <class Dev>
bool ahead_wanted(const DerivedFacts &f, Dev &dev) {
    const uint64_t bytes = f.ahead_bytes;
    uint64_t free_b = 0, total_b = 0;
    if (!dev.mem_info(free_b, total_b)) return false;
    // (never more than a quarter of the device by itself: a handle's derived tables are the caller's HBM too -- "ahead_rows" 1
    // builds them whatever their size, movi_index_info reports them)
    return bytes <= total_b / 4 && free_b > bytes + std::max<uint64_t>(2ull << 30, bytes / 2);
}
// The builder tallies every row: its share replaces a sample's.  *serves_count: DevIndex::rows2_count of the copy just built.
template <class Dev>
bool build_ahead(DerivedPolicy &p, Dev &dev, bool by_itself, bool *serves_count = nullptr) {
    double share = 0.0;
    bool serves = false;
    if (!dev.build_ahead(by_itself, share, serves)) return false;
    p.ahead_no_ff = share;
    p.ahead_tallied = true;
    if (serves_count) *serves_count = serves;
    return true;
}

// The derived tables of the PML walk -- top-of-walk table (256 MB at K = 12, a few ms), look-ahead rows (16 B per row), deep rows --:
// built by movi_index_prepare, or by the first PML query on the handle.  Nothing here fails the query: a table there is no room
// for (or a device in trouble, which the walk's own launch will report) is done without.
template <class Dev>
void ensure_pml_tables(DerivedPolicy &p, const DerivedFacts &f, Dev &dev, bool from_prepare) {
    if (p.kmer_auto > 0 && !f.held[kTabKmer] && kmer_eligible(f)) {
        if (!dev.build_kmer((uint32_t)p.kmer_auto)) p.kmer_auto = 0;
    }
    // (after movi_index_prepare the header's promise holds: query calls allocate nothing and build nothing -- a copy that was declined
    // for lack of memory is asked for again by the next explicit movi_index_prepare, never from inside a query, which may be under
    // stream capture or in the middle of a streaming run)
    if (p.ahead_auto > 0 && !f.held[kTabAhead] && ahead_eligible(f) && (from_prepare || !p.prepared)) {
        // (declined for lack of memory: the device is asked again after 64 calls, not in every one -- hipMemGetInfo per chunk of
        // a streaming run -- and two processes sharing a GPU that both pass the check and then collide switch the auto-build off)
        if (p.ahead_retry_in > 0) p.ahead_retry_in -= 1;
        else if (!ahead_wanted(f, dev)) p.ahead_retry_in = 63;
        else if (!build_ahead(p, dev, true)) p.ahead_auto = 0;
    }
    // The deep rows, beside the look-ahead rows (batches of short reads walk on the one, long reads on the other: launch_pml): tables of up
    // to kDeepAutoRows rows whose positions mostly reach their LF target without a fast-forward -- real text: the builder of the
    // look-ahead rows has tallied it, else a sample does -- three bases per gather need two such arrivals in a row (uniformly random
    // run sequences, 0.51: 62.4 -> 61.2 Gbases/s; the pangenome BWT, 0.83: 80.3 -> 89.6 with reset masks out)
    if (p.deep_auto > 0 && !f.held[kTabDeep] && deep_eligible(f) && f.r <= kDeepAutoRows && (from_prepare || !p.prepared)) {
        if (!p.ahead_tallied) sample_no_ff(p, dev);
        uint64_t free_b = 0, total_b = 0;
        if (p.ahead_tallied && p.ahead_no_ff < kAheadCountRatio) {
            p.deep_auto = 0;                                   // (the table's own statistic declines, for good)
        } else if (!dev.mem_info(free_b, total_b) || free_b < f.deep_bytes + (2ull << 30) || !dev.build_deep(deep_hint_width(p, f))) {
            p.deep_auto = 0;                                   // (no room, or a device in trouble: the walk stays on the look-ahead rows)
        }
    }
}

// The derived tables of the count query (MEM and k-mer queries search the same way) -- row-start checkpoints, interval table, and the
// look-ahead rows where the table's own statistic says the search will use them --: built by movi_index_prepare, or by the first count
// query on the handle.  false: the checkpoints, the one table the search cannot do without, could not be built -- the call fails.
template <class Dev>
bool ensure_count_tables(DerivedPolicy &p, const DerivedFacts &f, Dev &dev, bool from_prepare) {
    if (!f.held[kTabCkpt] && !dev.build_ckpt()) return false;
    if (p.ftab_auto > 0 && !f.held[kTabFtab] && ftab_eligible(f)) {       // the interval table (256 MB at K = 12)
        if (!dev.build_ftab((uint32_t)p.ftab_auto)) p.ftab_auto = 0;
    }
    // (round 5: the count query's default is the lane state machine on the PLAIN rows, launch_count; the look-ahead copy serves
    // count_kernel_v0 only, i.e. "count_variant" 0)
    if (f.count_variant == 0 && p.ahead_auto > 0 && !f.held[kTabAhead] && !p.count_declined_ahead && ahead_eligible(f) &&
        (from_prepare || !p.prepared)) {
        // sampled first, so that a table that will not use the copy is not copied (16 B per row) to find out.  Only the table's
        // statistic declines for good; a device short of memory is asked again later (ahead_retry_in).
        bool serves_count = false;
        sample_no_ff(p, dev);
        if (!p.ahead_tallied) { /* the sample failed: the next call tries again */ }
        else if (p.ahead_no_ff < kAheadCountRatio) p.count_declined_ahead = true;
        else if (p.ahead_retry_in > 0) p.ahead_retry_in -= 1;
        else if (!ahead_wanted(f, dev)) p.ahead_retry_in = 63;
        else if (!build_ahead(p, dev, true, &serves_count)) p.ahead_auto = 0;
        else if (!serves_count) {
            // (the copy's own tally -- every row, not a sample -- says the count query is better off on the plain rows: the copy
            // is not kept for a caller who may never ask for PMLs; the first PML query builds it again, 85 us per 14 M rows)
            dev.drop(kTabAhead);
            p.count_declined_ahead = true;
        }
    }
    return true;
}

// The four build-now options: `which` is dropped and not built by itself any more -- the caller's choice from here on --, then built
// where `value` is not 0 (K of the two lookup tables; 1 for the two row copies) and the table is eligible.
enum class TableRequest { kDone, kIneligible, kBuildFailed };
template <class Dev>
TableRequest request_table(DerivedPolicy &p, const DerivedFacts &f, Dev &dev, DerivedTable which, uint32_t value) {
    dev.drop(which);
    bool eligible = false, built = false;
    switch (which) {
    case kTabKmer: p.kmer_auto = 0; eligible = kmer_eligible(f); break;
    case kTabFtab: p.ftab_auto = 0; eligible = ftab_eligible(f); break;
    case kTabAhead:
        p.ahead_auto = 0;
        dev.drop(kTabDeep);            // it is about what the PML walk runs on: the deep rows, which would take precedence over either answer,
        p.deep_auto = 0;               // go (and are not built by themselves any more; "deep_rows" 1 brings them back)
        eligible = ahead_eligible(f);
        break;
    case kTabDeep: p.deep_auto = 0; eligible = deep_eligible(f); break;
    default: return TableRequest::kIneligible;
    }
    if (value == 0) return TableRequest::kDone;
    if (!eligible) return TableRequest::kIneligible;
    switch (which) {
    case kTabKmer: built = dev.build_kmer(value); break;
    case kTabFtab: built = dev.build_ftab(value); break;
    case kTabAhead: built = build_ahead(p, dev, false); break;
    default: built = dev.build_deep(deep_hint_width(p, f)); break;
    }
    return built ? TableRequest::kDone : TableRequest::kBuildFailed;
}

// "chain_rows" 0 / 1: dropped and not built by itself any more, then built where asked.
template <class Dev>
TableRequest request_chain(DerivedPolicy &p, const DerivedFacts &f, Dev &dev, uint32_t value) {
    dev.drop(kTabChain);
    p.chain_auto = 0;
    if (value == 0) return TableRequest::kDone;
    if (!chain_eligible(f)) return TableRequest::kIneligible;
    return dev.build_chain() ? TableRequest::kDone : TableRequest::kBuildFailed;
}

// movi_index_prepare: an explicit call asks the device now, whatever an earlier one was told ...
inline void on_prepare(DerivedPolicy &p) { p.ahead_retry_in = 0; }
// ... and once it has gone through, query calls build nothing any more (a prepare that fails leaves the handle as it was)
inline void on_prepared(DerivedPolicy &p) { p.prepared = true; }

}  // namespace movi
