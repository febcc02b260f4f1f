// The plan of a *_host call (movi_abi.hip), made before its loop runs: how the call comes down and whether it overlaps (plan_host_call,
// HostCall::settle), and its chunks, each with its own way down (plan_chunks).  Facts in, decisions out: no HIP in here, so that
// tests/host/host_plan_driver.cpp prints the plans without a GPU (tests/test_host_plan_cpu.py, tests/golden/host_plan_table.txt).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace movi {

// Reads are cut into chunks so that the staging buffers stay bounded whatever the input size:
// about kChunkBases bases per launch -- but never so few READS that the GPU runs empty.  One lane
// walks one read, so a chunk of long reads (2^28 bases = 27 k reads of 10 kbp) would leave most of
// the 524 k lane slots idle and the walk latency-bound; such chunks grow until they hold
// kMinChunkReads reads or kMaxChunkBases bases (3 B of device memory per base, 6 GiB).
constexpr uint64_t kChunkBases = 1ull << 28;
constexpr uint64_t kMinChunkReads = 1ull << 18;
constexpr uint64_t kMaxChunkBases = 1ull << 31;
// The overlapped path (page-locked caller buffers) wants several chunks per call -- chunk i+1 goes up and chunk i-1 comes
// down while chunk i is walked, and the kernels of neighbouring chunks share the GPU -- so it cuts finer: about an
// eighth of the call, between 2^22 and 2^28 bases, and at least 2^15 reads (a download can only start when a walk
// has finished, so chunks must be short; the lanes in flight are those of the kPipeAhead chunks being walked, and a
// read takes as long as it takes however few lanes walk beside it -- long reads are best cut into just those
// kPipeAhead chunks: 100 k x 10 kbp as 3 x 33 k reads 57 ms, as 8 x 12.5 k reads 85 ms, synchronous 74 ms).
constexpr uint64_t kPipeMinBases = 1ull << 22;
constexpr uint64_t kPipeMinReads = 1ull << 15;
constexpr uint64_t kPipeTargetChunks = 8;
constexpr uint64_t kPipeMaskChunks = 16;
// Queries whose per-read results vary in length (MEMs, k-mer runs; run_compact) go through the handle's staging in chunks of about
// kCompactChunkBases bases (at least kCompactChunkReads reads, at most kCompactMaxChunkBases: the device stages elem_bytes per base,
// twice -- the kernel's output and its compacted copy).  The k-mer occurrence query (8 bytes per base staged on the device, work handed
// out per k-mer: no minimum of reads) goes through it in chunks of kKmerOccChunkBases bases, or of "pipe_chunk_bases" where that is set.
constexpr uint64_t kKmerOccChunkBases = 1ull << 26;
constexpr uint64_t kCompactChunkBases = 1ull << 25;
constexpr uint64_t kCompactChunkReads = 1ull << 18;
constexpr uint64_t kCompactMaxChunkBases = 1ull << 27;

// THE rule by which reads become chunks: as many reads as stay within `target` bases, at least one, and at least `min_reads` of them
// while that stays within `max_bases`.  head[k] != 0 is the target of chunk k = 0, 1 alone (the overlapped path's small first chunks).
struct CutRule {
    uint64_t target = kChunkBases, min_reads = kMinChunkReads, max_bases = kMaxChunkBases;
    uint64_t head[2] = {0, 0};
};

// One chunk of a call: reads [first, first + nr), whose nb bases start at position b0 of the caller's arrays; for PML / ZML calls its way
// down (`masks`: reset masks that the host expands, else the u16 vector by DMA) and the bit its first base has in its first mask word.
struct HostChunk {
    uint64_t first = 0, nr = 0, b0 = 0, nb = 0;
    bool masks = false;
    uint32_t phase = 0;
};

// The end of the chunk that starts at read `first` (the offsets are non-decreasing: check_offsets).  Two binary searches, not a scan:
// where the target ends, and -- only if that is short of min_reads -- where min_reads or max_bases end; the chunk is the longer of
// the two.  That is where the scan "take the next read while it fits the target, or while there are fewer than min_reads and it fits
// max_bases" stops, both conditions being monotone in the read.
inline uint64_t chunk_end(const uint64_t *offs, uint64_t n_reads, uint64_t first, uint64_t target, uint64_t min_reads, uint64_t max_bases) {
    const uint64_t *lo = offs + first + 1, *end = offs + n_reads + 1;
    uint64_t last = (uint64_t)(std::upper_bound(lo, end, offs[first] + target) - offs) - 1;
    if (last - first < min_reads) {
        const uint64_t cap = (uint64_t)(std::upper_bound(lo, end, offs[first] + max_bases) - offs) - 1;
        last = std::max(last, std::min(first + min_reads, cap));
    }
    return std::min(std::max(last, first + 1), n_reads);
}

inline std::vector<HostChunk> cut_chunks(const uint64_t *offs, uint64_t n_reads, const CutRule &rule) {
    std::vector<HostChunk> chunks;
    for (uint64_t first = 0; first < n_reads;) {
        const size_t k = chunks.size();
        const uint64_t last = chunk_end(offs, n_reads, first, k < 2 && rule.head[k] ? rule.head[k] : rule.target, rule.min_reads, rule.max_bases);
        HostChunk c;
        c.first = first; c.nr = last - first; c.b0 = offs[first]; c.nb = offs[last] - offs[first];
        c.phase = (uint32_t)((c.b0 - offs[0]) & 31u);
        chunks.push_back(c);
        first = last;
    }
    return chunks;
}

// What crosses the link for bases [b0, b0 + nb) of reads packed two bits per base: the bytes from byte b0 >> 2 of the caller's buffer that
// cover them (a byte that two chunks share goes up with both).
inline size_t packed_span_bytes(uint64_t b0, uint64_t nb) { return (size_t)(((b0 + nb + 3) >> 2) - (b0 >> 2)); }

// A chunk's offsets relative to its first base, as the device reads them; returns launch_pml's segment-policy hint: the chunk's longest
// read is (1) / is not (0) more than 1.5 x its mean.  One pass: the longest read is found while the offsets are written.
inline int fill_relative_offsets(uint64_t *rel, const uint64_t *offs, const HostChunk &c) {
    uint64_t longest = 0;
    for (uint64_t i = 0; i <= c.nr; i++) {
        rel[i] = offs[c.first + i] - c.b0;
        if (i && rel[i] - rel[i - 1] > longest) longest = rel[i] - rel[i - 1];
    }
    return (c.nr && longest * 2 > (c.nb / c.nr) * 3) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------- the call

enum class HostQuery {
    kMl,             // PML / ZML (ml_host): the u16 vector, the reset-mask words, or neither (--no-output) come back
    kLogs,           // PML + per-base logs: synchronous
    kSaEntries,      // 8 bytes per base come down, the locate walk is ~100 gathers per base: synchronous, nothing to overlap
    kPerRead,        // count, classify: per-read results, only the upload to hide
    kMultiClassify,  // per-read results, and the PML vector where the caller wants it (then synchronous); never page-locks by itself
    kCompact,        // MEMs, k-mer runs (run_compact): synchronous, chunks of their own size
    kKmerOcc         // 8 bytes per base come down and a lane owns k-mers, not reads: synchronous, chunks by bases alone
};
enum class HostRoute { kVector = 0, kMasks = 1, kMixed = 2 };

struct HostFacts {
    HostQuery query = HostQuery::kMl;
    bool zml = false;
    uint64_t total = 0, n_reads = 0;                   // bases and reads of the call (n_reads > 0)
    bool want_vector = false, want_words = false;      // kMl / kMultiClassify: the caller's u16 vector; kMl: the caller's mask words
    bool reads_pinned = false, vector_pinned = false;  // the caller's buffers are page-locked as they stand
    size_t small_bytes = 0;                            // per-read results: page-locked bytes per read of a chunk in flight
};
struct HostOptions {                                   // the handle's, by their movi_set_option names
    int host_overlap = 1, host_autopin = 1, host_masks = -1, host_mask_share = 70;
    uint64_t pipe_chunk_bases = 0;
    bool seg_seen = false;                             // the last overlapped call's long reads were walked segment-parallel
    int seg_len = 0;
};

// The way down of a PML call's u16 vector: as it is (2 bytes per base over PCIe, no host work where the caller's vector is
// page-locked) or as reset masks (1/8 byte per base) that the host's worker threads expand into the caller's vector -- the DMA engine
// and the host's cores are two resources.  "host_masks": -1 = masks for calls of >= 2^22 bases (no page-locking of the vector; with the
// words handed to the pool by a host function on the chunk's stream and sixteen chunks per call this way alone runs at 33 - 34 Gbases/s
// on 1 M x 150 bp, the vector's at 22.7, the 1 B / base upload's floor is 36.7), 0 = never masks, 1 = masks for every call, 2 = both
// ways side by side, `host_mask_share` percent of the bases as masks (31 - 34: no better than masks alone since the host function;
// profiles/r06_host_path.txt).
inline HostRoute host_route(const HostFacts &f, const HostOptions &o) {
    if (f.query != HostQuery::kMl) return HostRoute::kVector;
    if (f.want_words) return HostRoute::kMasks;
    if (f.zml || !f.want_vector) return HostRoute::kVector;
    if (o.host_masks > 0) return o.host_masks >= 2 ? HostRoute::kMixed : HostRoute::kMasks;
    return o.host_masks < 0 && f.total >= (1ull << 22) ? HostRoute::kMasks : HostRoute::kVector;
}

// A call in two steps.  plan_host_call says what the facts decide: the route, whether the buffers as they stand allow the overlapped
// path, and if not whether page-locking them for the call is worth trying (`pin_reads`, `pin_vector`: hipHostRegister can fail, so the
// caller tries and reports back).  settle(pinned_now) then fixes `overlapped`, the route and the cut.
struct HostCall {
    HostFacts facts;
    HostOptions opt;
    HostRoute route = HostRoute::kVector;
    bool pinned = false;                 // the caller's buffers allow the overlapped path (as they stand; after settle: or page-locked for the call)
    bool pin_reads = false, pin_vector = false;
    // ---- from settle() on
    bool overlapped = false;             // run_pipelined, else run_chunked / run_compact
    bool vector_down = false;            // 2 bytes per base come down by DMA
    bool words_in_block = false;         // overlapped: a slot's page-locked block also holds the chunk's reset-mask words, behind the per-read results
    size_t small_bytes = 0;              // page-locked bytes per read that fetch / harvest use
    CutRule rule;

    void settle(bool pinned_now) {
        pinned = pinned || pinned_now;
        // (a mixed call whose buffers are not page-locked: one way down for the whole call.  One whose buffers are, but which "host_overlap"
        // 0 sends down the synchronous path, stays mixed and deals its chunks there)
        if (route == HostRoute::kMixed && !pinned) route = HostRoute::kMasks;
        overlapped = pinned && opt.host_overlap != 0;
        // (vector_down: the way down bounds such a call, and with every read going up at once beside it the downloads ran 8 % slower:
        // those calls feed their uploads from the loop)
        vector_down = route != HostRoute::kMasks && facts.query == HostQuery::kMl && facts.want_vector;
        words_in_block = route != HostRoute::kVector;
        small_bytes = facts.small_bytes;
        rule = CutRule();
        if (facts.query == HostQuery::kCompact) { rule.target = kCompactChunkBases; rule.min_reads = kCompactChunkReads; rule.max_bases = kCompactMaxChunkBases; }
        if (facts.query == HostQuery::kKmerOcc) { rule.target = opt.pipe_chunk_bases ? opt.pipe_chunk_bases : kKmerOccChunkBases; rule.min_reads = 1; }
        if (!overlapped) return;
        // (calls whose results -- all or part of them -- come down as reset masks for the host's worker pool are cut twice as fine: the pool's
        // work arrives earlier and more evenly; 1 M x 150 bp: masks alone 22.9 -> 32.4 Gbases/s, both ways down 30 -> 33.9; finer still and
        // the walks no longer fill the GPU: profiles/r06_host_path.txt)
        uint64_t target = facts.total / (words_in_block ? kPipeMaskChunks : kPipeTargetChunks);
        target = target < kPipeMinBases ? kPipeMinBases : (target > kChunkBases ? kChunkBases : target);
        rule.target = target;
        rule.min_reads = kPipeMinReads;
        // Long reads are cut into few, big chunks because a read takes its time however few lanes walk beside it -- unless the
        // reads are walked segment-parallel, which the host only knows afterwards: a caller whose last call was (a stream of
        // batches of the same kind of reads) gets chunks of >= 2^12 reads from then on, whose downloads start earlier.
        if (opt.seg_seen && opt.seg_len > 0 && facts.total / facts.n_reads >= 2ull * (uint64_t)opt.seg_len) rule.min_reads = 1ull << 12;
        if (opt.pipe_chunk_bases) { rule.target = opt.pipe_chunk_bases; rule.min_reads = 1; return; }
        // (the first download can only start when the first walk is over: the first two chunks are a quarter and half the size -- not
        // where masks come down: a chunk's masks are 1/16 of its vector, and sixteen equal chunks ran 8 % faster than the same with a
        // half-size second one)
        for (int k = 0; k < 2 && !words_in_block; k++)
            if ((target >> (2 - k)) >= kPipeMinBases) rule.head[k] = target >> (2 - k);
    }
    // ALL THE READS GO UP AHEAD OF THE LOOP (overlapped calls of up to 2^31 bases, into the handle's call-wide staging; no room for it:
    // chunk by chunk): see run_pipelined
    bool upload_ahead(size_t n_chunks) const { return overlapped && n_chunks > 1 && facts.total <= (1ull << 31) && !vector_down; }
};

// Could the call overlap at all, were its buffers page-locked?  (Asked before the runtime is: whether a buffer is page-locked costs a call.)
// Queries with per-read results (count, bins) only have their upload to hide.  A read takes as long as it takes: with
// long reads the last chunk's walk starts when the last byte has arrived and lasts as long as the whole batch's would
// (100 k x 10 kbp, bins: 43 ms overlapped, 38 ms synchronous); with short reads the walks are short against the
// transfers and overlapping pays (1 M x 150 bp: count 20.6 -> 25.1, bins 21.8 -> 28.8 Gbases/s).
inline bool overlap_possible(const HostFacts &f) {
    const bool small_worth = f.total != 0 && f.total / f.n_reads <= 2048;
    switch (f.query) {
    case HostQuery::kMl: return f.total != 0;
    case HostQuery::kPerRead: return small_worth;
    case HostQuery::kMultiClassify: return !f.want_vector && small_worth;
    default: return false;
    }
}
// ... and does it then need the caller's vector page-locked beside the reads?  (masks: only the reads -- the vector is written by host threads)
inline bool needs_pinned_vector(const HostFacts &f, const HostOptions &o) {
    return f.query == HostQuery::kMl && f.want_vector && host_route(f, o) != HostRoute::kMasks;
}

inline HostCall plan_host_call(const HostFacts &f, const HostOptions &o) {
    HostCall c;
    c.facts = f;
    c.opt = o;
    c.route = host_route(f, o);
    c.pinned = overlap_possible(f) && f.reads_pinned && (!needs_pinned_vector(f, o) || f.vector_pinned);
    // A big call on PAGEABLE buffers (what a std::vector-holding caller passes: INTEGRATION.md's stub): page-lock them for the
    // duration of the call and take the overlapped path.  Registering touched memory runs at hundreds of GB/s (DESIGN.md section
    // 5), so on >= 2^27 bases it is paid back several times over (the synchronous path: 12.4 Gbases/s PCIe-inclusive).
    // "host_autopin" 0 turns it off; anything that fails there falls back to the synchronous path.
    // (the overlapped path cuts a call into pieces of >= 2^15 reads: it needs at least three of them to overlap anything;
    // --multi-classify never page-locks by itself)
    c.pin_reads = !c.pinned && overlap_possible(f) && f.query != HostQuery::kMultiClassify && o.host_autopin && o.host_overlap &&
                  f.total >= (1ull << 27) && f.n_reads >= 3 * kPipeMinReads;
    c.pin_vector = c.pin_reads && needs_pinned_vector(f, o);
    return c;
}

// The call's chunks, in order -- which is the order they are launched in, by run_chunked's loop and by run_pipelined's up() alike --,
// each with its way down.  A mixed call deals its chunks by `host_mask_share` as it goes: a chunk comes down as masks if the bases
// launched as masks so far, this chunk's included, stay within the share (so the first chunk comes down as it is: its DMA starts
// when its walk ends).  (Tried: walks that leave both on the device and a choice at download time by the pool's backlog -- 28.1
// against 29.9 Gbases/s for the plain deal; a call's tail cut into halving chunks -- 27.3 against 28.1: profiles/r06_host_path.txt.)
inline std::vector<HostChunk> plan_chunks(const HostCall &call, const uint64_t *offs, uint64_t n_reads) {
    std::vector<HostChunk> chunks = cut_chunks(offs, n_reads, call.rule);
    uint64_t dealt = 0, dealt_as_masks = 0;                       // bases launched so far / of them by the mask route
    for (HostChunk &c : chunks) {
        if (call.route == HostRoute::kMasks) c.masks = true;
        else if (call.route == HostRoute::kMixed) {
            c.masks = (dealt_as_masks + c.nb) * 100 <= (uint64_t)call.opt.host_mask_share * (dealt + c.nb);
            dealt += c.nb;
            if (c.masks) dealt_as_masks += c.nb;
        }
    }
    return chunks;
}

}  // namespace movi
