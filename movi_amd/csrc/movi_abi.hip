// movi_abi.hip -- the extern "C" boundary of libmovi_hip.so (see include/movi_hip.h).
// Host-side C++ only: index.movi parsing, device residency, launches, transfers.
// There is deliberately NO CPU compute path here: without a HIP device every
// query entry point fails with MOVI_ERR_NO_DEVICE / MOVI_ERR_HIP.
#include "../../include/movi_hip.h"
#include "movi_kernels.hpp"
#include "movi_host_plan.hpp"
#include "movi_derived.hpp"
#include "movi_expand_host.hpp"
#include "movi_pack_host.hpp"
#include "movi_build.hpp"
#include "movi_text.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>
#include <fcntl.h>
#include <rccl/rccl.h>           // types and prototypes only: librccl.so.1 is bound at first use (movi_index_replicate)
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

using namespace movi;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int fail_hip(hipError_t e, const char *what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e) + " (hipError " + std::to_string((int)e) + ")";
    // the failure is REPORTED here: the thread's sticky last-error is cleared so that a later launch on this thread (callers may
    // tolerate this failure -- e.g. a staging reservation that did not fit) does not read it back as its own (hipGetLastError)
    (void)hipGetLastError();
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? MOVI_ERR_NO_DEVICE : MOVI_ERR_HIP;
}
#define HIP_TRY(expr)                                            \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) return fail_hip(e_, #expr);        \
    } while (0)

constexpr uint32_t kMoviMagic = 0x4D4F5649u;   // include/utils.hpp:29

bool mode_supported(uint32_t m) {
    return m == MOVI_MODE_REGULAR_THRESHOLDS || m == MOVI_MODE_BLOCKED_THRESHOLDS || m == MOVI_MODE_SAMPLED_THRESHOLDS ||
           m == MOVI_MODE_SAMPLED || m == MOVI_MODE_REGULAR || m == MOVI_MODE_BLOCKED;
}
bool mode_blocked(uint32_t m) { return m == MOVI_MODE_BLOCKED_THRESHOLDS || m == MOVI_MODE_BLOCKED; }
bool mode_sampled(uint32_t m) { return m == MOVI_MODE_SAMPLED_THRESHOLDS || m == MOVI_MODE_SAMPLED; }
// USE_THRESHOLDS, include/utils.hpp:145
bool mode_has_thresholds(uint32_t m) {
    return m == MOVI_MODE_REGULAR_THRESHOLDS || m == MOVI_MODE_BLOCKED_THRESHOLDS || m == MOVI_MODE_SAMPLED_THRESHOLDS;
}
size_t mode_row_bytes(uint32_t m) {             // MoveRow::row_size, include/move_row.hpp:104-120
    return (m == MOVI_MODE_REGULAR_THRESHOLDS || m == MOVI_MODE_REGULAR) ? 8 : (mode_blocked(m) ? 6 : 3);
}

struct Reader {
    const uint8_t *p;
    size_t n, pos = 0;
    // overflow-safe: `len` comes from file fields and may be anything
    bool get(void *dst, size_t len) {
        if (len > n - pos) return false;
        memcpy(dst, p + pos, len);
        pos += len;
        return true;
    }
    bool skip(size_t len) {
        if (len > n - pos) return false;
        pos += len;
        return true;
    }
};

}  // namespace

// the calling thread's message, for the entry points that live outside this file (movi_pack_host.cpp)
int movi::set_last_error(int code, const char *msg) { return fail(code, msg); }

// The handle's derived tables: one owner for the five device blocks and for what each publishes into the kernels' view of the index.
// publish() is the only writer of those DevIndex fields: it runs after every build and every drop, and once when the handle is made.
struct DerivedTables {
    DevPtr<uint4> kmer;              // top-of-walk table ("kmer_k" option)
    DevPtr<uint4> ftab;              // the count query's interval table ("ftab_k" option)
    DevPtr<uint8_t> rows2;           // look-ahead rows ("ahead_rows" option), 16 bytes per row
    DevPtr<uint8_t> rows3;           // deep rows ("deep_rows" option), 21.33 bytes per row: what the PML walk runs on where the policy builds them
    DevPtr<uint64_t> ckpt;           // row-start checkpoints: built lazily by the first count query
    DevPtr<uint8_t> rows4;           // chain rows ("chain_rows" option), 32 bytes per row: pml_kernel_chain walks on them (the kernels' view has no field for them: PmlCall::chain_rows)
    uint32_t kmer_k = 0, ftab_k = 0;
    uint64_t rows2_tail = 0;
    uint32_t rows2_count = 0, hints = 0;
    DeepMap deep{0, 0, 0, 0};        // the field map rows3 was built in
    bool held(DerivedTable t) const {
        return t == kTabChain ? (bool)rows4 : t == kTabKmer ? (bool)kmer : t == kTabFtab ? (bool)ftab : t == kTabAhead ? (bool)rows2 : t == kTabDeep ? (bool)rows3 : (bool)ckpt;
    }
    void reset(DerivedTable t) {
        switch (t) {
        case kTabKmer: kmer.reset(); kmer_k = 0; break;
        case kTabFtab: ftab.reset(); ftab_k = 0; break;
        case kTabAhead: rows2.reset(); rows2_tail = 0; rows2_count = hints = 0; break;
        case kTabDeep: rows3.reset(); deep = DeepMap{0, 0, 0, 0}; break;
        case kTabChain: rows4.reset(); break;
        default: ckpt.reset(); break;
        }
    }
    void publish(DevIndex &v) const {
        v.kmer = kmer.get(); v.kmer_k = kmer_k;
        v.ftab = ftab.get(); v.ftab_k = ftab_k;
        v.rows2 = rows2.get(); v.rows2_tail = rows2_tail; v.rows2_count = rows2_count; v.hints = hints;
        v.rows3 = rows3.get(); v.deep_id_mask = deep.id_mask; v.deep_id_bits = deep.id_bits; v.deep_j3_shift = deep.j3_shift; v.deep_hint_bits = deep.hint_bits;
        v.row_start_ckpt = ckpt.get();
    }
    // One size per table of r rows (K: of the two lookup tables): what its builder allocates, and what movi_index_info reports of a table
    // the handle holds -- but for the checkpoints, whose report has a formula of its own (below)
    static size_t bytes(DerivedTable t, uint64_t r, uint32_t K) {
        switch (t) {
        case kTabKmer: case kTabFtab: return (size_t)16 << (2 * K);
        case kTabAhead: return ahead_rows_bytes(r);
        case kTabDeep: return deep_rows_bytes(r);
        case kTabChain: return chain_rows_bytes(r);
        default: return (((r + (1ull << kPrefixShift) - 1) >> kPrefixShift) + 1) * sizeof(uint64_t);   // ceil(r / 32) + 1 entries
        }
    }
    double held_bytes(DerivedTable t, uint64_t r) const { return held(t) ? (double)bytes(t, r, t == kTabKmer ? kmer_k : ftab_k) : 0.0; }
    // "ckpt_bytes" has always reported r / 32 + 2 entries: 8 bytes more than are allocated where r is a multiple of 32, the same
    // elsewhere.  The two formulas differ by up to 8 bytes and both stay as they are.
    double ckpt_bytes_reported(uint64_t r) const { return ckpt ? (double)((r >> kPrefixShift) + 2) * 8.0 : 0.0; }
};

struct movi_index {
    int device = 0;
    movi_index_desc_t desc{};
    std::vector<uint32_t> id_blocks_host;
    std::vector<uint64_t> sep_rows_host;         // separators indexes: rows of the separator, ascending
    std::vector<uint64_t> sep_vals_host;         //   their ThresholdsRow (4 x u16 in one u64)
    std::vector<uint16_t> sep_thr_raw;           //   the file's two tables, kept for movi_index_get_desc-style round trips
    std::vector<uint64_t> sep_map_raw;
    DevPtr<uint64_t> d_sep_rows, d_sep_vals;
    std::vector<uint64_t> tally_host;            // mode 7: tally_ids widened to u64, [alphabet][n_tally]
    DevPtr<uint64_t> d_tally;
    DevPtr<uint8_t> d_rows;          // the resident table: the handle's, or borrowed (caller rows adopted by movi_index_create_from_device_rows)
    size_t rows_bytes = 0;
    DevPtr<uint8_t> d_code_of;
    DevPtr<uint32_t> d_id_blocks;
    DerivedTables tables;            // the derived tables and what they publish into `dev` ...
    DerivedPolicy policy;            // ... and which of them are built when (movi_derived.hpp)
    DevPtr<DevStats> d_stats;
    // locate: the attached sampled suffix array (movi_ssa_build / movi_ssa_load) and the locate rows derived from the table for its rate
    DevPtr<uint4> d_loc;             // 16 bytes per row (movi_sa.hpp)
    DevPtr<uint64_t> d_samples;      // length / sa_rate + 1 entries
    uint64_t sa_rate = 0;            // 0 = no sampled suffix array attached
    // Movi Color: the attached colour tables (movi_color_build / movi_color_load), on the host as the file holds them and on the device
    std::vector<uint16_t> color_flat;            // flat_colors
    std::vector<uint64_t> color_inds;            // doc_set_flat_inds, r entries (empty = no tables attached)
    std::vector<uint32_t> color_taxa;            // to_taxon_id of the build (empty after a load)
    uint32_t color_species = 0;
    DevPtr<uint16_t> d_color_flat;
    DevPtr<uint64_t> d_color_inds;
    DevBuf color_scratch;                        // the counters of movi_multi_classify_device calls that ask for no counter rows
    uint64_t color_scratch_bytes = 256ull << 20; // "color_scratch_bytes": what movi_index_prepare(MOVI_PREPARE_COLOR) reserves
    uint64_t color_chunk_keys = 0;               // "color_chunk_keys": BWT positions per chunk of the builder (0 = by the device's free memory)
    uint32_t color_chunks = 0;                   // what the last build took
    double color_seconds[3] = {0, 0, 0};         // ... and its seconds: walks, sorts, numbering
    DevIndex dev{};
    int kmode = 0;                   // row layout the kernels run on: desc.mode, except 6 for sampled-thresholds (expanded)
    LaunchCfg cfg;
    // device staging of the *_host entry points: grow-only, kept across calls (a hipMalloc / hipFree pair per call and
    // buffer cost more than the copies themselves); released by movi_index_destroy or movi_set_option("release_scratch")
    enum { kBases = 0, kOffs, kErr, kOut, kA, kB, kS, kMask, kTmp, kPacked, kExcPos, kExcByte, kScratchSlots };   // (kMask: a chunk's reset-mask words; kTmp: the u16 vector of a mask call whose path has no mask output of its own; kPacked: 2-bit packed reads on their way to kBases; kExcPos / kExcByte: their call's exception list, the handle's only)
    DevBuf scratch[kScratchSlots];
    SegWorkspace seg_ws;             // segment-parallel long reads (launch_pml): device workspace of the handle's own calls
    PinnedBuf h_rel;                 // synchronous path: a chunk's relative offsets (u64 entries), page-locked and kept (a fresh 2 MB vector per
                                     // call was page faults + a staged copy: ~0.3 ms of a 2 ms call)
    // the overlapped form of the *_host entry points (page-locked caller buffers, movi_host_alloc): kPipeSlots chunks in
    // flight, each on its own stream with its own device staging, counters and a small page-locked block for what
    // travels with a chunk (relative offsets up; error bytes, per-read results and counters down)
    struct PipeSlot {
        hipStream_t s = nullptr;
        hipEvent_t ev = nullptr;                 // the slot's walk has finished
        hipEvent_t ev_up = nullptr;              // the slot's chunk has arrived
        DevBuf d[kScratchSlots];
        DevPtr<DevStats> d_stats;
        SegWorkspace seg_ws;                     // segment-parallel long reads: this slot's device workspace
        PinnedBuf h;
        void release() {                         // the slot's stream drains, then what it may touch goes
            if (s) (void)hipStreamSynchronize(s);
            seg_ws.release();
            for (DevBuf &b : d) b.release();
            d_stats.reset();
            h.release();
            if (ev) (void)hipEventDestroy(ev);
            if (ev_up) (void)hipEventDestroy(ev_up);
            if (s) (void)hipStreamDestroy(s);
            ev = ev_up = nullptr;
            s = nullptr;
        }
    };
    enum { kPipeSlots = 6, kPipeAhead = 3 };   // slots; chunks going up or being walked while one comes down (2: -14 %, 4: the same)
    PipeSlot pipe[kPipeSlots];
    hipStream_t pipe_up = nullptr;   // every chunk's upload, in order (uploads on separate streams share the link and all arrive late)
    std::vector<hipEvent_t> pipe_ev; // chunk i of a call has arrived (calls whose reads go up ahead of the loop into scratch[kBases])
    int locate_matches_stages = 3;   // measurement hook ("locate_matches_stages"): movi_locate_matches_device stops after the searches and the scan (1), after the expansion (2: d_positions holds packed positions), or runs whole (3)
    uint64_t pipe_chunk_bases = 0;   // test hook ("pipe_chunk_bases"): chunk size of the overlapped path, 0 = its policy
    LaunchInfo last_launch;          // what the last query call launched (movi_last_launch)
    bool host_autopin = true;        // big *_host calls on pageable buffers page-lock them for the call ("host_autopin")
    bool host_overlap = true;        // page-locked buffers take the overlapped path ("host_overlap" 0: one upload, the walk, one download)
    bool seg_seen = false;           // the last PML / ZML host call on long reads was walked segment-parallel (chunk policy below)
    // the segment plan's probe verdict of the last batch of long reads, kept for the next calls on batches of the same shape (a stream of
    // batches of one kind of reads): the probe is a 0.4 ms read-back in front of a 5 ms walk (profiles/r06_few_long_reads.txt)
    int seg_cache_verdict = -1, seg_cache_left = 0;
    uint32_t seg_cache_key = 0;
    uint64_t reserved_result_bases = 0, reserved_reads = 0;   // "reserve_host_results" / "reserve_host_reads": what the mask words' scratch is reserved for
    int pml_via_mask = -1;           // "pml_via_mask": the walk's u16 vector through reset masks that its wavefronts expand themselves (-1: batches of short reads)
    int host_mask_share = 70;        // "host_mask_share": percent of a mixed call's bases that come down as masks (the rest as the vector itself)
    int host_masks = -1;             // "host_masks": movi_pml_host brings reset masks down and expands them on host worker threads (-1: calls of >= 2^22 bases into a pageable vector)
    int host_threads = 0;            // "host_threads": workers of the host-side expansion (0 = host_threads_default())
    // movi_pml_device's reset-mask words (its default route for batches of short reads), apart from the *_host staging: reserved by
    // movi_index_prepare(MOVI_PREPARE_PML) for kPrepareMaskBases bases in kPrepareMaskReads reads, by "reserve_device_masks", and grown
    // by a bigger call outside a stream capture.  A graph captured over a call keeps the buffer's address, so a buffer a captured call
    // has used is never freed by a growth: it is retired and kept until release_scratch / movi_index_destroy (GraphSafeBuf).
    GraphDevBuf::Retired graph_retired;
    GraphDevBuf dmask{&graph_retired};
    // the park queue of the mask walk's parked lanes (DevIndex::park_q; "park_lanes"): records of kParkRecBytes, reserved with the mask words
    // and grown, retired and freed by the same rules (a retired queue goes on the same list)
    GraphDevBuf dpark{&graph_retired};
private:
    // The members free device memory: the handle dies under its own device (movi_index_replicate makes handles on several devices
    // from one thread), which movi_index_destroy sets -- the only way out.
    ~movi_index() = default;
    friend int movi_index_destroy(movi_index_t *ix);
};

static void release_scratch(movi_index *ix);
static const char *const kNoSsa = "no sampled suffix array is attached to this index: build one with movi_ssa_build (`movi build-SA`) or "
                                  "load ssa.movi with movi_ssa_load";
static const char *const kNoColor = "no colour tables are attached to this index: build them with movi_color_build (`movi color`) or load "
                                    "doc_sets_flat.bin with movi_color_load";
// The counters of one chunk of reads of movi_multi_classify_device: at least one read's row
static hipError_t reserve_color_scratch(movi_index *ix) {
    return grow(ix->color_scratch, std::max<size_t>((size_t)ix->color_scratch_bytes, (size_t)ix->color_species * 4));
}
constexpr uint64_t kPrepareMaskBases = 1ull << 28;   // movi_index_prepare's reservation of movi_pml_device's mask words (1 M x 150 bp fits)
constexpr uint64_t kPrepareMaskReads = 1ull << 22;
// the lanes a wavefront of a call on this handle may park: what "park_lanes" asks for, or what plan_pml's own rule can pick
static int park_lanes_wanted(const movi_index *ix) { return ix->cfg.park_lanes > 0 ? ix->cfg.park_lanes : (ix->cfg.park_lanes < 0 ? kParkLanesAuto : 0); }
// bytes of the queue of a call of n_reads reads: one record per lane of the second launch's grid, as launch_pml counts them for any block
// of up to 256 threads (blocks x wavefronts per block <= wavefronts of reads + 3; the grid is whole blocks)
static size_t park_queue_bytes(uint64_t n_reads, int lanes) {
    const uint64_t recs = (((n_reads + 63) / 64 + 3) * (uint64_t)lanes + 255) / 256 * 256;
    return kParkHeadBytes + (size_t)recs * kParkRecBytes;
}
// Is `s` being captured into a graph?  A query that cannot tell (hipErrorStreamCaptureImplicit: the null stream while another stream
// captures in global mode) answers yes: the callers then take the route that allocates nothing.  *known_active (optional): the query
// succeeded and said that `s` itself is capturing.
static bool stream_capturing(hipStream_t s, bool *known_active = nullptr) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (known_active) *known_active = false;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    if (known_active) *known_active = st == hipStreamCaptureStatusActive;
    return st != hipStreamCaptureStatusNone;
}
// The queue a mask walk of n_reads reads can be lent, in records (0: none -- parking is off, or the call is being captured and the queue
// it would need is not there yet): what the plan is told, before anything is grown.
static uint64_t park_queue_offer(const movi_index *ix, uint64_t n_reads, bool capturing) {
    const int lanes = park_lanes_wanted(ix);
    if (lanes <= 0) return 0;
    const size_t need = park_queue_bytes(n_reads, lanes);
    if (capturing && need > ix->dpark.cap()) return 0;
    return (std::max(need, ix->dpark.cap()) - kParkHeadBytes) / kParkRecBytes;
}
// Lends that queue: grown outside a stream capture only.  false: the queue could not be grown, the call runs with parking off.
static bool lend_park_queue(movi_index *ix, uint64_t n_reads, bool capturing, MaskArgs &m) {
    const size_t need = park_queue_bytes(n_reads, park_lanes_wanted(ix));
    if (!capturing && grow(ix->dpark, need) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (capturing) ix->dpark.mark_in_graph();
    m.park_q = ix->dpark.ptr();
    m.park_cap = (ix->dpark.cap() - kParkHeadBytes) / kParkRecBytes;
    return true;
}
// The upload stream of the overlapped host paths.  Streams of one priority share a handful of hardware queues, and a chunk's stream that
// landed on the upload stream's queue had its walk queued behind the copies' completion packets (every sixth chunk waited for uploads that
// were not its own: 0.1 ms of a dry upload stream each time, profiles/r06_host_path.txt).  A stream of another priority gets a queue of
// its own kind.
static hipError_t create_upload_stream(hipStream_t *s) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
        if (hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

extern "C" {

const char *movi_last_error(void) { return g_err.c_str(); }
int movi_version(void) { return 100; }

int movi_device_count(int *count) {
    if (!count) return fail(MOVI_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail_hip(e, "hipGetDeviceCount"); }
    *count = n;
    return MOVI_OK;
}

// MoveStructure::deserialize, src/move_structure_io.cpp:471-511: v2 header
// (include/utils.hpp:32-61) | end_bwt_idx thresholds / next_down / next_up (3 x 4 x u64,
// :145-151) | alphamap (:153-157) | alphabet (:159-169) | u16 nt_splitting, bool constant
// (:171-172) | r rows (:361-397) | three overflow tables (:219-237) | counts and the
// base intervals (:269-287) | mode 8: id_blocks + block_size (:305-324) | with separators: their
// thresholds and the row -> entry map (:415-433).
int movi_index_parse(const void *h_image, size_t image_bytes, movi_index_desc_t *desc,
                     size_t *rows_offset, size_t *rows_bytes) {
    if (!h_image || !desc) return fail(MOVI_ERR_ARG, "NULL argument");
    Reader rd{static_cast<const uint8_t *>(h_image), image_bytes};
    uint8_t hdr[48];
    if (!rd.get(hdr, 48)) return fail(MOVI_ERR_FORMAT, "index image shorter than the 48-byte header");
    uint32_t magic;
    memcpy(&magic, hdr, 4);
    if (magic != kMoviMagic)
        return fail(MOVI_ERR_FORMAT, "invalid magic number in header: not a Movi 2.x index file");
    memset(desc, 0, sizeof(*desc));
    desc->mode = hdr[7];
    if (!mode_supported(desc->mode))
        return fail(MOVI_ERR_FORMAT, "index mode " + std::to_string(desc->mode) + " is not supported (only blocked=2, regular=3, "
                                         "sampled=5, regular-thresholds=6, sampled-thresholds=7 and blocked-thresholds=8; the "
                                         "Movi-1 style types large / constant / split are not)");
    memcpy(&desc->length, hdr + 16, 8);
    memcpy(&desc->r, hdr + 24, 8);
    memcpy(&desc->end_bwt_idx, hdr + 40, 8);
    // ids are 36 bits in every supported row layout (move_row_configs.hpp:34-51), so r < 2^36 -- which also keeps
    // every product of r below with a row size far from wrapping a u64
    if (desc->r == 0 || desc->r >= (1ull << 36) || desc->end_bwt_idx >= desc->r)
        return fail(MOVI_ERR_FORMAT, "corrupt header (r / end_bwt_idx)");
    if (!rd.get(desc->end_bwt_idx_thresholds, 32) || !rd.skip(64)) return fail(MOVI_ERR_FORMAT, "truncated index (basic data)");
    uint64_t amap_n = 0;
    if (!rd.get(&amap_n, 8) || amap_n != 256) return fail(MOVI_ERR_FORMAT, "unexpected alphamap size");
    uint64_t amap[256];
    if (!rd.get(amap, sizeof(amap))) return fail(MOVI_ERR_FORMAT, "truncated index (alphamap)");
    uint64_t asz = 0;
    if (!rd.get(&asz, 8) || asz == 0 || asz > 8) return fail(MOVI_ERR_FORMAT, "unexpected alphabet size");
    if (!rd.get(desc->alphabet, asz)) return fail(MOVI_ERR_FORMAT, "truncated index (alphabet)");
    // MoveStructure::use_separator, src/move_structure.cpp:547-552: five symbols led by '%'
    const bool sep = asz == 5 && desc->alphabet[0] == '%';
    if (asz > 4 && !sep)
        return fail(MOVI_ERR_FORMAT, "alphabet has " + std::to_string(asz) +
                                         " symbols: only DNA (<= 4) and separator ('%' + ACGT) indexes are supported");
    desc->alphabet_size = (uint32_t)asz;
    for (int c = 0; c < 256; c++) desc->code_of[c] = (c < 128 && amap[c] < asz) ? (uint8_t)amap[c] : 0xFF;
    if (sep) desc->code_of[(int)'%'] = 0xFF;               // check_alphabet, move_structure.cpp:384-388
    if (!rd.skip(3)) return fail(MOVI_ERR_FORMAT, "truncated index (flags)");
    const size_t row_b = mode_row_bytes(desc->mode);
    const size_t roff = rd.pos;
    if (desc->r > (image_bytes - rd.pos) / row_b || !rd.skip(desc->r * row_b))
        return fail(MOVI_ERR_FORMAT, "truncated index (move rows)");
    const bool sampled = mode_sampled(desc->mode);
    if (sampled) {                                         // read_tally_table, move_structure_io.cpp:338-349
        if (!rd.get(&desc->tally_checkpoints, 4) || desc->tally_checkpoints == 0)
            return fail(MOVI_ERR_FORMAT, "truncated index (tally checkpoints)");
        if (!rd.get(&desc->n_tally, 8)) return fail(MOVI_ERR_FORMAT, "truncated index (tally table)");
        desc->tally_ids = rd.p + rd.pos;
        if (desc->n_tally > image_bytes / (asz * 5) || !rd.skip(desc->n_tally * asz * 5))
            return fail(MOVI_ERR_FORMAT, "truncated index (tally table)");
        if (desc->n_tally < desc->r / desc->tally_checkpoints + 2)
            return fail(MOVI_ERR_FORMAT, "tally table does not cover the rows");
    }
    for (int t = 0; t < 3; t++) {
        uint64_t sz = 0;
        if (!rd.get(&sz, 8)) return fail(MOVI_ERR_FORMAT, "truncated index (overflow tables)");
        if (sz != 0) return fail(MOVI_ERR_FORMAT, "non-empty overflow table in a mode 6/8 index");
    }
    uint64_t csz = 0;
    if (!rd.get(&csz, 8) || csz > 8 || !rd.skip(csz * 8)) return fail(MOVI_ERR_FORMAT, "truncated index (counts)");
    uint64_t k = 0;
    if (!rd.get(&k, 8) || k != asz + 1) return fail(MOVI_ERR_FORMAT, "unexpected base-interval table size");
    if (!rd.get(desc->last_runs, k * 8) || !rd.get(desc->last_offsets, k * 8) ||
        !rd.get(desc->first_runs, k * 8) || !rd.get(desc->first_offsets, k * 8))
        return fail(MOVI_ERR_FORMAT, "truncated index (base intervals)");
    if (mode_blocked(desc->mode)) {
        if (!rd.get(&desc->n_blocks, 8)) return fail(MOVI_ERR_FORMAT, "truncated index (id blocks)");
        // the id_blocks payload stays in the image; callers locate it via desc->id_blocks
        desc->id_blocks = reinterpret_cast<const uint32_t *>(rd.p + rd.pos);
        if (desc->n_blocks > image_bytes / (asz * 4) || !rd.skip(desc->n_blocks * asz * 4))
            return fail(MOVI_ERR_FORMAT, "truncated index (id blocks)");
        desc->block_size = desc->mode == MOVI_MODE_BLOCKED ? 4194304 : 1048576;   // BLOCK_SIZE, move_row_configs.hpp:73 / :102
        uint64_t bs = 0;
        if (rd.get(&bs, 8)) desc->block_size = bs;         // move_structure_io.cpp:321-323
        // n_blocks * block_size >= r without the product (either factor is a file field)
        if (desc->block_size == 0 || desc->n_blocks == 0 || (desc->r - 1) / desc->block_size >= desc->n_blocks)
            return fail(MOVI_ERR_FORMAT, "id blocks do not cover the table");
    }
    if (sep && mode_has_thresholds(desc->mode)) {          // read_separators_thresholds, move_structure_io.cpp:415-433 (USE_THRESHOLDS)
        if (!rd.get(&desc->n_separator_thresholds, 8)) return fail(MOVI_ERR_FORMAT, "truncated index (separator thresholds)");
        desc->separator_thresholds = rd.p + rd.pos;
        if (desc->n_separator_thresholds > image_bytes / 8 || !rd.skip(desc->n_separator_thresholds * 8))
            return fail(MOVI_ERR_FORMAT, "truncated index (separator thresholds)");
        if (!rd.get(&desc->n_separator_map, 8)) return fail(MOVI_ERR_FORMAT, "truncated index (separator map)");
        desc->separator_map = rd.p + rd.pos;
        if (desc->n_separator_map > image_bytes / 16 || !rd.skip(desc->n_separator_map * 16))
            return fail(MOVI_ERR_FORMAT, "truncated index (separator map)");
    }
    if (rows_offset) *rows_offset = roff;
    if (rows_bytes) *rows_bytes = desc->r * row_b;
    return MOVI_OK;
}

static int finish_create(movi_index *ix) {
    const movi_index_desc_t &d = ix->desc;
    HIP_TRY(dev_alloc(ix->d_code_of, 256));
    HIP_TRY(hipMemcpy(ix->d_code_of.get(), d.code_of, 256, hipMemcpyHostToDevice));
    if (mode_blocked(d.mode)) {
        const size_t nb = (size_t)d.n_blocks * d.alphabet_size;
        if (nb == 0 || ix->id_blocks_host.size() != nb) return fail(MOVI_ERR_ARG, "the blocked modes need id_blocks");
        HIP_TRY(dev_alloc(ix->d_id_blocks, nb * 4));
        HIP_TRY(hipMemcpy(ix->d_id_blocks.get(), ix->id_blocks_host.data(), nb * 4, hipMemcpyHostToDevice));
    }
    const bool sep = d.alphabet_size == 5;
    if (sep && !ix->sep_rows_host.empty()) {
        const size_t ns = ix->sep_rows_host.size();
        HIP_TRY(dev_alloc(ix->d_sep_rows, ns * 8));
        HIP_TRY(dev_alloc(ix->d_sep_vals, ns * 8));
        HIP_TRY(hipMemcpy(ix->d_sep_rows.get(), ix->sep_rows_host.data(), ns * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ix->d_sep_vals.get(), ix->sep_vals_host.data(), ns * 8, hipMemcpyHostToDevice));
    }
    if (mode_sampled(d.mode)) {
        if (ix->tally_host.empty()) return fail(MOVI_ERR_ARG, "the sampled modes need tally_ids");
        HIP_TRY(dev_alloc(ix->d_tally, ix->tally_host.size() * 8));
        HIP_TRY(hipMemcpy(ix->d_tally.get(), ix->tally_host.data(), ix->tally_host.size() * 8, hipMemcpyHostToDevice));
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ix->device));
    ix->cfg.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char *pl = getenv("MOVI_PAIR_LOADS")) ix->cfg.pair_loads = atoi(pl) > 0 ? 1 : (atoi(pl) < 0 ? -1 : 0);   // A/B and test hook: every handle's default for "pair_loads"
    HIP_TRY(dev_alloc(ix->d_stats, sizeof(DevStats)));
    HIP_TRY(hipMemset(ix->d_stats.get(), 0, sizeof(DevStats)));
    DevIndex &v = ix->dev;
    v.rows = ix->d_rows.get();
    v.id_blocks = ix->d_id_blocks.get();
    v.code_of = ix->d_code_of.get();
    ix->tables.publish(v);                                   // (none yet)
    v.r = d.r;
    v.end_bwt_idx = d.end_bwt_idx;
    v.n_blocks = d.n_blocks;
    v.block_size = d.block_size ? d.block_size : 1;
    v.block_shift = 0xFFFFFFFFu;
    if ((v.block_size & (v.block_size - 1)) == 0) {
        v.block_shift = 0;
        while ((1ull << v.block_shift) < v.block_size) v.block_shift++;
    }
    v.sigma = d.alphabet_size;
    v.sep = sep ? 1u : 0u;
    v.n_sep = (uint32_t)ix->sep_rows_host.size();
    v.sep_rows = ix->d_sep_rows.get();
    v.sep_vals = reinterpret_cast<const uint2 *>(ix->d_sep_vals.get());
    v.tally = ix->d_tally.get();
    v.tally_len = d.n_tally;
    v.tally_cp = d.tally_checkpoints ? d.tally_checkpoints : 1;
    v.idx32 = d.r < 0xFFFFFFFFull ? 1u : 0u;
    for (int i = 0; i < 4; i++) v.end_thr[i] = d.end_bwt_idx_thresholds[i];
    for (int i = 0; i < 6; i++) {
        v.first_runs[i] = d.first_runs[i];
        v.first_offsets[i] = d.first_offsets[i];
        v.last_runs[i] = d.last_runs[i];
        v.last_offsets[i] = d.last_offsets[i];
    }
    // ---- resident row layout: ONE for every index type.  Blocked- and sampled-* tables are expanded to regular-thresholds
    // rows once, on the GPU, by the reference's get_id (needs the complete device view above: get_id reads first_runs /
    // id_blocks / tally).  Blocked: aligned 8-byte rows with the id inside instead of 2-byte-aligned 6-byte rows + a
    // check-point lookup per LF (count +7-10 %, ZML +28 %, PML +2-4 %, measured); sampled: see expand_sampled_kernel.
    // (the threshold-less `regular` / `blocked` types keep 12-bit lengths: their resident layout is the `regular` one, kmode 3)
    ix->kmode = (int)d.mode;
    if (d.mode != MOVI_MODE_REGULAR_THRESHOLDS && d.mode != MOVI_MODE_REGULAR) {
        const bool blocked = mode_blocked(d.mode);
        DevPtr<uint8_t> rows6;
        HIP_TRY(dev_alloc(rows6, (size_t)d.r * 8 + 16));
        hipError_t e = hipMemset(rows6.get(), 0, (size_t)d.r * 8 + 16);
        if (e == hipSuccess) e = blocked ? expand_blocked_rows((int)d.mode, v, rows6.get(), nullptr) : expand_sampled_rows((int)d.mode, v, rows6.get(), nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return fail_hip(e, "expanding the rows to the resident layout");
        ix->d_rows = std::move(rows6);                                    // the file-format copy goes (an adopted buffer stays the caller's)
        ix->d_tally.reset();                                              // sampled: only get_id needed the checkpoints
        v.rows = ix->d_rows.get();
        v.tally = nullptr;
        ix->kmode = d.mode == MOVI_MODE_BLOCKED ? MOVI_MODE_REGULAR : MOVI_MODE_REGULAR_THRESHOLDS;
    }
    return MOVI_OK;
}

static int check_desc(const movi_index_desc_t *desc) {
    if (!desc) return fail(MOVI_ERR_ARG, "desc is NULL");
    if (!mode_supported(desc->mode)) return fail(MOVI_ERR_ARG, "unsupported mode");
    if (mode_sampled(desc->mode) &&
        (!desc->tally_ids || desc->tally_checkpoints == 0 || desc->n_tally < desc->r / desc->tally_checkpoints + 2))
        return fail(MOVI_ERR_ARG, "mode 7 needs tally_checkpoints / tally_ids covering the rows");
    if (desc->r == 0 || desc->end_bwt_idx >= desc->r) return fail(MOVI_ERR_ARG, "bad r / end_bwt_idx");
    if (desc->r >= (1ull << 36)) return fail(MOVI_ERR_ARG, "2^36 rows or more: ids are 36 bits in every row layout");
    if (mode_blocked(desc->mode) &&
        (desc->block_size == 0 || desc->n_blocks == 0 || (desc->r - 1) / desc->block_size >= desc->n_blocks ||
         desc->n_blocks > (1ull << 36)))
        return fail(MOVI_ERR_ARG, "id blocks do not cover the table");
    if (desc->alphabet_size == 0 || desc->alphabet_size > 5) return fail(MOVI_ERR_ARG, "alphabet_size must be 1..5");
    if (desc->alphabet_size == 5) {
        if (desc->alphabet[0] != '%') return fail(MOVI_ERR_ARG, "a 5-symbol alphabet must be '%' + ACGT (separators)");
        if ((desc->n_separator_thresholds && !desc->separator_thresholds) || (desc->n_separator_map && !desc->separator_map))
            return fail(MOVI_ERR_ARG, "separator tables missing");
        if (desc->n_separator_map > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "too many separator rows");
    }
    return MOVI_OK;
}

static movi_index *new_handle(int device, const movi_index_desc_t *desc) {
    movi_index *ix = new movi_index();
    ix->device = device;
    ix->desc = *desc;
    if (mode_blocked(desc->mode) && desc->id_blocks)
        ix->id_blocks_host.assign(desc->id_blocks, desc->id_blocks + (size_t)desc->n_blocks * desc->alphabet_size);
    ix->desc.id_blocks = nullptr;
    if (desc->alphabet_size == 5) {
        // separators_thresholds[separators_thresholds_map[row]] flattened into two arrays sorted by row
        const size_t nt = (size_t)desc->n_separator_thresholds, nm = (size_t)desc->n_separator_map;
        ix->sep_thr_raw.resize(nt * 4);
        if (nt) memcpy(ix->sep_thr_raw.data(), desc->separator_thresholds, nt * 8);
        ix->sep_map_raw.resize(nm * 2);
        if (nm) memcpy(ix->sep_map_raw.data(), desc->separator_map, nm * 16);
        std::vector<std::pair<uint64_t, uint64_t>> kv(nm);
        for (size_t e = 0; e < nm; e++) kv[e] = {ix->sep_map_raw[2 * e], ix->sep_map_raw[2 * e + 1]};
        std::sort(kv.begin(), kv.end());
        for (const auto &e : kv) {
            uint64_t packed = 0;                          // a key pointing past the table reads as zeros
            if (e.second < nt) memcpy(&packed, ix->sep_thr_raw.data() + e.second * 4, 8);
            ix->sep_rows_host.push_back(e.first);
            ix->sep_vals_host.push_back(packed);
        }
    }
    ix->desc.separator_thresholds = nullptr;
    ix->desc.separator_map = nullptr;
    if (mode_sampled(desc->mode)) {
        const size_t ne = (size_t)desc->n_tally * desc->alphabet_size;
        const uint8_t *p = static_cast<const uint8_t *>(desc->tally_ids);
        ix->tally_host.resize(ne);
        for (size_t e = 0; e < ne; e++) {                 // MoveTally::get, include/move_row.hpp:28-38
            uint32_t right;
            memcpy(&right, p + e * 5, 4);
            ix->tally_host[e] = (uint64_t)right | ((uint64_t)p[e * 5 + 4] << 32);
        }
    }
    ix->desc.tally_ids = nullptr;
    ix->rows_bytes = (size_t)desc->r * mode_row_bytes(desc->mode);
    // MOVI_PML_VIA_MASK = 0 / 1: the handle's initial "pml_via_mask" (the test suite re-runs its PML parity files with 1: every PML
    // vector then comes from reset masks, expanded on the device or by the host's worker threads)
    if (const char *e = getenv("MOVI_PML_VIA_MASK")) {
        if (e[0] == '0' || e[0] == '1') { ix->pml_via_mask = e[0] - '0'; ix->host_masks = e[0] - '0'; }
    }
    return ix;
}

// Mode 7: the resident table is the file's 3-byte rows widened to one aligned dword each (kernels: load_row<7>);
// `packed` is a device buffer with the file bytes.  The handle owns the widened copy.
static hipError_t adopt_widened(movi_index *ix, const uint8_t *d_packed) {
    DevPtr<uint32_t> wide;
    hipError_t e = dev_alloc(wide, (size_t)ix->desc.r * 4 + 16);
    if (e != hipSuccess) return e;
    e = hipMemset(wide.get(), 0, (size_t)ix->desc.r * 4 + 16);
    if (e == hipSuccess) e = widen_rows(d_packed, ix->desc.r, wide.get(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    ix->d_rows = DevPtr<uint8_t>(reinterpret_cast<uint8_t *>(wide.release()));
    return hipSuccess;
}

// Rows that sit in a fresh file mapping (movi_index_load): every page the copy reads is a minor fault away, and a
// pageable hipMemcpy takes those faults one by one on the calling thread.  So the rows go up in 64 MiB pieces while a
// few helper threads touch the pages of the next piece.
static hipError_t upload_from_mapping(uint8_t *d_rows, const uint8_t *h_rows, size_t bytes) {
    constexpr size_t kPiece = 64ull << 20;
    constexpr unsigned kTouchers = 4;
    auto touch = [&](size_t a, size_t b) {
        std::vector<std::thread> th;
        const size_t span = (b - a + kTouchers - 1) / kTouchers;
        for (unsigned t = 0; t < kTouchers; t++) {
            const size_t lo = a + t * span, hi = std::min(b, lo + span);
            if (lo >= hi) break;
            th.emplace_back([=]() {
                volatile uint8_t sink = 0;
                for (size_t o = lo; o < hi; o += 4096) sink = sink + h_rows[o];
                (void)sink;
            });
        }
        for (auto &x : th) x.join();
    };
    touch(0, std::min(bytes, kPiece));
    for (size_t off = 0; off < bytes; off += kPiece) {
        const size_t n = std::min(kPiece, bytes - off), next = off + kPiece;
        std::thread ahead;
        if (next < bytes) ahead = std::thread([&, next]() { touch(next, std::min(bytes, next + kPiece)); });
        hipError_t e = hipMemcpy(d_rows + off, h_rows + off, n, hipMemcpyHostToDevice);
        if (ahead.joinable()) ahead.join();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// DIR/index.movi (open_index_read, src/move_structure_io.cpp:16-41: then DIR/movi_index.bin; or the file itself) mapped,
// not read: the header and side tables are parsed in place and the row table -- all but a few kB of the file -- goes
// from the page cache to the GPU without a copy into a process buffer (the reference's --mmap; an 8 GB index no longer
// passes through an 8 GB std::vector first).
struct MappedIndex {
    void *p = MAP_FAILED;
    size_t n = 0;
    int open_index(const char *path) {
        std::string cand[3] = {std::string(path) + "/index.movi", std::string(path) + "/movi_index.bin", std::string(path)};
        int fd = -1;
        struct stat sb{};
        for (auto &c : cand) {
            fd = open(c.c_str(), O_RDONLY | O_CLOEXEC);
            if (fd < 0) continue;
            // size and type of the file that was OPENED (a stat() of the path before the open could describe another file)
            if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) break;
            close(fd);
            fd = -1;
        }
        if (fd < 0) return fail(MOVI_ERR_IO, std::string("Failed to open the index file at: ") + path);
        n = (size_t)sb.st_size;
        if (n == 0) { close(fd); return fail(MOVI_ERR_IO, std::string("Failed to read the index file at: ") + path); }
        p = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (p == MAP_FAILED) return fail(MOVI_ERR_IO, std::string("Failed to read the index file at: ") + path);
        (void)madvise(p, n, MADV_WILLNEED);
        return MOVI_OK;
    }
    ~MappedIndex() {
        if (p != MAP_FAILED) { const std::string keep = g_err; munmap(p, n); g_err = keep; }
    }
};

static int index_create(int device, const movi_index_desc_t *desc, const void *h_rows, movi_index_t **out, bool from_mapping) {
    if (!out || !h_rows) return fail(MOVI_ERR_ARG, "NULL argument");
    *out = nullptr;
    int rc = check_desc(desc);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    movi_index *ix = new_handle(device, desc);
    hipError_t e = dev_alloc(ix->d_rows, ix->rows_bytes + 16);
    if (e == hipSuccess)
        e = from_mapping ? upload_from_mapping(ix->d_rows.get(), static_cast<const uint8_t *>(h_rows), ix->rows_bytes)
                         : hipMemcpy(ix->d_rows.get(), h_rows, ix->rows_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { movi_index_destroy(ix); return fail_hip(e, "uploading the move rows"); }
    if (mode_sampled(desc->mode)) {
        const DevPtr<uint8_t> packed = std::move(ix->d_rows);
        e = adopt_widened(ix, packed.get());
        if (e != hipSuccess) { movi_index_destroy(ix); return fail_hip(e, "widening the 3-byte rows"); }
    }
    rc = finish_create(ix);
    if (rc) { std::string keep = g_err; movi_index_destroy(ix); g_err = keep; return rc; }
    *out = ix;
    return MOVI_OK;
}

int movi_index_create(int device, const movi_index_desc_t *desc, const void *h_rows, movi_index_t **out) {
    return index_create(device, desc, h_rows, out, false);
}

int movi_index_create_from_device_rows(int device, const movi_index_desc_t *desc, const void *d_rows,
                                       movi_index_t **out) {
    if (!out || !d_rows) return fail(MOVI_ERR_ARG, "NULL argument");
    *out = nullptr;
    int rc = check_desc(desc);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(d_rows) & 7u) != 0) return fail(MOVI_ERR_ARG, "d_rows must be 8-byte aligned");
    HIP_TRY(hipSetDevice(device));
    movi_index *ix = new_handle(device, desc);
    ix->d_rows = borrowed<uint8_t, DeviceMem>(const_cast<uint8_t *>(static_cast<const uint8_t *>(d_rows)));
    if (mode_sampled(desc->mode)) {   // private copy; the caller's buffer is not kept
        hipError_t e = adopt_widened(ix, static_cast<const uint8_t *>(d_rows));
        if (e != hipSuccess) { movi_index_destroy(ix); return fail_hip(e, "widening the 3-byte rows"); }
    }
    rc = finish_create(ix);
    if (rc) { std::string keep = g_err; movi_index_destroy(ix); g_err = keep; return rc; }
    *out = ix;
    return MOVI_OK;
}

int movi_index_load(int device, const char *path, movi_index_t **out) {
    if (!path || !out) return fail(MOVI_ERR_ARG, "NULL argument");
    *out = nullptr;
    MappedIndex m;
    int rc = m.open_index(path);
    if (rc) return rc;
    movi_index_desc_t desc;
    size_t roff = 0, rbytes = 0;
    rc = movi_index_parse(m.p, m.n, &desc, &roff, &rbytes);
    if (rc == MOVI_OK) rc = index_create(device, &desc, static_cast<const uint8_t *>(m.p) + roff, out, true);
    return rc;
}

}  // extern "C"

// ---------------------------------------------------------------- one index on several GPUs: RCCL broadcast
namespace {

// librccl.so.1 is 570 MB of code objects for every collective, datatype and topology; a process that serves one GPU
// (every path but this one) never needs it, and mapping it costs more than a small query.  So it is bound here, when
// the first replicated index is made -- by name, with the image's own header for the types.  No RCCL, no replica.
struct Rccl {
    void *so = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string err;
    bool load() {
        if (so) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (so) break;
        }
        if (!so) { const char *m = dlerror(); err = std::string("librccl.so.1 could not be loaded: ") + (m ? m : "?"); return false; }
        auto sym = [&](const char *n) -> void * {
            void *p = dlsym(so, n);
            if (!p && err.empty()) err = std::string("librccl.so.1 lacks ") + n;
            return p;
        };
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
        Broadcast = reinterpret_cast<decltype(Broadcast)>(sym("ncclBroadcast"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        if (!err.empty()) { dlclose(so); so = nullptr; return false; }
        return true;
    }
};
Rccl g_rccl;

int replicate(const movi_index_desc_t *desc, const void *h_rows, const int *devices, int n, movi_index_t **out,
              bool from_mapping) {
    if (!out || !h_rows || !devices) return fail(MOVI_ERR_ARG, "NULL argument");
    if (n < 1 || n > 64) return fail(MOVI_ERR_ARG, "the number of devices must be in [1, 64]");
    for (int i = 0; i < n; i++) out[i] = nullptr;
    int rc = check_desc(desc);
    if (rc) return rc;
    int visible = 0;
    HIP_TRY(hipGetDeviceCount(&visible));
    for (int i = 0; i < n; i++) {
        if (devices[i] < 0 || devices[i] >= visible)
            return fail(MOVI_ERR_NO_DEVICE, "device " + std::to_string(devices[i]) + " requested but only " + std::to_string(visible) + " visible");
        for (int j = 0; j < i; j++)
            if (devices[j] == devices[i]) return fail(MOVI_ERR_ARG, "the devices of a replicated index must be distinct");
    }
    // One GPU: nothing crosses xGMI, so a missing librccl is no reason to fail (`movi query --gpus 1`); when the library is
    // there the one-rank communicator still runs -- the same calls as N ranks, which is how 1-GPU boxes test this path.
    const bool have_rccl = g_rccl.load();
    if (!have_rccl && n > 1) return fail(MOVI_ERR_HIP, g_rccl.err);
    const size_t rows_bytes = (size_t)desc->r * mode_row_bytes(desc->mode);
    std::vector<DevPtr<uint8_t>> d_rows((size_t)n);
    std::vector<hipStream_t> streams((size_t)n, nullptr);
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    bool comms_up = false;
    auto cleanup = [&](bool keep_rows) {
        const std::string keep = g_err;
        for (int i = 0; i < n; i++) {
            (void)hipSetDevice(devices[i]);
            if (streams[i]) (void)hipStreamDestroy(streams[i]);
            if (comms_up && comms[i]) (void)g_rccl.CommDestroy(comms[i]);
            if (!keep_rows) d_rows[i].reset();
        }
        g_err = keep;
    };
    auto hip_fail = [&](hipError_t e, const char *what) { const int c = fail_hip(e, what); cleanup(false); return c; };
    auto nccl_fail = [&](ncclResult_t r, const char *what) {
        const int c = fail(MOVI_ERR_HIP, std::string(what) + ": " + g_rccl.GetErrorString(r));
        cleanup(false);
        return c;
    };
    // the table's only trip over PCIe: host (or file mapping) -> devices[0]
    for (int i = 0; i < n; i++) {
        hipError_t e = hipSetDevice(devices[i]);
        if (e == hipSuccess) e = dev_alloc(d_rows[i], rows_bytes + 16);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking);
        if (e != hipSuccess) return hip_fail(e, "allocating the move rows");
    }
    {
        hipError_t e = hipSetDevice(devices[0]);
        if (e == hipSuccess)
            e = from_mapping ? upload_from_mapping(d_rows[0].get(), static_cast<const uint8_t *>(h_rows), rows_bytes)
                             : hipMemcpy(d_rows[0].get(), h_rows, rows_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "uploading the move rows");
    }
    // ... and from there to every other GPU: one broadcast over xGMI, all ranks driven by this process.
    // (librccl prints a version banner with printf when the first communicator comes up; the caller's stdout may be the
    // query's output -- `movi query --stdout` -- so stdout points at stderr while RCCL initialises)
    struct StdoutToStderr {
        int saved = -1;
        StdoutToStderr() { fflush(stdout); saved = dup(1); if (saved >= 0) dup2(2, 1); }
        ~StdoutToStderr() { fflush(stdout); if (saved >= 0) { dup2(saved, 1); close(saved); } }
    };
    if (have_rccl) {
        ncclResult_t r;
        {
            StdoutToStderr quiet;
            r = g_rccl.CommInitAll(comms.data(), n, devices);
        }
        if (r != ncclSuccess) return nccl_fail(r, "ncclCommInitAll");
        comms_up = true;
        r = g_rccl.GroupStart();
        if (r != ncclSuccess) return nccl_fail(r, "ncclGroupStart");
        for (int i = 0; i < n && r == ncclSuccess; i++) {
            (void)hipSetDevice(devices[i]);
            r = g_rccl.Broadcast(d_rows[i].get(), d_rows[i].get(), rows_bytes, ncclUint8, 0, comms[i], streams[i]);
        }
        const ncclResult_t rg = g_rccl.GroupEnd();
        if (r != ncclSuccess) return nccl_fail(r, "ncclBroadcast");
        if (rg != ncclSuccess) return nccl_fail(rg, "ncclGroupEnd");
    }
    for (int i = 0; i < n; i++) {
        hipError_t e = hipSetDevice(devices[i]);
        if (e == hipSuccess) e = hipStreamSynchronize(streams[i]);
        if (e != hipSuccess) return hip_fail(e, "the RCCL broadcast of the move rows");
    }
    // every GPU builds its own resident layout from the file-format rows it now holds
    for (int i = 0; i < n; i++) {
        hipError_t e = hipSetDevice(devices[i]);
        if (e != hipSuccess) { for (int j = 0; j < i; j++) { movi_index_destroy(out[j]); out[j] = nullptr; } return hip_fail(e, "hipSetDevice"); }
        movi_index *ix = new_handle(devices[i], desc);
        ix->d_rows = std::move(d_rows[i]);                     // the handle's from here on
        int rci = MOVI_OK;
        if (mode_sampled(desc->mode)) {
            const DevPtr<uint8_t> packed = std::move(ix->d_rows);
            e = adopt_widened(ix, packed.get());
            if (e != hipSuccess) rci = fail_hip(e, "widening the 3-byte rows");
        }
        if (rci == MOVI_OK) rci = finish_create(ix);
        if (rci != MOVI_OK) {
            const std::string keep = g_err;
            movi_index_destroy(ix);
            for (int j = 0; j < i; j++) { movi_index_destroy(out[j]); out[j] = nullptr; }
            g_err = keep;
            cleanup(false);
            return rci;
        }
        out[i] = ix;
    }
    cleanup(true);
    return MOVI_OK;
}

}  // namespace

extern "C" {

int movi_index_replicate(const movi_index_desc_t *desc, const void *h_rows, const int *devices, int n, movi_index_t **out) {
    return replicate(desc, h_rows, devices, n, out, false);
}

int movi_index_load_replicated(const char *path, const int *devices, int n, movi_index_t **out) {
    if (!path || !out || !devices) return fail(MOVI_ERR_ARG, "NULL argument");
    for (int i = 0; i < n; i++) out[i] = nullptr;
    MappedIndex m;
    int rc = m.open_index(path);
    if (rc) return rc;
    movi_index_desc_t desc;
    size_t roff = 0, rbytes = 0;
    rc = movi_index_parse(m.p, m.n, &desc, &roff, &rbytes);
    if (rc == MOVI_OK) rc = replicate(&desc, static_cast<const uint8_t *>(m.p) + roff, devices, n, out, true);
    return rc;
}

int movi_index_destroy(movi_index_t *ix) {
    if (!ix) return MOVI_OK;
    (void)hipSetDevice(ix->device);
    release_scratch(ix);
    delete ix;
    return MOVI_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ derived tables
// Which tables exist when is decided in movi_derived.hpp; here is what its rules are handed: the facts of the handle, and the device.

// A builder's tally: kTallySlots pairs of counters on the device (movi_kernels.hip: tally_add), added up here.
constexpr size_t kTallyBytes = 2u * kTallySlots * sizeof(unsigned long long);
static hipError_t read_tally(const unsigned long long *d_tally, unsigned long long (&sum)[2], hipStream_t s) {
    std::vector<unsigned long long> h(2u * kTallySlots);
    hipError_t e = hipMemcpyAsync(h.data(), d_tally, kTallyBytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    sum[0] = sum[1] = 0;
    if (e == hipSuccess) for (uint32_t i = 0; i < kTallySlots; ++i) { sum[0] += h[2 * i]; sum[1] += h[2 * i + 1]; }
    return e;
}

static DerivedFacts derived_facts(const movi_index *ix) {
    DerivedFacts f;
    f.kmode = ix->kmode;
    f.r = ix->desc.r;
    f.dna = ix->dev.sigma - ix->dev.sep == 4;
    f.count_variant = ix->cfg.count_variant;
    f.ahead_bytes = ahead_rows_bytes(ix->desc.r);
    f.deep_bytes = deep_rows_bytes(ix->desc.r);
    f.chain_bytes = chain_rows_bytes(ix->desc.r);
    for (int t = 0; t < kDerivedTables; t++) f.held[t] = ix->tables.held((DerivedTable)t);
    return f;
}

// The device interface of movi_derived.hpp's rules on stream `s`: each builder allocates, launches, waits -- chunks of the overlapped host
// path walk on other streams --, moves the table into the holder and publishes it; `facts.held` follows every build and drop.  A build
// that fails leaves its message and code behind (rc) and the thread's last error cleared: the rules decide whether the caller hears of it.
struct DerivedDev {
    movi_index *ix;
    hipStream_t s;
    DerivedFacts &facts;
    int rc = MOVI_OK;
    bool failed(hipError_t e, const char *what) {
        rc = fail_hip(e, what);
        (void)hipGetLastError();
        return false;
    }
    bool published() {
        ix->tables.publish(ix->dev);
        for (int t = 0; t < kDerivedTables; t++) facts.held[t] = ix->tables.held((DerivedTable)t);
        return true;
    }
    bool mem_info(uint64_t &free_b, uint64_t &total_b) {
        size_t f = 0, t = 0;
        if (hipMemGetInfo(&f, &t) != hipSuccess) { (void)hipGetLastError(); return false; }
        free_b = f; total_b = t;
        return true;
    }
    // The statistic over a sample of the table's rows (every 16th), before anything is built.
    bool sample_no_ff(double &share) {
        DevPtr<unsigned long long> tally;
        unsigned long long h_tally[2] = {0, 0};
        hipError_t e = dev_alloc(tally, kTallyBytes);
        if (e == hipSuccess) e = hipMemsetAsync(tally.get(), 0, kTallyBytes, s);
        if (e == hipSuccess) e = tally_no_ff_share(ix->kmode, ix->dev, 16, tally.get(), s);
        if (e == hipSuccess) e = read_tally(tally.get(), h_tally, s);
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }
        share = h_tally[1] ? (double)h_tally[0] / (double)h_tally[1] : 0.0;
        return true;
    }
    bool build_kmer(uint32_t K) {
        DevPtr<uint4> table;
        hipError_t e = dev_alloc(table, DerivedTables::bytes(kTabKmer, ix->desc.r, K));
        if (e == hipSuccess) e = build_kmer_table(ix->dev, K, table.get(), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return failed(e, "building the top-of-walk table");
        ix->tables.kmer = std::move(table);
        ix->tables.kmer_k = K;
        return published();
    }
    bool build_ftab(uint32_t K) {
        DevPtr<uint4> table;
        hipError_t e = dev_alloc(table, DerivedTables::bytes(kTabFtab, ix->desc.r, K));
        if (e == hipSuccess) e = movi::build_ftab(ix->kmode, ix->dev, K, table.get(), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return failed(e, "building the count query's interval table");
        ix->tables.ftab = std::move(table);
        ix->tables.ftab_k = K;
        return published();
    }
    bool build_ckpt() {
        DevPtr<uint64_t> ckpt;
        hipError_t e = dev_alloc(ckpt, DerivedTables::bytes(kTabCkpt, ix->desc.r, 0));
        if (e == hipSuccess) e = build_row_start_ckpt(ix->kmode, ix->d_rows.get(), ix->desc.r, ckpt.get(), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);        // other streams (the overlapped host path) may use it next
        if (e != hipSuccess) return failed(e, "building the row-start checkpoints");
        ix->tables.ckpt = std::move(ckpt);
        return published();
    }
    // hint_bits: 2 or 4, as deep_map_for gives it for this table (deep_hint_width)
    bool build_deep(int hint_bits) {
        DevPtr<uint8_t> rows3;
        hipError_t e = dev_alloc(rows3, DerivedTables::bytes(kTabDeep, ix->desc.r, 0));
        if (e == hipSuccess) e = build_deep_rows(ix->kmode, ix->dev, hint_bits, rows3.get(), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return failed(e, "building the deep rows");
        ix->tables.rows3 = std::move(rows3);
        ix->tables.deep = deep_map_for(ix->desc.r, hint_bits);
        return published();
    }
    bool build_chain() {
        DevPtr<uint8_t> rows4;
        hipError_t e = dev_alloc(rows4, DerivedTables::bytes(kTabChain, ix->desc.r, 0));
        if (e == hipSuccess) e = build_chain_rows(ix->kmode, ix->dev, rows4.get(), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return failed(e, "building the chain rows");
        ix->tables.rows4 = std::move(rows4);
        return published();
    }
    // share: the builder's tally over every row; serves_count: what the copy publishes as DevIndex::rows2_count
    bool build_ahead(bool by_itself, double &share, bool &serves_count) {
        DevPtr<uint8_t> rows2;
        hipError_t e = dev_alloc(rows2, DerivedTables::bytes(kTabAhead, ix->desc.r, 0));
        uint64_t tail = 0;
        DevPtr<unsigned long long> tally;
        unsigned long long h_tally[2] = {0, 0};
        if (e == hipSuccess) e = dev_alloc(tally, kTallyBytes);
        if (e == hipSuccess) e = hipMemsetAsync(tally.get(), 0, kTallyBytes, s);
        if (e == hipSuccess) e = build_ahead_rows(ix->kmode, ix->dev, rows2.get(), &tail, s, tally.get());
        if (e == hipSuccess) e = read_tally(tally.get(), h_tally, s);
        if (e != hipSuccess) return failed(e, "building the look-ahead rows");
        share = h_tally[1] ? (double)h_tally[0] / (double)h_tally[1] : 0.0;
        serves_count = ahead_serves_count(by_itself, share);
        ix->tables.rows2 = std::move(rows2);
        ix->tables.rows2_tail = tail;
        ix->tables.hints = ahead_rows_hinted(ix->desc.r) ? 1u : 0u;   // (the copy's ids are 32 bits wide and its spare bits hold reposition hints)
        ix->tables.rows2_count = serves_count ? 1u : 0u;
        return published();
    }
    void drop(DerivedTable which) {
        ix->tables.reset(which);
        published();
    }
};

static void pml_tables(movi_index *ix, hipStream_t s, bool from_prepare = false) {
    DerivedFacts f = derived_facts(ix);
    DerivedDev dev{ix, s, f};
    ensure_pml_tables(ix->policy, f, dev, from_prepare);
    ensure_chain_rows(ix->policy, f, dev, from_prepare);     // (beside the deep rows, from the tally the rules above have taken)
}
static int count_tables(movi_index *ix, hipStream_t s, bool from_prepare = false) {
    DerivedFacts f = derived_facts(ix);
    DerivedDev dev{ix, s, f};
    return ensure_count_tables(ix->policy, f, dev, from_prepare) ? MOVI_OK : dev.rc;
}
// The four build-now options behind their range checks; `refusal`: what an ineligible index is told
static int request_derived(movi_index *ix, DerivedTable which, int64_t value, const char *refusal) {
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());                         // no walk may be reading the table that goes away
    DerivedFacts f = derived_facts(ix);
    DerivedDev dev{ix, nullptr, f};
    switch (request_table(ix->policy, f, dev, which, (uint32_t)value)) {
    case TableRequest::kIneligible: return fail(MOVI_ERR_ARG, refusal);
    case TableRequest::kBuildFailed: return dev.rc;
    default: return MOVI_OK;
    }
}

extern "C" {

int movi_index_get_desc(const movi_index_t *ix, movi_index_desc_t *desc) {
    if (!ix || !desc) return fail(MOVI_ERR_ARG, "NULL argument");
    *desc = ix->desc;
    desc->id_blocks = nullptr;
    desc->separator_thresholds = nullptr;
    desc->separator_map = nullptr;
    desc->tally_ids = nullptr;
    return MOVI_OK;
}

int movi_index_device_rows(const movi_index_t *ix, const void **d_rows, size_t *bytes) {
    if (!ix || !d_rows || !bytes) return fail(MOVI_ERR_ARG, "NULL argument");
    *d_rows = ix->d_rows.get();
    // blocked- / sampled-thresholds: the resident table is the EXPANDED one (r rows of the 8-byte regular-thresholds layout)
    *bytes = ix->kmode != (int)ix->desc.mode ? (size_t)ix->desc.r * 8 : ix->rows_bytes;
    return MOVI_OK;
}

int movi_set_option(movi_index_t *ix, const char *key, int64_t value) {
    if (!ix || !key) return fail(MOVI_ERR_ARG, "NULL argument");
    if (!strcmp(key, "pml_variant")) {
        if (value != -1 && value != 0 && value != 1 && value != 14)
            return fail(MOVI_ERR_ARG, "pml_variant must be -1 (auto), 0, 1 or 14");
        ix->cfg.pml_variant = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "zml_variant")) {
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "zml_variant must be -1 (auto), 0 or 1");
        ix->cfg.zml_variant = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "count_variant")) {                     // A/B: -1 = the launch policy, 0 = count_kernel_v0, 1 = the lane state machine
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "count_variant must be -1 (auto), 0 or 1");
        ix->cfg.count_variant = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "color_chunk_keys")) {                  // the colour builder: BWT positions per chunk (0 = by the device's free memory; small: a test hook)
        if (value < 0) return fail(MOVI_ERR_ARG, "color_chunk_keys must be >= 0");
        ix->color_chunk_keys = (uint64_t)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "color_scratch_bytes")) {               // movi_multi_classify_device's counter scratch: reads go through it in chunks
        if (value < 4) return fail(MOVI_ERR_ARG, "color_scratch_bytes must be at least 4");
        ix->color_scratch_bytes = (uint64_t)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "idx64")) {                             // test hook: run the 64-bit-index kernel instantiations
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "idx64 must be 0 or 1");
        ix->dev.idx32 = (value == 0 && ix->desc.r < 0xFFFFFFFFull) ? 1u : 0u;
        return MOVI_OK;
    }
    if (!strcmp(key, "block_threads")) {
        // every query kernel is compiled with __launch_bounds__(256)
        if (value != 0 && value != 64 && value != 128 && value != 192 && value != 256)
            return fail(MOVI_ERR_ARG, "block_threads must be 0 (auto), 64, 128, 192 or 256");
        ix->cfg.block_threads = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "classify_fused")) {                    // -1 auto, 1: vector + bins in one kernel, 0: walk, then a streaming pass over the vectors
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "classify_fused must be -1, 0 or 1");
        ix->cfg.classify_fused = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "pair_loads")) {                        // the lanes of a pair fetch their row windows together (A/B)
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "pair_loads must be -1 (auto), 0 or 1");
        ix->cfg.pair_loads = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "zml_ahead")) {                         // 1: the ZML state machine walks on the look-ahead rows where they exist (A/B: measured no faster)
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "zml_ahead must be 0 or 1");
        ix->cfg.zml_ahead = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "out_ring")) {                          // A/B: the PML kernels' output ring in LDS (-1 = the launch policy)
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "out_ring must be -1, 0 or 1");
        ix->cfg.out_ring = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "repo_hints")) {                        // A/B: mismatches whose scan leaves the row window jump by the look-ahead rows' reposition hints
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "repo_hints must be 0 or 1");
        ix->cfg.hints = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "inwin_repo")) {                        // A/B: repositions inside the row window resolved in the same iteration
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "inwin_repo must be 0 or 1");
        ix->cfg.inwin = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "release_scratch")) {                   // give back the device staging the *_host entry points keep
        (void)hipSetDevice(ix->device);
        release_scratch(ix);
        return MOVI_OK;
    }
    // device staging of the synchronous *_host calls reserved up front (it is grow-only and otherwise grows inside the first big call:
    // three hipMallocs, ~1.2 ms of a 3 ms call of 2^25 bases): the reads of a call of up to `value` bases / its u16 result vector /
    // the per-read buffers of up to `value` reads
    if (!strcmp(key, "reserve_host_bases") || !strcmp(key, "reserve_host_results") || !strcmp(key, "reserve_host_reads")) {
        if (value < 0 || (uint64_t)value > (1ull << 40)) return fail(MOVI_ERR_ARG, std::string(key) + " out of range");
        HIP_TRY(hipSetDevice(ix->device));
        const size_t v = (size_t)value;
        if (!strcmp(key, "reserve_host_bases")) {
            HIP_TRY(grow(ix->scratch[movi_index::kBases], v));
        } else if (!strcmp(key, "reserve_host_results")) {
            HIP_TRY(grow(ix->scratch[movi_index::kOut], v * 2));
            // (round 6: a PML vector is written through reset masks on the device -- their words, for as many reads as "reserve_host_reads" says)
            ix->reserved_result_bases = std::max<uint64_t>(ix->reserved_result_bases, v);
            HIP_TRY(grow(ix->scratch[movi_index::kMask], (size_t)pml_mask_words(ix->reserved_reads, ix->reserved_result_bases, 31u) * 4));
        } else {                                             // "reserve_host_reads"
            ix->reserved_reads = std::max<uint64_t>(ix->reserved_reads, v);
            if (ix->reserved_result_bases)
                HIP_TRY(grow(ix->scratch[movi_index::kMask], (size_t)pml_mask_words(ix->reserved_reads, ix->reserved_result_bases, 31u) * 4));
            HIP_TRY(grow(ix->scratch[movi_index::kOffs], (v + 1) * 8));
            HIP_TRY(grow(ix->scratch[movi_index::kErr], v));
            HIP_TRY(ix->h_rel.reserve((v + 1) * 8, (v + 1) * 8));   // (a reservation: exactly what was asked for)
        }
        return MOVI_OK;
    }
    if (!strcmp(key, "locate_matches_stages")) {             // measurement hook (tools/locate_matches_bench.py): the call's steps timed apart
        if (value < 1 || value > 3) return fail(MOVI_ERR_ARG, "locate_matches_stages must be 1 (search + scan), 2 (+ expansion) or 3 (the whole call)");
        ix->locate_matches_stages = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "pipe_chunk_bases")) {                  // test hook: many small chunks through the overlapped host path
        if (value < 0) return fail(MOVI_ERR_ARG, "pipe_chunk_bases must be >= 0");
        ix->pipe_chunk_bases = (uint64_t)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "seg_len")) {                           // segment-parallel long reads (PML): 0 = off
        if (value != 0 && (value < 32 || value > (1 << 24) || (value & 31) != 0))
            return fail(MOVI_ERR_ARG, "seg_len must be 0 (off) or a multiple of 32 in [32, 2^24]");
        ix->cfg.seg_len = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "seg_probe")) {                         // 0: segment eligible batches whatever the probe would say (tests)
        if (value < 0 || value > 2) return fail(MOVI_ERR_ARG, "seg_probe must be 0, 1 or 2");
        ix->cfg.seg_probe = (int)value;                      // 2: the caller's "seg_verdict" decides, nothing is read back
        return MOVI_OK;
    }
    if (!strcmp(key, "seg_verdict")) {
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "seg_verdict must be 0 or 1");
        ix->cfg.seg_verdict = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "pml_via_mask")) {                      // the walk's u16 vector through reset masks its wavefronts expand themselves (-1: the policy)
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "pml_via_mask must be -1, 0 or 1");
        ix->pml_via_mask = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "host_masks")) {                        // movi_pml_host: masks down + expansion on host worker threads (-1: the policy)
        if (value < -1 || value > 2) return fail(MOVI_ERR_ARG, "host_masks must be -1, 0, 1 or 2");
        ix->host_masks = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "host_mask_share")) {                   // mixed calls of movi_pml_host: percent of the bases that take the mask route
        if (value < 0 || value > 100) return fail(MOVI_ERR_ARG, "host_mask_share must be 0 .. 100");
        ix->host_mask_share = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "fused_expand")) {                      // A/B: 0 = a mask walk whose caller wants the vector leaves the expansion to the pml_expand_* kernels
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "fused_expand must be 0 or 1");
        ix->cfg.fused_expand = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "park_lanes")) {                        // the mask walk's parked lanes: -1 = the policy (plan_pml), 0 = off, 1 .. 63 = a wavefront stops at that many walking lanes (A/B)
        if (value < -1 || value > 63) return fail(MOVI_ERR_ARG, "park_lanes must be -1 .. 63");
        ix->cfg.park_lanes = (int)value;
        if (ix->dmask.cap() != 0 && park_lanes_wanted(ix) > 0) {   // where the mask words are reserved, so is the queue (no room: such calls park nothing)
            HIP_TRY(hipSetDevice(ix->device));
            if (grow(ix->dpark, park_queue_bytes(kPrepareMaskReads, park_lanes_wanted(ix))) != hipSuccess) (void)hipGetLastError();
        }
        return MOVI_OK;
    }
    if (!strcmp(key, "ff_skip")) {                           // the PML walk's fast-forward skip (DevIndex::ff_skip): -1 = the policy (ff_skip_on), 0 = off, 1 = on wherever the walk has entries (A/B)
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "ff_skip must be -1, 0 or 1");
        ix->cfg.ff_skip = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "reserve_device_masks")) {            // device scratch for the mask words of movi_pml_device calls of up to `value` bases (and as many reads / 16)
        if (value < 0 || (uint64_t)value > (1ull << 40)) return fail(MOVI_ERR_ARG, "reserve_device_masks out of range");
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(grow(ix->dmask, (size_t)pml_mask_words((uint64_t)value / 16 + 1, (uint64_t)value, 0) * 4));
        return MOVI_OK;
    }
    if (!strcmp(key, "host_threads")) {                      // workers of the host-side mask expansion (0 = as many as the process may run on)
        if (value < 0 || value > 256) return fail(MOVI_ERR_ARG, "host_threads must be 0 .. 256");
        ix->host_threads = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "host_autopin")) {                      // 0: pageable buffers always take the synchronous path (A/B)
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "host_autopin must be 0 or 1");
        ix->host_autopin = value != 0;
        return MOVI_OK;
    }
    if (!strcmp(key, "host_overlap")) {                      // 0: the *_host calls never cut themselves into overlapped pieces (a caller
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "host_overlap must be 0 or 1");   // that pipelines chunk-sized calls itself)
        ix->host_overlap = value != 0;
        return MOVI_OK;
    }
    if (!strcmp(key, "stage_reads")) {                       // A/B: reads of short-read wavefronts staged through LDS
        if (value != 0 && value != 1) return fail(MOVI_ERR_ARG, "stage_reads must be 0 or 1");
        ix->cfg.stage_reads = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "kmer_k")) {                            // top-of-walk table: 0 = none, K in [1, 12] = build it now
        if (value < 0 || value > 12) return fail(MOVI_ERR_ARG, "kmer_k must be in [0, 12]");
        return request_derived(ix, kTabKmer, value, "the top-of-walk table serves PML walks on DNA (ACGT) *-thresholds indexes only");
    }
    if (!strcmp(key, "ahead_rows")) {                        // look-ahead rows: 0 = none (freed), 1 = build them now
        if (value < 0 || value > 1) return fail(MOVI_ERR_ARG, "ahead_rows must be 0 or 1");
        if (ix->tables.rows4 || ix->policy.chain_auto > 0) {     // a statement about what the PML walk runs on: the chain rows go like the deep rows, and come back on request only
            HIP_TRY(hipSetDevice(ix->device));
            HIP_TRY(hipDeviceSynchronize());
            DerivedFacts f = derived_facts(ix);
            DerivedDev dev{ix, nullptr, f};
            (void)request_chain(ix->policy, f, dev, 0);
        }
        return request_derived(ix, kTabAhead, value, "look-ahead rows serve PML walks on *-thresholds indexes only");   // (the deep rows go with them)
    }
    if (!strcmp(key, "deep_rows")) {                         // deep rows: 0 = none (freed), 1 = build them now
        if (value < 0 || value > 1) return fail(MOVI_ERR_ARG, "deep_rows must be 0 or 1");
        return request_derived(ix, kTabDeep, value, "deep rows serve PML walks on *-thresholds indexes of fewer than 2^28 - 1 rows only");
    }
    if (!strcmp(key, "chain_rows")) {                        // chain rows: -1 = the policy's own rule again (ensure_chain_rows), 0 = none (freed), 1 = build them now
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "chain_rows must be -1, 0 or 1");
        if (value < 0) { ix->policy.chain_auto = 1; return MOVI_OK; }
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(hipDeviceSynchronize());                     // no walk may be reading the table that goes away
        DerivedFacts f = derived_facts(ix);
        DerivedDev dev{ix, nullptr, f};
        switch (request_chain(ix->policy, f, dev, (uint32_t)value)) {
        case TableRequest::kIneligible: return fail(MOVI_ERR_ARG, "chain rows serve PML walks on *-thresholds indexes of fewer than 2^28 - 1 rows only");
        case TableRequest::kBuildFailed: return dev.rc;
        default: return MOVI_OK;
        }
    }
    if (!strcmp(key, "deep_hint_bits")) {                    // width of a deep row's reposition hints: -1 = the default, 2 (reach 3, wide ids) or 4 (reach 15, narrow ids); takes effect when the deep rows are next built (A/B)
        if (value != -1 && value != 2 && value != 4) return fail(MOVI_ERR_ARG, "deep_hint_bits must be -1, 2 or 4");
        ix->policy.deep_hint_bits = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "deep")) {                              // the walk on the deep rows the handle holds: -1 = batches of short reads, 0 never, 1 always (A/B)
        if (value < -1 || value > 1) return fail(MOVI_ERR_ARG, "deep must be -1, 0 or 1");
        ix->cfg.deep = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "ftab_k")) {                            // count query's interval table: 0 = none, K in [1, 12] = build it now
        if (value < 0 || value > 12) return fail(MOVI_ERR_ARG, "ftab_k must be in [0, 12]");
        return request_derived(ix, kTabFtab, value, "the count query's interval table serves DNA (ACGT) indexes only");
    }
    if (!strcmp(key, "kmer_lookahead")) {                    // k-mer query: -1 = by k and the text's length, 0 = no look-ahead, n in [2, 16] = split k / n
        if (value != 0 && value != -1 && (value < 2 || value > 16)) return fail(MOVI_ERR_ARG, "kmer_lookahead must be -1, 0 or in [2, 16]");
        ix->cfg.kmer_lookahead = (int)value;
        return MOVI_OK;
    }
    if (!strcmp(key, "waves_per_cu")) {
        if (value < 0 || value > 32) return fail(MOVI_ERR_ARG, "waves_per_cu must be in [0,32]");
        ix->cfg.waves_per_cu = (int)value;
        return MOVI_OK;
    }
    return fail(MOVI_ERR_ARG, std::string("unknown option: ") + key);
}

// ---------------------------------------------------------------------------- PML

// One PML or ZML call on device pointers, as every entry point hands it to pml_call / zml_call: the reads, where the results go (`out`;
// PML: null = verdict bins only, or mask.words / mask.phase = reset masks are the result) and the stream; the calls fill in the handle's
// part (mode, ix, cfg, info).  A chunk in flight of a *_host call brings its own counters, segment workspace, length hint, probe verdict and
// scratch slots; a device-pointer call leaves them null and runs on the handle's (ix->dmask, ix->scratch[kTmp], the park queue).
struct MlRequest : PmlCall {
    bool lend_masks = false;                 // PML: `out` may come through mask words in scratch, where "pml_via_mask" and the plan say so
    DevBuf *chunk = nullptr;                 // the chunk's scratch slots: kMask and kTmp are this call's
};

// What the PML and ZML calls share behind their argument checks: the device, and the call's counters cleared.  *no_alloc: `s` is being
// captured, the call must not allocate.
static int ml_begin(movi_index_t *ix, uint64_t n_reads, DevStats *d_stats, hipStream_t s, bool *no_alloc) {
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), s));
    // (under a capture the counters are cleared by a kernel as well: a memset NODE behind kernel nodes -- an unpack captured in front of
    // this call -- was seen to replay with a stale pattern; an uncaptured call makes the HIP calls it always made)
    bool active = false;
    *no_alloc = stream_capturing(s, &active);
    if (active) HIP_TRY(launch_stats_reset(d_stats, s));
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    return MOVI_OK;
}

static int zml_call(movi_index_t *ix, const MlRequest &r) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (r.n_reads == 0) return MOVI_OK;
    if (!r.offs || (r.n_bases && (!r.bases || !r.out))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    DevStats *d_stats = r.stats ? r.stats : ix->d_stats.get();
    bool no_alloc = false;
    if (int rc = ml_begin(ix, r.n_reads, d_stats, r.stream, &no_alloc)) return rc;
    HIP_TRY(launch_zml(ix->kmode, ix->dev, r.bases, r.offs, r.n_reads, r.n_bases, r.out, r.err, d_stats, r.order, ix->cfg,
                       r.stream, r.seg_ws ? r.seg_ws : &ix->seg_ws, r.ragged_hint, r.seg_verdict, &ix->last_launch));
    return MOVI_OK;
}

// Every PML call.  The derived tables first, so that the plan sees the handle's final facts; then the plan (plan_pml: the one place that
// says where the results leave the walk); then the scratch the planned route needs, and nothing else.
// The vector THROUGH RESET MASKS (lend_masks; "pml_via_mask" 1: wherever the walk can, -1, the default: batches of short reads, 0: never):
// the mask words live in scratch (device-pointer calls: ix->dmask, which movi_index_prepare reserves for kPrepareMaskBases bases and
// "reserve_device_masks" for more).  A bigger batch grows them -- but never under a stream capture: a captured call whose words do not fit
// is planned as the plain vector, which needs no scratch, and a buffer a captured call has used is retired on growth, not freed
// (GraphSafeBuf).
static int pml_call(movi_index_t *ix, const MlRequest &r) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!mode_has_thresholds(ix->desc.mode))
        return fail(MOVI_ERR_ARG, "PML needs thresholds: on a `regular`, `blocked` or `sampled` index the reference repositions "
                                  "randomly (reposition_randomly), which cannot be reproduced; use --zml or --count, or a "
                                  "*-thresholds index");
    if (r.n_reads == 0) return MOVI_OK;
    const bool bins_only = r.cls.bin_width != 0 && !r.out;
    const bool masks = r.mask.words != nullptr;
    if (masks && (r.cls.bin_width != 0 || r.cls.log_ff)) return fail(MOVI_ERR_ARG, "reset masks: plain PML queries only");
    if (!r.offs || (r.n_bases && (!r.bases || (!r.out && !bins_only && !masks)))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    PmlCall c = r;
    c.mode = ix->kmode; c.ix = &ix->dev; c.cfg = &ix->cfg; c.info = &ix->last_launch;
    if (!c.stats) c.stats = ix->d_stats.get();                   // (the pipelined host path counts per chunk in flight ...
    if (!c.seg_ws) c.seg_ws = &ix->seg_ws;                       //  ... and keeps a segment workspace per chunk in flight)
    bool no_alloc = false;
    if (int rc = ml_begin(ix, r.n_reads, c.stats, r.stream, &no_alloc)) return rc;
    // the first PML query on a handle builds its derived tables -- unless movi_index_prepare did (--logs runs on the first kernel, which
    // uses none of them)
    if (r.cls.log_ff == nullptr) pml_tables(ix, r.stream);
    // what the caller wants: masks, or the vector -- with mask words lent where there is a vector to write, the option allows it and, under
    // a capture, the handle's words hold the batch already
    const size_t lent_bytes = (size_t)pml_mask_words(r.n_reads, r.n_bases, 0) * 4;
    const bool lends = r.lend_masks && r.out && ix->pml_via_mask != 0 && (r.chunk || !no_alloc || lent_bytes <= ix->dmask.cap());
    // (the park queue's capacity is one of the plan's inputs; the queue itself is lent behind the plan, to the device-pointer calls that
    // write masks -- parked or not, as ever)
    PmlAsk ask = pml_ask(c, masks ? PmlWant::kMasks : lends ? PmlWant::kVectorLendsMasks : PmlWant::kVector, ix->pml_via_mask);
    ask.park_cap = r.chunk ? 0 : park_queue_offer(ix, r.n_reads, no_alloc);
    ask.park_queue = ask.park_cap > 0;
    c.chain_rows = ix->tables.rows4.get();
    PmlRoute route = plan_pml(facts(ix->dev, c.chain_rows != nullptr), ix->cfg, r.n_reads, r.n_bases, ask);
    if (route.lent_masks()) {
        HIP_TRY(r.chunk ? grow(r.chunk[movi_index::kMask], lent_bytes) : grow(ix->dmask, lent_bytes));
        if (!r.chunk && no_alloc) ix->dmask.mark_in_graph();
        c.mask.words = r.chunk ? r.chunk[movi_index::kMask].as<uint32_t>() : ix->dmask.as<uint32_t>();
    }
    if (ask.park_queue && (masks || route.lent_masks()) && !lend_park_queue(ix, r.n_reads, no_alloc, c.mask)) route.park_lanes = 0, route.park_grid = 0;
    if (route.needs_tmp) {                                       // (masks by way of a vector: grow-only device scratch, the handle's or the chunk's)
        DevBuf &tmp = r.chunk ? r.chunk[movi_index::kTmp] : ix->scratch[movi_index::kTmp];
        HIP_TRY(grow(tmp, r.n_bases * 2));
        c.mask.tmp_pml = tmp.as<uint16_t>();
    }
    // (device-pointer calls: the probe's verdict is remembered for the next 15 calls on batches of the same shape -- mean read length
    // and read count to a factor of two --: such calls then enqueue the walk without the probe and its read-back.  Either verdict
    // gives the same answers; a stale one costs speed for at most those calls.  "seg_probe" 0 / 2 never probe anyway.)
    int cached = -1;
    const bool use_cache = r.seg_verdict == nullptr && ix->cfg.seg_probe == 1 && r.n_bases / r.n_reads >= 2ull * (uint64_t)std::max(ix->cfg.seg_len, 1);
    const uint32_t key = use_cache ? ((uint32_t)(63 - __builtin_clzll(r.n_bases / r.n_reads)) << 8) | (uint32_t)(63 - __builtin_clzll(r.n_reads)) : 0u;
    if (use_cache) {
        if (ix->seg_cache_left > 0 && ix->seg_cache_key == key) { cached = ix->seg_cache_verdict; ix->seg_cache_left -= 1; }
        c.seg_verdict = &cached;
    }
    const int before = cached;
    HIP_TRY(launch_pml(c, route));
    if (use_cache && before < 0 && cached >= 0) { ix->seg_cache_verdict = cached; ix->seg_cache_key = key; ix->seg_cache_left = 15; }
    return MOVI_OK;
}

int movi_pml_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                    uint64_t n_bases, uint16_t *d_out_pml, uint8_t *d_read_err, const uint32_t *d_read_order,
                    void *stream) {
    MlRequest r;
    r.bases = d_bases; r.offs = d_offsets; r.n_reads = n_reads; r.n_bases = n_bases;
    r.out = d_out_pml; r.err = d_read_err; r.order = d_read_order; r.stream = static_cast<hipStream_t>(stream);
    r.lend_masks = true;
    return pml_call(ix, r);
}

int movi_pml_mask_words(uint64_t n_reads, uint64_t n_bases, uint64_t first_base, uint64_t *n_words) {
    if (!n_words) return fail(MOVI_ERR_ARG, "n_words is NULL");
    *n_words = pml_mask_words(n_reads, n_bases, (uint32_t)(first_base & 31u));
    return MOVI_OK;
}

int movi_pml_mask_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                         uint64_t n_bases, uint64_t first_base, uint32_t *d_mask_words, uint8_t *d_read_err,
                         const uint32_t *d_read_order, void *stream) {
    if (n_reads && !d_mask_words) return fail(MOVI_ERR_ARG, "NULL device buffer");
    MlRequest r;
    r.bases = d_bases; r.offs = d_offsets; r.n_reads = n_reads; r.n_bases = n_bases;
    r.mask.words = d_mask_words; r.mask.phase = (uint32_t)(first_base & 31u);
    r.err = d_read_err; r.order = d_read_order; r.stream = static_cast<hipStream_t>(stream);
    return pml_call(ix, r);
}

int movi_pml_expand_device(movi_index_t *ix, const uint32_t *d_mask_words, const uint64_t *d_offsets, uint64_t n_reads,
                           uint64_t n_bases, uint64_t first_base, uint16_t *d_out_pml, void *stream) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) return MOVI_OK;
    if (!d_mask_words || !d_offsets || (n_bases && !d_out_pml)) return fail(MOVI_ERR_ARG, "NULL device buffer");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(launch_pml_expand(d_mask_words, d_offsets, n_reads, n_bases, (uint32_t)(first_base & 31u), d_out_pml,
                              static_cast<hipStream_t>(stream)));
    return MOVI_OK;
}

int movi_zml_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                    uint64_t n_bases, uint16_t *d_out_zml, uint8_t *d_read_err, const uint32_t *d_read_order,
                    void *stream) {
    MlRequest r;
    r.bases = d_bases; r.offs = d_offsets; r.n_reads = n_reads; r.n_bases = n_bases;
    r.out = d_out_zml; r.err = d_read_err; r.order = d_read_order; r.stream = static_cast<hipStream_t>(stream);
    return zml_call(ix, r);
}

int movi_last_launch(const movi_index_t *ix, movi_launch_info_t *info) {
    if (!ix || !info) return fail(MOVI_ERR_ARG, "NULL argument");
    memset(info, 0, sizeof(*info));
    static_assert(sizeof(info->kernel) == sizeof(ix->last_launch.kernel), "kernel name buffers differ");
    memcpy(info->kernel, ix->last_launch.kernel, sizeof(info->kernel));
    info->variant = ix->last_launch.variant;
    info->block_threads = ix->last_launch.block_threads;
    info->waves_per_cu = ix->last_launch.waves_per_cu;
    info->segmented = ix->last_launch.segmented;
    info->idx64 = ix->last_launch.idx64;
    info->staged = ix->last_launch.staged;
    info->ahead = ix->last_launch.ahead;
    return MOVI_OK;
}

int movi_launch_log(char *buf, size_t cap, size_t *needed) {
    const size_t n = take_launch_log(buf, cap);
    if (needed) *needed = n + 1;
    return MOVI_OK;
}

int movi_index_info(const movi_index_t *ix, const char *key, double *value) {
    if (!ix || !key || !value) return fail(MOVI_ERR_ARG, "NULL argument");
    const double rows = ix->kmode != (int)ix->desc.mode ? (double)ix->desc.r * 8.0 : (double)ix->rows_bytes;
    const DerivedTables &tab = ix->tables;
    const double kmer = tab.held_bytes(kTabKmer, ix->desc.r), ftab = tab.held_bytes(kTabFtab, ix->desc.r);
    const double ahead = tab.held_bytes(kTabAhead, ix->desc.r), deep = tab.held_bytes(kTabDeep, ix->desc.r);
    const double ckpt = tab.ckpt_bytes_reported(ix->desc.r), chain = tab.held_bytes(kTabChain, ix->desc.r);
    const double locate = ix->sa_rate ? (double)locate_rows_bytes(ix->desc.r) + (double)(ix->desc.length / ix->sa_rate + 1) * 8.0 : 0.0;
    const double color = ix->d_color_inds ? (double)ix->color_flat.size() * 2.0 + (double)ix->color_inds.size() * 8.0 : 0.0;
    if (!strcmp(key, "rows_bytes")) *value = rows;
    else if (!strcmp(key, "locate_bytes")) *value = locate;
    else if (!strcmp(key, "kmer_bytes")) *value = kmer;
    else if (!strcmp(key, "ftab_bytes")) *value = ftab;
    else if (!strcmp(key, "ahead_rows_bytes")) *value = ahead;
    else if (!strcmp(key, "deep_rows_bytes")) *value = deep;
    else if (!strcmp(key, "chain_rows_bytes")) *value = chain;
    else if (!strcmp(key, "deep_hint_bits")) *value = tab.rows3 ? (double)tab.deep.hint_bits : 0.0;   // width of a hint in the deep rows the handle holds (0 = it holds none)
    else if (!strcmp(key, "ckpt_bytes")) *value = ckpt;
    else if (!strcmp(key, "color_bytes")) *value = color;
    else if (!strcmp(key, "color_taxa")) *value = (double)ix->color_taxa.size();      // to_taxon_id entries held (0 after a load)
    else if (!strcmp(key, "color_chunks")) *value = (double)ix->color_chunks;
    else if (!strcmp(key, "color_walk_seconds")) *value = ix->color_seconds[0];
    else if (!strcmp(key, "color_sort_seconds")) *value = ix->color_seconds[1];
    else if (!strcmp(key, "color_number_seconds")) *value = ix->color_seconds[2];
    else if (!strcmp(key, "derived_bytes")) *value = kmer + ftab + ahead + deep + chain + ckpt + locate + color;
    else if (!strcmp(key, "ahead_no_ff")) *value = ix->policy.ahead_tallied ? ix->policy.ahead_no_ff : -1.0;
    else if (!strcmp(key, "device_scratch_bytes")) {         // device scratch the *_device calls hold: mask words (retired ones too), vector, segment workspace
        *value = (double)ix->dmask.held_bytes() + (double)ix->dpark.cap() + (double)ix->scratch[movi_index::kTmp].cap() + (double)ix->seg_ws.cap() +
                 (double)ix->color_scratch.cap();      // (held_bytes: the live words and the handle's retired blocks, queues among them)
    }
    else if (!strcmp(key, "park_lanes")) *value = (double)ix->last_launch.park_lanes;   // what the last PML call's mask walk parked at (0 = it parked nothing)
    else if (!strcmp(key, "ff_skip")) *value = (double)ix->last_launch.ff_skip;         // 1 = the last PML call's walk ran with the fast-forward skip
    else if (!strcmp(key, "parked_reads")) {               // reads the last query call's first launch handed to its second (waits for the device; not under a stream capture)
        unsigned long long parked = 0;
        HIP_TRY(hipSetDevice(ix->device));
        HIP_TRY(hipDeviceSynchronize());
        if (ix->last_launch.park_lanes > 0 && ix->dpark.ptr()) HIP_TRY(hipMemcpy(&parked, ix->dpark.ptr(), sizeof(parked), hipMemcpyDeviceToHost));   // (the queue's head)
        *value = (double)parked;
    }
    else if (!strcmp(key, "host_staging_bytes")) {          // device staging the synchronous *_host calls hold at the moment
        double b = 0.0;
        for (const DevBuf &buf : ix->scratch) b += (double)buf.cap();
        *value = b;
    }
    else return fail(MOVI_ERR_ARG, std::string("unknown info key: ") + key);
    return MOVI_OK;
}

int movi_last_stats(movi_index_t *ix, void *stream, movi_query_stats_t *stats) {
    if (!ix || !stats) return fail(MOVI_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    DevStats h{};
    HIP_TRY(hipMemcpy(&h, ix->d_stats.get(), sizeof(h), hipMemcpyDeviceToHost));
    stats->bases = 0;                      // not tracked on the device: the *_host entry points fill it in
    stats->fast_forwards = h.fast_forwards;
    stats->scans = h.scans;
    stats->repositions = h.repositions;
    stats->errors = h.errors;
    stats->lane_steps = h.lane_steps;
    stats->wave_steps = h.wave_steps;
    stats->segments = h.segments;
    stats->rewalked = h.rewalked;
    return MOVI_OK;
}

}  // extern "C"

namespace {

// Where a *_host call's bases come from: the caller's ASCII bytes (h_bases, indexed by offsets[]), or reads packed two bits per base
// plus their exception list (include/movi_hip.h): those go up as they are, a quarter of the bytes, and every chunk is unpacked on the
// device into the staging the ASCII bytes would have been copied to.  The ASCII form makes exactly the HIP calls it always made.
struct ReadSource {
    const uint8_t *ascii = nullptr;
    bool two_bit = false;
    const uint8_t *packed = nullptr;
    const uint64_t *exc_pos = nullptr;
    const uint8_t *exc_byte = nullptr;
    uint64_t n_exc = 0;
    ReadSource(const uint8_t *h_bases) : ascii(h_bases) {}
    ReadSource(const uint8_t *h_packed, const uint64_t *h_exc_pos, const uint8_t *h_exc_byte, uint64_t n)
        : two_bit(true), packed(h_packed), exc_pos(h_exc_pos), exc_byte(h_exc_byte), n_exc(n) {}
    // what crosses the link for bases [b0, b0 + nb): where it starts in the caller's buffer and how long it is
    const uint8_t *up_from(uint64_t b0) const { return two_bit ? packed + (b0 >> 2) : ascii + b0; }
    size_t up_bytes(uint64_t b0, uint64_t nb) const { return two_bit ? packed_span_bytes(b0, nb) : (size_t)nb; }
};
// A chunk of a packed call: d_packed holds the caller's packed bytes from byte b0 >> 2 on; its slice of the exception list (already on the
// device, the whole call's) is found on the host.  Two kernels on the chunk's stream (movi_walk_pack.hip).
hipError_t unpack_chunk(const ReadSource &src, const void *d_exc_pos, const void *d_exc_byte, const void *d_packed, uint64_t b0, uint64_t nb,
                        void *d_bases, hipStream_t s) {
    const uint64_t *end = src.exc_pos + src.n_exc;
    const uint64_t *lo = std::lower_bound(src.exc_pos, end, b0), *hi = std::lower_bound(lo, end, b0 + nb);
    const size_t skip = (size_t)(lo - src.exc_pos);
    return launch_unpack_reads(static_cast<const uint8_t *>(d_packed), b0 & 3u, nb, static_cast<const uint64_t *>(d_exc_pos) + skip,
                               static_cast<const uint8_t *>(d_exc_byte) + skip, (uint64_t)(hi - lo), b0, static_cast<uint8_t *>(d_bases), s);
}

// Where one chunk of a *_host call lives: the stream it runs on, its counters, its device staging (the handle's in the
// synchronous path, a pipeline slot's in the overlapped one) and, overlapped only, page-locked room for per-read results.
struct ChunkCtx {
    movi_index *ix = nullptr;
    hipStream_t s = nullptr;
    DevStats *d_stats = nullptr;
    DevBuf *d = nullptr;             // kScratchSlots of them
    uint8_t *h_small = nullptr;
    SegWorkspace *seg_ws = nullptr;
    int ragged_hint = -1;            // the chunk's longest read is (1) / is not (0) more than 1.5 x its mean: launch_pml's segment policy
    int *seg_verdict = nullptr;      // one probe per call: the first chunk's verdict serves the others (launch_pml_segmented)
    HostPool::Group *grp = nullptr;  // overlapped path: the slot's group of worker-pool tasks (what reads the slot's page-locked block)
    bool async = false;
    bool delivered = false;          // overlapped path, set by fetch(): a host function on the chunk's stream hands its mask words on, harvest() need not
    template <typename T>
    hipError_t alloc(int slot, size_t bytes, T **out) {
        hipError_t e = grow(d[slot], bytes);
        *out = d[slot].template as<T>();
        return e;
    }
    // the chunk as a PML / ZML call: its reads, stream, counters, segment state and scratch slots (the caller adds where the results go)
    MlRequest request(const HostChunk &c, const uint8_t *db, const uint64_t *dof, uint8_t *derr) const {
        MlRequest r;
        r.bases = db; r.offs = dof; r.n_reads = c.nr; r.n_bases = c.nb; r.err = derr; r.stream = s;
        r.stats = d_stats; r.seg_ws = seg_ws; r.ragged_hint = ragged_hint; r.seg_verdict = seg_verdict; r.chunk = d;
        return r;
    }
    // device -> host: straight into the caller's buffer (synchronous path, or a page-locked destination) ...
    hipError_t down(void *h_dst, const void *d_src, size_t bytes) {
        if (!bytes) return hipSuccess;
        return async ? hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, s)
                     : hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost);
    }
    // ... or, overlapped path with a destination that may be pageable (a copy into pageable memory would hold the host
    // until the kernel is done): into the slot's page-locked block at `small_off`; harvest() moves it on
    hipError_t down_small(void *h_dst, size_t small_off, const void *d_src, size_t bytes) {
        return down(async ? static_cast<void *>(h_small + small_off) : h_dst, d_src, bytes);
    }
};

// Page-locked (hipHostMalloc / hipHostRegister) host memory?  Pageable pointers are unknown to the runtime.
bool is_pinned(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

}  // namespace

// Every stream of the handle -- the upload stream here, a slot's in PipeSlot::release -- drains before a buffer it may touch goes.
static void release_scratch(movi_index *ix) {
    if (ix->pipe_up) {
        (void)hipStreamSynchronize(ix->pipe_up);
        (void)hipStreamDestroy(ix->pipe_up);
        ix->pipe_up = nullptr;
    }
    for (hipEvent_t e : ix->pipe_ev) (void)hipEventDestroy(e);
    ix->pipe_ev.clear();
    for (auto &sl : ix->pipe) sl.release();
    for (DevBuf &b : ix->scratch) b.release();
    ix->seg_ws.release();
    ix->color_scratch.release();
    ix->dmask.release();                                   // (graphs captured over movi_pml_device on this handle are invalid from here on)
    ix->dpark.release();
    ix->h_rel.release();
}

namespace {

// The offsets are the caller's: every *_host entry point validates them all before they size a chunk, an
// allocation or a copy (and before the device is touched, so the check is testable without one).
int check_offsets(const uint64_t *h_offsets, uint64_t n_reads) {
    // one branch-free pass (a decreasing pair wraps to >= 2^63, an overlong read is >= 2^32: either way high bits);
    // the slow pass below only runs to name the first offender
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n_reads; i++) bad |= (h_offsets[i + 1] - h_offsets[i]) >> 32;
    if (!bad) return MOVI_OK;
    for (uint64_t i = 0; i < n_reads; i++) {
        if (h_offsets[i + 1] < h_offsets[i]) return fail(MOVI_ERR_ARG, "read offsets are not non-decreasing");
        if (h_offsets[i + 1] - h_offsets[i] > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "a read is longer than 2^32 - 1 bases");
    }
    return MOVI_OK;
}

template <typename Counters>                                 // (DevStats, or what movi_last_stats made of them)
void add_stats(movi_query_stats_t *acc, uint64_t nb, const Counters &h) {
    acc->bases += nb;
    acc->fast_forwards += h.fast_forwards;
    acc->scans += h.scans;
    acc->repositions += h.repositions;
    acc->errors += h.errors;
    acc->lane_steps += h.lane_steps;
    acc->wave_steps += h.wave_steps;
    acc->segments += h.segments;
    acc->rewalked += h.rewalked;
}

// A packed call's exception list goes up once, ahead of every chunk's bytes: synchronously, or (overlapped path) on the upload stream.
int upload_exceptions(movi_index *ix, const ReadSource &src, bool on_upload_stream) {
    if (!src.two_bit || !src.n_exc) return MOVI_OK;
    DevBuf &pos = ix->scratch[movi_index::kExcPos], &byte = ix->scratch[movi_index::kExcByte];
    const size_t n = (size_t)src.n_exc;
    hipError_t e = hipSuccess;
    if (on_upload_stream && !ix->pipe_up) e = create_upload_stream(&ix->pipe_up);
    if (e == hipSuccess) e = grow(pos, n * 8);
    if (e == hipSuccess) e = grow(byte, n);
    if (e == hipSuccess) e = on_upload_stream ? hipMemcpyAsync(pos.ptr(), src.exc_pos, n * 8, hipMemcpyHostToDevice, ix->pipe_up)
                                              : hipMemcpy(pos.ptr(), src.exc_pos, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = on_upload_stream ? hipMemcpyAsync(byte.ptr(), src.exc_byte, n, hipMemcpyHostToDevice, ix->pipe_up)
                                              : hipMemcpy(byte.ptr(), src.exc_byte, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) return MOVI_OK;
    if (on_upload_stream && ix->pipe_up) (void)hipStreamSynchronize(ix->pipe_up);
    return fail_hip(e, "uploading the exception list");
}

// One kind of query behind a *_host entry point, over the call's planned chunks (movi_host_plan.hpp):
//   launch(ctx, chunk, d_bases, d_offs, d_err)   allocates the chunk's result staging from ctx and enqueues the kernel;
//   fetch(ctx, chunk)                            enqueues the results' way back (ctx.down / ctx.down_small);
//   harvest(h_small, chunk, group, delivered)    overlapped path only, after the chunk's stream has drained: per-read
//                                                results from the page-locked block to the caller's arrays.
template <typename Launch, typename Fetch>
int run_chunked(movi_index *ix, const ReadSource &src, const uint64_t *h_offsets, const std::vector<HostChunk> &chunks,
                uint8_t *h_read_err, movi_query_stats_t *stats, Launch launch, Fetch fetch) {
    memset(stats, 0, sizeof(*stats));
    if (int rc = upload_exceptions(ix, src, false)) return rc;
    int seg_verdict = -1;
    ChunkCtx ctx;
    ctx.ix = ix;
    ctx.seg_verdict = &seg_verdict;
    ctx.d_stats = ix->d_stats.get();
    ctx.d = ix->scratch;
    ctx.seg_ws = &ix->seg_ws;
    for (const HostChunk &c : chunks) {
        uint8_t *d_bases = nullptr, *d_err = nullptr;
        uint64_t *d_offs = nullptr;
        static const bool trace = getenv("MOVI_TRACE_HOST_CALLS") != nullptr;   // diagnostic: where a synchronous host call's time goes, to stderr
        double tr[8] = {0};
        auto stamp = [&](int k) { if (trace) tr[k] = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        stamp(0);
        HIP_TRY(ctx.alloc(movi_index::kBases, c.nb, &d_bases));
        HIP_TRY(ctx.alloc(movi_index::kOffs, (c.nr + 1) * 8, &d_offs));
        HIP_TRY(ctx.alloc(movi_index::kErr, c.nr, &d_err));
        HIP_TRY(grow_entries(ix->h_rel, (size_t)(c.nr + 1)));
        uint64_t *rel = ix->h_rel.as<uint64_t>();             // (read by the copy below before the call returns: hipMemcpy is synchronous)
        ctx.ragged_hint = fill_relative_offsets(rel, h_offsets, c);
        // No length sort here: on ragged batches handing the lanes out longest-first measured
        // slightly SLOWER (31.1 vs 32.8 Gbases/s, log-normal lengths) -- the walk is bound by the
        // memory system, not by lane occupancy, and the dispatcher already refills whole blocks.
        stamp(1);
        if (c.nb && !src.two_bit) HIP_TRY(hipMemcpy(d_bases, src.ascii + c.b0, c.nb, hipMemcpyHostToDevice));
        if (c.nb && src.two_bit) {                            // a quarter of the bytes go up; the null stream unpacks them ahead of the walk
            void *d_packed = nullptr;
            HIP_TRY(ctx.alloc(movi_index::kPacked, src.up_bytes(c.b0, c.nb), &d_packed));
            HIP_TRY(hipMemcpy(d_packed, src.up_from(c.b0), src.up_bytes(c.b0, c.nb), hipMemcpyHostToDevice));
            HIP_TRY(unpack_chunk(src, ix->scratch[movi_index::kExcPos].ptr(), ix->scratch[movi_index::kExcByte].ptr(), d_packed, c.b0, c.nb, d_bases, nullptr));
        }
        stamp(2);
        HIP_TRY(hipMemcpy(d_offs, rel, (c.nr + 1) * 8, hipMemcpyHostToDevice));
        stamp(3);
        int rc = launch(ctx, c, d_bases, d_offs, d_err);
        if (rc) return rc;
        stamp(4);
        movi_query_stats_t st{};
        rc = movi_last_stats(ix, nullptr, &st);
        if (rc) return rc;
        stamp(5);
        rc = fetch(ctx, c);
        if (rc) return rc;
        stamp(6);
        if (h_read_err) HIP_TRY(hipMemcpy(h_read_err + c.first, d_err, c.nr, hipMemcpyDeviceToHost));
        stamp(7);
        if (trace)
            fprintf(stderr, "[movi_hip] host call: %llu reads %llu bases | staging + offsets %.3f | bases up %.3f | offsets up %.3f | launch %.3f | walk + counters %.3f | "
                            "results down %.3f | error bytes down %.3f ms\n", (unsigned long long)c.nr, (unsigned long long)c.nb, (tr[1] - tr[0]) * 1e3, (tr[2] - tr[1]) * 1e3,
                    (tr[3] - tr[2]) * 1e3, (tr[4] - tr[3]) * 1e3, (tr[5] - tr[4]) * 1e3, (tr[6] - tr[5]) * 1e3, (tr[7] - tr[6]) * 1e3);
        add_stats(stats, c.nb, st);
    }
    return MOVI_OK;
}

// One kind of query whose per-read results vary in length (MEMs, k-mer runs) behind a *_host entry point: the reads go through the
// handle's staging in chunks of about kCompactChunkBases bases (at least kCompactChunkReads reads, at most kCompactMaxChunkBases:
// the device stages elem_bytes per base, twice -- the kernel's output and its compacted copy), every chunk's results are compacted on
// the device and come down behind those of the chunks before it.
//   device(d_bases, d_offs, nr, nb, d_out, d_n, d_err)   enqueues the query on the null stream: read i's results from d_out + elem_bytes *
//                                                        d_offs[i], their number in d_n[i], a second u32 per read in d_n[nr + i] if `second`.
struct CompactOut {
    size_t elem_bytes;         // of one result
    void *h_out;               // the caller's array of `cap` results; *n_total = the number found (set even when they do not fit)
    uint64_t cap, *n_total;
    uint32_t *h_n;             // results per read
    bool second;               // the kernel writes a second u32 per read ...
    uint32_t *h_second;        // ... which comes down here (optional)
    uint8_t *h_read_err;       // optional
    const char *what;          // the overflow message between the two numbers
};
template <typename Device>
int run_compact(movi_index *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, const CompactOut &o,
                movi_query_stats_t *stats, Device device) {
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HIP_TRY(hipSetDevice(ix->device));
    DevBuf *d = ix->scratch;
    HostFacts facts;
    facts.query = HostQuery::kCompact;
    facts.total = h_offsets[n_reads] - h_offsets[0];
    facts.n_reads = n_reads;
    HostCall call = plan_host_call(facts, HostOptions());
    call.settle(false);
    std::vector<uint64_t> rel;
    uint64_t total = 0, errors = 0;
    bool overflow = false;
    for (const HostChunk &c : plan_chunks(call, h_offsets, n_reads)) {
        const uint64_t first = c.first, nr = c.nr, nb = c.nb;
        HIP_TRY(grow(d[movi_index::kBases], nb));
        HIP_TRY(grow(d[movi_index::kOffs], (nr + 1) * 8));
        HIP_TRY(grow(d[movi_index::kErr], nr));
        HIP_TRY(grow(d[movi_index::kOut], nb * o.elem_bytes));
        HIP_TRY(grow(d[movi_index::kA], nr * (o.second ? 8 : 4)));
        HIP_TRY(grow(d[movi_index::kB], (nr + 1) * 8));
        rel.resize(nr + 1);
        (void)fill_relative_offsets(rel.data(), h_offsets, c);
        if (nb) HIP_TRY(hipMemcpy(d[movi_index::kBases].ptr(), h_bases + c.b0, nb, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d[movi_index::kOffs].ptr(), rel.data(), (nr + 1) * 8, hipMemcpyHostToDevice));
        const uint64_t *d_offs = d[movi_index::kOffs].as<uint64_t>();
        uint32_t *d_n = d[movi_index::kA].as<uint32_t>();
        uint64_t *d_first = d[movi_index::kB].as<uint64_t>();
        int rc = device(d[movi_index::kBases].as<uint8_t>(), d_offs, nr, nb, d[movi_index::kOut].ptr(), d_n, d[movi_index::kErr].as<uint8_t>());
        if (rc) return rc;
        // compaction on the device: the per-read counts' prefix, then only the results found come down
        HIP_TRY(launch_count_scan(d_n, nr, d_first, nullptr));
        DevStats h{};
        HIP_TRY(hipMemcpy(&h, ix->d_stats.get(), sizeof(h), hipMemcpyDeviceToHost));
        uint64_t found = 0;
        HIP_TRY(hipMemcpy(o.h_n + first, d_n, nr * 4, hipMemcpyDeviceToHost));
        if (o.h_second) HIP_TRY(hipMemcpy(o.h_second + first, d_n + nr, nr * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&found, d_first + nr, 8, hipMemcpyDeviceToHost));
        if (!overflow && total + found <= o.cap) {
            if (found) {
                HIP_TRY(grow(d[movi_index::kS], found * o.elem_bytes));
                HIP_TRY(launch_gather(d[movi_index::kOut].ptr(), o.elem_bytes, d_offs, d_n, nr, d_first, d[movi_index::kS].ptr(), nullptr));
                HIP_TRY(hipMemcpy(static_cast<uint8_t *>(o.h_out) + total * o.elem_bytes, d[movi_index::kS].ptr(), found * o.elem_bytes, hipMemcpyDeviceToHost));
            }
        } else overflow = true;
        if (o.h_read_err) HIP_TRY(hipMemcpy(o.h_read_err + first, d[movi_index::kErr].ptr(), nr, hipMemcpyDeviceToHost));
        total += found;
        errors += h.errors;
        if (stats) add_stats(stats, nb, h);
    }
    if (o.n_total) *o.n_total = total;
    if (overflow) return fail(MOVI_ERR_ARG, std::to_string(total) + o.what + std::to_string(o.cap));
    if (errors)
        return fail(MOVI_ERR_INVARIANT, std::to_string(errors) + " read(s) hit a move-structure invariant violation (corrupt index?)");
    return MOVI_OK;
}

// The same call with the caller's bases (and, for PML / ZML, result vector) in page-locked memory: kPipeSlots chunks in
// flight, each on its own stream -- upload, walk, download -- so that the three overlap across chunks: the call then
// costs about what its slowest leg does (2 B per base coming down: ~28 Gbases/s on a 56 GB/s link) instead of the
// sum of the three.
// A chunk's download is enqueued only once its walk HAS finished (the host waits on an event), never behind it as a
// dependent copy: a copy that waits for a kernel sits in its SDMA ring as a poll packet and holds up every copy queued
// after it -- the next chunk's upload included.  Enqueued that way (the first version) the timeline was strictly serial,
// chunk after chunk (rocprofv3 --memory-copy-trace), and the call no faster than the synchronous one.
template <typename Launch, typename Fetch, typename Harvest>
int run_pipelined(movi_index *ix, const HostCall &call, const ReadSource &src, const uint64_t *h_offsets, const std::vector<HostChunk> &chunks,
                  uint8_t *h_read_err, movi_query_stats_t *stats, Launch launch, Fetch fetch, Harvest harvest) {
    memset(stats, 0, sizeof(*stats));
    movi_query_stats_t acc{};
    const uint64_t total = call.facts.total, n_reads = call.facts.n_reads;
    const size_t small_bytes = call.small_bytes, mask_word_bytes = call.words_in_block ? 4 : 0;
    uint8_t *all = nullptr;                                    // the call's reads in one device buffer (set below, ahead of the loop), or chunk by chunk
    uint8_t *all_packed = nullptr;                             // packed calls: what went up ahead of the loop, from byte chunks[0].b0 >> 2 of the caller's buffer
    constexpr int S = movi_index::kPipeSlots;
    // a slot: 0 free, 1 walking (upload + kernel enqueued), 2 coming down; its chunk; whether fetch() already handed the chunk's results on
    struct InFlight { int stage = 0; HostChunk c{}; bool delivered = false; } fl[S];
    HostPool::Group grp[S];                                    // host-side work a slot's harvest has handed to the worker pool (it reads the slot's page-locked block)
    // layout of a slot's page-locked block
    auto off_err = [](uint64_t nr) { return (size_t)(nr + 1) * 8; };
    auto off_small = [&](uint64_t nr) { return (off_err(nr) + (size_t)nr + 15) & ~(size_t)15; };
    // (mask_word_bytes = 4: the block also holds the chunk's reset-mask words, behind the per-read results)
    auto off_stats = [&](uint64_t nr, uint64_t nb) {
        return (off_small(nr) + (size_t)nr * small_bytes + (mask_word_bytes ? (size_t)pml_mask_words(nr, nb, 31u) * mask_word_bytes : 0) + 15) & ~(size_t)15;
    };
    int seg_verdict = -1;
    auto ctx_of = [&](int k, uint64_t nr) {
        movi_index::PipeSlot &sl = ix->pipe[k];
        ChunkCtx ctx;
        ctx.ix = ix;
        ctx.seg_verdict = &seg_verdict;
        ctx.s = sl.s;
        ctx.d_stats = sl.d_stats.get();
        ctx.d = sl.d;
        ctx.h_small = sl.h.as<uint8_t>() + off_small(nr);
        ctx.seg_ws = &sl.seg_ws;
        ctx.async = true;
        ctx.grp = &grp[k];
        return ctx;
    };
    // a chunk's stream has drained: counters, error bytes, per-read results
    auto finish = [&](int k) -> int {
        movi_index::PipeSlot &sl = ix->pipe[k];
        InFlight &f = fl[k];
        if (f.stage == 0) return MOVI_OK;
        f.stage = 0;
        HIP_TRY(hipStreamSynchronize(sl.s));
        DevStats h;
        const uint8_t *blk = sl.h.as<uint8_t>();
        memcpy(&h, blk + off_stats(f.c.nr, f.c.nb), sizeof(h));
        add_stats(&acc, f.c.nb, h);
        if (h_read_err) memcpy(h_read_err + f.c.first, blk + off_err(f.c.nr), f.c.nr);
        harvest(blk + off_small(f.c.nr), f.c, &grp[k], f.delivered);
        return MOVI_OK;
    };
    // chunk ci goes up into slot k and is walked
    auto up = [&](int k, size_t ci) -> int {
        const HostChunk &c = chunks[ci];
        movi_index::PipeSlot &sl = ix->pipe[k];
        if (int rc = finish(k)) return rc;
        HostPool::get().wait(&grp[k]);                       // (the slot's block is about to be rewritten)
        if (!sl.s) HIP_TRY(hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking));
        if (!sl.ev) HIP_TRY(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
        if (!sl.ev_up) HIP_TRY(hipEventCreateWithFlags(&sl.ev_up, hipEventDisableTiming));
        if (!ix->pipe_up) HIP_TRY(create_upload_stream(&ix->pipe_up));
        if (!sl.d_stats) HIP_TRY(dev_alloc(sl.d_stats, sizeof(DevStats)));
        HIP_TRY(grow_block(sl.h, off_stats(c.nr, c.nb) + sizeof(DevStats)));
        ChunkCtx ctx = ctx_of(k, c.nr);
        uint8_t *d_bases = nullptr, *d_err = nullptr, *d_packed = nullptr;
        uint64_t *d_offs = nullptr;
        if (all) d_bases = all + (c.b0 - chunks[0].b0);
        else HIP_TRY(ctx.alloc(movi_index::kBases, c.nb, &d_bases));
        if (all_packed) d_packed = all_packed + ((c.b0 >> 2) - (chunks[0].b0 >> 2));
        else if (src.two_bit) HIP_TRY(ctx.alloc(movi_index::kPacked, src.up_bytes(c.b0, c.nb), &d_packed));
        HIP_TRY(ctx.alloc(movi_index::kOffs, (c.nr + 1) * 8, &d_offs));
        HIP_TRY(ctx.alloc(movi_index::kErr, c.nr, &d_err));
        uint64_t *rel = sl.h.as<uint64_t>();
        ctx.ragged_hint = fill_relative_offsets(rel, h_offsets, c);
        fl[k].c = c;
        fl[k].delivered = false;
        fl[k].stage = 1;                                     // from here on the streams hold work that touches caller memory
        // (the upload stream carries the bases alone, copy behind copy: with the chunk's offsets in between, every chunk left it idle for
        // ~40 us -- a fifth of a 9.4 MB copy; the offsets go up on the chunk's own stream, ahead of its walk: profiles/r06_host_path.txt)
        if (!all) {
            if (c.nb) HIP_TRY(hipMemcpyAsync(src.two_bit ? d_packed : d_bases, src.up_from(c.b0), src.up_bytes(c.b0, c.nb), hipMemcpyHostToDevice, ix->pipe_up));
            HIP_TRY(hipEventRecord(sl.ev_up, ix->pipe_up));
            HIP_TRY(hipMemcpyAsync(d_offs, rel, (c.nr + 1) * 8, hipMemcpyHostToDevice, sl.s));
        } else {
            // (by a kernel that reads the slot's page-locked block, not by the copy engine: that one has the whole call's reads queued)
            HIP_TRY(launch_copy_words(d_offs, rel, c.nr + 1, sl.s));
        }
        HIP_TRY(hipStreamWaitEvent(sl.s, all ? ix->pipe_ev[ci] : sl.ev_up, 0));
        // (packed calls: the chunk's own stream unpacks what has arrived into the place the ASCII copy lands in; the upload stream carries copies alone)
        if (src.two_bit)
            HIP_TRY(unpack_chunk(src, ix->scratch[movi_index::kExcPos].ptr(), ix->scratch[movi_index::kExcByte].ptr(), d_packed, c.b0, c.nb, d_bases, sl.s));
        if (int rc = launch(ctx, c, d_bases, d_offs, d_err)) return rc;
        HIP_TRY(hipEventRecord(sl.ev, sl.s));
        return MOVI_OK;
    };
    // slot k's walk is over: its results start their way down
    auto down = [&](int k) -> int {
        movi_index::PipeSlot &sl = ix->pipe[k];
        const HostChunk &c = fl[k].c;
        HIP_TRY(hipEventSynchronize(sl.ev));
        ChunkCtx ctx = ctx_of(k, c.nr);
        const int rc = fetch(ctx, c);
        fl[k].delivered = ctx.delivered;
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(sl.h.as<uint8_t>() + off_err(c.nr), sl.d[movi_index::kErr].ptr(), c.nr, hipMemcpyDeviceToHost, sl.s));
        HIP_TRY(hipMemcpyAsync(sl.h.as<uint8_t>() + off_stats(c.nr, c.nb), sl.d_stats.get(), sizeof(DevStats), hipMemcpyDeviceToHost, sl.s));
        fl[k].stage = 2;
        return MOVI_OK;
    };
    // chunks that have arrived on the host are harvested as soon as the loop comes by, not when their slot is needed again:
    // a harvest may have real work to hand on (the mask path's expansion runs on the host's worker threads beside the next walks)
    auto finish_arrived = [&]() -> int {
        for (int k = 0; k < S; k++) {
            if (fl[k].stage != 2) continue;
            const hipError_t q = hipStreamQuery(ix->pipe[k].s);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); continue; }
            if (int rc = finish(k)) return rc;
        }
        return MOVI_OK;
    };
    // kPipeAhead chunks going up or being walked (their kernels share the GPU: the lanes in flight are the sum of
    // theirs) while one comes down; twice as many slots, so that a slot's previous chunk has long arrived on the host
    // when the slot is reused (with kPipeAhead + 1 slots every upload waited for the download issued just before it,
    // and the downloads did not queue back to back)
    int rc = MOVI_OK;
    const size_t n = chunks.size();
    size_t next_up = 0;
    if (int rce = upload_exceptions(ix, src, true)) return rce;   // ahead of every chunk's bytes on the upload stream
    // ALL THE READS GO UP AHEAD OF THE LOOP (calls of up to 2^31 bases, into the handle's call-wide staging): the copies queued behind one
    // another, an event behind each, and a chunk's walk waits for its event.  Enqueued chunk by chunk from the loop -- three ahead of the
    // walk being waited for -- the upload stream ran dry two or three times per call (0.1 ms each), and the upload is what bounds the
    // call.  (The chunks' offsets then must not travel by the copy engine: they would queue behind the whole call's reads.)
    if (call.upload_ahead(n)) {
        hipError_t e = hipSuccess;
        if (!ix->pipe_up) e = create_upload_stream(&ix->pipe_up);
        if (e == hipSuccess) e = grow(ix->scratch[movi_index::kBases], total);
        if (e == hipSuccess && src.two_bit) e = grow(ix->scratch[movi_index::kPacked], src.up_bytes(chunks[0].b0, total));
        while (e == hipSuccess && ix->pipe_ev.size() < n) {
            hipEvent_t ev = nullptr;
            e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (e == hipSuccess) ix->pipe_ev.push_back(ev);
        }
        if (e == hipSuccess) {
            all = ix->scratch[movi_index::kBases].as<uint8_t>();
            if (src.two_bit) all_packed = ix->scratch[movi_index::kPacked].as<uint8_t>();
            for (size_t i = 0; i < n && e == hipSuccess; i++) {
                const HostChunk &c = chunks[i];
                // (packed: the bytes that cover the chunk; a byte that two chunks share goes up with both, to the same place)
                if (c.nb) e = hipMemcpyAsync(src.two_bit ? all_packed + ((c.b0 >> 2) - (chunks[0].b0 >> 2)) : all + (c.b0 - chunks[0].b0), src.up_from(c.b0),
                                             src.up_bytes(c.b0, c.nb), hipMemcpyHostToDevice, ix->pipe_up);
                if (e == hipSuccess) e = hipEventRecord(ix->pipe_ev[i], ix->pipe_up);
            }
            if (e != hipSuccess) {                            // copies may be in flight: nothing reads the caller's buffers when the call returns
                (void)hipStreamSynchronize(ix->pipe_up);
                return fail_hip(e, "uploading the reads");
            }
        } else {
            (void)hipGetLastError();                          // no room for the call-wide staging: chunk by chunk (the plan's fall-back)
        }
    }
    for (size_t i = 0; i < n && rc == MOVI_OK; i++) {
        for (; next_up < n && next_up < i + (size_t)movi_index::kPipeAhead && rc == MOVI_OK; next_up++) rc = up((int)(next_up % S), next_up);
        if (rc == MOVI_OK) rc = down((int)(i % S));
        if (rc == MOVI_OK) rc = finish_arrived();
    }
    for (size_t j = 0; j < (size_t)S && rc == MOVI_OK; j++) rc = finish((int)((n + j) % S));   // oldest first
    if (rc != MOVI_OK) {
        // whatever happened, nothing may still be reading or writing the caller's buffers when the call returns
        const std::string keep = g_err;
        if (ix->pipe_up) (void)hipStreamSynchronize(ix->pipe_up);
        for (int k = 0; k < S; k++)
            if (ix->pipe[k].s) (void)hipStreamSynchronize(ix->pipe[k].s);
        g_err = keep;
    }
    // (after the streams have drained: a stream's host function may hand work to the pool; also on errors: the workers write caller memory)
    for (int k = 0; k < S; k++) HostPool::get().wait(&grp[k]);
    *stats = acc;
    if (rc == MOVI_OK && total / n_reads >= 2ull * (uint64_t)(ix->cfg.seg_len > 0 ? ix->cfg.seg_len : 1)) ix->seg_seen = acc.segments != 0;
    return rc;
}

// The handle's options as the plan reads them.
HostOptions host_options(const movi_index *ix) {
    HostOptions o;
    o.host_overlap = ix->host_overlap; o.host_autopin = ix->host_autopin; o.host_masks = ix->host_masks; o.host_mask_share = ix->host_mask_share;
    o.pipe_chunk_bases = ix->pipe_chunk_bases; o.seg_seen = ix->seg_seen; o.seg_len = ix->cfg.seg_len;
    return o;
}

// A settled call (movi_host_plan.hpp) through the loop it chose, over the chunks planned for it.
template <typename Launch, typename Fetch, typename Harvest>
int run_host(movi_index *ix, const HostCall &call, const ReadSource &src, const uint64_t *h_offsets, uint8_t *h_read_err,
             movi_query_stats_t *stats, Launch launch, Fetch fetch, Harvest harvest) {
    movi_query_stats_t local{};
    const std::vector<HostChunk> chunks = plan_chunks(call, h_offsets, call.facts.n_reads);
    int rc = call.overlapped ? run_pipelined(ix, call, src, h_offsets, chunks, h_read_err, &local, launch, fetch, harvest)
                             : run_chunked(ix, src, h_offsets, chunks, h_read_err, &local, launch, fetch);
    if (stats) *stats = local;
    if (rc) return rc;
    if (local.errors)
        return fail(MOVI_ERR_INVARIANT, std::to_string(local.errors) +
                                            " read(s) hit a move-structure invariant violation (corrupt index?)");
    return MOVI_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------- page-locked host memory

int movi_host_alloc(size_t bytes, void **out) {
    if (!out) return fail(MOVI_ERR_ARG, "out is NULL");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return MOVI_OK;
}

int movi_host_free(void *p) {
    if (!p) return MOVI_OK;
    HIP_TRY(hipHostFree(p));
    return MOVI_OK;
}

// ------------------------------------------------------------- index.movi from a run-length BWT (movi_walk_build.hip)

int movi_build_from_rlbwt(int device, uint32_t mode, const uint8_t *h_heads, const uint64_t *h_lens, const uint64_t *h_thr,
                          uint64_t original_r, void **h_image, size_t *image_bytes) {
    if (h_image) *h_image = nullptr;
    if (image_bytes) *image_bytes = 0;
    if (!h_heads || !h_lens || !h_image || !image_bytes) return fail(MOVI_ERR_ARG, "NULL argument");
    if (!mode_supported(mode)) return fail(MOVI_ERR_ARG, "unsupported mode");
    if (mode_has_thresholds(mode) && !h_thr) return fail(MOVI_ERR_ARG, "the *-thresholds types need h_thr");
    // everything a kernel of the builder relies on, before any device call
    RlbwtInfo info;
    RlbwtArray which;
    std::string why;
    if (!rlbwt_check(h_heads, h_lens, mode_has_thresholds(mode) ? h_thr : nullptr, original_r, info, which, why))
        return fail(MOVI_ERR_ARG, std::string(which == kRlbwtHeads ? "h_heads: " : which == kRlbwtLens ? "h_lens: " : "h_thr: ") + why);
    HIP_TRY(hipSetDevice(device));
    const int rc = build_from_rlbwt(mode, h_heads, h_lens, mode_has_thresholds(mode) ? h_thr : nullptr, original_r, info, h_image, image_bytes, why);
    return rc == MOVI_OK ? MOVI_OK : fail(rc, why);
}

// ------------------------------------------------------------- the run-length BWT and index.movi from a text (movi_walk_text.hip)

namespace {
int text_build_checked(int device, const uint8_t *h_text, uint64_t n, const movi_text_build_opts_t *opts, bool with_thr,
                       uint8_t **heads, uint64_t **lens, uint64_t **thr, uint64_t *original_r, movi_text_build_stats_t *stats) {
    std::string why;
    if (!text_check(h_text, n, why)) return fail(MOVI_ERR_ARG, why);         // before any device call
    HIP_TRY(hipSetDevice(device));
    TextBuildStats st;
    const int rc = rlbwt_from_text(h_text, n, with_thr, opts ? opts->lcp_chunk : 0u, opts && opts->verify != 0u,
                                   opts ? opts->max_device_bytes : 0ull, heads, lens, thr, original_r, st, why);
    if (stats) {
        stats->n_positions = st.n_positions; stats->original_r = st.original_r; stats->device_bytes = st.device_bytes;
        stats->rounds = st.rounds; stats->verified = st.verified;
        for (int k = 0; k < 6; k++) stats->seconds[k] = st.seconds[k];
    }
    return rc == MOVI_OK ? MOVI_OK : fail(rc, why);
}
}  // namespace

int movi_text_device_bytes(uint64_t n, uint64_t *bytes) {
    if (!bytes) return fail(MOVI_ERR_ARG, "bytes is NULL");
    *bytes = 0;
    if (n == 0 || n > kTextMaxChars) return fail(MOVI_ERR_ARG, "n is " + std::to_string(n) + ": 1 .. " + std::to_string(kTextMaxChars) + " characters are served");
    *bytes = text_device_bytes(n + 1);
    return MOVI_OK;
}

int movi_rlbwt_from_text(int device, const uint8_t *h_text, uint64_t n, const movi_text_build_opts_t *opts, uint8_t **h_heads,
                         uint64_t **h_lens, uint64_t **h_thr, uint64_t *original_r, movi_text_build_stats_t *stats) {
    if (h_heads) *h_heads = nullptr;
    if (h_lens) *h_lens = nullptr;
    if (h_thr) *h_thr = nullptr;
    if (original_r) *original_r = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!h_heads) return fail(MOVI_ERR_ARG, "h_heads is NULL");
    if (!h_lens) return fail(MOVI_ERR_ARG, "h_lens is NULL");
    if (!h_thr) return fail(MOVI_ERR_ARG, "h_thr is NULL");
    if (!original_r) return fail(MOVI_ERR_ARG, "original_r is NULL");
    return text_build_checked(device, h_text, n, opts, true, h_heads, h_lens, h_thr, original_r, stats);
}

int movi_build_from_text(int device, uint32_t mode, const uint8_t *h_text, uint64_t n, const movi_text_build_opts_t *opts,
                         void **h_image, size_t *image_bytes, movi_text_build_stats_t *stats) {
    if (h_image) *h_image = nullptr;
    if (image_bytes) *image_bytes = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!h_image) return fail(MOVI_ERR_ARG, "h_image is NULL");
    if (!image_bytes) return fail(MOVI_ERR_ARG, "image_bytes is NULL");
    if (!mode_supported(mode)) return fail(MOVI_ERR_ARG, "mode " + std::to_string(mode) + " is not supported");
    uint8_t *heads = nullptr;
    uint64_t *lens = nullptr, *thr = nullptr, R = 0;
    const bool with_thr = mode_has_thresholds(mode);
    int rc = text_build_checked(device, h_text, n, opts, with_thr, &heads, &lens, &thr, &R, stats);
    if (rc == MOVI_OK) {
        RlbwtInfo info;
        RlbwtArray which;
        std::string why;
        if (!rlbwt_check(heads, lens, thr, R, info, which, why)) rc = fail(MOVI_ERR_ARG, "h_text: its run-length BWT is out of the table builder's scope: " + why);
        else {
            rc = build_from_rlbwt(mode, heads, lens, thr, R, info, h_image, image_bytes, why);
            if (rc != MOVI_OK) rc = fail(rc, why);
        }
    }
    for (void *p : {(void *)heads, (void *)lens, (void *)thr})
        if (p) (void)hipHostFree(p);
    return rc;
}

int movi_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return fail(MOVI_ERR_ARG, "NULL or empty range");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return MOVI_OK;
}

int movi_host_unregister(void *p) {
    if (!p) return MOVI_OK;
    HIP_TRY(hipHostUnregister(p));
    return MOVI_OK;
}

// Page-locks a caller's pageable range for the duration of one big *_host call ("host_autopin"); releases it on scope exit.
struct AutoPin {
    void *p = nullptr;
    bool pin(void *q, size_t bytes) {                        // true: the range is page-locked now (by us or already)
        if (!q || !bytes) return false;
        // page-locked already only if BOTH ends are (a caller -- or another thread's call on an adjacent slice of the same
        // buffer -- may have registered part of the span); a partly registered span cannot be registered again: synchronous path
        const bool first = is_pinned(q), last = is_pinned(static_cast<char *>(q) + bytes - 1);
        if (first && last) return true;
        if (first || last) return false;
        if (hipHostRegister(q, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        p = q;
        return true;
    }
    ~AutoPin() {
        if (!p) return;
        const std::string keep = g_err;
        (void)hipHostUnregister(p);
        (void)hipGetLastError();
        g_err = keep;
    }
};

// A caller's buffer and the part of it one call touches.
struct HostSpan {
    const void *buf = nullptr, *from = nullptr;
    size_t bytes = 0;
};
// A *_host call's plan in its two steps (movi_host_plan.hpp), with the acts between them: the runtime is asked which buffers are
// page-locked -- only where the answer matters -- and page-locks for the call (`pins`, released by the entry point's scope) what
// the plan finds worth trying.
static HostCall plan_call(const movi_index *ix, HostFacts f, const HostSpan &reads, const HostSpan &vector, AutoPin (&pins)[2]) {
    const HostOptions o = host_options(ix);
    f.reads_pinned = overlap_possible(f) && is_pinned(reads.buf);
    f.vector_pinned = f.reads_pinned && needs_pinned_vector(f, o) && is_pinned(vector.buf);
    HostCall call = plan_host_call(f, o);
    call.settle(call.pin_reads && pins[0].pin(const_cast<void *>(reads.from), reads.bytes) &&
                (!call.pin_vector || pins[1].pin(const_cast<void *>(vector.from), vector.bytes)));
    return call;
}
// every query but PML / ZML: only the reads matter; `small_bytes` of per-read results are page-locked per read of a chunk in flight
static HostCall plan_reads_call(const movi_index *ix, HostQuery query, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                                   size_t small_bytes, bool want_vector, AutoPin (&pins)[2]) {
    HostFacts f;
    f.query = query;
    f.total = h_offsets[n_reads] - h_offsets[0];
    f.n_reads = n_reads;
    f.want_vector = want_vector;
    f.small_bytes = small_bytes;
    return plan_call(ix, f, HostSpan{h_bases, h_bases ? h_bases + h_offsets[0] : nullptr, (size_t)f.total}, HostSpan{}, pins);
}

// What the host's worker threads expand: a chunk's reset-mask words into its part of the caller's vector (`out` is the whole call's).
static ExpandJob expand_job(const uint32_t *words, const uint64_t *h_offsets, const HostChunk &c, uint16_t *out) {
    ExpandJob j;
    j.words = words; j.offs = h_offsets; j.o0 = c.b0; j.phase = c.phase; j.ibase = c.first; j.i0 = c.first; j.i1 = c.first + c.nr;
    j.out = out;
    return j;
}

// h_mask_words != NULL: the reset masks themselves are the result (movi_pml_mask_host).  Otherwise, PML with "host_masks": the
// walk writes masks, only they cross PCIe (1/8 byte per base instead of 2) and the u16 vector is expanded into the caller's buffer
// by the host's worker threads (movi_expand_host.cpp) -- in the overlapped path beside the walks of the chunks that follow.
// A chunk's reset-mask words have arrived in its slot's page-locked block (host function on the chunk's stream: no HIP call in here).
struct DeliverArg {
    const uint32_t *words = nullptr;
    uint32_t *mask_dst = nullptr;     // movi_pml_mask_host: where the words belong in the caller's array
    size_t mask_bytes = 0;
    bool expand = false;              // movi_pml_host: the worker pool expands them into the caller's vector
    ExpandJob job;
    int threads = 0;
    HostPool::Group *group = nullptr;
};
static void deliver_on_stream(void *p) {
    DeliverArg *a = static_cast<DeliverArg *>(p);
    if (a->mask_dst) memcpy(a->mask_dst, a->words, a->mask_bytes);
    if (a->expand) expand_parallel(a->job, a->threads, a->group);
    delete a;
}

static int ml_host(bool zml, movi_index_t *ix, const ReadSource &src, const uint64_t *h_offsets, uint64_t n_reads,
                  uint16_t *h_out_pml, uint8_t *h_read_err, movi_query_stats_t *stats, uint32_t *h_mask_words = nullptr) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MOVI_OK; }
    // h_out_pml == NULL: the walk runs, error bytes and counters come back, the vectors stay on the device and are dropped
    // (`movi query --no-output`: the reference computes and discards)
    if (!h_offsets || (h_offsets[n_reads] != h_offsets[0] && !(src.two_bit ? src.packed : src.ascii))) return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    if (src.two_bit) {                                        // the exception list is the caller's too: all of it, before the device is touched
        if (src.n_exc && (!src.exc_pos || !src.exc_byte)) return fail(MOVI_ERR_ARG, "NULL exception list");
        if (!exceptions_in_order(src.exc_pos, src.n_exc, h_offsets[0], h_offsets[n_reads]))
            return fail(MOVI_ERR_ARG, "exception positions are not strictly ascending inside [offsets[0], offsets[n_reads])");
    }
    HIP_TRY(hipSetDevice(ix->device));
    const uint64_t o0 = h_offsets[0], span = h_offsets[n_reads] - o0;
    // The call's way down (the u16 vector as it is, as reset masks that the host expands, or both side by side), whether it overlaps and
    // every chunk's own way: movi_host_plan.hpp
    HostFacts facts;
    facts.zml = zml;
    facts.total = span;
    facts.n_reads = n_reads;
    facts.want_vector = h_out_pml != nullptr;
    facts.want_words = h_mask_words != nullptr;
    AutoPin pins[2];
    const HostCall call = plan_call(ix, facts, HostSpan{src.two_bit ? src.packed : src.ascii, src.up_from(o0), src.up_bytes(o0, span)},
                                    HostSpan{h_out_pml, h_out_pml ? h_out_pml + o0 : nullptr, (size_t)span * 2}, pins);
    const int threads = ix->host_threads > 0 ? ix->host_threads : host_threads_default();
    auto launch = [&](ChunkCtx &c, const HostChunk &k, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        MlRequest r = c.request(k, db, dof, derr);
        if (k.masks) {
            r.mask.phase = k.phase;
            HIP_TRY(c.alloc(movi_index::kMask, (size_t)pml_mask_words(k.nr, k.nb, k.phase) * 4, &r.mask.words));
            return pml_call(ix, r);
        }
        HIP_TRY(c.alloc(movi_index::kOut, k.nb * 2, &r.out));
        if (zml) return zml_call(ix, r);
        r.lend_masks = true;      // (the vector itself comes down: on the device it is written through reset masks where the plan says so)
        return pml_call(ix, r);
    };
    // a chunk's mask words in the layout of movi_pml_mask_words: how many, and where they belong in the caller's array
    auto n_words = [](const HostChunk &k) { return (size_t)(((k.nb + k.phase) >> 5) + k.nr); };
    auto words_dst = [&](const HostChunk &k) { return h_mask_words + ((k.b0 - o0) >> 5) + k.first; };
    // what a chunk's masks are to the host: the words land in `words`; they are the result, or the vector is expanded from them
    auto deliver = [&](const uint32_t *words, const HostChunk &k, HostPool::Group *g) {
        if (h_mask_words) memcpy(words_dst(k), words, n_words(k) * 4);
        if (h_out_pml) expand_parallel(expand_job(words, h_offsets, k, h_out_pml), threads, g);
    };
    // (the results are found through the chunk's own staging: with chunks in flight, launch() of the next chunk has
    // run before fetch() of this one)
    std::vector<uint32_t> sync_words;                        // synchronous path: a chunk's words on their way through the host
    auto fetch = [&](ChunkCtx &c, const HostChunk &k) -> int {
        if (k.masks) {
            const size_t nw = n_words(k);
            if (c.async) {
                // into the slot's page-locked block, and on to the worker pool by a host function on the chunk's stream -- the moment the
                // words have arrived, not when the calling thread's loop next comes by (with 8 chunks per call the pool ran at 2/3 duty)
                HIP_TRY(c.down_small(nullptr, 0, c.d[movi_index::kMask].ptr(), nw * 4));
                DeliverArg *a = new DeliverArg;
                a->words = reinterpret_cast<const uint32_t *>(c.h_small);
                a->mask_dst = h_mask_words ? words_dst(k) : nullptr;
                a->mask_bytes = nw * 4;
                a->expand = h_out_pml != nullptr;
                a->job = expand_job(a->words, h_offsets, k, h_out_pml);
                a->threads = threads;
                a->group = c.grp;
                const hipError_t eh = hipLaunchHostFunc(c.s, deliver_on_stream, a);
                if (eh != hipSuccess) { delete a; (void)hipGetLastError(); return MOVI_OK; }   // harvest() does it instead
                c.delivered = true;
                return MOVI_OK;
            }
            if (h_mask_words && !h_out_pml) {                 // straight to where they belong
                HIP_TRY(hipMemcpy(words_dst(k), c.d[movi_index::kMask].ptr(), nw * 4, hipMemcpyDeviceToHost));
                return MOVI_OK;
            }
            sync_words.resize(nw);
            HIP_TRY(hipMemcpy(sync_words.data(), c.d[movi_index::kMask].ptr(), nw * 4, hipMemcpyDeviceToHost));
            deliver(sync_words.data(), k, nullptr);
            return MOVI_OK;
        }
        if (h_out_pml) HIP_TRY(c.down(h_out_pml + k.b0, c.d[movi_index::kOut].ptr(), k.nb * 2));
        return MOVI_OK;
    };
    auto harvest = [&](const uint8_t *h_small, const HostChunk &k, HostPool::Group *g, bool delivered) {
        if (k.masks && !delivered) deliver(reinterpret_cast<const uint32_t *>(h_small), k, g);
    };
    return run_host(ix, call, src, h_offsets, h_read_err, stats, launch, fetch, harvest);
}

// ------------------------------------------------------------- reads packed two bits per base (movi_pack_host.cpp, movi_walk_pack.hip)

int movi_reads_packed_bytes(uint64_t first_base, uint64_t n_bases, uint64_t *bytes) {
    if (!bytes) return fail(MOVI_ERR_ARG, "bytes is NULL");
    if (first_base + n_bases < first_base || first_base + n_bases + 3 < 3) return fail(MOVI_ERR_ARG, "first_base + n_bases overflows");
    *bytes = packed_bytes(first_base, n_bases);
    return MOVI_OK;
}

// (movi_reads_pack_host / movi_reads_unpack_host: pure host code, exported by movi_pack_host.cpp itself; their messages come through set_last_error)

// Two kernels on `stream` and nothing else: no allocation, no wait, capturable.  The exception list lives on the device, so it is
// not validated here: the kernel leaves a position outside the range alone.
int movi_reads_unpack_device(int device, const uint8_t *d_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *d_exc_pos,
                             const uint8_t *d_exc_byte, uint64_t n_exc, uint8_t *d_bases_out, void *stream) {
    if ((n_bases && (!d_packed || !d_bases_out)) || (n_exc && (!d_exc_pos || !d_exc_byte))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (first_base + n_bases < first_base || first_base + n_bases + 3 < 3) return fail(MOVI_ERR_ARG, "first_base + n_bases overflows");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_unpack_reads(d_packed, first_base, n_bases, d_exc_pos, d_exc_byte, n_exc, first_base, d_bases_out, static_cast<hipStream_t>(stream)));
    return MOVI_OK;
}

int movi_pml_packed_host(movi_index_t *ix, const uint8_t *h_packed, const uint64_t *h_exc_pos, const uint8_t *h_exc_byte, uint64_t n_exc,
                         const uint64_t *h_offsets, uint64_t n_reads, uint16_t *h_out_pml, uint8_t *h_read_err, movi_query_stats_t *stats) {
    return ml_host(false, ix, ReadSource(h_packed, h_exc_pos, h_exc_byte, n_exc), h_offsets, n_reads, h_out_pml, h_read_err, stats);
}

int movi_pml_mask_packed_host(movi_index_t *ix, const uint8_t *h_packed, const uint64_t *h_exc_pos, const uint8_t *h_exc_byte, uint64_t n_exc,
                              const uint64_t *h_offsets, uint64_t n_reads, uint32_t *h_mask_words, uint8_t *h_read_err,
                              movi_query_stats_t *stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads && !h_mask_words) return fail(MOVI_ERR_ARG, "NULL host buffer");
    return ml_host(false, ix, ReadSource(h_packed, h_exc_pos, h_exc_byte, n_exc), h_offsets, n_reads, nullptr, h_read_err, stats, h_mask_words);
}

int movi_pml_mask_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                       uint32_t *h_mask_words, uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (n_reads && !h_mask_words) return fail(MOVI_ERR_ARG, "NULL host buffer");
    return ml_host(false, ix, h_bases, h_offsets, n_reads, nullptr, h_read_err, stats, h_mask_words);
}

// Pure host code: no device is touched.
int movi_pml_expand_host(const uint32_t *h_mask_words, const uint64_t *h_offsets, uint64_t n_reads, uint16_t *h_out_pml,
                         int n_threads) {
    if (n_reads == 0) return MOVI_OK;
    if (!h_mask_words || !h_offsets || (h_offsets[n_reads] != h_offsets[0] && !h_out_pml)) return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HostChunk all;                                           // the whole call as one chunk
    all.nr = n_reads; all.b0 = h_offsets[0]; all.nb = h_offsets[n_reads] - h_offsets[0];
    expand_parallel(expand_job(h_mask_words, h_offsets, all, h_out_pml), n_threads, nullptr);
    return MOVI_OK;
}

int movi_pml_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                  uint16_t *h_out_pml, uint8_t *h_read_err, movi_query_stats_t *stats) {
    return ml_host(false, ix, h_bases, h_offsets, n_reads, h_out_pml, h_read_err, stats);
}

// `movi query --logs`: PMLs plus, per base, the fast-forwards and scan rows MoveQuery::add_fastforward / add_scan
// collect (ClsArgs::log_ff / log_scan).  Synchronous path, first kernel.
int movi_pml_logs_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                       uint16_t *h_out_pml, uint16_t *h_fastforwards, uint16_t *h_scans, uint8_t *h_read_err,
                       movi_query_stats_t *stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MOVI_OK; }
    if (!h_offsets || !h_fastforwards || !h_scans || (h_offsets[n_reads] != h_offsets[0] && (!h_bases || !h_out_pml)))
        return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HIP_TRY(hipSetDevice(ix->device));
    uint16_t *d_out = nullptr, *d_ff = nullptr, *d_sc = nullptr;
    auto launch = [&](ChunkCtx &c, const HostChunk &k, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        HIP_TRY(c.alloc(movi_index::kOut, k.nb * 2, &d_out));
        HIP_TRY(c.alloc(movi_index::kA, k.nb * 2, &d_ff));
        HIP_TRY(c.alloc(movi_index::kS, k.nb * 2, &d_sc));
        HIP_TRY(hipMemsetAsync(d_ff, 0, k.nb * 2, c.s));               // a read of one base has no LF: its entry stays 0
        HIP_TRY(hipMemsetAsync(d_sc, 0, k.nb * 2, c.s));
        MlRequest r;                                                   // (the handle's segment workspace: logs never reach the segment plan)
        r.bases = db; r.offs = dof; r.n_reads = k.nr; r.n_bases = k.nb; r.out = d_out; r.err = derr; r.stream = c.s;
        r.stats = c.d_stats;
        r.cls.log_ff = d_ff;
        r.cls.log_scan = d_sc;
        return pml_call(ix, r);
    };
    auto fetch = [&](ChunkCtx &c, const HostChunk &k) -> int {
        HIP_TRY(c.down(h_out_pml + k.b0, c.d[movi_index::kOut].ptr(), k.nb * 2));
        HIP_TRY(c.down(h_fastforwards + k.b0, c.d[movi_index::kA].ptr(), k.nb * 2));
        HIP_TRY(c.down(h_scans + k.b0, c.d[movi_index::kS].ptr(), k.nb * 2));
        return MOVI_OK;
    };
    auto harvest = [](const uint8_t *, const HostChunk &, HostPool::Group *, bool) {};
    AutoPin pins[2];
    return run_host(ix, plan_reads_call(ix, HostQuery::kLogs, h_bases, h_offsets, n_reads, 0, true, pins), h_bases, h_offsets, h_read_err, stats,
                    launch, fetch, harvest);
}

int movi_zml_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                  uint16_t *h_out_zml, uint8_t *h_read_err, movi_query_stats_t *stats) {
    return ml_host(true, ix, h_bases, h_offsets, n_reads, h_out_zml, h_read_err, stats);
}

// ----------------------------------------------------------------- classification

int movi_classify_device(movi_index_t *ix, const uint16_t *d_pml, const uint64_t *d_offsets, uint64_t n_reads,
                         uint32_t bin_width, uint32_t max_value_thr, uint32_t *d_bins_above, uint32_t *d_bins_below,
                         uint64_t *d_sum_max, void *stream) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) return MOVI_OK;
    if (!d_pml || !d_offsets || !d_bins_above || !d_bins_below || !d_sum_max) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (bin_width == 0) return fail(MOVI_ERR_ARG, "bin_width must be > 0");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(launch_classify(d_pml, d_offsets, n_reads, bin_width, max_value_thr, d_bins_above, d_bins_below, d_sum_max,
                            static_cast<hipStream_t>(stream)));
    return MOVI_OK;
}

constexpr uint64_t kClassifyTwoPassLen = 1024;          // mean read length from which vector + bins run as walk + pass (short reads: fused 71.5 against 63.5 on c2)
static int pml_classify_device(movi_index_t *ix, MlRequest r, uint32_t bin_width, uint32_t max_value_thr, uint32_t *d_bins_above,
                               uint32_t *d_bins_below, uint64_t *d_sum_max) {
    if (bin_width == 0) return fail(MOVI_ERR_ARG, "bin_width must be > 0");
    if (r.n_reads && (!d_bins_above || !d_bins_below || !d_sum_max)) return fail(MOVI_ERR_ARG, "NULL device buffer");
    // When the PML vector is wanted anyway, the bins are cheaper as a second, streaming pass over the resident vectors
    // (classify_kernel: 2 B per base at HBM speed) than fused into the walk: the running bins cost the latency-bound walk
    // ~20 instructions per emission and eight registers -- 100 k x 10 kbp: fused 46.9, walk + pass 53.6 Gbases/s
    // (profiles/r04_classify.txt).  Bins WITHOUT the vector (--classify --filter, --no-output) stay fused: nothing is
    // written at all (60.7).  "classify_fused" 1 / 0 forces either; the pass needs the error bytes (failed reads report
    // no bins), so without d_read_err the fused kernel runs.
    const bool two_pass = r.out != nullptr && r.err != nullptr && r.n_reads != 0 &&
                          (ix ? (ix->cfg.classify_fused == 0 || (ix->cfg.classify_fused < 0 && r.n_bases / r.n_reads >= kClassifyTwoPassLen)) : false);
    if (two_pass) {
        const int rc = pml_call(ix, r);
        if (rc != MOVI_OK) return rc;
        HIP_TRY(launch_classify(r.out, r.offs, r.n_reads, bin_width, max_value_thr, d_bins_above, d_bins_below, d_sum_max, r.stream,
                                r.err, r.n_bases));
        return MOVI_OK;
    }
    r.cls.bin_width = bin_width;
    r.cls.thr = max_value_thr;
    r.cls.above = d_bins_above;
    r.cls.below = d_bins_below;
    r.cls.sum_max = d_sum_max;
    return pml_call(ix, r);
}

int movi_pml_classify_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                             uint64_t n_bases, uint32_t bin_width, uint32_t max_value_thr, uint16_t *d_out_pml,
                             uint32_t *d_bins_above, uint32_t *d_bins_below, uint64_t *d_sum_max, uint8_t *d_read_err,
                             const uint32_t *d_read_order, void *stream) {
    MlRequest r;
    r.bases = d_bases; r.offs = d_offsets; r.n_reads = n_reads; r.n_bases = n_bases;
    r.out = d_out_pml; r.err = d_read_err; r.order = d_read_order; r.stream = static_cast<hipStream_t>(stream);
    return pml_classify_device(ix, r, bin_width, max_value_thr, d_bins_above, d_bins_below, d_sum_max);
}

int movi_pml_classify_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                           uint32_t bin_width, uint32_t max_value_thr, uint32_t *h_bins_above, uint32_t *h_bins_below,
                           uint64_t *h_sum_max, uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MOVI_OK; }
    if (!h_offsets || !h_bins_above || !h_bins_below || !h_sum_max || (h_offsets[n_reads] != h_offsets[0] && !h_bases))
        return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    if (bin_width == 0) return fail(MOVI_ERR_ARG, "bin_width must be > 0");
    HIP_TRY(hipSetDevice(ix->device));
    uint32_t *d_a = nullptr, *d_b = nullptr;
    uint64_t *d_s = nullptr;
    auto launch = [&](ChunkCtx &c, const HostChunk &k, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        HIP_TRY(c.alloc(movi_index::kA, k.nr * 4, &d_a));
        HIP_TRY(c.alloc(movi_index::kB, k.nr * 4, &d_b));
        HIP_TRY(c.alloc(movi_index::kS, k.nr * 8, &d_s));
        // bins reduced inside the PML kernel; no PML vector is written at all
        // (a chunk in flight of the overlapped host path brings its own segment workspace, length hint and the call's probe verdict:
        // without them every chunk fell back to the handle's workspace -- shared by chunks on different streams -- and probed again)
        return pml_classify_device(ix, c.request(k, db, dof, derr), bin_width, max_value_thr, d_a, d_b, d_s);
    };
    // page-locked block of a chunk in flight: sum_max[nr] | above[nr] | below[nr]
    auto fetch = [&](ChunkCtx &c, const HostChunk &k) -> int {
        HIP_TRY(c.down_small(h_sum_max + k.first, 0, c.d[movi_index::kS].ptr(), k.nr * 8));
        HIP_TRY(c.down_small(h_bins_above + k.first, k.nr * 8, c.d[movi_index::kA].ptr(), k.nr * 4));
        HIP_TRY(c.down_small(h_bins_below + k.first, k.nr * 12, c.d[movi_index::kB].ptr(), k.nr * 4));
        return MOVI_OK;
    };
    auto harvest = [&](const uint8_t *h, const HostChunk &k, HostPool::Group *, bool) {
        memcpy(h_sum_max + k.first, h, k.nr * 8);
        memcpy(h_bins_above + k.first, h + k.nr * 8, k.nr * 4);
        memcpy(h_bins_below + k.first, h + k.nr * 12, k.nr * 4);
    };
    AutoPin pins[2];
    return run_host(ix, plan_reads_call(ix, HostQuery::kPerRead, h_bases, h_offsets, n_reads, 16, false, pins), h_bases, h_offsets, h_read_err, stats,
                    launch, fetch, harvest);
}

// -------------------------------------------------------------------------- count

static int count_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                        uint64_t n_bases, uint64_t *d_matched, uint64_t *d_count, uint8_t *d_read_err,
                        const uint32_t *d_read_order, void *stream, DevStats *d_stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) return MOVI_OK;
    if (!d_offsets || !d_matched || !d_count || (n_bases && !d_bases)) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (!d_stats) d_stats = ix->d_stats.get();
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = count_tables(ix, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), s));
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    HIP_TRY(launch_count(ix->kmode, ix->dev, d_bases, d_offsets, n_reads, d_matched, d_count,
                         d_read_err, d_stats, d_read_order, ix->cfg, s, &ix->last_launch, n_bases));
    return MOVI_OK;
}

int movi_count_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                      uint64_t n_bases, uint64_t *d_matched, uint64_t *d_count, uint8_t *d_read_err,
                      const uint32_t *d_read_order, void *stream) {
    return count_device(ix, d_bases, d_offsets, n_reads, n_bases, d_matched, d_count, d_read_err, d_read_order, stream,
                        nullptr);
}

int movi_index_prepare(movi_index_t *ix, uint32_t what, void *stream, uint64_t *derived_bytes) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (what & ~(uint32_t)(MOVI_PREPARE_PML | MOVI_PREPARE_COUNT | MOVI_PREPARE_ZML | MOVI_PREPARE_SA | MOVI_PREPARE_COLOR))
        return fail(MOVI_ERR_ARG, "unknown MOVI_PREPARE_* bit");
    if ((what & MOVI_PREPARE_SA) && !ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    if ((what & MOVI_PREPARE_COLOR) && !ix->d_color_inds) return fail(MOVI_ERR_ARG, kNoColor);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    on_prepare(ix->policy);                                           // an explicit call asks the device now
    if ((what & MOVI_PREPARE_PML) && mode_has_thresholds(ix->desc.mode)) {
        pml_tables(ix, s, true);
        // the walk kernels live in translation units of their own: their code objects are loaded here, not by the first walk
        (void)(ix->dev.idx32 ? preload_walk_u32() : preload_walk_u64());
        (void)(ix->dev.idx32 ? preload_walkseg_u32() : preload_walkseg_u64());
        if (ix->tables.rows4) (void)preload_walk_chain();
        (void)preload_pack();                                        // (movi_reads_unpack_device in front of a captured walk)
        (void)hipGetLastError();
        // movi_pml_device's mask words for a default batch (a bigger "reserve_device_masks" stays): its first call allocates nothing.
        // No room is no failure -- an uncaptured call grows them, a captured one takes the packer route
        if (grow(ix->dmask, (size_t)pml_mask_words(kPrepareMaskReads, kPrepareMaskBases, 0) * 4) != hipSuccess) (void)hipGetLastError();
        // ... and the park queue of the same batch, where calls on this handle can park ("park_lanes"; no room: such calls park nothing)
        if (park_lanes_wanted(ix) > 0 && grow(ix->dpark, park_queue_bytes(kPrepareMaskReads, park_lanes_wanted(ix))) != hipSuccess) (void)hipGetLastError();
    }
    if (what & MOVI_PREPARE_COUNT) {
        const int rc = count_tables(ix, s, true);
        if (rc) return rc;
        (void)preload_kmer_occ(ix->kmode, ix->dev.idx32 != 0);          // (movi_kmer_occ_device captured without a warm-up call)
        (void)hipGetLastError();
    }
    if (what & MOVI_PREPARE_SA) {
        // the sampled suffix array and the locate rows were built when it was attached: only the kernels' code object is loaded here
        (void)preload_sa(ix->kmode, ix->dev.idx32 != 0);
        (void)preload_hits(ix->kmode, ix->dev.idx32 != 0);             // (movi_locate_matches_device captured without a warm-up call)
        (void)hipGetLastError();
    }
    if (what & MOVI_PREPARE_COLOR) {
        // the counter scratch of movi_multi_classify_device and its kernel's code object: the call then allocates nothing
        if (hipError_t e = reserve_color_scratch(ix); e != hipSuccess) return fail_hip(e, "reserving the counter scratch of --multi-classify");
        (void)preload_color(ix->kmode, ix->dev.idx32 != 0);
        (void)hipGetLastError();
    }
    on_prepared(ix->policy);
    // (MOVI_PREPARE_ZML: the parse walks on the plain rows and derives nothing -- accepted so that callers need not know)
    HIP_TRY(hipStreamSynchronize(s));
    if (derived_bytes) {
        double v = 0.0;
        (void)movi_index_info(ix, "derived_bytes", &v);
        *derived_bytes = (uint64_t)v;
    }
    return MOVI_OK;
}

int movi_count_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                    uint64_t *h_matched, uint64_t *h_count, uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return MOVI_OK; }
    if (!h_offsets || !h_matched || !h_count || (h_offsets[n_reads] != h_offsets[0] && !h_bases))
        return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HIP_TRY(hipSetDevice(ix->device));
    uint64_t *d_m = nullptr, *d_c = nullptr;
    auto launch = [&](ChunkCtx &c, const HostChunk &k, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        HIP_TRY(c.alloc(movi_index::kA, k.nr * 8, &d_m));
        HIP_TRY(c.alloc(movi_index::kS, k.nr * 8, &d_c));
        return count_device(ix, db, dof, k.nr, k.nb, d_m, d_c, derr, nullptr, c.s, c.d_stats);
    };
    // page-locked block of a chunk in flight: matched[nr] | count[nr]
    auto fetch = [&](ChunkCtx &c, const HostChunk &k) -> int {
        HIP_TRY(c.down_small(h_matched + k.first, 0, c.d[movi_index::kA].ptr(), k.nr * 8));
        HIP_TRY(c.down_small(h_count + k.first, k.nr * 8, c.d[movi_index::kS].ptr(), k.nr * 8));
        return MOVI_OK;
    };
    auto harvest = [&](const uint8_t *h, const HostChunk &k, HostPool::Group *, bool) {
        memcpy(h_matched + k.first, h, k.nr * 8);
        memcpy(h_count + k.first, h + k.nr * 8, k.nr * 8);
    };
    AutoPin pins[2];
    return run_host(ix, plan_reads_call(ix, HostQuery::kPerRead, h_bases, h_offsets, n_reads, 16, false, pins), h_bases, h_offsets, h_read_err, stats,
                    launch, fetch, harvest);
}

// -------------------------------------------------------------------------- MEM

static_assert(sizeof(movi_mem_t) == sizeof(MemOut) && sizeof(movi_mem_t) == 16, "movi_mem_t and MemOut differ");

}  // extern "C"

namespace {

// complement codes of the handle's alphabet: byte c = code_of[complement(alphabet[c])], 0xFF where that base is not in it
uint64_t complement_codes(const movi_index_desc_t &d) {
    uint64_t comp = ~0ull;
    for (uint32_t c = 0; c < d.alphabet_size && c < 8; c++) {
        const uint8_t ch = d.alphabet[c];
        const uint8_t cc = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : 0;
        const uint64_t v = cc ? d.code_of[cc] : 0xFFu;
        comp &= ~(0xFFull << (8 * c));
        comp |= v << (8 * c);
    }
    return comp;
}

int mem_device(movi_index *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
               uint32_t min_len, movi_mem_t *d_mems, uint32_t *d_n_mems, uint8_t *d_read_err, const uint32_t *d_read_order,
               hipStream_t s) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) return MOVI_OK;
    if (!d_offsets || !d_n_mems || (n_bases && (!d_bases || !d_mems))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    HIP_TRY(hipSetDevice(ix->device));
    int rc = count_tables(ix, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ix->d_stats.get(), 0, sizeof(DevStats), s));
    MemArgs a{};
    a.comp = complement_codes(ix->desc);
    a.min_len = min_len > 1u ? min_len : 1u;
    HIP_TRY(launch_mem(ix->kmode, ix->dev, a, d_bases, d_offsets, n_reads, reinterpret_cast<MemOut *>(d_mems), d_n_mems,
                       d_read_err, ix->d_stats.get(), d_read_order, s, &ix->last_launch));
    return MOVI_OK;
}

}  // namespace

extern "C" {

int movi_mem_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                    uint32_t min_len, movi_mem_t *d_mems, uint32_t *d_n_mems, uint8_t *d_read_err,
                    const uint32_t *d_read_order, void *stream) {
    return mem_device(ix, d_bases, d_offsets, n_reads, n_bases, min_len, d_mems, d_n_mems, d_read_err, d_read_order,
                      static_cast<hipStream_t>(stream));
}

int movi_mem_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t min_len,
                  uint32_t *h_n_mems, movi_mem_t *h_mems, uint64_t mems_cap, uint64_t *n_mems_total,
                  uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_mems_total) *n_mems_total = 0;
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (n_reads == 0) return MOVI_OK;
    if (!h_offsets || !h_n_mems || (h_offsets[n_reads] != h_offsets[0] && !h_bases) || (mems_cap && !h_mems))
        return fail(MOVI_ERR_ARG, "NULL host buffer");
    const CompactOut out{sizeof(movi_mem_t), h_mems, mems_cap, n_mems_total, h_n_mems, false, nullptr, h_read_err, " MEMs found, mems_cap is "};
    return run_compact(ix, h_bases, h_offsets, n_reads, out, stats,
                       [&](const uint8_t *db, const uint64_t *dof, uint64_t nr, uint64_t nb, void *d_out, uint32_t *d_n, uint8_t *d_err) {
                           return mem_device(ix, db, dof, nr, nb, min_len, static_cast<movi_mem_t *>(d_out), d_n, d_err, nullptr, nullptr);
                       });
}

// -------------------------------------------------------------------------- k-mers

static_assert(sizeof(movi_kmer_run_t) == sizeof(KmerRun) && sizeof(movi_kmer_run_t) == 8, "movi_kmer_run_t and KmerRun differ");

}  // extern "C"

namespace {

// The look-ahead's split for this k ("kmer_lookahead").  A look takes the k - step left bases of a window and pays only if it
// dies; a window that holds a substituted base still occurs by chance with probability ~ n / 4^length, so a look shorter than
// log4(n) + 2 bases (chance 1/16) mostly passes and is wasted: -1 picks step = min(k / 2, k - that length), none if k is too short
// (measured, profiles/kmer_bench.txt: at k = 31 on a 640 Mbase text the split k / 2 beats k / 3 and no look-ahead by 1.6x and
// 2.5x; at k = 15 any look-ahead is 1.9 - 2.2x slower than none).
uint32_t kmer_look_step(uint32_t k, uint64_t n, int policy) {
    if (policy == 0) return 0u;
    if (policy > 0) return k / (uint32_t)policy;
    uint32_t need = 2;                                   // ceil(log4(n)) + 2
    for (uint64_t v = 1; v < n && need < 64; v <<= 2) need += 1;
    if (k <= need) return 0u;
    return std::min(k / 2u, k - need);
}

int kmer_device(movi_index *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint32_t k,
                movi_kmer_run_t *d_runs, uint32_t *d_n_runs, uint32_t *d_found, uint8_t *d_read_err, const uint32_t *d_read_order,
                hipStream_t s) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (k == 0) return fail(MOVI_ERR_ARG, "k must be at least 1");
    if (n_reads == 0) return MOVI_OK;
    if (!d_offsets || !d_n_runs || (n_bases && (!d_bases || !d_runs))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    HIP_TRY(hipSetDevice(ix->device));
    int rc = count_tables(ix, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ix->d_stats.get(), 0, sizeof(DevStats), s));
    KmerArgs a{};
    a.k = k;
    a.step = kmer_look_step(k, ix->desc.length, ix->cfg.kmer_lookahead);
    HIP_TRY(launch_kmer(ix->kmode, ix->dev, a, d_bases, d_offsets, n_reads, reinterpret_cast<KmerRun *>(d_runs), d_n_runs, d_found,
                        d_read_err, ix->d_stats.get(), d_read_order, s, &ix->last_launch));
    return MOVI_OK;
}

}  // namespace

extern "C" {

int movi_kmer_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                     uint32_t k, movi_kmer_run_t *d_runs, uint32_t *d_n_runs, uint32_t *d_found, uint8_t *d_read_err,
                     const uint32_t *d_read_order, void *stream) {
    return kmer_device(ix, d_bases, d_offsets, n_reads, n_bases, k, d_runs, d_n_runs, d_found, d_read_err, d_read_order,
                       static_cast<hipStream_t>(stream));
}

int movi_kmer_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t k,
                   uint32_t *h_n_runs, uint32_t *h_found, movi_kmer_run_t *h_runs, uint64_t runs_cap, uint64_t *n_runs_total,
                   movi_query_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_runs_total) *n_runs_total = 0;
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (k == 0) return fail(MOVI_ERR_ARG, "k must be at least 1");
    if (n_reads == 0) return MOVI_OK;
    if (!h_offsets || !h_n_runs || (h_offsets[n_reads] != h_offsets[0] && !h_bases) || (runs_cap && !h_runs))
        return fail(MOVI_ERR_ARG, "NULL host buffer");
    const CompactOut out{sizeof(movi_kmer_run_t), h_runs, runs_cap, n_runs_total, h_n_runs, true, h_found, nullptr, " runs found, runs_cap is "};
    return run_compact(ix, h_bases, h_offsets, n_reads, out, stats,
                       [&](const uint8_t *db, const uint64_t *dof, uint64_t nr, uint64_t nb, void *d_out, uint32_t *d_n, uint8_t *d_err) {
                           return kmer_device(ix, db, dof, nr, nb, k, static_cast<movi_kmer_run_t *>(d_out), d_n, d_n + nr, d_err, nullptr, nullptr);
                       });
}

}  // extern "C"

// -------------------------------------------------------------------------- k-mer occurrences

namespace {

int kmer_occ_device(movi_index *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint32_t k,
                    uint64_t *d_occ, uint32_t *d_found, uint64_t *d_sum, uint8_t *d_read_err, hipStream_t s, DevStats *d_stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (k == 0) return fail(MOVI_ERR_ARG, "k must be at least 1");
    if (n_reads == 0) return MOVI_OK;
    if (!d_offsets || (n_bases && (!d_bases || !d_occ))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    HIP_TRY(hipSetDevice(ix->device));
    if (!d_stats) d_stats = ix->d_stats.get();
    int rc = count_tables(ix, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), s));
    HIP_TRY(launch_kmer_occ(ix->kmode, ix->dev, k, d_bases, d_offsets, n_reads, n_bases, d_occ, d_found, d_sum, d_read_err, d_stats,
                            ix->cfg.num_cus, s, &ix->last_launch));
    return MOVI_OK;
}

}  // namespace

extern "C" {

int movi_kmer_occ_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                         uint32_t k, uint64_t *d_occ, uint32_t *d_found, uint64_t *d_sum, uint8_t *d_read_err, void *stream) {
    return kmer_occ_device(ix, d_bases, d_offsets, n_reads, n_bases, k, d_occ, d_found, d_sum, d_read_err, static_cast<hipStream_t>(stream),
                           nullptr);
}

int movi_kmer_occ_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t k,
                       uint64_t *h_occ, uint32_t *h_found, uint64_t *h_sum, uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (k == 0) return fail(MOVI_ERR_ARG, "k must be at least 1");
    if (n_reads == 0) return MOVI_OK;
    if (!h_offsets || (h_offsets[n_reads] != h_offsets[0] && (!h_bases || !h_occ))) return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HIP_TRY(hipSetDevice(ix->device));
    uint64_t *d_occ = nullptr, *d_sum = nullptr;
    uint32_t *d_found = nullptr;
    auto launch = [&](ChunkCtx &c, const HostChunk &k_, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        HIP_TRY(c.alloc(movi_index::kS, k_.nb * 8, &d_occ));
        if (h_found) HIP_TRY(c.alloc(movi_index::kA, k_.nr * 4, &d_found));
        if (h_sum) HIP_TRY(c.alloc(movi_index::kB, k_.nr * 8, &d_sum));
        return kmer_occ_device(ix, db, dof, k_.nr, k_.nb, k, d_occ, h_found ? d_found : nullptr, h_sum ? d_sum : nullptr, derr, c.s, c.d_stats);
    };
    auto fetch = [&](ChunkCtx &c, const HostChunk &k_) -> int {
        HIP_TRY(c.down(h_occ + (k_.b0 - h_offsets[0]), d_occ, k_.nb * 8));
        if (h_found) HIP_TRY(c.down(h_found + k_.first, d_found, k_.nr * 4));
        if (h_sum) HIP_TRY(c.down(h_sum + k_.first, d_sum, k_.nr * 8));
        return MOVI_OK;
    };
    auto harvest = [](const uint8_t *, const HostChunk &, HostPool::Group *, bool) {};
    AutoPin pins[2];                                         // (kKmerOcc: chunk by chunk, synchronously)
    return run_host(ix, plan_reads_call(ix, HostQuery::kKmerOcc, h_bases, h_offsets, n_reads, 0, false, pins), h_bases, h_offsets, h_read_err,
                    stats, launch, fetch, harvest);
}

}  // extern "C"

// -------------------------------------------------------------------------- locate (sampled suffix array)

namespace {

void drop_ssa(movi_index *ix) {
    ix->d_loc.reset();
    ix->d_samples.reset();
    ix->sa_rate = 0;
}

LocArgs loc_args(const movi_index *ix) {
    LocArgs a;
    a.rows = ix->d_loc.get();
    a.samples = ix->d_samples.get();
    a.n = ix->desc.length;
    a.n_entries = ix->desc.length / ix->sa_rate + 1;
    a.rate = (uint32_t)ix->sa_rate;
    return a;
}

// The locate rows for `rate` and room for the samples; on success the array is attached (its entries still to be filled).
int attach_ssa(movi_index *ix, uint64_t rate, hipStream_t s) {
    if (rate == 0) return fail(MOVI_ERR_ARG, "the sample rate must be at least 1");
    if (rate > (1ull << 24)) return fail(MOVI_ERR_ARG, "sample rates above 2^24 are not supported (the locate rows keep the remainder in 24 bits)");
    if (ix->desc.r + 1 > 0x7FFFFFFFull)
        return fail(MOVI_ERR_ARG, "a sampled suffix array cannot be attached to a table of 2^31 - 1 rows or more yet (the prefix sum over the row "
                                  "lengths is one 32-bit-indexed device scan)");
    drop_ssa(ix);
    const uint64_t entries = ix->desc.length / rate + 1;
    DevPtr<uint4> loc;
    DevPtr<uint64_t> samples;
    hipError_t e = dev_alloc(loc, locate_rows_bytes(ix->desc.r));
    if (e == hipSuccess) e = dev_alloc(samples, entries * 8);
    uint64_t n_total = 0;
    if (e == hipSuccess) e = build_locate_rows(ix->kmode, ix->dev, rate, loc.get(), &n_total, s);
    if (e != hipSuccess) return fail_hip(e, "building the locate rows");                        // an error, never a walk without them
    if (n_total != ix->desc.length)
        return fail(MOVI_ERR_INVARIANT, "the row lengths add up to " + std::to_string(n_total) + ", the index header says " + std::to_string(ix->desc.length));
    ix->d_loc = std::move(loc);
    ix->d_samples = std::move(samples);
    ix->sa_rate = rate;
    return MOVI_OK;
}

int locate_device(movi_index *ix, uint64_t *d_pos, uint64_t n_items, hipStream_t s, DevStats *d_stats, bool clear_stats) {
    if (clear_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), s));
    HIP_TRY(launch_locate(ix->kmode, ix->dev, loc_args(ix), d_pos, n_items, d_stats, ix->cfg.num_cus, s, &ix->last_launch));
    return MOVI_OK;
}

int sa_entries_device(movi_index *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint16_t *d_pml,
                      uint64_t *d_sa, uint8_t *d_err, const uint32_t *d_order, hipStream_t s, DevStats *d_stats) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!mode_has_thresholds(ix->desc.mode))
        return fail(MOVI_ERR_ARG, "--sa-entries rides on the PML walk, which needs thresholds: use a *-thresholds index");
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    if (n_reads == 0) return MOVI_OK;
    if (!d_offsets || (n_bases && (!d_bases || !d_sa))) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    HIP_TRY(hipSetDevice(ix->device));
    if (!d_stats) d_stats = ix->d_stats.get();
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), s));
    LaunchInfo pos_info;
    HIP_TRY(launch_sa_pos(ix->dev, d_bases, d_offsets, n_reads, d_pml, d_sa, d_err, d_stats, d_order, s, &pos_info));
    if (n_bases == 0) { ix->last_launch = pos_info; return MOVI_OK; }
    return locate_device(ix, d_sa, n_bases, s, d_stats, false);
}

bool read_exact(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

}  // namespace

extern "C" {

int movi_ssa_build(movi_index_t *ix, uint64_t rate, void *stream) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = attach_ssa(ix, rate, s)) return rc;
    uint32_t bad = 0;
    HIP_TRY(hipMemsetAsync(ix->d_stats.get(), 0, sizeof(DevStats), s));
    const hipError_t e = build_sampled_sa(ix->kmode, ix->dev, loc_args(ix), ix->d_samples.get(), ix->d_stats.get(), ix->cfg.num_cus, s, &bad, &ix->last_launch);
    if (e != hipSuccess) { drop_ssa(ix); return fail_hip(e, "building the sampled suffix array"); }
    if (bad) {
        drop_ssa(ix);
        return fail(MOVI_ERR_INVARIANT, "the sampled positions do not form one cycle under LF (" + std::to_string(bad) + " finding(s)): corrupt index?");
    }
    return MOVI_OK;
}

int movi_ssa_get(const movi_index_t *ix, uint64_t *rate, uint64_t *h_samples, uint64_t cap, uint64_t *n_samples) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    const uint64_t entries = ix->desc.length / ix->sa_rate + 1;
    if (rate) *rate = ix->sa_rate;
    if (n_samples) *n_samples = entries;
    if (!h_samples) return MOVI_OK;
    if (cap < entries) return fail(MOVI_ERR_ARG, "the sampled suffix array has " + std::to_string(entries) + " entries, cap is " + std::to_string(cap));
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipMemcpy(h_samples, ix->d_samples.get(), entries * 8, hipMemcpyDeviceToHost));
    return MOVI_OK;
}

int movi_ssa_save(movi_index_t *ix, const char *path) {
    if (!ix || !path) return fail(MOVI_ERR_ARG, "NULL argument");
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    HIP_TRY(hipSetDevice(ix->device));
    const uint64_t entries = ix->desc.length / ix->sa_rate + 1, r = ix->desc.r;
    std::vector<uint64_t> buf(entries);
    HIP_TRY(hipMemcpy(buf.data(), ix->d_samples.get(), entries * 8, hipMemcpyDeviceToHost));
    const std::string tmp = std::string(path) + ".tmp";                // renamed over `path` once complete: no partial ssa.movi
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(MOVI_ERR_IO, std::string("cannot write ") + tmp);
    // serialize_sampled_SA, src/move_structure_io.cpp:710-722
    bool ok = fwrite(&ix->sa_rate, 8, 1, f) == 1 && fwrite(&entries, 8, 1, f) == 1 && fwrite(buf.data(), 8, entries, f) == entries &&
              fwrite(&r, 8, 1, f) == 1;
    constexpr uint64_t kPiece = 1ull << 22;                            // all_p back out of the locate rows, piece by piece
    DevPtr<uint64_t> piece;
    hipError_t e = ok ? dev_alloc(piece, std::min(r, kPiece) * 8) : hipSuccess;
    buf.resize(std::min(r, kPiece));
    for (uint64_t first = 0; ok && e == hipSuccess && first < r; first += kPiece) {
        const uint64_t cnt = std::min(kPiece, r - first);
        e = locate_rows_all_p(ix->d_loc.get(), first, cnt, ix->sa_rate, piece.get(), nullptr);
        if (e == hipSuccess) e = hipMemcpy(buf.data(), piece.get(), cnt * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) ok = fwrite(buf.data(), 8, cnt, f) == cnt;
    }
    piece.reset();
    ok = (fclose(f) == 0) && ok;
    if (e == hipSuccess && ok) ok = std::rename(tmp.c_str(), path) == 0;
    else (void)std::remove(tmp.c_str());
    if (e != hipSuccess) return fail_hip(e, "reading the locate rows back");
    if (!ok) return fail(MOVI_ERR_IO, std::string("writing ") + path + " failed");
    return MOVI_OK;
}

int movi_ssa_load(movi_index_t *ix, const char *path) {
    if (!ix || !path) return fail(MOVI_ERR_ARG, "NULL argument");
    FILE *f = fopen(path, "rb");
    if (!f)       // deserialize_sampled_SA, src/move_structure_io.cpp:724-730
        return fail(MOVI_ERR_IO, std::string("Failed to open sampled SA entries file at ") + path + "\nBuild the sampled SA by running the build-SA command.");
    uint64_t rate = 0, entries = 0, r = 0;
    std::vector<uint64_t> samples;
    bool ok = read_exact(f, &rate, 8) && read_exact(f, &entries, 8);
    const bool shape = ok && rate != 0 && entries == ix->desc.length / rate + 1;
    if (shape) {
        samples.resize(entries);
        ok = read_exact(f, samples.data(), entries * 8) && read_exact(f, &r, 8);
        if (ok && r == ix->desc.r) {                                   // all_p[r] follows and ends the file (its values are not read)
            const long at = ftell(f);
            ok = at >= 0 && fseek(f, 0, SEEK_END) == 0 && (uint64_t)ftell(f) == (uint64_t)at + r * 8;
        }
    }
    fclose(f);
    if (!ok) return fail(MOVI_ERR_FORMAT, std::string(path) + " is truncated");
    if (!shape) return fail(MOVI_ERR_FORMAT, std::string(path) + ": rate " + std::to_string(rate) + " with " + std::to_string(entries) +
                                                 " entries does not fit a text of " + std::to_string(ix->desc.length) + " positions");
    if (r != ix->desc.r) return fail(MOVI_ERR_FORMAT, std::string(path) + " was built for an index of " + std::to_string(r) + " rows, this one has " + std::to_string(ix->desc.r));
    HIP_TRY(hipSetDevice(ix->device));
    // (the file's all_p is not read: the locate rows hold the same prefix sums, recomputed from the table on the device)
    if (int rc = attach_ssa(ix, rate, nullptr)) return rc;
    const hipError_t e = hipMemcpy(ix->d_samples.get(), samples.data(), entries * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) { drop_ssa(ix); return fail_hip(e, "uploading the sampled suffix array"); }
    return MOVI_OK;
}

int movi_locate_device(movi_index_t *ix, uint64_t *d_positions_inout, uint64_t n_items, void *stream) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    if (n_items == 0) return MOVI_OK;
    if (!d_positions_inout) return fail(MOVI_ERR_ARG, "NULL device buffer");
    HIP_TRY(hipSetDevice(ix->device));
    return locate_device(ix, d_positions_inout, n_items, static_cast<hipStream_t>(stream), ix->d_stats.get(), true);
}

int movi_sa_entries_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                           uint16_t *d_out_pml, uint64_t *d_out_sa, uint8_t *d_read_err, const uint32_t *d_read_order, void *stream) {
    return sa_entries_device(ix, d_bases, d_offsets, n_reads, n_bases, d_out_pml, d_out_sa, d_read_err, d_read_order,
                             static_cast<hipStream_t>(stream), nullptr);
}

int movi_sa_entries_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint16_t *h_out_pml,
                         uint64_t *h_out_sa, uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!mode_has_thresholds(ix->desc.mode))
        return fail(MOVI_ERR_ARG, "--sa-entries rides on the PML walk, which needs thresholds: use a *-thresholds index");
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    if (n_reads == 0) return MOVI_OK;
    if (!h_offsets || (h_offsets[n_reads] != h_offsets[0] && (!h_bases || !h_out_sa))) return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HIP_TRY(hipSetDevice(ix->device));
    uint16_t *d_pml = nullptr;
    uint64_t *d_sa = nullptr;
    auto launch = [&](ChunkCtx &c, const HostChunk &k, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        if (h_out_pml) HIP_TRY(c.alloc(movi_index::kOut, k.nb * 2, &d_pml));
        HIP_TRY(c.alloc(movi_index::kS, k.nb * 8, &d_sa));
        return sa_entries_device(ix, db, dof, k.nr, k.nb, h_out_pml ? d_pml : nullptr, d_sa, derr, nullptr, c.s, c.d_stats);
    };
    auto fetch = [&](ChunkCtx &c, const HostChunk &k) -> int {
        if (h_out_pml) HIP_TRY(c.down(h_out_pml + k.b0, d_pml, k.nb * 2));
        HIP_TRY(c.down(h_out_sa + k.b0, d_sa, k.nb * 8));
        return MOVI_OK;
    };
    auto harvest = [](const uint8_t *, const HostChunk &, HostPool::Group *, bool) {};
    AutoPin pins[2];                                         // (kSaEntries: chunk by chunk, synchronously)
    return run_host(ix, plan_reads_call(ix, HostQuery::kSaEntries, h_bases, h_offsets, n_reads, 0, h_out_pml != nullptr, pins), h_bases, h_offsets,
                    h_read_err, stats, launch, fetch, harvest);
}

}  // extern "C"

// -------------------------------------------------------------------------- locate count and MEM hits

static_assert(sizeof(movi_match_t) == sizeof(HitsItem) && sizeof(movi_match_t) == 12, "movi_match_t and HitsItem differ");

namespace {

// A host call's chunks: about kHitsChunkBases bases of reads ("pipe_chunk_bases" where that is set) and at most kHitsChunkItems items
// (always whole reads: a read's items stay together); a chunk's positions are staged for kHitsChunkPositions of them and the chunk is
// run again with room for its total where that is more.
constexpr uint64_t kHitsChunkBases = 1ull << 26;
constexpr uint64_t kHitsChunkItems = 1ull << 22;
constexpr uint64_t kHitsChunkPositions = 1ull << 24;

int locate_matches_device(movi_index *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, const movi_match_t *d_items,
                          uint64_t n_items, uint32_t max_occ, uint64_t *d_occ, uint64_t *d_first, uint64_t *d_positions, uint64_t positions_cap,
                          uint8_t *d_item_err, void *d_work, uint64_t work_bytes, hipStream_t s) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (max_occ == 0) return fail(MOVI_ERR_ARG, "max_occ must be at least 1");
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    if (n_items >= kHitsMaxItems) return fail(MOVI_ERR_ARG, "2^31 - 1 items or more in one call (their prefix sum is one 32-bit-indexed device scan)");
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    if (!d_first || !d_work || (n_items && (!d_items || !d_occ || !d_offsets || (n_reads && !d_bases))) || (positions_cap && !d_positions))
        return fail(MOVI_ERR_ARG, "NULL device buffer");
    const uint64_t need = hits_work_layout(n_items).total;
    if (work_bytes < need)
        return fail(MOVI_ERR_ARG, "d_work holds " + std::to_string(work_bytes) + " bytes, " + std::to_string(n_items) + " items need " +
                                      std::to_string(need) + " (movi_locate_matches_work_bytes)");
    HIP_TRY(hipSetDevice(ix->device));
    int rc = count_tables(ix, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ix->d_stats.get(), 0, sizeof(DevStats), s));
    HIP_TRY(launch_locate_matches(ix->kmode, ix->dev, loc_args(ix), d_bases, d_offsets, n_reads, reinterpret_cast<const HitsItem *>(d_items), n_items,
                                  max_occ, d_occ, d_first, d_positions, positions_cap, d_item_err, d_work, work_bytes, ix->locate_matches_stages,
                                  ix->d_stats.get(), ix->cfg.num_cus, s, &ix->last_launch));
    return MOVI_OK;
}

}  // namespace

extern "C" {

int movi_locate_matches_work_bytes(uint64_t n_items, uint64_t *bytes) {
    if (!bytes) return fail(MOVI_ERR_ARG, "NULL argument");
    if (n_items >= kHitsMaxItems) return fail(MOVI_ERR_ARG, "2^31 - 1 items or more in one call (their prefix sum is one 32-bit-indexed device scan)");
    *bytes = hits_work_layout(n_items).total;
    return MOVI_OK;
}

int movi_locate_matches_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, const movi_match_t *d_items,
                               uint64_t n_items, uint32_t max_occ, uint64_t *d_occ, uint64_t *d_first, uint64_t *d_positions,
                               uint64_t positions_cap, uint8_t *d_item_err, void *d_work, uint64_t work_bytes, void *stream) {
    return locate_matches_device(ix, d_bases, d_offsets, n_reads, d_items, n_items, max_occ, d_occ, d_first, d_positions, positions_cap, d_item_err,
                                 d_work, work_bytes, static_cast<hipStream_t>(stream));
}

int movi_locate_matches_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, const movi_match_t *h_items,
                             uint64_t n_items, uint32_t max_occ, uint64_t *h_occ, uint64_t *h_first, uint64_t *h_positions, uint64_t positions_cap,
                             uint64_t *n_positions_total, uint8_t *h_item_err, movi_query_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_positions_total) *n_positions_total = 0;
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (max_occ == 0) return fail(MOVI_ERR_ARG, "max_occ must be at least 1");
    if (!h_first || (n_items && (!h_items || !h_occ)) || (n_reads && !h_offsets) || (positions_cap && !h_positions))
        return fail(MOVI_ERR_ARG, "NULL host buffer");
    for (uint64_t i = 1; i < n_items; i++)
        if (h_items[i].read < h_items[i - 1].read)
            return fail(MOVI_ERR_ARG, "the items are not ordered by read (item " + std::to_string(i) + ")");
    if (n_reads) {
        if (h_offsets[n_reads] != h_offsets[0] && !h_bases) return fail(MOVI_ERR_ARG, "NULL host buffer");
        if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    }
    if (!ix->sa_rate) return fail(MOVI_ERR_ARG, kNoSsa);
    h_first[0] = 0;
    if (n_items == 0) return MOVI_OK;
    HIP_TRY(hipSetDevice(ix->device));
    DevBuf *d = ix->scratch;
    const uint64_t n_text = ix->desc.length, per_item = std::min<uint64_t>(max_occ, n_text);
    const uint64_t target = ix->pipe_chunk_bases ? ix->pipe_chunk_bases : kHitsChunkBases;
    std::vector<uint64_t> rel;
    std::vector<movi_match_t> items;
    uint64_t total = 0, errors = 0, bad = 0, i0 = 0;
    bool overflow = false;
    // the items of reads at or past n_reads (bad items, the last of the ordered list) go with the last chunk, their read out of its range
    for (uint64_t first = 0; i0 < n_items;) {
        uint64_t last = n_reads, i1 = n_items;
        if (first < n_reads) {
            last = chunk_end(h_offsets, n_reads, first, target, 1, target);
            auto read_lt = [](const movi_match_t &m, uint64_t r) { return (uint64_t)m.read < r; };
            i1 = (uint64_t)(std::lower_bound(h_items + i0, h_items + n_items, last, read_lt) - h_items);
            if (i1 - i0 > kHitsChunkItems) {                 // fewer reads: those that hold the first kHitsChunkItems items, at least one
                last = std::max<uint64_t>(first + 1, h_items[i0 + kHitsChunkItems].read);
                i1 = (uint64_t)(std::lower_bound(h_items + i0, h_items + n_items, last, read_lt) - h_items);
            }
            if (last == n_reads) i1 = n_items;
        }
        if (i1 == i0) { first = last; continue; }            // a stretch of reads without items
        HostChunk c;
        c.first = first; c.nr = last - first;
        c.b0 = c.nr ? h_offsets[first] : 0; c.nb = c.nr ? h_offsets[last] - h_offsets[first] : 0;
        const uint64_t ni = i1 - i0;
        if (ni >= kHitsMaxItems) return fail(MOVI_ERR_ARG, "one read has 2^31 - 1 items or more");
        rel.assign(c.nr + 1, 0);
        if (c.nr) (void)fill_relative_offsets(rel.data(), h_offsets, c);
        items.assign(h_items + i0, h_items + i1);
        for (movi_match_t &m : items) m.read = (uint64_t)m.read < last ? (uint32_t)(m.read - first) : 0xFFFFFFFFu;
        const HitsWorkLayout w = hits_work_layout(ni);
        HIP_TRY(grow(d[movi_index::kBases], std::max<uint64_t>(c.nb, 1)));
        HIP_TRY(grow(d[movi_index::kOffs], (c.nr + 1) * 8));
        HIP_TRY(grow(d[movi_index::kErr], ni));
        HIP_TRY(grow(d[movi_index::kMask], ni * sizeof(movi_match_t)));
        HIP_TRY(grow(d[movi_index::kA], ni * 8));
        HIP_TRY(grow(d[movi_index::kB], (ni + 1) * 8));
        HIP_TRY(grow(d[movi_index::kTmp], w.total));
        if (c.nb) HIP_TRY(hipMemcpy(d[movi_index::kBases].ptr(), h_bases + c.b0, c.nb, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d[movi_index::kOffs].ptr(), rel.data(), (c.nr + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d[movi_index::kMask].ptr(), items.data(), ni * sizeof(movi_match_t), hipMemcpyHostToDevice));
        uint64_t cap = std::min(ni * per_item, kHitsChunkPositions), found = 0;
        DevStats h{};
        for (int pass = 0; pass < 2; pass++) {               // (a second pass only where the chunk's total is above the staging's first size)
            HIP_TRY(grow(d[movi_index::kS], std::max<uint64_t>(cap, 1) * 8));
            int rc = locate_matches_device(ix, d[movi_index::kBases].as<uint8_t>(), d[movi_index::kOffs].as<uint64_t>(), c.nr,
                                           d[movi_index::kMask].as<movi_match_t>(), ni, max_occ, d[movi_index::kA].as<uint64_t>(),
                                           d[movi_index::kB].as<uint64_t>(), d[movi_index::kS].as<uint64_t>(), cap, d[movi_index::kErr].as<uint8_t>(),
                                           d[movi_index::kTmp].ptr(), w.total, nullptr);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(&found, d[movi_index::kB].as<uint64_t>() + ni, 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&h, ix->d_stats.get(), sizeof(h), hipMemcpyDeviceToHost));
            if (found <= cap || overflow || total + found > positions_cap) break;     // (positions that will not be delivered are not staged)
            cap = found;
        }
        HIP_TRY(hipMemcpy(h_occ + i0, d[movi_index::kA].ptr(), ni * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_first + i0, d[movi_index::kB].ptr(), (ni + 1) * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = i0; i <= i1; i++) h_first[i] += total;       // (h_first[i1] is the next chunk's h_first[i0]: written again, the same)
        items.clear();
        {
            std::vector<uint8_t> err(ni);
            HIP_TRY(hipMemcpy(err.data(), d[movi_index::kErr].ptr(), ni, hipMemcpyDeviceToHost));
            for (uint8_t e : err) bad += e == 0xFFu ? 1u : 0u;
            if (h_item_err) memcpy(h_item_err + i0, err.data(), ni);
        }
        if (!overflow && total + found <= positions_cap) {
            if (found) HIP_TRY(hipMemcpy(h_positions + total, d[movi_index::kS].ptr(), found * 8, hipMemcpyDeviceToHost));
        } else overflow = true;
        total += found;
        errors += h.errors;
        if (stats) add_stats(stats, c.nb, h);
        i0 = i1;
        first = last;
    }
    if (n_positions_total) *n_positions_total = total;
    if (overflow) return fail(MOVI_ERR_ARG, std::to_string(total) + " positions listed, positions_cap is " + std::to_string(positions_cap));
    if (errors)
        return fail(MOVI_ERR_INVARIANT, std::to_string(errors) + " item(s) or position(s) hit a move-structure invariant violation (corrupt index?)");
    if (bad) return fail(MOVI_ERR_ARG, std::to_string(bad) + " item(s) address no stretch of a read (0xFF in h_item_err)");
    return MOVI_OK;
}

}  // extern "C"

// -------------------------------------------------------------------------- Movi Color (default colour mode)

namespace {

void drop_color(movi_index *ix) {
    ix->d_color_flat.reset();
    ix->d_color_inds.reset();
    ix->color_flat.clear();
    ix->color_inds.clear();
    ix->color_taxa.clear();
    ix->color_species = 0;
}

// ix->color_flat / color_inds / color_species are set: check them and put them on the device
int attach_color(movi_index *ix, const char *what) {
    const uint64_t fs = ix->color_flat.size();
    for (uint64_t i = 0; i < ix->color_inds.size(); i++) {               // every run's set lies inside the table and names known documents
        const uint64_t at = ix->color_inds[i];
        bool ok = at < fs && at + 1 + ix->color_flat[at] <= fs;
        for (uint64_t k = 0; ok && k < ix->color_flat[at]; k++) ok = ix->color_flat[at + 1 + k] < ix->color_species;
        if (!ok) {
            drop_color(ix);
            return fail(MOVI_ERR_FORMAT, std::string(what) + ": the document set of run " + std::to_string(i) + " does not lie inside the flat colour table "
                                         "or names a document beyond num_species");
        }
    }
    DevPtr<uint16_t> flat;
    DevPtr<uint64_t> inds;
    hipError_t e = dev_alloc(flat, std::max<size_t>(fs * 2, 8));
    if (e == hipSuccess) e = dev_alloc(inds, ix->color_inds.size() * 8);
    if (e == hipSuccess) e = hipMemcpy(flat.get(), ix->color_flat.data(), fs * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(inds.get(), ix->color_inds.data(), ix->color_inds.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) { drop_color(ix); return fail_hip(e, "uploading the colour tables"); }
    ix->d_color_flat = std::move(flat);
    ix->d_color_inds = std::move(inds);
    return MOVI_OK;
}

ColorTables color_tables(const movi_index *ix) {
    ColorTables ct;
    ct.flat = ix->d_color_flat.get();
    ct.inds = ix->d_color_inds.get();
    ct.flat_size = ix->color_flat.size();
    ct.num_species = ix->color_species;
    return ct;
}

int multi_classify_device(movi_index *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases, uint32_t min_len,
                          movi_mc_read_t *d_out, uint32_t *d_counts, uint16_t *d_pml, uint8_t *d_err, const uint32_t *d_order, hipStream_t s,
                          DevStats *d_stats, uint32_t *d_scratch = nullptr, size_t scratch_cap = 0) {
    // d_scratch / scratch_cap: counters of the caller's own for a call without counter rows (a chunk of a *_host call, which may run
    // beside other chunks of the same handle); nullptr: the handle's scratch -- one movi_multi_classify_device call at a time
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!mode_has_thresholds(ix->desc.mode))
        return fail(MOVI_ERR_ARG, "--multi-classify is a PML query, which needs thresholds: use a *-thresholds index");
    if (!ix->d_color_inds) return fail(MOVI_ERR_ARG, kNoColor);
    if (min_len > 255u) return fail(MOVI_ERR_ARG, "min_len is a uint8_t in the reference: at most 255");
    if (n_reads == 0) return MOVI_OK;
    if (!d_offsets || !d_out || (n_bases && !d_bases)) return fail(MOVI_ERR_ARG, "NULL device buffer");
    if (n_reads > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 reads in one call");
    HIP_TRY(hipSetDevice(ix->device));
    if (!d_stats) d_stats = ix->d_stats.get();
    const uint64_t S = ix->color_species;
    if (d_scratch && scratch_cap < S * 4) return fail(MOVI_ERR_ARG, "counter scratch smaller than one read's counters");
    if (!d_counts && !d_scratch && ix->color_scratch.cap() < S * 4) {    // not prepared: the scratch is reserved here, outside a capture only
        if (stream_capturing(s)) return fail(MOVI_ERR_ARG, "movi_multi_classify_device under a stream capture needs movi_index_prepare(MOVI_PREPARE_COLOR) first");
        HIP_TRY(reserve_color_scratch(ix));
    }
    // reads go through the counters chunk by chunk: at most "color_scratch_bytes" of them are live at a time
    if (!d_scratch) { d_scratch = ix->color_scratch.as<uint32_t>(); scratch_cap = ix->color_scratch.cap(); }
    const uint64_t budget = d_counts ? std::max<uint64_t>(ix->color_scratch_bytes, S * 4)
                                     : std::min<uint64_t>(scratch_cap, std::max<uint64_t>(ix->color_scratch_bytes, S * 4));
    const uint64_t chunk = std::max<uint64_t>(1, budget / (S * 4));
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), s));
    if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, n_reads * S * 4, s));
    for (uint64_t t0 = 0; t0 < n_reads; t0 += chunk) {
        const uint64_t t1 = std::min(n_reads, t0 + chunk);
        if (!d_counts) HIP_TRY(hipMemsetAsync(d_scratch, 0, (t1 - t0) * S * 4, s));
        HIP_TRY(launch_color(ix->dev, color_tables(ix), min_len, d_bases, d_offsets, t0, t1, d_pml, reinterpret_cast<McRead *>(d_out),
                             d_counts ? d_counts : d_scratch, d_counts != nullptr, d_err, d_stats, d_order, s, &ix->last_launch));
    }
    return MOVI_OK;
}

}  // namespace

extern "C" {

int movi_color_build(movi_index_t *ix, const uint64_t *doc_offsets, const uint32_t *doc_ids, uint64_t n_docs, void *stream) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!doc_offsets || n_docs == 0) return fail(MOVI_ERR_ARG, "no document offsets");
    if (n_docs > 0xFFFFFFFFull) return fail(MOVI_ERR_ARG, "more than 2^32 documents");
    for (uint64_t i = 0; i < n_docs; i++)
        if (doc_offsets[i] <= (i ? doc_offsets[i - 1] : 0))
            return fail(MOVI_ERR_ARG, "the document offsets must be strictly increasing and start above 0 (an empty document at entry " + std::to_string(i) + ")");
    // load_document_info, src/move_structure_io.cpp:659-687: no ids = i + 1; the ids in use, ascending, become 0 .. num_species - 1
    std::vector<uint32_t> raw(n_docs);
    for (uint64_t i = 0; i < n_docs; i++) raw[i] = doc_ids ? doc_ids[i] : (uint32_t)(i + 1);
    std::vector<uint32_t> taxa(raw);
    std::sort(taxa.begin(), taxa.end());
    taxa.erase(std::unique(taxa.begin(), taxa.end()), taxa.end());
    if (taxa.size() > 0xFFFFu) return fail(MOVI_ERR_ARG, "more than 65535 distinct document ids: the colour tables hold documents as uint16_t");
    std::vector<uint16_t> ids(n_docs);
    for (uint64_t i = 0; i < n_docs; i++) ids[i] = (uint16_t)(std::lower_bound(taxa.begin(), taxa.end(), raw[i]) - taxa.begin());
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ix->desc.r + 1 > 0x7FFFFFFFull)
        return fail(MOVI_ERR_ARG, "the colour builder cannot run on a table of 2^31 - 1 rows or more yet (it walks from a sampled suffix array, whose "
                                  "locate rows need one 32-bit-indexed device scan)");
    drop_color(ix);                                                      // (first: a build that fails leaves no tables attached, older ones included)
    if (!ix->sa_rate)                                                    // the text position of every BWT position comes from the samples
        if (int rc = movi_ssa_build(ix, 100, stream)) return rc;
    uint64_t *d_keys = nullptr, n_keys = 0, key_cap = 0;
    uint32_t bad = 0;
    const hipError_t e = build_color_keys(ix->kmode, ix->dev, loc_args(ix), doc_offsets, ids.data(), (uint32_t)n_docs, ix->color_chunk_keys,
                                          ix->cfg.num_cus, s, &d_keys, &n_keys, &bad, &ix->color_chunks, ix->color_seconds, &ix->last_launch, &key_cap);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(MOVI_ERR_HIP, "building the document sets: out of device memory -- the sorted unique (run, document) keys so far (" + std::to_string(n_keys) +
                                      ") and the next stretch of the text do not fit the key budget of " + std::to_string(key_cap) +
                                      " keys (two 8-byte buffers and the sort's scratch within half of the free device memory, at most 2^30 keys)");
    }
    if (e != hipSuccess) return fail_hip(e, "building the document sets");
    if (bad)
        return fail(MOVI_ERR_INVARIANT, "the walks from the sampled suffix array do not visit every BWT position exactly once (" + std::to_string(bad) +
                                            " finding(s)): corrupt index, or a sampled suffix array of another index?");
    DevPtr<uint64_t> keys_owner(d_keys);
    std::vector<uint64_t> keys(n_keys);
    const hipError_t e2 = hipMemcpy(keys.data(), d_keys, n_keys * 8, hipMemcpyDeviceToHost);
    keys_owner.reset();
    if (e2 != hipSuccess) return fail_hip(e2, "reading the document sets back");
    // build_doc_sets, src/move_structure_color.cpp:57-63: a set gets its number at the first run, in run order, that has it -- and
    // flat_and_serialize_colors_vectors, src/move_structure_io.cpp:515-534: sets laid out in that order, size first
    const auto tn = std::chrono::steady_clock::now();
    const uint64_t r = ix->desc.r;
    std::unordered_map<std::string, uint64_t> seen;
    std::vector<uint16_t> flat, docs;
    std::vector<uint64_t> inds(r);
    uint64_t k = 0;
    for (uint64_t i = 0; i < r; i++) {
        docs.clear();
        while (k < n_keys && (keys[k] >> 16) == i) docs.push_back((uint16_t)(keys[k++] & 0xFFFFu));
        if (docs.empty()) return fail(MOVI_ERR_INVARIANT, "run " + std::to_string(i) + " has no document");
        const auto ins = seen.emplace(std::string(reinterpret_cast<const char *>(docs.data()), docs.size() * 2), flat.size());
        if (ins.second) {
            flat.push_back((uint16_t)docs.size());
            flat.insert(flat.end(), docs.begin(), docs.end());
        }
        inds[i] = ins.first->second;
    }
    if (k != n_keys) return fail(MOVI_ERR_INVARIANT, "document keys beyond the last run");
    if (flat.size() >= (1ull << 40)) return fail(MOVI_ERR_ARG, "the flat colour table needs more than 40 bits of offset (MoveTally, include/move_row.hpp:13-26)");
    ix->color_seconds[2] = std::chrono::duration<double>(std::chrono::steady_clock::now() - tn).count();
    ix->color_flat.swap(flat);
    ix->color_inds.swap(inds);
    ix->color_species = (uint32_t)taxa.size();
    if (int rc = attach_color(ix, "movi_color_build")) return rc;
    ix->color_taxa.swap(taxa);
    return MOVI_OK;
}

int movi_color_get(const movi_index_t *ix, uint64_t *flat_size, uint16_t *h_flat, uint64_t flat_cap, uint64_t *h_inds, uint64_t inds_cap,
                   uint32_t *num_species, uint32_t *h_to_taxon_id, uint64_t taxa_cap) {
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (ix->color_inds.empty()) return fail(MOVI_ERR_ARG, kNoColor);
    if (flat_size) *flat_size = ix->color_flat.size();
    if (num_species) *num_species = ix->color_species;
    if ((h_flat && flat_cap < ix->color_flat.size()) || (h_inds && inds_cap < ix->color_inds.size()) || (h_to_taxon_id && taxa_cap < ix->color_taxa.size()))
        return fail(MOVI_ERR_ARG, "a buffer of movi_color_get is too small");
    if (h_flat) memcpy(h_flat, ix->color_flat.data(), ix->color_flat.size() * 2);
    if (h_inds) memcpy(h_inds, ix->color_inds.data(), ix->color_inds.size() * 8);
    if (h_to_taxon_id) memcpy(h_to_taxon_id, ix->color_taxa.data(), ix->color_taxa.size() * 4);
    return MOVI_OK;
}

int movi_color_save(movi_index_t *ix, const char *path) {
    if (!ix || !path) return fail(MOVI_ERR_ARG, "NULL argument");
    if (ix->color_inds.empty()) return fail(MOVI_ERR_ARG, kNoColor);
    // flat_and_serialize_colors_vectors, src/move_structure_io.cpp:542-546: u64 size | u16 flat_colors | r MoveTally (u32 low, u8 high)
    std::vector<uint8_t> tally(ix->color_inds.size() * 5);
    for (uint64_t i = 0; i < ix->color_inds.size(); i++) {
        const uint64_t v = ix->color_inds[i];
        const uint32_t lo = (uint32_t)v;
        memcpy(&tally[i * 5], &lo, 4);
        tally[i * 5 + 4] = (uint8_t)(v >> 32);
    }
    const std::string tmp = std::string(path) + ".tmp";                // renamed over `path` once complete
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(MOVI_ERR_IO, std::string("cannot write ") + tmp);
    const uint64_t fs = ix->color_flat.size();
    bool ok = fwrite(&fs, 8, 1, f) == 1 && fwrite(ix->color_flat.data(), 2, fs, f) == fs && fwrite(tally.data(), 1, tally.size(), f) == tally.size();
    ok = (fclose(f) == 0) && ok;
    if (ok) ok = std::rename(tmp.c_str(), path) == 0;
    else (void)std::remove(tmp.c_str());
    if (!ok) return fail(MOVI_ERR_IO, std::string("writing ") + path + " failed");
    return MOVI_OK;
}

int movi_color_load(movi_index_t *ix, const char *path, uint32_t num_species) {
    if (!ix || !path) return fail(MOVI_ERR_ARG, "NULL argument");
    if (num_species == 0 || num_species > 0xFFFFu) return fail(MOVI_ERR_ARG, "num_species must be between 1 and 65535");
    FILE *f = fopen(path, "rb");
    if (!f)       // deserialize_doc_sets_flat, src/move_structure_io.cpp:587-592
        return fail(MOVI_ERR_IO, std::string("[deserialize doc sets flat] Failed to open document sets flat file at ") + path);
    const uint64_t r = ix->desc.r;
    uint64_t fs = 0;
    bool ok = read_exact(f, &fs, 8);
    ok = ok && fseek(f, 0, SEEK_END) == 0;
    const long end = ok ? ftell(f) : -1;
    const bool shape = ok && end >= 8 && fs < (1ull << 40) && (uint64_t)end == 8 + fs * 2 + r * 5;
    std::vector<uint16_t> flat;
    std::vector<uint8_t> tally;
    if (shape) {
        flat.resize(fs);
        tally.resize(r * 5);
        ok = fseek(f, 8, SEEK_SET) == 0 && read_exact(f, flat.data(), fs * 2) && read_exact(f, tally.data(), r * 5);
    }
    fclose(f);
    if (!ok) return fail(MOVI_ERR_FORMAT, std::string(path) + " is truncated");
    if (!shape) return fail(MOVI_ERR_FORMAT, std::string(path) + ": a flat colour table of " + std::to_string(fs) + " entries and its length do not fit an index of " +
                                                 std::to_string(r) + " rows");
    HIP_TRY(hipSetDevice(ix->device));
    drop_color(ix);
    ix->color_inds.resize(r);
    for (uint64_t i = 0; i < r; i++) {
        uint32_t lo;
        memcpy(&lo, &tally[i * 5], 4);
        ix->color_inds[i] = (uint64_t)lo | ((uint64_t)tally[i * 5 + 4] << 32);
    }
    ix->color_flat.swap(flat);
    ix->color_species = num_species;
    return attach_color(ix, path);
}

int movi_multi_classify_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                               uint32_t min_len, movi_mc_read_t *d_out, uint32_t *d_counts, uint16_t *d_out_pml, uint8_t *d_read_err,
                               const uint32_t *d_read_order, void *stream) {
    return multi_classify_device(ix, d_bases, d_offsets, n_reads, n_bases, min_len, d_out, d_counts, d_out_pml, d_read_err, d_read_order,
                                 static_cast<hipStream_t>(stream), nullptr);
}

int movi_multi_classify_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t min_len,
                             movi_mc_read_t *h_out, uint32_t *h_counts, uint16_t *h_out_pml, uint8_t *h_read_err, movi_query_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ix) return fail(MOVI_ERR_ARG, "index handle is NULL");
    if (!mode_has_thresholds(ix->desc.mode))
        return fail(MOVI_ERR_ARG, "--multi-classify is a PML query, which needs thresholds: use a *-thresholds index");
    if (ix->color_inds.empty()) return fail(MOVI_ERR_ARG, kNoColor);
    if (n_reads == 0) return MOVI_OK;
    if (!h_offsets || !h_out || (h_offsets[n_reads] != h_offsets[0] && !h_bases)) return fail(MOVI_ERR_ARG, "NULL host buffer");
    if (int rc0 = check_offsets(h_offsets, n_reads)) return rc0;
    HIP_TRY(hipSetDevice(ix->device));
    const uint64_t S = ix->color_species;
    movi_mc_read_t *d_o = nullptr;
    uint32_t *d_c = nullptr;
    uint16_t *d_pml = nullptr;
    auto launch = [&](ChunkCtx &c, const HostChunk &k, const uint8_t *db, const uint64_t *dof, uint8_t *derr) -> int {
        const uint64_t nr = k.nr, nb = k.nb;
        HIP_TRY(c.alloc(movi_index::kA, nr * sizeof(movi_mc_read_t), &d_o));
        // the chunk's own counters, from its own staging (chunks of the overlapped path walk side by side): the caller's rows whole,
        // or scratch within "color_scratch_bytes" through which the chunk's reads go in turn
        const size_t cbytes = h_counts ? nr * S * 4 : (size_t)std::min<uint64_t>(nr * S * 4, std::max<uint64_t>(ix->color_scratch_bytes, S * 4));
        HIP_TRY(c.alloc(movi_index::kS, cbytes, &d_c));
        if (h_out_pml) HIP_TRY(c.alloc(movi_index::kOut, nb * 2, &d_pml));
        return multi_classify_device(ix, db, dof, nr, nb, min_len, d_o, h_counts ? d_c : nullptr, h_out_pml ? d_pml : nullptr, derr, nullptr, c.s,
                                     c.d_stats, h_counts ? nullptr : d_c, h_counts ? 0 : cbytes);
    };
    // page-locked block of a chunk in flight: out[nr] | counts[nr * S]
    auto fetch = [&](ChunkCtx &c, const HostChunk &k) -> int {
        const uint64_t first = k.first, nr = k.nr, b0 = k.b0, nb = k.nb;
        HIP_TRY(c.down_small(h_out + first, 0, c.d[movi_index::kA].ptr(), nr * sizeof(movi_mc_read_t)));
        if (h_counts) HIP_TRY(c.down_small(h_counts + first * S, nr * sizeof(movi_mc_read_t), c.d[movi_index::kS].ptr(), nr * S * 4));
        if (h_out_pml) HIP_TRY(c.down(h_out_pml + b0, c.d[movi_index::kOut].ptr(), nb * 2));
        return MOVI_OK;
    };
    auto harvest = [&](const uint8_t *h, const HostChunk &k, HostPool::Group *, bool) {
        const uint64_t first = k.first, nr = k.nr;
        memcpy(h_out + first, h, nr * sizeof(movi_mc_read_t));
        if (h_counts) memcpy(h_counts + first * S, h + nr * sizeof(movi_mc_read_t), nr * S * 4);
    };
    // chunked through the host loop like the count query; overlapped where the reads sit in page-locked memory and no vector comes down
    AutoPin pins[2];
    return run_host(ix, plan_reads_call(ix, HostQuery::kMultiClassify, h_bases, h_offsets, n_reads, sizeof(movi_mc_read_t) + (h_counts ? S * 4 : 0),
                                        h_out_pml != nullptr, pins), h_bases, h_offsets, h_read_err, stats, launch, fetch, harvest);
}

}  // extern "C"
