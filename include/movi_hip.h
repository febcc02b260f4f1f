/*
 * movi_hip.h -- C-ABI of libmovi_hip.so, the MI355X (gfx950) query engine.
 *
 * The reference (mohsenzakeri/Movi) has no FFI seam: its CLI driver calls C++
 * members directly.  This header declares, as plain C, exactly the calls a
 * Movi maintainer would bind in place of those members for the PML / count
 * query path (see INTEGRATION.md for the reference-side stub):
 *
 *   reference member (file:line under /root/reference)           replaced by
 *   ------------------------------------------------------------------------
 *   MoveStructure::deserialize      src/move_structure_io.cpp:471-511   movi_index_load / movi_index_create
 *   std::vector<MoveRow> rlbwt + side tables  include/move_structure.hpp:339-380   movi_index_desc_t
 *   ReadProcessor::process_latency_hiding (PML)  src/read_processor.cpp:641-730   movi_pml_host / movi_pml_device
 *   MoveStructure::query_pml        src/move_structure_query.cpp:234-474  movi_pml_host / movi_pml_device
 *   MoveStructure::query_backward_search  src/move_structure_search.cpp:340-352   movi_count_host / movi_count_device
 *   ReadProcessor::backward_search + compute_match_count  src/read_processor.cpp:610-620,1096-1175   movi_count_host / movi_count_device
 *   Classifier::classify (bins)     src/classifier.cpp:99-143           movi_classify_device / movi_pml_classify_device / movi_pml_classify_host
 *   MoveStructure::query_zml        src/move_structure_query.cpp:690-785  movi_zml_host / movi_zml_device
 *   MoveStructure::query_mems  src/mem_finder.cpp:7-145  movi_mem_host / movi_mem_device
 *   MoveStructure::query_all_kmers  src/sequitur.cpp:322-421  movi_kmer_host / movi_kmer_device
 *   MoveStructure::get_SA_entries  src/move_structure.cpp:35-48  movi_locate_device / movi_sa_entries_host / movi_sa_entries_device
 *   MoveStructure::find_sampled_SA_entries  src/move_structure_build.cpp:1174-1212  movi_ssa_build
 *   MoveStructure::build (--preprocessed)  src/move_structure_build.cpp:17-72, :240-324  movi_build_from_rlbwt
 *   prepare_ref + pfp-thresholds + MoveStructure::build  src/movi_launcher.cpp:190-242, src/prepare_ref.cpp  movi_rlbwt_from_text / movi_build_from_text
 *   MoveStructure::serialize_sampled_SA / deserialize_sampled_SA  src/move_structure_io.cpp:710-744  movi_ssa_save / movi_ssa_load
 *   MoveStructure::build_doc_pats / build_doc_sets  src/move_structure_color.cpp:4-72  movi_color_build
 *   MoveStructure::flat_and_serialize_colors_vectors / deserialize_doc_sets_flat  src/move_structure_io.cpp:513-548,587-607  movi_color_save / movi_color_load
 *   ReadProcessor::process_char (multi-classify)  src/read_processor.cpp:122-186  movi_multi_classify_host / movi_multi_classify_device
 *   MoveQuery::add_ml / matching_lens  include/move_query.hpp:26-38 (filled by process_char, src/read_processor.cpp:193-215)
 *                                                                       movi_pml_mask_device / movi_pml_mask_host (one reset bit per base)
 *                                                                       + movi_pml_expand_device / movi_pml_expand_host (bits -> u16 vector)
 *
 * Conventions: every entry point returns an int status (MOVI_OK == 0) and never
 * throws; movi_last_error() gives the message for the calling thread.  One
 * movi_index_t per GPU; calls on one handle are serialised by the caller;
 * distinct handles may be driven from distinct host threads / processes.
 * Pointers named d_* are device pointers on the handle's GPU, h_* host pointers.
 * No torch / C++ types appear in any signature.
 */
#ifndef MOVI_HIP_H
#define MOVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOVI_OK              0
#define MOVI_ERR_ARG        -1   /* bad argument                                        */
#define MOVI_ERR_FORMAT     -2   /* not a v2 index.movi of mode 5 / 6 / 7 / 8, or unsupported */
#define MOVI_ERR_IO         -3   /* file could not be read                               */
#define MOVI_ERR_HIP        -4   /* a HIP runtime call failed (message has the code)     */
#define MOVI_ERR_NO_DEVICE  -5   /* no usable gfx950 device: there is NO CPU fallback    */
#define MOVI_ERR_INVARIANT  -6   /* a walk hit one of the reference's "this should not
                                    happen" throws (move_structure.cpp:63-65,72-75;
                                    move_structure_query.cpp:582-598); per-read flags say which */

#define MOVI_MODE_REGULAR_THRESHOLDS 6   /* 8-byte rows, include/move_row.hpp:131-142 */
#define MOVI_MODE_BLOCKED_THRESHOLDS 8   /* 6-byte rows, include/move_row.hpp:128-142.  On upload get_id (blocked id + check
                                            point + first_runs, src/move_structure.cpp:91-102) is evaluated once per row and
                                            the rows rewritten in the mode-6 layout: one resident layout, one set of kernels */
#define MOVI_MODE_SAMPLED_THRESHOLDS 7   /* 3-byte rows without ids + sampled id table, move_row.hpp:122-127.  On upload
                                            the ids are recovered once, on the GPU, by MoveStructure::get_id
                                            (src/move_structure.cpp:104-283) and the rows rewritten in the mode-6
                                            layout: queries run the regular-thresholds kernels on identical rows */

#define MOVI_MODE_SAMPLED 5              /* like 7 without thresholds (10-bit lengths, move_row_configs.hpp:107-118).  Count and
                                            ZML queries only: PML on an index without thresholds repositions RANDOMLY in the
                                            reference (reposition_randomly) and is refused (MOVI_ERR_ARG) */

#define MOVI_MODE_REGULAR 3              /* 8-byte rows like 6 with 12-bit lengths and no thresholds (move_row_configs.hpp:21-32):
                                            resident as stored.  Count and ZML only, as for MOVI_MODE_SAMPLED */
#define MOVI_MODE_BLOCKED 2              /* 6-byte rows like 8 with a 24-bit blocked id and no thresholds (:54-75); expanded at
                                            upload to the MOVI_MODE_REGULAR layout.  Count and ZML only */

typedef struct movi_index movi_index_t;

/* The in-memory result of MoveStructure::deserialize for modes 6 / 8: the packed
 * row table (bytes exactly as stored in index.movi) plus the small side tables. */
typedef struct movi_index_desc {
    uint32_t mode;                    /* MOVI_MODE_*                                   */
    uint32_t alphabet_size;           /* <= 4 DNA symbols, or 5 = '%' + ACGT (movi build --separators) */
    uint64_t r;                       /* number of move rows                           */
    uint64_t length;                  /* BWT length n                                  */
    uint64_t end_bwt_idx;             /* row holding the terminator                    */
    uint64_t end_bwt_idx_thresholds[4];
    uint8_t  alphabet[8];             /* code -> ASCII                                 */
    uint8_t  code_of[256];            /* ASCII -> alphamap code (0..3; 1..4 with separators), 0xFF = illegal in a
                                         read (not in the alphabet, or the separator: check_alphabet, move_structure.cpp:383-397) */
    uint64_t first_runs[8], first_offsets[8], last_runs[8], last_offsets[8];  /* k = alphabet_size+1 used */
    uint64_t n_blocks;                /* mode 8: id_blocks is [alphabet_size][n_blocks] */
    uint64_t block_size;              /* mode 8                                        */
    const uint32_t *id_blocks;        /* mode 8, host pointer; NULL for mode 6          */
    /* Separators indexes only (alphabet "%ACGT"): the explicit thresholds of the separator's rows,
     * MoveStructure::separators_thresholds / separators_thresholds_map (include/move_structure.hpp:344-346)
     * exactly as read_separators_thresholds (src/move_structure_io.cpp:415-433) finds them in the file.
     * Host pointers (may be unaligned, into the parsed image); copied by movi_index_create*. */
    uint64_t n_separator_thresholds;
    const void *separator_thresholds;     /* n x ThresholdsRow { uint16_t values[4] }       */
    uint64_t n_separator_map;
    const void *separator_map;            /* n x { uint64_t row, uint64_t entry }           */
    /* Sampled-thresholds indexes only (mode 7): MoveStructure::tally_checkpoints / tally_ids
     * (include/move_structure.hpp:361-363) as read_tally_table (src/move_structure_io.cpp:338-349) finds them:
     * [alphabet_size][n_tally] 5-byte MoveTally entries (u32 low | u8 high, include/move_row.hpp:13-40). */
    uint32_t tally_checkpoints;
    uint32_t reserved_;
    uint64_t n_tally;
    const void *tally_ids;                /* host pointer, may be unaligned                 */
} movi_index_desc_t;

/* Per-query statistics (whole batch), for the algorithmic-bytes formula. */
typedef struct movi_query_stats {
    uint64_t bases;                   /* sum of read lengths                           */
    uint64_t fast_forwards;           /* rows stepped over in fast_forward             */
    uint64_t scans;                   /* rows stepped over in reposition scans / interval shrink */
    uint64_t repositions;             /* bases that took the mismatch branch           */
    uint64_t errors;                  /* reads whose error flag is set                 */
    uint64_t lane_steps;              /* lane state machines only: iterations in which a lane had work ...   */
    uint64_t wave_steps;              /* ... and iterations run by its wavefront: SIMT efficiency =
                                       * lane_steps / (64 * wave_steps); 0 / 0 from the other kernels        */
    uint64_t segments;                /* PML, segment-parallel path ("seg_len"): segments the reads were cut into (0: path not taken) */
    uint64_t rewalked;                /* ... and reads walked again from end to end because a boundary did not fall into step       */
} movi_query_stats_t;

const char *movi_last_error(void);
int movi_version(void);
int movi_device_count(int *count);

/* ---- index ------------------------------------------------------------------ */

/* Parse DIR/index.movi (fallback DIR/movi_index.bin, as
 * src/move_structure_io.cpp:16-32) or the file itself on the host and upload it. */
int movi_index_load(int device, const char *index_dir_or_file, movi_index_t **out);

/* Parse an index.movi image already in host memory (no upload): fills desc and
 * the offset/size of the row table inside the image.  Pure host code. */
int movi_index_parse(const void *h_image, size_t image_bytes, movi_index_desc_t *desc,
                     size_t *rows_offset, size_t *rows_bytes);

/* Upload host tables.  h_rows = r * row_bytes bytes as in the file. */
int movi_index_create(int device, const movi_index_desc_t *desc, const void *h_rows,
                      movi_index_t **out);

/* Adopt a row table that already lives on the device (e.g. received by an RCCL
 * broadcast into a caller-owned buffer).  The caller keeps ownership of d_rows
 * and must keep it alive until movi_index_destroy (modes 7 / 8: the rows are copied
 * -- expanded to the regular-thresholds layout, see MOVI_MODE_SAMPLED_THRESHOLDS --
 * so the buffer may be released after the call). */
int movi_index_create_from_device_rows(int device, const movi_index_desc_t *desc,
                                       const void *d_rows, movi_index_t **out);

/* One index on several GPUs of this node (`movi query --gpus N`; BASELINE north_star: "the shared index broadcast once
 * via RCCL over xGMI").  Replaces N runs of MoveStructure::deserialize (src/move_structure_io.cpp:471-511; the
 * reference has no multi-device form).  The file-format rows (8 / 6 / 3 bytes per row) cross PCIe ONCE, to
 * devices[0]; one RCCL broadcast -- single process: ncclCommInitAll, then ncclBroadcast per device inside
 * ncclGroupStart / ncclGroupEnd, root devices[0] -- carries them to the other GPUs over xGMI; every GPU then builds
 * its own resident layout (blocked / sampled types: expanded on that GPU).  out[i] is the handle on devices[i];
 * devices must be distinct.  n == 1 takes the same path (a communicator of one rank).  librccl.so.1 is bound when the
 * first of these calls is made (dlopen: 570 MB of code objects that the single-GPU paths never need); if it cannot be
 * loaded the call fails with MOVI_ERR_HIP -- there is no fallback to N uploads.
 * movi_index_load_replicated: the same from DIR/index.movi (mapped, as movi_index_load). */
int movi_index_replicate(const movi_index_desc_t *desc, const void *h_rows, const int *devices, int n,
                         movi_index_t **out);
int movi_index_load_replicated(const char *index_dir_or_file, const int *devices, int n, movi_index_t **out);

/* Build the handle's derived tables NOW instead of inside the first query: `what` = MOVI_PREPARE_PML (top-of-walk table,
 * 256 MB at K = 12; look-ahead rows, 16 bytes per row, where the device has room for them and half as much again, never more
 * than a quarter of the device by itself; round 6: the deep rows, 21.33 bytes per row, beside them for real-text tables of at most
 * 50 M rows -- "deep_rows") | MOVI_PREPARE_COUNT (row-start checkpoints, 8 bytes per 32 rows; interval table,
 * 256 MB; nothing else: since round 5 the count query's default is the lane state machine on the PLAIN rows -- the look-ahead rows
 * are built for it only under "count_variant" 0, the base-synchronous kernel of rounds 1 - 4, and then where a sample of the table
 * says the search will use them) | MOVI_PREPARE_ZML (nothing: accepted for symmetry).  Honours the options set before it ("kmer_k", "ftab_k", "ahead_rows": a table the caller built or switched
 * off is left alone).  Waits for the builders; *derived_bytes (optional) = bytes of device memory the handle's derived tables
 * hold afterwards (movi_index_info "derived_bytes").  MOVI_PREPARE_PML also reserves the reset-mask words of movi_pml_device's
 * default route ("pml_via_mask") for a batch of up to 2^28 bases in up to 2^22 reads (50 MB; 1 M reads of 150 bp take 23 MB of
 * them; a bigger "reserve_device_masks", before or after, stays).  After it the *_device entry points of those queries allocate
 * nothing and build nothing on this handle (batches of long reads still grow the segment workspace on their first call; an
 * uncaptured movi_pml_device call on a batch whose mask words outgrow the reservation grows it): they can be captured into a HIP
 * graph without a warm-up call.  A movi_pml_device call made under a stream capture never allocates: a batch whose mask words do
 * not fit takes the route without masks (same answers).  A later growth keeps a mask buffer that a captured call used (movi_index_info
 * "device_scratch_bytes" counts it) until "release_scratch" or movi_index_destroy, so such graphs stay valid until then -- and
 * "release_scratch" invalidates every graph captured on the handle.  A look-ahead copy that was declined for lack of device memory is
 * asked for again by the next movi_index_prepare call only, never from inside a query.  Not calling it is fine: the first query does the
 * same, lazily (and then retries a declined copy every 64 calls). */
#define MOVI_PREPARE_PML 1u
#define MOVI_PREPARE_COUNT 2u
#define MOVI_PREPARE_ZML 4u
#define MOVI_PREPARE_SA 8u     /* locate: loads the kernels of movi_sa_entries_device / movi_locate_device / movi_locate_matches_device.  The sampled suffix array and the
                                  locate rows are built when the array is attached (movi_ssa_build / movi_ssa_load), so a handle without
                                  one is MOVI_ERR_ARG here */
int movi_index_prepare(movi_index_t *ix, uint32_t what, void *stream, uint64_t *derived_bytes);

int movi_index_destroy(movi_index_t *ix);
int movi_index_get_desc(const movi_index_t *ix, movi_index_desc_t *desc);   /* id_blocks = NULL */
/* Device pointer + size of the resident row table.  Mode 6: the file's bytes.  Modes 7 / 8: the expanded table, r x 8
 * bytes in the regular-thresholds layout (not what movi_index_create_from_device_rows takes for a mode-7 / 8
 * descriptor: broadcast the file bytes for that). */
int movi_index_device_rows(const movi_index_t *ix, const void **d_rows, size_t *bytes);

/* ---- PML -------------------------------------------------------------------- */

/* Reads are the concatenated ASCII bases; offsets has n_reads+1 entries (bytes).
 * out_pml[offsets[i] + k] = PML of base (len_i - 1 - k) of read i, i.e. emission
 * order (last base first), the order MoveQuery::matching_lens / the BPF record
 * hold (include/move_query.hpp:26-38, src/utils.cpp:202-246), u16-clamped.
 * d_read_err (optional, n_reads bytes): 0, or the code of the reference throw the walk
 * ran into (1 LF destination >= r, 2 >= 65535 fast-forwards, 3/4 no run below/above);
 * such a read reports all-zero PMLs.
 * d_read_order (optional, n_reads u32): a permutation of the reads; lane slot t works on read
 * d_read_order[t].  Results stay indexed by read.  A hook for callers with their own
 * scheduling; sorting by length measured no gain on MI355X, so the host entry
 * points pass NULL.  At most 2^32 reads per call, each shorter than 2^32 bases.
 * n_bases: the *_device entry points size device scratch from it, so it must be >= offsets[n_reads], and the batch
 * must start at offsets[0] == 0 (pass a sub-batch as its own d_bases / d_offsets / d_out_pml pointers with offsets
 * rebased to 0, not as a window into a larger offsets array).  A batch that breaks this is still answered correctly
 * -- the segment plan checks the offsets on the device and stands down -- but only by one lane per read.
 * Asynchronous on `stream` (a hipStream_t, NULL = the null stream) -- except that a batch of long reads that
 * qualifies for the segment-parallel walk ("seg_len" below) makes the call wait for a short probe of the batch
 * (under a millisecond, a 4-byte read-back) before it enqueues the walk.  Callers that capture the stream into a
 * graph or pipeline several streams set "seg_probe" = 2 and state the verdict themselves ("seg_verdict"): nothing
 * is read back then and the call never waits.  The FIRST PML (count) query on a handle also builds the handle's derived
 * tables -- top-of-walk ("kmer_k") / interval ("ftab_k") table, look-ahead rows ("ahead_rows"): allocations, a few ms of
 * kernels, a wait -- unless those options were set beforehand: make one warm-up call (or set the options) before capturing.
 * One query call per handle at a time: the counters behind movi_last_stats, the segment workspace and what
 * movi_last_launch reports belong to the handle, so two *_device calls on one handle must not be in flight together
 * even on different streams (the *_host entry points pipeline internally with per-chunk copies of all three). */
int movi_pml_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                    uint64_t n_reads, uint64_t n_bases, uint16_t *d_out_pml, uint8_t *d_read_err,
                    const uint32_t *d_read_order, void *stream);

/* Same, host buffers in and out; uploads, runs, downloads, synchronises.
 * stats may be NULL.  With h_bases and h_out_pml in PAGE-LOCKED memory (movi_host_alloc /
 * movi_host_register below) the call is overlapped: the reads are cut into chunks that travel through six
 * slots with their own streams -- up to three chunks going up or being walked while one comes down -- so that
 * upload, walks and download run at the same time (results are identical; DESIGN.md has the rates).  Pageable
 * buffers take the synchronous path -- unless the call is big (>= 2^27 bases and >= 3 x 2^15 reads): then it page-locks the
 * caller's buffers for its duration (hipHostRegister / hipHostUnregister: practically free for touched memory) and overlaps
 * all the same ("host_autopin" 0 turns that off).  h_out_pml == NULL: the walk runs and its error bytes and counters come back,
 * but no vector crosses PCIe (`movi query --no-output`: the reference computes and discards, src/movi.cpp:268-389). */
int movi_pml_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets,
                  uint64_t n_reads, uint16_t *h_out_pml, uint8_t *h_read_err,
                  movi_query_stats_t *stats);

/* `movi query --logs` (src/movi_parser.cpp:95; MoveQuery::add_fastforward / add_scan, include/move_query.hpp:51-53, collected
 * by ReadProcessor::process_char src/read_processor.cpp:99-121 and written by output_logs src/utils.cpp:268-289): the PML
 * query with two more u16 values per base, in emission order like the PMLs -- h_fastforwards[offsets[i] + k] = rows the
 * LF from base k to base k + 1 fast-forwarded over (the read's last entry repeats the one before it, as the reference's
 * strand does when it writes the read out; a read of one base: 0), h_scans[offsets[i] + k] = rows base k's reposition
 * scanned.  Runs the first, base-synchronous kernel: a diagnostic path, not a fast one.  (The third file of --logs, the
 * per-base wall-clock costs of a CPU strand, has no counterpart on a GPU lane; the CLI writes zeros.) */
int movi_pml_logs_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                       uint16_t *h_out_pml, uint16_t *h_fastforwards, uint16_t *h_scans, uint8_t *h_read_err,
                       movi_query_stats_t *stats);

/* Device-side counters of the last movi_pml_device / movi_count_device call on
 * this handle; synchronises `stream` first. */
int movi_last_stats(movi_index_t *ix, void *stream, movi_query_stats_t *stats);

/* What the last query call on this handle launched: which kernel the launch policy picked (the name as rocprofv3
 * prints it, template arguments included) and with which shape.  The policy lives in the library, so measurement code
 * asks instead of assuming (bench.py's roofline.kernel). */
typedef struct movi_launch_info {
    char kernel[96];
    int32_t variant;                  /* PML: 0, 1, 14 ("pml_variant"); ZML: 0, 1; count: 0, 1 ("count_variant")     */
    int32_t block_threads;
    int32_t waves_per_cu;             /* cap on resident wavefronts per CU that was applied (0 = none)             */
    int32_t segmented;                /* 1 = the segment-parallel plan ran around that kernel                       */
    int32_t idx64;                    /* 1 = the 64-bit row-index instantiation                                     */
    int32_t staged;                   /* > 0: every lane keeps the next `staged` bases of its read in LDS ("stage_reads";
                                         336 at the default occupancy cap, 256 on the look-ahead rows); 0: no staging */
    int32_t ahead;                    /* 1 = the walk ran on the look-ahead rows ("ahead_rows"), 2 = on the deep rows ("deep_rows"), 3 = on the chain rows ("chain_rows") */
    int32_t reserved_;
} movi_launch_info_t;
int movi_last_launch(const movi_index_t *ix, movi_launch_info_t *info);
/* Diagnostic (process-wide): the first call switches a log of the walk kernel's launches on; every call copies the DISTINCT
 * kernel names launched since the previous call into buf (one per line, NUL-terminated, truncated to cap) and clears the
 * log; *needed (optional) = bytes a complete copy takes.  Unlike movi_last_launch it sees the K1 / K3 launches of the
 * segment-parallel plan too: tests/test_kernel_coverage_gpu.py holds every instantiation the library was built with to the
 * oracle through it. */
int movi_launch_log(char *buf, size_t cap, size_t *needed);

/* What the handle holds in HBM besides the row table, and what its builders measured (no reference counterpart; the
 * derived tables of "kmer_k" / "ahead_rows" / "ftab_k" are built by the first query that can use them, so this is how a
 * caller sees their cost).  Keys: "rows_bytes" (the resident row table), "kmer_bytes", "ftab_bytes", "ahead_rows_bytes",
 * "ckpt_bytes" (0 = not built), "color_bytes" (attached colour tables), "color_taxa" (to_taxon_id entries held), "color_chunks" and
 * "color_walk_seconds" / "color_sort_seconds" / "color_number_seconds" (the last movi_color_build), "locate_bytes" (the locate rows and the samples of an attached sampled suffix array), "derived_bytes" (their sum), "ahead_no_ff" (share of the table's BWT
 * positions that reach their LF target without a fast-forward, tallied when the look-ahead rows are built: 0.83 on the
 * pangenome BWT, 0.51 on a uniformly random run sequence; -1 = not tallied yet), "device_scratch_bytes" (device scratch the
 * *_device calls hold: movi_pml_device's mask words -- retired buffers that captured graphs may still use included --, the u16 vector
 * of a movi_pml_mask_device call whose path has no mask output, the segment workspace, the park queue), "host_staging_bytes" (the
 * *_host calls' device staging), "park_lanes" (what the last PML call's mask walk parked at: 0 = it parked nothing), "ff_skip" (1 = the last PML call's walk ran with the fast-forward skip), "deep_hint_bits" (width of a
 * reposition hint in the deep rows the handle holds: 4 or 2; 0 = it holds none) and "parked_reads"
 * (reads the last movi_pml_device / movi_pml_mask_device call's first launch handed to its second; waits for the device, so not under a
 * stream capture).  Unknown key: MOVI_ERR_ARG. */
int movi_index_info(const movi_index_t *ix, const char *key, double *value);

/* ---- PML as reset masks (round 6) ----------------------------------------------- */

/* What the PML path PRODUCES is one bit per base.  process_char either increments match_len or zeroes it
 * (src/read_processor.cpp:193-215: match -> match_len + 1; mismatch + reposition or illegal character -> 0) and
 * MoveQuery::add_ml (include/move_query.hpp:26-38) records min(match_len, 65535): PML[k] = reset(k) ? 0 : PML[k - 1] + 1,
 * the run length since the last reset.  These entry points hand over the reset bits instead of the u16 vector -- 1/16 of
 * the bytes over PCIe and into host memory -- and the two expanders turn them back into exactly the vector movi_pml_* write
 * (u16 clamp included; MoveQuery::matching_lens is filled from them: INTEGRATION.md).
 *
 * Layout: 32-bit words.  Bit (k % 32) of word  W(i) + k / 32,  W(i) = ((first_base + offsets[i]) >> 5) - (first_base >> 5) + i,
 * belongs to emission step k of read i (k = 0: the read's LAST base, as in movi_pml_device); 1 = its PML is 0.  Every read
 * starts a word of its own and no prefix sum over the reads is needed (floor((o + l) / 32) + 1 >= floor(o / 32) + ceil(l / 32));
 * bits of a read's last word beyond its length are 0; words between two reads' ranges ("gap words") are unspecified.
 * first_base = position of this batch's first base in the caller's whole read set (0 for a stand-alone batch): consecutive
 * sub-batches of one read set then write word for word what one call over the whole set would -- sub-batch (first read f, first
 * base b) starts at word (b >> 5) + f of the whole.  movi_pml_mask_words: words the batch's array must hold.
 * A read that hit one of the reference's throws (d_read_err) reports every base as a reset, i.e. all-zero PMLs.
 * The default walk writes the words itself (one 4-byte store per 32 bases); batches it hands to another path -- long reads walked
 * segment-parallel, tables of fewer than 8 rows, "stage_reads" 0 -- write their vector to device scratch of the handle (2 bytes per
 * base, grow-only: those calls may allocate) and pack it.  Other arguments and conventions as movi_pml_device. */
int movi_pml_mask_words(uint64_t n_reads, uint64_t n_bases, uint64_t first_base, uint64_t *n_words);
int movi_pml_mask_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                         uint64_t n_reads, uint64_t n_bases, uint64_t first_base, uint32_t *d_mask_words,
                         uint8_t *d_read_err, const uint32_t *d_read_order, void *stream);
/* masks -> the u16 vector of movi_pml_device, on the device (streaming: 2 bytes written per base) */
int movi_pml_expand_device(movi_index_t *ix, const uint32_t *d_mask_words, const uint64_t *d_offsets,
                           uint64_t n_reads, uint64_t n_bases, uint64_t first_base, uint16_t *d_out_pml, void *stream);
/* Host buffers in, masks out: h_mask_words holds movi_pml_mask_words(n_reads, offsets[n_reads] - offsets[0], 0) words, laid out
 * with first_base = 0 relative to offsets[0].  Only 1/8 byte per base comes back over PCIe. */
int movi_pml_mask_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets,
                       uint64_t n_reads, uint32_t *h_mask_words, uint8_t *h_read_err, movi_query_stats_t *stats);
/* masks -> u16 vector on the HOST: pure CPU code (no device needed), n_threads worker threads (0 = three quarters of
 * the CPUs the process may use -- its affinity mask capped by the cgroup's CPU quota --, at most 24).  h_out_pml[offsets[i] + k] as movi_pml_host writes it; offsets need not start at 0 (the masks are laid out
 * relative to offsets[0], as movi_pml_mask_host writes them). */
int movi_pml_expand_host(const uint32_t *h_mask_words, const uint64_t *h_offsets, uint64_t n_reads,
                         uint16_t *h_out_pml, int n_threads);

/* ---- 2-bit packed reads --------------------------------------------------------- */

/* movi_pml_host and movi_pml_mask_host are bound by their upload: one byte per base over PCIe.  Callers that hold their reads
 * packed -- or pack while they parse -- hand them over as they are, a quarter of the bytes, and the
 * GPU unpacks them into the byte per base that every walk stages from.  unpack(pack(x)) == x for every byte value, so every
 * query sees exactly the bytes it would have seen; check_alphabet's verdict on a byte stays where it is, in code_of.
 *
 * The format.  Two bits per base, four bases per byte: base b lives in byte b >> 2 at bits 2 * (b & 3).  The codes are fixed,
 * A = 0, C = 1, G = 2, T = 3, whatever the index's alphabet is.  b is the ABSOLUTE base index, the numbering offsets[] uses:
 * as with h_bases, a call whose offsets[0] is not 0 still indexes the packed buffer from its start.  Reads are not byte-aligned
 * and there is no second offsets array.  Unused bits of the last byte are 0 when written and ignored when read.
 * Every byte that is not upper-case 'A' / 'C' / 'G' / 'T' is an EXCEPTION -- 'N', lower case, '%', '#', bytes >= 128.  In the
 * packed stream an exception has code 0; the sparse list says what it was: exc_pos[m], absolute base indexes, strictly
 * ascending, and exc_byte[m], the original bytes.  The unpackers restore each one exactly.
 * Cost: an exception takes 9 bytes (8 of position, 1 of value) against the 3/4 byte per base that packing saves: beyond about
 * one exception per 36 bases, ASCII input is the smaller upload.
 *
 * movi_reads_packed_bytes: *bytes = (first_base + n_bases + 3) >> 2, what a packed buffer that holds bases [0, first_base +
 * n_bases) takes.
 * movi_reads_pack_host: h_bases[j] is base first_base + j; its code goes to the packed buffer at the absolute position.  Bits
 * of the first byte that belong to bases before first_base are kept (batch after batch is appended to one buffer); bits of the
 * last byte past the range are written 0.  At most exc_cap exceptions are written, *n_exc = how many there are: with more than
 * exc_cap the call returns MOVI_ERR_ARG, *n_exc says what to allocate, and nothing past the caps was written.  Pure host code,
 * n_threads workers on slices aligned to four bases (0 = the default of movi_pml_expand_host; inputs of less than 2^16 bases
 * per worker use fewer).
 * movi_reads_unpack_host: the exact inverse, h_bases_out[j] = base first_base + j.  Exceptions that are not strictly ascending
 * inside [first_base, first_base + n_bases): MOVI_ERR_ARG.
 * movi_reads_unpack_device: the same on the GPU -- the building block for every query: unpack into a buffer of the caller's,
 * then call any *_device entry point on it.  d_packed is indexed like the host buffer, byte b >> 2 from its start, with no
 * alignment asked of it: the kernel fetches the aligned 4-byte words the needed bytes lie in.  d_bases_out needs no alignment
 * either (a 16-byte aligned one leaves in 16-byte stores throughout).  Two kernels on `stream` (a hipStream_t) and nothing
 * else: the call allocates nothing, waits for nothing and can be captured into a graph (movi_index_prepare(MOVI_PREPARE_PML)
 * loads the kernels' code object; otherwise the first call does).  The list lives on the device and is not checked: an
 * exception outside the range is left alone. */
int movi_reads_packed_bytes(uint64_t first_base, uint64_t n_bases, uint64_t *bytes);
int movi_reads_pack_host(const uint8_t *h_bases, uint64_t first_base, uint64_t n_bases, uint8_t *h_packed, uint64_t *h_exc_pos,
                         uint8_t *h_exc_byte, uint64_t exc_cap, uint64_t *n_exc, int n_threads);
int movi_reads_unpack_host(const uint8_t *h_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *h_exc_pos,
                           const uint8_t *h_exc_byte, uint64_t n_exc, uint8_t *h_bases_out, int n_threads);
int movi_reads_unpack_device(int device, const uint8_t *d_packed, uint64_t first_base, uint64_t n_bases, const uint64_t *d_exc_pos,
                             const uint8_t *d_exc_byte, uint64_t n_exc, uint8_t *d_bases_out, void *stream);

/* movi_pml_host / movi_pml_mask_host on packed reads: same chunks, same walks, same way down, same results word for word; only
 * where a chunk's bases come from differs.  The packed bytes that cover a chunk go up -- overlapped when h_packed is page-locked,
 * and big calls on pageable buffers page-lock it for their duration, as for h_bases --, the whole exception list goes up once,
 * and the chunk's stream unpacks into the handle's staging ahead of its walk.  n_exc positions must be strictly ascending and
 * inside [offsets[0], offsets[n_reads]) (MOVI_ERR_ARG, checked before the device is touched).  Other arguments as there. */
int movi_pml_packed_host(movi_index_t *ix, const uint8_t *h_packed, const uint64_t *h_exc_pos, const uint8_t *h_exc_byte,
                         uint64_t n_exc, const uint64_t *h_offsets, uint64_t n_reads, uint16_t *h_out_pml, uint8_t *h_read_err,
                         movi_query_stats_t *stats);
int movi_pml_mask_packed_host(movi_index_t *ix, const uint8_t *h_packed, const uint64_t *h_exc_pos, const uint8_t *h_exc_byte,
                              uint64_t n_exc, const uint64_t *h_offsets, uint64_t n_reads, uint32_t *h_mask_words,
                              uint8_t *h_read_err, movi_query_stats_t *stats);

/* ---- binary classification bins ------------------------------------------------ */

/* The per-read reduction of Classifier::classify (src/classifier.cpp:99-143) over PML vectors
 * that are already on the device: bins of bin_width PMLs in emission order, the last bin
 * absorbing a remainder shorter than bin_width; per read the number of bins whose maximum is
 * >= max_value_thr (bins_above) / below it, and the sum of the bin maxima.  The verdict is
 * FOUND iff bins_above / (bins_above + bins_below) > 0.5; the report's average is
 * sum_max / (bins_above + bins_below).  max_value_thr = max(percentile, 3) + 1 from
 * DIR/movi.pml.nulldb (src/classifier.cpp:30-33). */
int movi_classify_device(movi_index_t *ix, const uint16_t *d_pml, const uint64_t *d_offsets,
                         uint64_t n_reads, uint32_t bin_width, uint32_t max_value_thr,
                         uint32_t *d_bins_above, uint32_t *d_bins_below, uint64_t *d_sum_max,
                         void *stream);

/* PML query with the reduction above FUSED into the walk (each lane keeps its running bin maximum
 * in registers): one kernel, and with d_out_pml == NULL no PML vector is written at all -- what
 * `movi query --classify --filter / --no-output` needs.  d_out_pml != NULL writes the vectors too
 * (`--classify` with BPF output).  Other arguments as movi_pml_device / movi_classify_device. */
int movi_pml_classify_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                             uint64_t n_reads, uint64_t n_bases, uint32_t bin_width,
                             uint32_t max_value_thr, uint16_t *d_out_pml, uint32_t *d_bins_above,
                             uint32_t *d_bins_below, uint64_t *d_sum_max, uint8_t *d_read_err,
                             const uint32_t *d_read_order, void *stream);

/* Host buffers in, bins out (16 bytes back per read instead of 2 per base); uses the fused kernel
 * without a PML vector. */
int movi_pml_classify_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets,
                           uint64_t n_reads, uint32_t bin_width, uint32_t max_value_thr,
                           uint32_t *h_bins_above, uint32_t *h_bins_below, uint64_t *h_sum_max,
                           uint8_t *h_read_err, movi_query_stats_t *stats);

/* ---- count (backward search) -------------------------------------------------- */

/* Per read: matched = len - pos_on_r and count = rows in the last non-empty
 * interval, the two numbers src/utils.cpp:248-256 prints (`--no-prefetch`
 * semantics, src/move_structure_search.cpp:340-352). */
int movi_count_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                      uint64_t n_reads, uint64_t n_bases, uint64_t *d_matched, uint64_t *d_count,
                      uint8_t *d_read_err, const uint32_t *d_read_order, void *stream);

int movi_count_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets,
                    uint64_t n_reads, uint64_t *h_matched, uint64_t *h_count, uint8_t *h_read_err,
                    movi_query_stats_t *stats);

/* ---- MEM finding (maximal exact matches) --------------------------------------- */

/* `movi query --mem`: MoveStructure::query_mems (src/mem_finder.cpp:7-145).
 *
 * Terms.  Read P of length m; minimum length L (-l / --min-mem-length), L' = max(L, 1).  A base is illegal when
 * desc.code_of[byte] == 0xFF (N, lower case, the separator '%', bytes >= 128: check_alphabet, move_structure.cpp:383-397).
 * occ(X) = occurrences of X in the indexed text T (= MoveInterval::count); rc(X) = reverse complement (A<->T, C<->G).
 *   bw[e] = the largest l such that P[e-l+1 .. e] has no illegal base and occ > 0 (a plain backward search);
 *   fw[s] = the largest l such that P[s .. s+l) has no illegal base and occ(rc(P[s .. s+l))) > 0, cnt[s] = that occ
 *           (a backward search over comp(P[s]), comp(P[s+1]), ...: forward_search_step, move_structure_search.cpp:336-338).
 * The search (query_mem_bml, mem_finder.cpp:27-103, over those arrays; for L <= 1 the reference runs query_all_mems,
 * :105-145, whose output on legal reads is this loop with L' = 1):
 *     pos = 0
 *     while pos + L' <= m:
 *         w = pos + L' - 1
 *         if bw[w] < L':  pos = w - bw[w] + 1; continue      # window absent: skip past the failing base
 *         if fw[pos] < L': pos += 1; continue                # cannot happen on a text closed under rc
 *         e = pos + fw[pos]
 *         emit (start = pos, end = e, count = cnt[pos])      # end exclusive, as MoveQuery::add_mem
 *         if e == m: break
 *         pos = max(pos + 1, e - bw[e] + 1)                  # next left end (mem_finder.cpp:83-101)
 * Closed texts: every index `movi build --separators` makes is closed under rc, and so is every single-record index.
 * There the output is exactly the MEMs of length >= L', by increasing start:
 *     { (s, s + fw[s], cnt[s]) : fw[s] >= L', s == 0 or fw[s-1] <= fw[s] }.
 *
 * Where this deviates from the reference:
 *   1. Illegal bases are barriers in both directions: a MEM never contains one.  The reference is not well defined there
 *      (forward_search_step('N') extends with complement('N') == 'A', utils.cpp:87-91; initialize_backward_search on an
 *      illegal base indexes first_runs out of range).  On legal reads the two agree.
 *   2. The reference checks --ftab-k against L (mem_finder.cpp:37-56), and with K > L its size_t / int32_t comparisons let
 *      the left extension run past pos.  Here the answers depend neither on whether an interval table is used nor on its K.
 *   3. On a text that is not closed under rc (a multi-record index built without --separators: its record junctions are
 *      not rc-symmetric) the reference's bidirectional interval (extend_bidirectional, move_structure_search.cpp:66-120) is
 *      meaningless and can throw "reverse complement might not be present" (:254-256).  The answer here is still the loop
 *      above, each side computed by its own backward search.
 *   4. count is the full 64-bit occ.  The reference's mem_t::count is uint16_t, filled by an implicit conversion
 *      (move_query.hpp:42-49), so the reference prints count mod 2^16; the CLI prints that value (its output bytes match).
 *
 * Device layout: MEM j of read i is d_mems[offsets[i] + j] for j < d_n_mems[i] (a read has at most max(0, len - L' + 1)
 * MEMs, so the buffer of offsets[n] entries holds them all; no prefix sum, no atomics, deterministic).  Slots past
 * d_n_mems[i] are unspecified.  Buffers, offsets, d_read_err, d_read_order and the stream as for movi_count_device; a read
 * that hits one of the reference's throws gets d_n_mems[i] = 0 and its error code.  The call uses the count query's derived
 * tables (row-start checkpoints, interval table): after movi_index_prepare(MOVI_PREPARE_COUNT) it allocates and builds
 * nothing and may be captured into a graph without a warm-up call.  movi_last_stats / movi_last_launch report on it. */
typedef struct movi_mem { uint32_t start, end; uint64_t count; } movi_mem_t;    /* 16 bytes, end exclusive */

int movi_mem_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                    uint32_t min_len, movi_mem_t *d_mems, uint32_t *d_n_mems, uint8_t *d_read_err,
                    const uint32_t *d_read_order, void *stream);

/* Host form, compact: h_n_mems[i] per read, and the MEMs of read 0, then read 1, ... in h_mems; *n_mems_total = their sum.
 * mems_cap = offsets[n] - offsets[0] always suffices.  With a smaller cap and more MEMs than fit the call returns
 * MOVI_ERR_ARG and still fills h_n_mems and *n_mems_total (h_mems is then incomplete).  Runs chunk by chunk, synchronously;
 * each chunk is compacted on the device, so only the MEMs found cross the link. */
int movi_mem_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t min_len,
                  uint32_t *h_n_mems, movi_mem_t *h_mems, uint64_t mems_cap, uint64_t *n_mems_total,
                  uint8_t *h_read_err, movi_query_stats_t *stats);

/* ---- k-mer presence ------------------------------------------------------------- */

/* `movi query --kmer [-k K]`: MoveStructure::query_all_kmers / query_kmers_from (src/sequitur.cpp:257-421, the non-count
 * branch) over initialize_backward_search / try_ftab / backward_search (src/move_structure_search.cpp:169-293).
 *
 * Terms.  Read P of length m, k >= 1.  Illegal bases and bw[] as for MEM finding above: bw[e] = the largest l such that
 * P[e-l+1 .. e] has no illegal base and occurs in the indexed text.  The k-mer starting at p (ending at e = p + k - 1) is
 * *found* iff bw[e] >= k.  The reference's walk, with every skipping rule taken out (none of them changes the answer):
 *     e = m - 1
 *     while e >= k - 1:
 *         if bw[e] < k:  e -= 1;  continue
 *         L = e - bw[e] + 1
 *         emit run (start = L, count = bw[e] - k + 1)        # the k-mers starting at L, L + 1, ..., L + count - 1
 *         e = L + k - 2
 *     found = sum of the counts = #{ p : the k-mer at p is found };   all = m - k + 1
 * Runs come out by decreasing start (the order of the reference's "pos:count " string, MoveQuery::add_kmer,
 * include/move_query.hpp:12-19).  A run is greedy, not maximal: it is the longest match ending at the first found end met
 * from the right, and the k-mer ending at L + k - 2 may be found again and start the next run.  The runs of a read are
 * disjoint and cover exactly the found k-mers.
 *
 * Where this deviates from the reference:
 *   1. Illegal bases are barriers.  A read that is empty, all illegal, or whose cursor would run off its left end simply
 *      ends with the runs found so far; the reference reads out of bounds there (query_seq[-1]; the int32_t against size_t
 *      comparison in `while (pos_on_r >= k - 1)`).
 *   2. --ftab-k >= k makes the reference's look-ahead step negative and its ftab skip wrong.  Here the answers depend
 *      neither on whether an interval table is used, nor on its K, nor on which dead ends the kernel skips ("kmer_lookahead").
 *   3. k = 1 follows the loop above (runs = the stretches of legal bases that occur).  The reference special-cases k = 1 and
 *      emits nothing.
 *   4. `all` is not returned: the caller computes m - k + 1 (the reference does so in 64-bit unsigned arithmetic, so a read
 *      shorter than k prints the wrapped value; the CLI prints that).  k = 0 is MOVI_ERR_ARG.
 *
 * Device layout: run j of read i is d_runs[offsets[i] + j] for j < d_n_runs[i] (a read has at most max(0, len - k + 1) runs,
 * so the buffer of offsets[n] entries holds them all; no prefix sum, no atomics, deterministic).  Slots past d_n_runs[i] are
 * unspecified.  d_found[i] = the read's found k-mers (d_found may be NULL).  Buffers, offsets, d_read_err, d_read_order and
 * the stream as for movi_mem_device; a read that hits one of the reference's throws gets d_n_runs[i] = d_found[i] = 0 and its
 * error code.  The call uses the count query's derived tables: after movi_index_prepare(MOVI_PREPARE_COUNT) it allocates and
 * builds nothing and may be captured into a graph without a warm-up call.  movi_last_stats / movi_last_launch report on it
 * (lane_steps = backward-search steps taken, wave_steps = iterations of the wavefronts: what a skipping policy is judged by). */
typedef struct movi_kmer_run { uint32_t start, count; } movi_kmer_run_t;      /* 8 bytes */

int movi_kmer_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                     uint32_t k, movi_kmer_run_t *d_runs, uint32_t *d_n_runs, uint32_t *d_found, uint8_t *d_read_err,
                     const uint32_t *d_read_order, void *stream);

/* Host form, compact: h_n_runs[i] and h_found[i] (may be NULL) per read, and the runs of read 0, then read 1, ... in h_runs;
 * *n_runs_total = their number.  runs_cap = offsets[n] - offsets[0] always suffices.  With a smaller cap and more runs than
 * fit the call returns MOVI_ERR_ARG and still fills h_n_runs, h_found and *n_runs_total (h_runs is then incomplete).  Runs
 * chunk by chunk, synchronously; each chunk is compacted on the device, so only the runs found cross the link.  A read that
 * hits an invariant violation makes the call return MOVI_ERR_INVARIANT (its h_n_runs[i] is 0). */
int movi_kmer_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t k,
                   uint32_t *h_n_runs, uint32_t *h_found, movi_kmer_run_t *h_runs, uint64_t runs_cap, uint64_t *n_runs_total,
                   movi_query_stats_t *stats);

/* ---- k-mer occurrences ------------------------------------------------------------ */

/* `movi query --kmer-occ [-k K]`: how often every k-mer of a read occurs in the indexed text.  This is NOT the reference's
 * --kmer-count (src/sequitur.cpp:14-255: a bidirectional-search experiment on a --separators index that prints two totals and
 * its skipping counters), which stays refused; the contract here is stated on occurrences in the text.
 *
 * Terms.  Read P of length m, k >= 1, all = max(0, m - k + 1).  A base is legal when the search would look it up (A, C, G, T).
 * For 0 <= p < all:
 *     occ[p] = the number of occurrences of P[p .. p+k) in the indexed text   if its k bases are all legal
 *            = 0                                                              otherwise
 * -- the `count` movi_count_device reports for that k-mer as a read of its own when its `matched` is k, and 0 when matched < k.
 * Occurrences across the record junctions of an index built without --separators count, exactly as they do there.
 *     found = #{ p : occ[p] > 0 },   sum = the sum of occ[p] (64 bits).
 * The answers depend neither on whether an interval table is used ("ftab_k"), nor on its K, nor on the row-index width ("idx64").
 *
 * Device layout: d_occ[offsets[i] + p] = occ[p] of read i for p < all; the read's other k - 1 slots are 0, so every one of the
 * n_bases slots is defined.  n_bases must EQUAL offsets[n_reads], as for movi_sa_entries_device.  (The offsets live on the device,
 * so a wrong n_bases cannot be refused; the call stays inside its buffers whatever it is: no slot at or past n_bases is touched, no
 * base there is read, a read that reaches past n_bases gets no k-mer and 0xFF in d_read_err, and slots past offsets[n_reads] are
 * left as they were.)  d_found, d_sum and d_read_err (per read) are each optional.  There is no d_read_order: work is handed out
 * per k-mer, not per read -- a lane owns the slots lane, lane + stride, ... and takes up its next slot when a search ends, like
 * movi_locate_device's lists --, so there is nothing to reorder.
 * A k-mer whose search hits one of the reference's LF throws (a corrupt table) becomes an ERROR SLOT: ~0xFF | the code, bit 63
 * set, which no count has (MOVI_OCC_IS_ERROR); it is counted in movi_last_stats' `errors`, and its read reports that code -- its
 * first error slot's -- in d_read_err[i] and found = sum = 0.  A corrupt table ends the call, it does not hang it.
 * k == 0, NULL required buffers and more than 2^32 reads: MOVI_ERR_ARG.  Asynchronous on `stream`.  The call uses the count query's
 * derived tables only (row-start checkpoints, interval table) and no scratch: after movi_index_prepare(MOVI_PREPARE_COUNT) it
 * allocates and builds nothing and may be captured into a graph without a warm-up call.  movi_last_launch names the occurrence
 * kernel; movi_last_stats: lane_steps = interval steps taken, wave_steps = iterations of the wavefronts (lane_steps /
 * (64 * wave_steps) = the occupancy of the strided lists). */
#define MOVI_OCC_IS_ERROR(v) (((uint64_t)(v) >> 63) != 0)    /* an error slot: ~0xFF | kErr code of the LF move that threw */

int movi_kmer_occ_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                         uint32_t k, uint64_t *d_occ, uint32_t *d_found, uint64_t *d_sum, uint8_t *d_read_err, void *stream);

/* Host form: h_occ in the same layout relative to h_offsets[0] (h_occ[h_offsets[i] - h_offsets[0] + p]); h_found, h_sum and
 * h_read_err per read, each optional.  Runs chunk by chunk through the handle's staging, synchronously, like
 * movi_sa_entries_host (8 bytes per base come down); a chunk is a stretch of reads of about 2^26 bases, or of "pipe_chunk_bases"
 * where that option is set.  A k-mer that became an error slot makes the call return MOVI_ERR_INVARIANT after everything else
 * was answered. */
int movi_kmer_occ_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t k,
                       uint64_t *h_occ, uint32_t *h_found, uint64_t *h_sum, uint8_t *h_read_err, movi_query_stats_t *stats);

/* ---- locate: suffix-array entries from a sampled suffix array ------------------- */

/* `movi build-SA` and `movi query --sa-entries`: where in the indexed text a match lies.
 *
 * Terms.  n = desc.length BWT positions; SA[p] = the text position of the suffix at BWT position p; an LF step goes from the
 * position of text position t to that of t - 1, and from text position 0 to BWT position 0, whose entry is n - 1.  A sampled
 * suffix array of rate R holds SA[0], SA[R], SA[2R], ...: n / R + 1 entries (find_sampled_SA_entries sizes it so; where R
 * divides n the last entry addresses no position and is 0).
 * The entry of a position p (get_SA_entries): d LF steps from p reach the first sampled position q; the answer is SA[q] + d.
 * It is NOT reduced modulo n: with m = the smallest sampled entry, the answer is SA[p] for SA[p] >= m and SA[p] + n below --
 * the walk passed text position 0 and stopped at BWT position 0.  The reference returns the same.
 *
 * A position is a (row, offset) pair packed into one u64 by MOVI_POS_PACK: rows are those of the resident table
 * (movi_index_device_rows), offset < the row's length.  MOVI_POS_NONE is no position: movi_locate_device leaves it as it is.
 *
 * movi_ssa_build: the array for `rate` (1 .. 2^24, else MOVI_ERR_ARG), on the device, from the table alone -- every sampled
 * position walks to the next sampled position down the text (the locate kernel, one LF step taken first), which links the
 * samples into one list from sample 0; ranking that list by pointer jumping gives every entry.  MOVI_ERR_INVARIANT if the list
 * does not visit every sample exactly once (a corrupt table).  Works on every index type.  The call also derives the LOCATE ROWS,
 * 16 bytes per row: the row and the quotient / remainder by `rate` of the BWT position of its first character, so that a locate
 * step is one gather.  Both are counted by movi_index_info "locate_bytes" / "derived_bytes"; failing to allocate them is an error.
 * Attaching an array replaces the one before it and frees that one's samples and locate rows: a graph captured over
 * movi_sa_entries_device / movi_locate_device still points at them and must be captured again, not replayed.  A table of 2^31 - 1
 * rows or more cannot attach an array yet (MOVI_ERR_ARG): the prefix sum over the row lengths is one 32-bit-indexed device scan.
 * Waits for its kernels.
 * movi_ssa_save / movi_ssa_load: INDEX/ssa.movi, byte for byte serialize_sampled_SA's file: u64 rate, u64 count, the entries,
 * u64 r, all_p[r] (the BWT position of every row's first character).  Loading takes the rate from the file, checks the count
 * against the text's length, the trailing r against the index and the file's length against r (MOVI_ERR_FORMAT; all_p itself is
 * recomputed from the table, not read) and derives the locate rows for that rate.  Saving writes PATH.tmp and renames it: a failed
 * save leaves no partial ssa.movi;
 * a missing file is MOVI_ERR_IO with the reference's hint to run build-SA.
 * movi_ssa_get: rate and entry count (either pointer may be NULL), and the entries if h_samples is given (cap < count:
 * MOVI_ERR_ARG). */
#define MOVI_POS_OFFSET_BITS 12
#define MOVI_POS_PACK(row, offset) (((uint64_t)(row) << MOVI_POS_OFFSET_BITS) | (uint64_t)(offset))
#define MOVI_POS_ROW(pos) ((uint64_t)(pos) >> MOVI_POS_OFFSET_BITS)
#define MOVI_POS_OFFSET(pos) ((uint64_t)(pos) & ((1u << MOVI_POS_OFFSET_BITS) - 1u))
#define MOVI_POS_NONE (~(uint64_t)0)

int movi_ssa_build(movi_index_t *ix, uint64_t rate, void *stream);
int movi_ssa_save(movi_index_t *ix, const char *path);
int movi_ssa_load(movi_index_t *ix, const char *path);
int movi_ssa_get(const movi_index_t *ix, uint64_t *rate, uint64_t *h_samples, uint64_t cap, uint64_t *n_samples);

/* In place: d_positions_inout[i] holds a packed position on entry and its suffix-array entry on return.  A lane owns the items
 * lane, lane + stride, ... and takes up its next item when a walk ends, so walks of very different lengths keep the wavefronts
 * full.  An item that is not a position of the table, or whose walk breaks one of the table's invariants (the reference's throws
 * in LF_move; more than n steps), becomes MOVI_POS_NONE and is counted in movi_last_stats' `errors`: a corrupt table ends the
 * call, it does not hang it.  Asynchronous on `stream`; allocates nothing; capturable.  Without an attached sampled suffix
 * array: MOVI_ERR_ARG (the message names build-SA).  movi_last_stats: lane_steps = LF steps taken, wave_steps = iterations of
 * the wavefronts (lane_steps / (64 * wave_steps) = the occupancy of the strided lists). */
int movi_locate_device(movi_index_t *ix, uint64_t *d_positions_inout, uint64_t n_items, void *stream);

/* The PML query that also says where: d_out_sa[offsets[i] + k] = the suffix-array entry of the position the walk stands at after
 * base (len_i - 1 - k) of read i was processed and before the LF step to the next one -- what query_pml hands to get_SA_entries
 * (src/move_structure_query.cpp:354-357), in emission order like the PMLs.  An illegal base leaves the state as it is and still
 * records an entry.  d_out_pml (optional): the PML vector of movi_pml_device.  One lane per read walks the plain rows (no derived
 * table of the PML walk is used) and writes the packed positions into d_out_sa; the locate kernel then turns them into entries
 * in place.  A read that hits one of the reference's throws reports its code in d_read_err, all-zero PMLs and MOVI_POS_NONE in
 * every slot.  *-thresholds indexes only.  Buffers, offsets, d_read_err, d_read_order and the stream as for movi_pml_device, except
 * that n_bases must EQUAL offsets[n_reads]: the locate kernel takes every one of the n_bases slots for a position.
 * With a sampled suffix array attached the call allocates and builds nothing: it may be captured into a graph without a warm-up
 * call (movi_index_prepare(MOVI_PREPARE_SA) loads the kernels beforehand).  Without one: MOVI_ERR_ARG. */
int movi_sa_entries_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                           uint16_t *d_out_pml, uint64_t *d_out_sa, uint8_t *d_read_err, const uint32_t *d_read_order, void *stream);

/* Host buffers in and out (h_out_pml optional), chunk by chunk through the handle's staging, synchronously.  A read or a walk
 * that breaks an invariant makes the call return MOVI_ERR_INVARIANT after everything else was answered. */
int movi_sa_entries_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint16_t *h_out_pml,
                         uint64_t *h_out_sa, uint8_t *h_read_err, movi_query_stats_t *stats);

/* ---- locate count and MEM hits --------------------------------------------------- */

/* `movi query --count --locate` and `movi query --mem --locate`: where in the indexed text a counted match or a MEM lies.
 * Deviates from the reference: there is none -- the reference has no such mode, so the contract is stated on the text itself.
 *
 * Terms.  T is the indexed text of n = desc.length characters, terminator included: every record of the FASTA cleaned (anything but
 * A, C, G, T becomes A) and followed by its reverse complement, with a '%' after each of them in an index built with --separators.
 * A MATCH ITEM is (read, start, end) with 0 <= start < end <= len(read), and X = P[start .. end) of that read P.
 *     occ(X)  = the number of t with T[t .. t + |X|) == X.  Occurrences across the record junctions of an index built without
 *               --separators count, exactly as for the count query.  occ(X) = 0 if X holds an illegal base (not an error).
 *     hits(X) = those t in BWT order, that is, by increasing rank of the suffix T[t ..].
 * With a cap max_occ >= 1 the item reports listed = min(occ, max_occ) and the first `listed` elements of hits(X).
 * Positions lie in [0, n): the "+ n" of get_SA_entries for walks that pass text position 0 (above) does not leak out.
 * The answers depend neither on whether an interval table is used ("ftab_k"), nor on the row-index width ("idx64"), nor on the sample
 * rate of the attached suffix array.
 * (How they come about: the interval [s, e] the backward search over X ends on is the range of BWT positions whose suffix starts with
 * X, so occ = e - s + 1 and hits(X) = SA[s], SA[s + 1], ...; a position's entry is SA[p] or SA[p] + n, so t = entry mod n.)
 *
 * Device form.  d_occ[i] = occ of item i in full 64 bits; d_first[0 .. n_items] = the exclusive prefix sum of `listed`, so
 * d_first[n_items] = the total; the positions of item i are d_positions[d_first[i] .. d_first[i + 1]) as far as they lie below
 * positions_cap.  Slots at or past min(total, positions_cap) are not touched, and a total above the cap is no error of the device
 * call: the caller reads d_first[n_items].  Four steps on `stream`: the interval searches (one lane owns the items lane, lane + stride,
 * ... and takes up its next item when a search ends, like movi_locate_device's lists), a device scan over the n_items + 1 values of
 * `listed` (n_items < 2^31 - 1 per call, else MOVI_ERR_ARG: the scan is 32-bit-indexed), the expansion of the intervals into packed
 * positions, and the locate walks in place on them, which store text positions.  (The walks are movi_locate_device's, in a kernel of
 * this call's own: it reads the number of slots from d_first[n_items] on the device, where that one takes it from the host.)
 * The scan's temporary storage, its input and the per-item intervals live in the caller's d_work, of at least
 * movi_locate_matches_work_bytes(n_items) bytes (host only; about 33 bytes per item).
 * The call is asynchronous on `stream`.  With a sampled suffix array attached and after
 * movi_index_prepare(MOVI_PREPARE_COUNT | MOVI_PREPARE_SA) it allocates and builds nothing and may be captured into a graph without
 * a warm-up call.  Too small a d_work, max_occ == 0, NULL required buffers (d_first and d_work always; d_items, d_occ, d_offsets and
 * d_bases with n_items > 0; d_positions with positions_cap > 0) and no suffix array attached are each MOVI_ERR_ARG; the last names
 * build-SA in its message.
 * A bad item (read >= n_reads, start >= end, end past the read) gets occ = listed = 0 and 0xFF in d_item_err (optional); no byte
 * outside the read is read.  An item whose search hits one of the reference's LF throws gets its kErr* code there and
 * occ = listed = 0; a position whose expansion or locate walk breaks an invariant of the table becomes MOVI_POS_NONE, as in
 * movi_locate_device.  Both are counted in movi_last_stats' `errors`.  A corrupt table ends the call, it does not hang it.
 * movi_last_launch names the last kernel launched (the walk's; the search's when positions_cap is 0). */
typedef struct movi_match { uint32_t read, start, end; } movi_match_t;   /* 12 bytes, end exclusive */

int movi_locate_matches_work_bytes(uint64_t n_items, uint64_t *bytes);   /* host only */

int movi_locate_matches_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                               const movi_match_t *d_items, uint64_t n_items, uint32_t max_occ, uint64_t *d_occ, uint64_t *d_first,
                               uint64_t *d_positions, uint64_t positions_cap, uint8_t *d_item_err, void *d_work, uint64_t work_bytes,
                               void *stream);

/* Host form: h_occ[n_items], h_first[n_items + 1] and the positions of item 0, then item 1, ... in h_positions;
 * *n_positions_total = h_first[n_items].  Items must be ordered by `read`, else MOVI_ERR_ARG, checked on the host before the device
 * is touched.  Runs chunk by chunk through the handle's staging, synchronously, like movi_sa_entries_host; a chunk is a stretch of
 * reads of about 2^26 bases ("pipe_chunk_bases" where that option is set) together with its items, and its reads go up with it --
 * a caller that has just run the count or MEM query on the same reads uploads them a second time, which is accepted: from 10 positions
 * per item on the locate walks are four fifths of the call and more (profiles/locate_matches.txt).  A positions_cap that is too small behaves like mems_cap of movi_mem_host: MOVI_ERR_ARG,
 * with h_occ, h_first and the total still filled (h_positions is then incomplete).  Error items or MOVI_POS_NONE slots make the call
 * return MOVI_ERR_INVARIANT, and bad items (0xFF in h_item_err, optional) MOVI_ERR_ARG, after everything else was answered. */
int movi_locate_matches_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                             const movi_match_t *h_items, uint64_t n_items, uint32_t max_occ, uint64_t *h_occ, uint64_t *h_first,
                             uint64_t *h_positions, uint64_t positions_cap, uint64_t *n_positions_total, uint8_t *h_item_err,
                             movi_query_stats_t *stats);

/* ---- Movi Color: multi-class classification, default colour mode ---------------- */

/* `movi color`, `movi build --color` and `movi query --multi-classify`: which documents (species) a read comes from.
 *
 * Terms.  The indexed text is a concatenation of n_docs documents; doc_offsets[i] is the text position where document i ends
 * (exclusive; DIR/ref.fa.doc_offsets, load_document_info, src/move_structure_io.cpp:643-657).  The document of text position t is the
 * first i with t < doc_offsets[i]; what lies past the last end -- the terminator -- belongs to the last document
 * (build_doc_pats, src/move_structure_color.cpp:4-24).  doc_ids[i] (DIR/ref.fa.doc_ids; NULL: i + 1) is the taxon of document i; the
 * taxa in use, ascending, are numbered 0 .. num_species - 1 and to_taxon_id maps back (:659-687).  The set of a run is the set of
 * numbers of the documents its BWT positions lie in (build_doc_sets, src/move_structure_color.cpp:27-72).
 * The colour tables (flat_and_serialize_colors_vectors, src/move_structure_io.cpp:513-548): flat_colors, u16, every distinct set
 * stored once as its size followed by its sorted members, sets in the order of the first run, in run order, that has them; and per run
 * the offset of its set in flat_colors.  DIR/doc_sets_flat.bin is, byte for byte, u64 flat_colors_size | flat_colors | r offsets as
 * 5-byte MoveTally (u32 low, u8 high: include/move_row.hpp:13-39; doc_set_flat_inds, include/move_structure.hpp:296).
 *
 * movi_color_build: the tables, from the index and the offsets alone.  The text position of every BWT position comes from the
 * attached sampled suffix array; if none is attached one is built with movi_ssa_build at rate 100 and STAYS attached (replacing
 * nothing; a later movi_ssa_build / movi_ssa_load replaces it as usual).  Every sample walks down the text to the previous one and
 * writes the key (row << 16) | document of every position it passes; the keys are sorted and made unique on the device (hipCUB), in
 * chunks of samples sized from hipMemGetInfo ("color_chunk_keys": at most this many positions per chunk); numbering equal sets in
 * first-appearance order runs on the host.  Offsets must be strictly increasing and above 0 (MOVI_ERR_ARG: the reference's
 * one-step-per-position rule and a search agree only then); at most 65535 distinct taxa.  MOVI_ERR_INVARIANT if the walks do not visit
 * every BWT position exactly once, or a run is left without a document: never a wrong table.  A table of 2^31 - 1 rows or more is
 * MOVI_ERR_ARG, as for the sampled suffix array.  Replaces attached tables; once the arguments are accepted, a build that fails --
 * in movi_ssa_build or in its own walks -- leaves none attached.  Waits.
 * movi_color_save / movi_color_load: DIR/doc_sets_flat.bin.  Loading checks the file's length against r and every run's set against
 * the table and num_species (MOVI_ERR_FORMAT); a missing file is MOVI_ERR_IO with the reference's message naming the path.
 * movi_color_get: the tables as held (any pointer may be NULL; a cap too small: MOVI_ERR_ARG); h_inds as u64; h_to_taxon_id is known
 * after a build only (0 entries after a load). */
#define MOVI_PREPARE_COLOR 16u  /* movi_index_prepare: reserves the counter scratch of movi_multi_classify_device ("color_scratch_bytes",
                                   default 256 MB, at least one read's counters) and loads its kernel; without attached colour tables
                                   MOVI_ERR_ARG */
int movi_color_build(movi_index_t *ix, const uint64_t *doc_offsets, const uint32_t *doc_ids, uint64_t n_docs, void *stream);
int movi_color_save(movi_index_t *ix, const char *path);
int movi_color_load(movi_index_t *ix, const char *path, uint32_t num_species);
int movi_color_get(const movi_index_t *ix, uint64_t *flat_size, uint16_t *h_flat, uint64_t flat_cap, uint64_t *h_inds, uint64_t inds_cap,
                   uint32_t *num_species, uint32_t *h_to_taxon_id, uint64_t taxa_cap);

/* The PML query with ReadProcessor::process_char's multi-class scoring (src/read_processor.cpp:122-186) fused into the walk.  For
 * every base, last base first: the LF step (not at the read's first base); then, BEFORE the base is compared, if the match length
 * carried over from the base before is >= min_len (0 .. 255): colors_count += 1, and for every member d of the set of the row the
 * walk stands on, in stored order: counter[d] += 1, and if d is not the best document it becomes the best one (the old best
 * becoming second) when there is none or its counter is STRICTLY greater than the best's, else the second when there is none or its
 * counter is strictly greater than the second's.  (A flat offset >= flat_colors_size is skipped.)  Then the base is processed as in
 * the PML walk and its match length added to sum_ml (uint32_t, as in the reference).  Ties are decided by the order of the bases
 * and of the members, so one lane scores one read from end to end.
 * d_out[i]: best / second (0xFFFF = none), colors_count, sum_ml, and the counters of best and second (0 where there is none).  d_counts (optional): num_species u32 per read, the counters; when
 * NULL they live in the handle's scratch and the reads go through it in chunks of scratch / (4 * num_species) reads.  d_out_pml
 * (optional) as movi_pml_device.  A read that hits one of the reference's throws reports its code in d_read_err, no document, zero
 * counters and all-zero PMLs.  *-thresholds indexes with attached colour tables only (MOVI_ERR_ARG otherwise).  After
 * movi_index_prepare(MOVI_PREPARE_COLOR) the call allocates and builds nothing and may be captured into a graph. */
typedef struct movi_mc_read { uint16_t best, second; uint32_t colors_count, sum_ml, best_count, second_count, reserved_; } movi_mc_read_t;   /* 24 bytes */

int movi_multi_classify_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads, uint64_t n_bases,
                               uint32_t min_len, movi_mc_read_t *d_out, uint32_t *d_counts, uint16_t *d_out_pml, uint8_t *d_read_err,
                               const uint32_t *d_read_order, void *stream);
/* Host buffers in and out (h_counts, h_out_pml optional), chunk by chunk through the host loop like movi_count_host (overlapped where
 * the reads are page-locked and no vector comes down).  Every chunk has counters of its own in its staging, so chunks in flight
 * together do not meet: with h_counts its counter rows whole, without them scratch within "color_scratch_bytes". */
int movi_multi_classify_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets, uint64_t n_reads, uint32_t min_len,
                             movi_mc_read_t *h_out, uint32_t *h_counts, uint16_t *h_out_pml, uint8_t *h_read_err, movi_query_stats_t *stats);

/* ---- index.movi from a run-length BWT ----------------------------------------- */

/* MoveStructure::build() with --preprocessed (src/move_structure_build.cpp:17-72, :240-324): the move table from the BWT's run heads,
 * run lengths and, for the *-thresholds types, one threshold per run in pfp-thresholds' .thr_pos convention -- on the device, without
 * the reference's n + 1-bit vector: run starts by a prefix sum, the runs cut at the sorted distinct thresholds and into pieces of
 * the type's MAX_RUN_LENGTH, LF of the row heads by a per-character sum, id / offset by a binary search per row, the threshold bits
 * from the nearest row below of every other character, blocked ids (block size halved until they fit the row's id field, the bound
 * the reference applies in every round, src/move_structure_build.cpp:956) or the tally table, then the
 * packed rows.  *h_image is the index.movi file, byte for byte serialize()'s with zero header padding, in page-locked memory:
 * release it with movi_host_free; movi_index_parse reads it as it is.
 * h_heads[k] / h_lens[k]: the byte and the length of the k-th maximal run, original_r of them; the terminator is byte 0.  h_thr: NULL
 * for the types without thresholds (2, 3, 5), where it is not read.  Checked on the host before any device call, MOVI_ERR_ARG with
 * the array and the reason in the message: a NULL argument, an unsupported mode, no run, a run of length zero, 2^40 characters or
 * more, two neighbouring runs with one head, a terminator count other than 1, an alphabet outside the engine's scope (at most 4
 * symbols, or '%' + 4: then the table is a separator table, as in the reference), a threshold above the text's length.
 * More than 2^31 - 2 runs, or rows once the runs are cut, is MOVI_ERR_ARG too: hipcub's item counts are int (chunked scans: not yet).
 * The text's length may be anything below 2^40.  A threshold strictly inside a row after the cut is MOVI_ERR_INVARIANT (an internal
 * error: nothing is packed).  Every device allocation is freed on every return path; a failed call leaves *h_image NULL.
 * Not a capture-safe entry point: it allocates, reads sizes back and waits. */
int movi_build_from_rlbwt(int device, uint32_t mode, const uint8_t *h_heads, const uint64_t *h_lens, const uint64_t *h_thr /* NULL for modes 2, 3, 5 */,
                          uint64_t original_r, void **h_image, size_t *image_bytes);      /* release with movi_host_free */

/* ---- the run-length BWT, the thresholds and index.movi from a text ---------------- */

/* What the reference's external pipeline (prepare_ref, then pfp-thresholds: src/movi_launcher.cpp:190-242, src/prepare_ref.cpp) hands to
 * MoveStructure::build(), from the text itself, on the device.  h_text: the cleaned text of n characters as prepare_ref leaves it
 * (records, reverse complements, separators); any byte 1 .. 255 is a character here, the DNA scope is the table builder's check.  The
 * builder appends the terminator 0: N = n + 1 BWT positions.
 * Stages: the suffix array by prefix doubling (a radix sort of one 64-bit key per suffix and round, the first round on 8 characters;
 * every round sorts all suffixes), the BWT and its maximal runs, the LCP array by Kasai's algorithm with one lane per lcp_chunk
 * neighbouring text positions (exact; at most N + lanes x the longest repeat character comparisons, 8 per step), and the thresholds in
 * pfp-thresholds' .thr_pos convention: for run k with head c starting at s, the previous run of c ending at e, the LEFTMOST position
 * of the minimum of lcp[e + 1 .. s]; 0 where c has not occurred before.  The terminator and '%' are characters like the others.
 * verify = 1: the suffix array is a permutation and the rank array its inverse; every neighbouring pair is in order by its first
 * characters and, those being equal, by the ranks of the suffixes one further on; the LCP equals a direct comparison at 4096 seeded
 * positions (only where the LCP is computed).  A finding is MOVI_ERR_INVARIANT and nothing is returned.
 * Checked on the host before any device call, MOVI_ERR_ARG with the argument in the message: a NULL pointer, n = 0, a byte 0 in the
 * text (with its position), n above MOVI_TEXT_MAX_CHARS (ranks and positions are 32 bits).
 * Memory: the plan's peak is a formula over N alone (movi_text_device_bytes; 29.1 bytes per character and hipcub's scratch: min(N, 2^30) + 32 MiB).  It is compared with the
 * device's free memory, or with max_device_bytes, before the first allocation; a refusal is MOVI_ERR_ARG and names both figures.
 * Every device allocation is freed on every return path; a failed call leaves the outputs NULL.  The three arrays are page-locked:
 * release each with movi_host_free.  Not capture-safe entry points: they allocate, read sizes back and wait.
 * movi_build_from_text: movi_rlbwt_from_text, the checks of movi_build_from_rlbwt (alphabet, run counts) and its table builder; for the
 * types without thresholds (2, 3, 5) the LCP and threshold passes are skipped.  stats may be NULL. */
#define MOVI_TEXT_MAX_CHARS 4293918720ull   /* 2^32 - 2^20 */
typedef struct movi_text_build_opts {   /* NULL = all defaults */
    uint32_t lcp_chunk;          /* text positions per lane of the LCP pass, 0 = default (N / 2^17 held to 64 .. 1024) */
    uint32_t verify;             /* 1 = the verify stage */
    uint64_t max_device_bytes;   /* 0 = what the device reports free; else plan as if only this much were */
    uint64_t reserved_[3];
} movi_text_build_opts_t;
typedef struct movi_text_build_stats {
    uint64_t n_positions, original_r, device_bytes;   /* N, the runs, the peak of device bytes held */
    uint32_t rounds, verified;                        /* sorts of the prefix doubling; 1 = the verify stage ran and found nothing */
    double seconds[6];                                /* upload | suffix sort | BWT and runs | LCP | thresholds | verify */
} movi_text_build_stats_t;
int movi_text_device_bytes(uint64_t n, uint64_t *bytes);   /* the plan's device bytes for a text of n characters; host only */
int movi_rlbwt_from_text(int device, const uint8_t *h_text, uint64_t n, const movi_text_build_opts_t *opts,
                         uint8_t **h_heads, uint64_t **h_lens, uint64_t **h_thr, uint64_t *original_r,
                         movi_text_build_stats_t *stats /* may be NULL */);       /* release the three with movi_host_free */
int movi_build_from_text(int device, uint32_t mode, const uint8_t *h_text, uint64_t n, const movi_text_build_opts_t *opts,
                         void **h_image, size_t *image_bytes, movi_text_build_stats_t *stats);

/* ---- page-locked host memory --------------------------------------------------- */

/* The reference keeps reads and results in std::string / std::vector of its MoveQuery objects
 * (include/move_query.hpp:14-60); a caller that wants the *_host entry points to overlap their
 * transfers with the walk keeps them in page-locked memory instead: either allocated here
 * (hipHostMalloc) or its own buffers registered once (hipHostRegister) and reused across calls.
 * The *_host entry points detect it per call (movi_pml_host / movi_zml_host: h_bases and the
 * result vector; movi_count_host / movi_pml_classify_host: h_bases -- their per-read results are
 * small and may stay pageable). */
int movi_host_alloc(size_t bytes, void **out);
int movi_host_free(void *p);
int movi_host_register(void *p, size_t bytes);
int movi_host_unregister(void *p);

/* ---- tuning ------------------------------------------------------------------- */

/* Kernel variant / launch knobs, for A/B measurement (bench.py --variant).
 * Unknown keys return MOVI_ERR_ARG.  Keys: "pml_variant" (-1 = auto, 0 = first kernel (the one `--logs` runs on),
 * 1 = base-synchronous packed I/O, 14 = the lane state machine over row windows, software-pipelined: what auto
 * selects.  7 / 10 / 13 -- the row-at-a-time state machine, the hop-by-hop advance, lane refill -- were A/B variants that
 * never earned a default and were removed in round 5: DESIGN.md section 3),
 * "block_threads" (0 = auto, 64, 128, 192 or 256: the kernels' launch bound), "waves_per_cu"
 * (0 = the launch policy's cap, else at most this many wavefronts resident per CU), "idx64" (1 = run the kernel instantiations for
 * tables of 2^32 rows and more, whatever the size: a test hook), "release_scratch" (any value: frees the
 * device staging buffers that the *_host entry points keep, grow-only, across calls, and the scratch of the *_device calls -- graphs
 * captured on the handle are invalid afterwards), "host_overlap" (0: a *_host call is never cut into overlapped pieces, whatever memory
 * its buffers are in -- one upload, the walk, one download; for a caller that pipelines chunk-sized calls itself and keeps its reads in page-locked
 * memory for the direct upload, as `movi query` does; default 1), "reserve_host_bases" / "reserve_host_results" /
 * "reserve_host_reads" (that staging reserved up front instead of inside the first big call: the reads of a synchronous *_host call of
 * up to this many bases, its u16 result vector, the per-read buffers of up to this many reads; movi_index_info "host_staging_bytes"
 * tells what is held), "pipe_chunk_bases"
 * (bases per chunk of the overlapped host path, 0 = its own policy: a test hook), "locate_matches_stages" (a measurement hook:
 * movi_locate_matches_device stops after its searches and scan (1) or after the expansion (2: d_positions then holds packed
 * positions); 3, the default, is the whole call), "seg_len" (PML: batches whose mean
 * read length is at least twice this many bases are walked segment-parallel -- every read cut into segments of about
 * seg_len bases walked by their own lanes, stitched where the walks fall into step, reads that do not walked again:
 * identical results; ZML parses likewise; default 2048, 0 = off, else a multiple of 32; batches too small to fill the GPU
 * even so get shorter segments, down to 512), "seg_probe" (1, the default: an eligible batch
 * is cut into segments only if a probe of some of its reads finds that walks started mid-read fall into step within a
 * few hundred bases -- noisy long reads do, reads with 0.1 % errors and less do not and are better off with one lane
 * per read --; 0 = cut whatever the probe would say: a test hook; 2 = no probe, no length reduction, nothing read back:
 * "seg_verdict" (1 = cut, 0 = do not, the default) decides and the *_device calls stay asynchronous), "kmer_k"
 * (top-of-walk table: every walk starts in the same state, so its state after the last K bases of a read is a function
 * of those K bases -- one 16-byte table lookup replaces the first K row gathers of every read and segment; left alone the
 * first PML query on a DNA *-thresholds index builds the K = 12 table (256 MB, a few ms: that one call waits for it);
 * 0 = no table, 1..12 = build that one now), "stage_reads" (1, the default: every lane of the default walk copies the
 * next stretch of its read -- 256 bases at the occupancy cap of the look-ahead rows, 336 in small launches -- into the block's LDS and
 * takes its bases from there instead of re-fetching the read's cache line for every 16 bases; long reads roll through the
 * stretch; 0 = off: A/B),
 * "ahead_rows" (look-ahead rows: a second copy of the table, 16 bytes per row, in which each row's 128-byte line also holds
 * what the rows' LF targets look like -- character, length, offset, their own target --, so that a base that matches at the
 * target without a fast-forward is resolved, and its PML emitted, without fetching the target: two bases per gather on
 * real reads (+40 % on the cache-resident pangenome table); the count query walks both ends of its interval on them the
 * same way (+20 %; built by itself, the copy serves the count query only on tables whose positions mostly reach their LF
 * target without a fast-forward -- the builder tallies it --, which BWTs of real text do and random run sequences do
 * not).  Left alone, the first PML query builds them wherever the device has room for the copy and half as much again
 * (with the pair-shared gathers below they pay at every table size measured, 14 M to 1 B rows), the first count query where
 * a sample of the table says its search will use them.  1 = build now,
 * 0 = none (freed).  (Entries two rows deep -- "chain rows", three bases per gather -- were built in round 4, bit-exact, and
 * measured 10 - 38 % slower: profiles/r04_chain_rows.txt; removed),
 * "repo_hints" (1, the default: in the look-ahead copy of a table of fewer than 2^32 - 1 rows the rows' spare bits hold, per
 * threshold slot, how many rows beyond its window's edge the nearest run of that base lies -- a mismatch whose scan leaves the
 * window then gathers the scan's END in its next iteration instead of walking there window by window; 0 = ignore them: A/B),
 * "count_variant" (-1, the default: the count query runs as a lane state machine over row windows -- zml_kernel_flat<..., CNT = 1>,
 * by pairs of lanes on tables of 2 GB and more ("pair_loads") -- wherever it can: tables of 8 rows and more, batches of 16 bases
 * and more; 0 = count_kernel_v0, the base-synchronous kernel of rounds 1 - 4 (on the look-ahead rows where the table's statistic
 * admits them); 1 = the state machine or an error),
 * "inwin_repo" (1, the default: a reposition whose target run is one of the row window's other rows is resolved in
 * the iteration that sees the mismatch; 0 = off: A/B),
 * "pair_loads" (pair-shared gathers: the two lanes of a pair fetch each row window together, each lane one 16-byte half of
 * it in the same load instruction, halves exchanged through DPP -- one translation request and one 32-byte access where a
 * lane's own two loads are two of each; -1, the default: on for walked tables of 2 GB and more, where translation requests
 * bound the walk -- 1 B rows 32 -> 44 Gbases/s together with the look-ahead rows; the ZML parse fetches its two windows per
 * iteration the same way there: 16.8 -> 25.0 --; 1 / 0 = always / never: A/B),
 * "out_ring" (the PML kernels' PMLs leave through a ring in LDS -- one 2-byte LDS write per PML, a finished group of 16 as
 * two 16-byte stores -- instead of being packed in registers: a ninth fewer vector instructions per iteration; -1, the
 * default: batches whose mean read length is at least 1024, the shape that is bound by its own instruction stream (100 k x
 * 10 kbp: +5.7 %); 1 / 0 = wherever the block's LDS holds it / never: A/B),
 * "classify_fused" (movi_pml_classify_device with a PML vector: -1, the default: reads of mean length >= 1024 are walked
 * first and their bins reduced from the resident vectors by a wavefront per read -- faster than bins fused into the walk
 * there --, shorter ones fused; 1 = always fused, 0 = always two passes),
 * "kmer_lookahead" (the k-mer query's skipping of dead ends.  Before an end whose window holds the base the last search died
 * on, the window's left part is tried first, from at most `step` bases left of the end and never left of that base -- the
 * reference's look-ahead, src/sequitur.cpp:339-370, taken only where it is likely to die.  -1, the default: step = min(k / 2,
 * k - (log4(text length) + 2)), none when k is shorter than that -- a look shorter than log4(n) + 2 bases mostly passes and is
 * wasted; n in [2, 16]: step = k / n (3 = the reference's); 0 = every end searched from its own base.  Never changes an
 * answer: A/B, profiles/kmer_bench.txt),
 * "zml_ahead" (1: the ZML parse walks on the look-ahead rows where they exist -- a third fewer iterations, no faster: off
 * by default),
 * "pml_via_mask" (round 6; PML as reset masks.  movi_pml_device: the walk writes one bit per base and every wavefront expands its reads'
 * words into the u16 vector itself when its walks are over -- -1, the default: batches of short reads (mean length < 1024: c2 78.4 ->
 * 86.7 Gbases/s, 1 B rows 42.3 -> 46.0); 1 = wherever the walk can write masks; 0 = the walk writes the vector itself (register packer /
 * LDS ring), "host_masks" (movi_pml_host: -1, the default: a call of >= 2^22 bases brings only the masks down and expands them into the
 * caller's vector on host worker threads beside the walks of the later chunks -- 1/16 of the bytes over PCIe, no page-locking of the
 * vector: 22.7 -> 33 - 34 Gbases/s on 1 M x 150 bp; 1 = every call; 2 = both ways down side by side, "host_mask_share" percent
 * (default 70) of the bases as masks, the rest as the vector itself by DMA into a page-locked vector; 0 = never masks: a caller whose
 * own threads are busy, like `movi query`),
 * "fused_expand" (1, the default; 0 = the expansion by kernels of their own behind the walk: A/B),
 * "park_lanes" (parked lanes of the mask walk, movi_pml_device / movi_pml_mask_device: a wavefront leaves its loop when at most N of its
 * lanes still walk, parks their state in a queue in device scratch and retires its other reads; a second launch of the same kernel behind
 * it on the same stream resumes the parked reads 64 to a wavefront.  -1, the default: the launch policy decides (plan_pml: big batches of
 * short reads -- and picks 0 there: c2 is slower at every N from 2 to 16 although SIMT rises, profiles/park_lanes.txt); 0 = off; 1 .. 63 = N wherever the walk writes
 * masks itself, and for the vector only on the fused route.  Same answers and counters either way.  The queue is reserved with the mask
 * words by movi_index_prepare, or by this option on a handle that holds mask words; it never grows under a stream capture: a captured call
 * whose queue does not fit parks nothing),
 * "ff_skip" (fast-forward skip of the PML walk on the look-ahead and the deep rows: where a row's entry shows that the offset arrives at
 * or beyond the length of the LF target j, fast_forward passes j whatever the next base is, so the walk gathers the window of j + 1 with
 * that fast-forward taken instead of j's.  -1, the default: the launch policy decides per layout (ff_skip_on: on on the deep rows -- c2 88.0 -> 89.8 Gbases/s --, off on the look-ahead rows, where it gains 0.5 - 4.7 % when forced on: profiles/ff_skip.txt section 5);
 * 0 = off; 1 = on wherever the walk has entries.  Same vectors, error bytes and counters either way; fewer lane and wavefront steps:
 * profiles/ff_skip.txt), "reserve_device_masks" (device scratch
 * for the mask words of movi_pml_device calls of up to this many bases, reserved now instead of inside the first such call; grow-only,
 * beside what movi_index_prepare reserves),
 * "host_threads" (worker threads of the host-side expansion, 0 = three quarters of the CPUs the process may use -- affinity mask capped by the cgroup's quota --, at most 24),
 * "chain_rows" (a fourth layout of the table for the PML walk of short reads -- 32 bytes per row, windows of two rows, every row with
 * what the walk reads at its next THREE LF targets: up to four bases per gather, in a kernel of its own name, pml_kernel_chain;
 * movi_last_launch "ahead" 3.  -1, the default: the first PML query (or movi_index_prepare) builds them BESIDE the deep rows -- which
 * long reads and segment plans keep walking on -- where the deep rows' own conditions hold, the table has at least 12 Mi rows, its
 * share of positions that reach their LF target without a fast-forward ("ahead_no_ff") is at least 0.80 and the device has room for
 * them and 2 GiB more; 1 = build now (thresholds types of fewer than 2^28 - 1 rows, else refused), 0 = none (freed).  "ahead_rows"
 * 0 / 1 frees them too.  movi_index_info "chain_rows_bytes" = ((r + 1) / 2) * 64 where the handle holds them, counted in
 * "derived_bytes".  Same vectors, mask words, error bytes and counters as on every other layout: profiles/chain_rows.txt),
 * "deep_rows" (round 6: a third layout of the table for the PML walk of short reads -- 21.33 bytes per row, windows of three rows, every
 * row with what the walk reads at its LF target AND at that row's target: up to three bases per gather.  Left alone, the first PML query
 * (or movi_index_prepare) builds them, beside the look-ahead rows, for tables of at most 50 M rows whose positions mostly reach their LF
 * target without a fast-forward (real text); 1 = build now (tables of fewer than 2^28 - 1 rows), 0 = none (freed).  "ahead_rows" 0 / 1
 * frees them too: it is a statement about what the walk runs on), "deep_hint_bits" (width of the deep rows' reposition hints, one per
 * threshold slot of a row: how many rows beyond the edge of the row's three-row window a reposition scan ends, so that the walk gathers
 * the target's window next instead of walking there window by window.  4 = reach 15, held beside 26-bit row ids: tables of at most
 * 2^26 - 1 rows, in the same bytes -- tables of 2^26 rows and more keep 28-bit ids and 2-bit hints whatever is asked; 2 = reach 3 with
 * 28-bit ids; -1, the default: 4 (c2 89.6 -> 91.0 Gbases/s, c2mid 72.9 -> 74.9: profiles/deep_hints.txt).  It takes effect when the
 * deep rows are next built ("deep_rows" 1, movi_index_prepare or the first PML query); movi_index_info "deep_hint_bits" says what the
 * rows the handle holds were built with.  Building looks up to 15 rows past either edge instead of 3: 0.89 -> 1.18 ms for 14 M rows,
 * once per handle.  Same vectors, error bytes and counters at either width; fewer lane and wavefront steps: A/B), "deep" (-1, the default: batches whose mean read length is below
 * 1024 walk on the deep rows where the handle holds them; 0 = never, 1 = always, the segment plan's launches included: A/B),
 * "ftab_k" (the count query's interval table -- the backward-search interval after the last K bases of a read by one lookup,
 * the reference's own ftab (src/move_structure_search.cpp:66-167) put to work for --count; left alone the first count query
 * on a DNA index builds the K = 12 table (256 MB); 0 = none, 1..12 = build that one now). */
int movi_set_option(movi_index_t *ix, const char *key, int64_t value);

/* ---- ZML (Ziv-Merhav cross parse) ---------------------------------------------- */

/* `movi query --zml`: MoveStructure::query_zml (src/move_structure_query.cpp:690-785) without
 * multi-classify.  Same buffers, layout, error and ordering conventions as movi_pml_device:
 * out_zml[offsets[i] + k] = match length recorded for base (len_i - 1 - k) of read i = the
 * number of bases of its greedy backward-search phrase to its right, u16-clamped; illegal
 * bases give 0 and end the phrase.  These are the values of the reference's --no-prefetch
 * path; its strand scheduler appends one extra entry to a read whose first base is illegal
 * (reset_backward_search skips to pos -1, src/read_processor.cpp:1006-1013, and the caller adds
 * again, :704), which this engine does not reproduce.  Batches of long reads are parsed segment-parallel like PML walks
 * ("seg_len"; the call then waits for a short probe of the batch before it enqueues the parse). */
int movi_zml_device(movi_index_t *ix, const uint8_t *d_bases, const uint64_t *d_offsets,
                    uint64_t n_reads, uint64_t n_bases, uint16_t *d_out_zml, uint8_t *d_read_err,
                    const uint32_t *d_read_order, void *stream);

int movi_zml_host(movi_index_t *ix, const uint8_t *h_bases, const uint64_t *h_offsets,
                  uint64_t n_reads, uint16_t *h_out_zml, uint8_t *h_read_err,
                  movi_query_stats_t *stats);

#ifdef __cplusplus
}
#endif
#endif /* MOVI_HIP_H */
