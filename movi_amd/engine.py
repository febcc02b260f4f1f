"""Host-side mirror of the reference's query interface over the C-ABI.

Reference seam (file:line under /root/reference) -> here:
  MoveStructure::deserialize          src/move_structure_io.cpp:471-511  -> MoveIndex.load / from_image
  MoveStructure::query_pml(MoveQuery&) src/move_structure_query.cpp:234   -> MoveIndex.query_pml
  ReadProcessor::process_latency_hiding src/read_processor.cpp:641        -> MoveIndex.query_pml (batched)
  MoveStructure::query_backward_search src/move_structure_search.cpp:340  -> MoveIndex.query_count
  MoveStructure::query_mems           src/mem_finder.cpp:7-145           -> MoveIndex.query_mems
  MoveStructure::query_all_kmers      src/sequitur.cpp:322-421           -> MoveIndex.query_kmers
  (no reference seam: occurrences per k-mer, include/movi_hip.h)        -> MoveIndex.query_kmer_occ
  MoveStructure::get_SA_entries       src/move_structure.cpp:35-48       -> MoveIndex.locate / query_sa_entries
  (no reference seam: text positions of count and MEM hits, movi_hip.h) -> MoveIndex.locate_matches
  MoveStructure::find_sampled_SA_entries src/move_structure_build.cpp:1174 -> MoveIndex.build_ssa (save_ssa / load_ssa: ssa.movi)
  MoveStructure::build (--preprocessed) src/move_structure_build.cpp:17-72 -> build_image
  prepare_ref + pfp-thresholds + build  src/movi_launcher.cpp:190-242    -> rlbwt_from_text / build_image_from_text

All compute happens in libmovi_hip.so on the GPU; this file only marshals
buffers.  Errors are MoviError (the reference throws std::runtime_error).
"""
import ctypes as C

import numpy as np

from ._lib import IndexDescC, LaunchInfoC, QueryStatsC, TextBuildOptsC, TextBuildStatsC, check, lib


# movi_mem_t: one maximal exact match, end exclusive; count = occurrences of the match's reverse complement (64 bits)
MEM_DTYPE = np.dtype([("start", np.uint32), ("end", np.uint32), ("count", np.uint64)])
# movi_kmer_run_t: the k-mers starting at start, start + 1, ..., start + count - 1 are found
KMER_RUN_DTYPE = np.dtype([("start", np.uint32), ("count", np.uint32)])


class IndexDesc:
    """Python view of movi_index_desc_t."""

    def __init__(self, c):
        self.mode = int(c.mode)
        self.alphabet_size = int(c.alphabet_size)
        self.r = int(c.r)
        self.length = int(c.length)
        self.end_bwt_idx = int(c.end_bwt_idx)
        self.end_bwt_idx_thresholds = list(c.end_bwt_idx_thresholds)
        self.alphabet = bytes(c.alphabet[: self.alphabet_size])
        self.code_of = bytes(c.code_of)
        k = self.alphabet_size + 1
        self.first_runs = list(c.first_runs[:k])
        self.first_offsets = list(c.first_offsets[:k])
        self.last_runs = list(c.last_runs[:k])
        self.last_offsets = list(c.last_offsets[:k])
        self.n_blocks = int(c.n_blocks)
        self.block_size = int(c.block_size)
        self.row_bytes = {6: 8, 8: 6, 7: 3, 5: 3, 3: 8, 2: 6}[self.mode]


def parse_index_image(image):
    """movi_index_parse: (IndexDesc, raw C desc, rows_offset, rows_bytes).  Host only, no GPU."""
    buf = np.frombuffer(image, np.uint8)
    c = IndexDescC()
    off, nb = C.c_size_t(0), C.c_size_t(0)
    check(lib().movi_index_parse(buf.ctypes.data, buf.size, C.byref(c), C.byref(off), C.byref(nb)))
    return IndexDesc(c), c, off.value, nb.value


def build_image(heads, lens, thr, mode, device=0):
    """movi_build_from_rlbwt: the bytes of index.movi from a run-length BWT, built on the GPU.  heads: one byte per maximal
    run (bytes or uint8), lens: the runs' lengths, thr: one threshold per run in the .thr_pos convention (None for the types
    without thresholds: 2, 3, 5).  MoveIndex.from_image takes the result."""
    heads = np.ascontiguousarray(np.frombuffer(heads, np.uint8) if isinstance(heads, (bytes, bytearray)) else heads, np.uint8)
    lens = np.ascontiguousarray(lens, np.uint64)
    if lens.size != heads.size:
        raise ValueError("heads and lens differ in length")
    if thr is not None:
        thr = np.ascontiguousarray(thr, np.uint64)
        if thr.size != heads.size:
            raise ValueError("heads and thr differ in length")
    img, nbytes = C.c_void_p(), C.c_size_t(0)
    check(lib().movi_build_from_rlbwt(int(device), int(mode), heads.ctypes.data, lens.ctypes.data,
                                      thr.ctypes.data if thr is not None else None, heads.size, C.byref(img), C.byref(nbytes)))
    try:
        return C.string_at(img.value, nbytes.value)
    finally:
        lib().movi_host_free(img)


class TextBuildStats:
    """Python view of movi_text_build_stats_t."""
    STAGES = ("upload", "suffix_sort", "bwt_runs", "lcp", "thresholds", "verify")

    def __init__(self, c):
        self.n_positions = int(c.n_positions)
        self.original_r = int(c.original_r)
        self.device_bytes = int(c.device_bytes)
        self.rounds = int(c.rounds)
        self.verified = int(c.verified)
        self.seconds = dict(zip(self.STAGES, (float(x) for x in c.seconds)))


def _text_args(text, lcp_chunk, verify, max_device_bytes):
    text = np.ascontiguousarray(np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else text, np.uint8)
    opts = TextBuildOptsC(lcp_chunk=int(lcp_chunk), verify=1 if verify else 0, max_device_bytes=int(max_device_bytes))
    return text, opts


def text_device_bytes(n):
    """movi_text_device_bytes: the device bytes the plan of a text of n characters needs.  Host only."""
    out = C.c_uint64(0)
    check(lib().movi_text_device_bytes(int(n), C.byref(out)))
    return out.value


def rlbwt_from_text(text, lcp_chunk=0, verify=False, max_device_bytes=0, device=0):
    """movi_rlbwt_from_text: (heads uint8, lens uint64, thr uint64, TextBuildStats) of the cleaned text (bytes or uint8, no byte 0,
    without the terminator), built on the GPU: suffix array, BWT, LCP, thresholds in the .thr_pos convention."""
    text, opts = _text_args(text, lcp_chunk, verify, max_device_bytes)
    heads, lens, thr, r, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(0), TextBuildStatsC()
    check(lib().movi_rlbwt_from_text(int(device), text.ctypes.data, text.size, C.byref(opts), C.byref(heads), C.byref(lens), C.byref(thr),
                                     C.byref(r), C.byref(st)))
    try:
        return (np.frombuffer(C.string_at(heads.value, r.value), np.uint8), np.frombuffer(C.string_at(lens.value, r.value * 8), np.uint64),
                np.frombuffer(C.string_at(thr.value, r.value * 8), np.uint64), TextBuildStats(st))
    finally:
        for p in (heads, lens, thr):
            lib().movi_host_free(p)


def build_image_from_text(text, mode, lcp_chunk=0, verify=False, max_device_bytes=0, device=0, stats=None):
    """movi_build_from_text: the bytes of index.movi of the cleaned text, everything on the GPU.  stats (optional): a list that
    receives the call's TextBuildStats."""
    text, opts = _text_args(text, lcp_chunk, verify, max_device_bytes)
    img, nbytes, st = C.c_void_p(), C.c_size_t(0), TextBuildStatsC()
    check(lib().movi_build_from_text(int(device), int(mode), text.ctypes.data, text.size, C.byref(opts), C.byref(img), C.byref(nbytes),
                                     C.byref(st)))
    if stats is not None:
        stats.append(TextBuildStats(st))
    try:
        return C.string_at(img.value, nbytes.value)
    finally:
        lib().movi_host_free(img)


def _pack_reads(reads):
    """list of bytes -> (uint8 bases, uint64 offsets[n+1])."""
    lens = np.fromiter((len(r) for r in reads), np.uint64, len(reads))
    offs = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    bases = np.frombuffer(b"".join(bytes(r) for r in reads), np.uint8) if len(reads) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(bases), offs


class _PinnedBlock:
    """Page-locked host bytes (movi_host_alloc); numpy views keep it alive through __array_interface__."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        check(lib().movi_host_alloc(nbytes, C.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            if self.ptr:
                lib().movi_host_free(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def pinned_empty(n, dtype):
    """A numpy array of n elements in page-locked host memory (movi_host_alloc): with the reads and the result
    vector in such arrays the *_host entry points overlap upload, walk and download (include/movi_hip.h)."""
    dt = np.dtype(dtype)
    blk = _PinnedBlock(max(int(n) * dt.itemsize, 1))
    return np.asarray(blk)[: int(n) * dt.itemsize].view(dt)


def mask_words(n_reads, n_bases, first_base=0):
    """movi_pml_mask_words: 32-bit words the reset masks of a batch take."""
    n = C.c_uint64(0)
    check(lib().movi_pml_mask_words(int(n_reads), int(n_bases), int(first_base), C.byref(n)))
    return int(n.value)


def expand_masks_host(words, offs, threads=0, out=None):
    """movi_pml_expand_host: reset-mask words -> the u16 PML vector (pure host code, worker threads)."""
    words = np.ascontiguousarray(words, np.uint32)
    offs = np.ascontiguousarray(offs, np.uint64)
    if out is None:
        out = np.zeros(int(offs[-1]), np.uint16)
    check(lib().movi_pml_expand_host(words.ctypes.data, offs.ctypes.data, offs.size - 1, out.ctypes.data, int(threads)))
    return out


def masks_of_pml(pml, offs, first_base=0):
    """The reset-mask words of a PML vector (numpy; test helper): bit = (PML == 0), layout of include/movi_hip.h.
    Returns (words, valid) -- valid marks the words that belong to a read (gap words are unspecified)."""
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    n = offs.size - 1
    rel = offs - offs[0]
    words = np.zeros(mask_words(n, int(rel[-1]), first_base), np.uint32)
    valid = np.zeros(words.size, bool)
    lens = np.diff(rel)
    if n == 0 or rel[-1] == 0:
        return words, valid
    w0 = ((first_base + rel[:-1]) >> 5) - (first_base >> 5) + np.arange(n)
    read_of = np.repeat(np.arange(n), lens)
    k = np.arange(int(rel[-1])) - np.repeat(rel[:-1], lens)
    z = np.asarray(pml[int(offs[0]):int(offs[-1])]) == 0
    widx = w0[read_of] + (k >> 5)
    np.bitwise_or.at(words, widx[z], (np.uint32(1) << (k[z] & 31).astype(np.uint32)))
    valid[widx] = True
    return words, valid


def packed_bytes(first_base, n_bases):
    """movi_reads_packed_bytes: bytes of a 2-bit packed buffer that holds bases [0, first_base + n_bases)."""
    n = C.c_uint64(0)
    check(lib().movi_reads_packed_bytes(int(first_base), int(n_bases), C.byref(n)))
    return int(n.value)


def pack_reads(bases, first_base=0, threads=0, packed=None, exc_cap=None):
    """movi_reads_pack_host: uint8 bases (bases[j] = base first_base + j) -> (packed uint8, exc_pos uint64, exc_byte uint8), the
    2-bit format of include/movi_hip.h: four bases per byte at their ABSOLUTE position, every byte that is not upper-case ACGT in the
    sparse exception list.  `packed`: a buffer to append to (e.g. pinned_empty(packed_bytes(...), np.uint8)); a fresh one otherwise.
    `exc_cap`: room for the exceptions (default: a first guess, grown once if it does not fit)."""
    bases = np.ascontiguousarray(np.frombuffer(bases, np.uint8) if isinstance(bases, (bytes, bytearray)) else bases, np.uint8)
    if packed is None:
        packed = np.zeros(packed_bytes(first_base, bases.size), np.uint8)
    assert packed.dtype == np.uint8 and packed.size >= packed_bytes(first_base, bases.size) and packed.flags.c_contiguous
    cap = int(exc_cap) if exc_cap is not None else max(16, bases.size // 64)
    while True:
        pos, byte, n = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint8), C.c_uint64(0)
        rc = lib().movi_reads_pack_host(bases.ctypes.data, int(first_base), bases.size, packed.ctypes.data, pos.ctypes.data,
                                        byte.ctypes.data, cap, C.byref(n), int(threads))
        if rc == -1 and n.value > cap and exc_cap is None:   # (MOVI_ERR_ARG with the needed count: once more with that much room)
            cap = int(n.value)
            continue
        check(rc)
        return packed, pos[:n.value], byte[:n.value]


def unpack_reads(packed, first_base, n_bases, exc_pos=None, exc_byte=None, threads=0):
    """movi_reads_unpack_host: the exact inverse of pack_reads, on the host -> uint8[n_bases]."""
    packed = np.ascontiguousarray(packed, np.uint8)
    pos = np.ascontiguousarray(exc_pos if exc_pos is not None else [], np.uint64)
    byte = np.ascontiguousarray(exc_byte if exc_byte is not None else [], np.uint8)
    assert pos.size == byte.size
    out = np.zeros(int(n_bases), np.uint8)
    check(lib().movi_reads_unpack_host(packed.ctypes.data, int(first_base), int(n_bases), pos.ctypes.data, byte.ctypes.data, pos.size,
                                       out.ctypes.data, int(threads)))
    return out


class QueryStats:
    def __init__(self, c):
        self.bases = int(c.bases)
        self.fast_forwards = int(c.fast_forwards)
        self.scans = int(c.scans)
        self.repositions = int(c.repositions)
        self.errors = int(c.errors)
        self.lane_steps = int(c.lane_steps)
        self.wave_steps = int(c.wave_steps)
        self.segments = int(c.segments)
        self.rewalked = int(c.rewalked)

    def __repr__(self):
        return "QueryStats(bases=%d, ff=%d, scans=%d, repositions=%d, errors=%d)" % (
            self.bases, self.fast_forwards, self.scans, self.repositions, self.errors)


class MoveIndex:
    """A move-structure index resident on one GPU."""

    def __init__(self, handle, keepalive=None, device=0):
        self._h = handle
        self._keep = keepalive
        self.device = int(device)
        c = IndexDescC()
        check(lib().movi_index_get_desc(self._h, C.byref(c)))
        self.desc = IndexDesc(c)

    # -- construction ---------------------------------------------------------
    @classmethod
    def load(cls, index_dir_or_file, device=0):
        h = C.c_void_p()
        check(lib().movi_index_load(device, str(index_dir_or_file).encode(), C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_image(cls, image, device=0):
        buf = np.frombuffer(image, np.uint8)
        _, c, off, _ = parse_index_image(buf)
        h = C.c_void_p()
        check(lib().movi_index_create(device, C.byref(c), buf.ctypes.data + off, C.byref(h)))
        return cls(h, device=device)

    @classmethod
    def from_device_rows(cls, cdesc, d_rows_ptr, device=0, keepalive=None):
        """Adopt a device-resident row table (e.g. an RCCL-broadcast torch tensor)."""
        h = C.c_void_p()
        check(lib().movi_index_create_from_device_rows(device, C.byref(cdesc), C.c_void_p(d_rows_ptr), C.byref(h)))
        return cls(h, keepalive=keepalive, device=device)

    @classmethod
    def load_replicated(cls, index_dir_or_file, devices):
        """movi_index_load_replicated: one handle per device; the rows cross PCIe once (to devices[0]) and reach the
        other GPUs through one RCCL broadcast."""
        n = len(devices)
        devs = (C.c_int * n)(*[int(d) for d in devices])
        hs = (C.c_void_p * n)()
        check(lib().movi_index_load_replicated(str(index_dir_or_file).encode(), devs, n, hs))
        return [cls(C.c_void_p(hs[i]), device=devices[i]) for i in range(n)]

    @classmethod
    def replicate_image(cls, image, devices):
        """movi_index_replicate from an index.movi image in host memory."""
        buf = np.frombuffer(image, np.uint8)
        _, c, off, _ = parse_index_image(buf)
        n = len(devices)
        devs = (C.c_int * n)(*[int(d) for d in devices])
        hs = (C.c_void_p * n)()
        check(lib().movi_index_replicate(C.byref(c), buf.ctypes.data + off, devs, n, hs))
        return [cls(C.c_void_p(hs[i]), device=devices[i]) for i in range(n)]

    def close(self):
        if getattr(self, "_h", None):
            lib().movi_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_rows(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(lib().movi_index_device_rows(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_option(self, key, value):
        check(lib().movi_set_option(self._h, key.encode(), int(value)))

    # -- host-buffer queries ----------------------------------------------------
    def query_pml_packed(self, bases, offs, want_err=False, out=None):
        """bases uint8[n_bases], offs uint64[n+1] -> (u16 PMLs in emission order, QueryStats[, err]).
        `out`: the caller's result array (e.g. pinned_empty(n_bases, np.uint16) next to pinned bases: overlapped path)."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        if out is None:
            out = np.zeros(bases.size, np.uint16)
        assert out.dtype == np.uint16 and out.size == bases.size and out.flags.c_contiguous
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_pml_host(self._h, bases.ctypes.data, offs.ctypes.data, n, out.ctypes.data,
                                 err.ctypes.data, C.byref(st))
        if want_err:
            return out, QueryStats(st), err[:n], rc
        check(rc)
        return out, QueryStats(st)

    def query_pml_mask_packed(self, bases, offs, want_err=False):
        """movi_pml_mask_host: (u32 reset-mask words laid out as include/movi_hip.h says, QueryStats[, err, rc])."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        words = np.zeros(mask_words(n, int(offs[-1] - offs[0])), np.uint32)
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_pml_mask_host(self._h, bases.ctypes.data, offs.ctypes.data, n, words.ctypes.data, err.ctypes.data,
                                      C.byref(st))
        if want_err:
            return words, QueryStats(st), err[:n], rc
        check(rc)
        return words, QueryStats(st)

    def query_pml_packed2(self, packed, exc_pos, exc_byte, offs, want_err=False, out=None):
        """movi_pml_packed_host: query_pml_packed on reads packed TWO BITS per base (pack_reads; "packed" in the neighbouring
        methods' names means "concatenated") -> (u16 PMLs in emission order, QueryStats[, err, rc])."""
        packed = np.ascontiguousarray(packed, np.uint8)
        pos, byte = np.ascontiguousarray(exc_pos, np.uint64), np.ascontiguousarray(exc_byte, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        if out is None:
            out = np.zeros(int(offs[-1]), np.uint16)
        assert out.dtype == np.uint16 and out.size >= int(offs[-1]) and out.flags.c_contiguous and pos.size == byte.size
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_pml_packed_host(self._h, packed.ctypes.data, pos.ctypes.data, byte.ctypes.data, pos.size, offs.ctypes.data, n,
                                        out.ctypes.data, err.ctypes.data, C.byref(st))
        if want_err:
            return out, QueryStats(st), err[:n], rc
        check(rc)
        return out, QueryStats(st)

    def query_pml_mask_packed2(self, packed, exc_pos, exc_byte, offs, want_err=False):
        """movi_pml_mask_packed_host: query_pml_mask_packed on reads packed two bits per base -> (u32 words, QueryStats[, err, rc])."""
        packed = np.ascontiguousarray(packed, np.uint8)
        pos, byte = np.ascontiguousarray(exc_pos, np.uint64), np.ascontiguousarray(exc_byte, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        assert pos.size == byte.size
        words = np.zeros(mask_words(n, int(offs[-1] - offs[0])), np.uint32)
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_pml_mask_packed_host(self._h, packed.ctypes.data, pos.ctypes.data, byte.ctypes.data, pos.size, offs.ctypes.data,
                                             n, words.ctypes.data, err.ctypes.data, C.byref(st))
        if want_err:
            return words, QueryStats(st), err[:n], rc
        check(rc)
        return words, QueryStats(st)

    def query_pml_logs_packed(self, bases, offs):
        """movi_pml_logs_host: (PMLs, per-base fast-forwards, per-base scan rows, QueryStats), all in emission order."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        out = np.zeros(bases.size, np.uint16)
        ff = np.zeros(bases.size, np.uint16)
        sc = np.zeros(bases.size, np.uint16)
        st = QueryStatsC()
        check(lib().movi_pml_logs_host(self._h, bases.ctypes.data, offs.ctypes.data, offs.size - 1, out.ctypes.data,
                                       ff.ctypes.data, sc.ctypes.data, None, C.byref(st)))
        return out, ff, sc, QueryStats(st)

    def query_pml(self, reads):
        """MoveStructure::query_pml for each read: list of u16 arrays, last base first
        (MoveQuery::matching_lens order)."""
        bases, offs = _pack_reads(reads)
        out, _ = self.query_pml_packed(bases, offs)
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(len(reads))]

    def query_zml_packed(self, bases, offs, out=None):
        """MoveStructure::query_zml (src/move_structure_query.cpp:690-785) for packed reads:
        (u16 match lengths in emission order, QueryStats)."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        if out is None:
            out = np.zeros(bases.size, np.uint16)
        assert out.dtype == np.uint16 and out.size == bases.size and out.flags.c_contiguous
        st = QueryStatsC()
        check(lib().movi_zml_host(self._h, bases.ctypes.data, offs.ctypes.data, n, out.ctypes.data, None,
                                  C.byref(st)))
        return out, QueryStats(st)

    def query_zml(self, reads):
        bases, offs = _pack_reads(reads)
        out, _ = self.query_zml_packed(bases, offs)
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(len(reads))]

    def classify_packed(self, bases, offs, bin_width, max_value_thr):
        """PML + Classifier::classify bins on the device: (bins_above, bins_below, sum_max) per read."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        a = np.zeros(max(n, 1), np.uint32)
        b = np.zeros(max(n, 1), np.uint32)
        s = np.zeros(max(n, 1), np.uint64)
        st = QueryStatsC()
        check(lib().movi_pml_classify_host(self._h, bases.ctypes.data, offs.ctypes.data, n, int(bin_width),
                                           int(max_value_thr), a.ctypes.data, b.ctypes.data, s.ctypes.data,
                                           None, C.byref(st)))
        return a[:n], b[:n], s[:n]

    def query_count_packed(self, bases, offs, want_err=False):
        """-> (matched, count, QueryStats[, per-read error bytes, return code])"""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        m = np.zeros(max(n, 1), np.uint64)
        c = np.zeros(max(n, 1), np.uint64)
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_count_host(self._h, bases.ctypes.data, offs.ctypes.data, n, m.ctypes.data,
                                   c.ctypes.data, err.ctypes.data if want_err else None, C.byref(st))
        if want_err:
            return m[:n], c[:n], QueryStats(st), err[:n], rc
        check(rc)
        return m[:n], c[:n], QueryStats(st)

    def query_count(self, reads):
        """query_backward_search per read: list of (matched, count) as printed by
        output_counts (src/utils.cpp:248-256: `matched/len\\tcount`)."""
        bases, offs = _pack_reads(reads)
        m, c, _ = self.query_count_packed(bases, offs)
        return [(int(m[i]), int(c[i])) for i in range(len(reads))]

    def query_mems_packed(self, bases, offs, min_len, want_err=False):
        """movi_mem_host -> (n_mems, mems, QueryStats[, per-read error bytes, return code]); mems is a structured array
        (MEM_DTYPE: start, end, count), compact: the MEMs of read 0, then read 1, ..."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        cap = int(offs[-1] - offs[0]) if n > 0 else 0
        nm = np.zeros(max(n, 1), np.uint32)
        mems = np.zeros(max(cap, 1), MEM_DTYPE)
        err = np.zeros(max(n, 1), np.uint8)
        total = C.c_uint64(0)
        st = QueryStatsC()
        rc = lib().movi_mem_host(self._h, bases.ctypes.data, offs.ctypes.data, n, int(min_len), nm.ctypes.data,
                                 mems.ctypes.data, cap, C.byref(total), err.ctypes.data if want_err else None, C.byref(st))
        out = mems[:total.value]
        if want_err:
            return nm[:n], out, QueryStats(st), err[:n], rc
        check(rc)
        return nm[:n], out, QueryStats(st)

    def query_mems(self, reads, min_len):
        """query_mems per read: list of [(start, end, count), ...] (end exclusive, count = full 64-bit occ)."""
        bases, offs = _pack_reads(reads)
        nm, mems, _ = self.query_mems_packed(bases, offs, min_len)
        out, k = [], 0
        for i in range(len(reads)):
            c = int(nm[i])
            out.append([(int(x["start"]), int(x["end"]), int(x["count"])) for x in mems[k:k + c]])
            k += c
        return out

    def query_kmers_packed(self, bases, offs, k, want_rc=False):
        """movi_kmer_host -> (n_runs, found, runs, QueryStats[, return code]); runs is a structured array (KMER_RUN_DTYPE:
        start, count), compact: the runs of read 0 (by decreasing start), then read 1, ..."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        cap = int(offs[-1] - offs[0]) if n > 0 else 0
        nr = np.zeros(max(n, 1), np.uint32)
        found = np.zeros(max(n, 1), np.uint32)
        runs = np.zeros(max(cap, 1), KMER_RUN_DTYPE)
        total = C.c_uint64(0)
        st = QueryStatsC()
        rc = lib().movi_kmer_host(self._h, bases.ctypes.data, offs.ctypes.data, n, int(k), nr.ctypes.data, found.ctypes.data,
                                  runs.ctypes.data, cap, C.byref(total), C.byref(st))
        out = runs[:total.value]
        if want_rc:
            return nr[:n], found[:n], out, QueryStats(st), rc
        check(rc)
        return nr[:n], found[:n], out, QueryStats(st)

    def query_kmers(self, reads, k):
        """query_all_kmers per read: (found, [(start, count), ...]) -- runs by decreasing start, found = sum of the counts."""
        bases, offs = _pack_reads(reads)
        nr, found, runs, _ = self.query_kmers_packed(bases, offs, k)
        out, j = [], 0
        for i in range(len(reads)):
            c = int(nr[i])
            out.append((int(found[i]), [(int(x["start"]), int(x["count"])) for x in runs[j:j + c]]))
            j += c
        return out

    def query_kmer_occ_packed(self, bases, offs, k, want_err=False):
        """movi_kmer_occ_host -> (occ, found, sum, QueryStats[, err, return code]); occ: one u64 per base, the k-mer at p of read i
        at offs[i] - offs[0] + p, the read's last k - 1 slots 0 (an error slot has bit 63 set: MOVI_OCC_IS_ERROR)."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        nb = int(offs[-1] - offs[0]) if n > 0 else 0
        occ = np.zeros(max(nb, 1), np.uint64)
        found = np.zeros(max(n, 1), np.uint32)
        total = np.zeros(max(n, 1), np.uint64)
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_kmer_occ_host(self._h, bases.ctypes.data, offs.ctypes.data, n, int(k), occ.ctypes.data, found.ctypes.data,
                                      total.ctypes.data, err.ctypes.data, C.byref(st))
        if want_err:
            return occ[:nb], found[:n], total[:n], QueryStats(st), err[:n], rc
        check(rc)
        return occ[:nb], found[:n], total[:n], QueryStats(st)

    def query_kmer_occ(self, reads, k):
        """`movi query --kmer-occ` per read: (found, sum, uint64 array of the max(0, len - k + 1) occurrence counts)."""
        bases, offs = _pack_reads(reads)
        occ, found, total, _ = self.query_kmer_occ_packed(bases, offs, k)
        out = []
        for i, r in enumerate(reads):
            b = int(offs[i])
            out.append((int(found[i]), int(total[i]), occ[b: b + max(0, len(r) - int(k) + 1)].copy()))
        return out

    # -- locate: sampled suffix array ---------------------------------------------
    POS_OFFSET_BITS = 12          # MOVI_POS_PACK
    POS_NONE = 0xFFFFFFFFFFFFFFFF

    def build_ssa(self, rate=100, stream=0):
        """movi_ssa_build: the sampled suffix array of `rate` (and the locate rows), built on the device and attached."""
        check(lib().movi_ssa_build(self._h, int(rate), C.c_void_p(stream) if stream else None))

    def save_ssa(self, path):
        """movi_ssa_save: the attached array as the reference's ssa.movi."""
        check(lib().movi_ssa_save(self._h, str(path).encode()))

    def load_ssa(self, path):
        check(lib().movi_ssa_load(self._h, str(path).encode()))

    def ssa(self):
        """(rate, the n / rate + 1 entries as uint64)."""
        rate, n = C.c_uint64(0), C.c_uint64(0)
        check(lib().movi_ssa_get(self._h, C.byref(rate), None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint64)
        check(lib().movi_ssa_get(self._h, None, out.ctypes.data, out.size, None))
        return int(rate.value), out

    def locate(self, rows, offs):
        """Suffix-array entries (uint64, not reduced modulo n) of the BWT positions (rows[i], offs[i]) of the resident table."""
        import torch
        pos = (np.asarray(rows, np.uint64) << np.uint64(self.POS_OFFSET_BITS)) | np.asarray(offs, np.uint64)
        if pos.size == 0:
            check(lib().movi_locate_device(self._h, None, 0, None))
            return pos
        with torch.cuda.device(self.device):
            d = torch.from_numpy(pos.view(np.int64)).cuda()
            self.locate_device(d.data_ptr(), pos.size)
            st = self.last_stats()
            out = d.cpu().numpy().view(np.uint64)
        if st.errors:
            from ._lib import MoviError
            raise MoviError(-6, "%d position(s) are not positions of the table or hit a move-structure invariant violation "
                                "(corrupt index?)" % st.errors)
        return out

    def query_sa_entries_packed(self, bases, offs, want_err=False, want_pml=True):
        """movi_sa_entries_host -> (u64 entries in emission order, u16 PMLs or None, QueryStats[, err, rc])."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        sa = np.zeros(bases.size, np.uint64)
        pml = np.zeros(bases.size, np.uint16) if want_pml else None
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_sa_entries_host(self._h, bases.ctypes.data, offs.ctypes.data, n, pml.ctypes.data if want_pml else None,
                                        sa.ctypes.data, err.ctypes.data, C.byref(st))
        if want_err:
            return sa, pml, QueryStats(st), err[:n], rc
        check(rc)
        return sa, pml, QueryStats(st)

    def query_sa_entries(self, reads):
        """`movi query --sa-entries` per read: list of uint64 arrays, last base first like the PMLs."""
        bases, offs = _pack_reads(reads)
        sa, _, _ = self.query_sa_entries_packed(bases, offs, want_pml=False)
        return [sa[int(offs[i]): int(offs[i + 1])] for i in range(len(reads))]

    # -- locate count and MEM hits ------------------------------------------------
    MATCH_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("end", "<u4")])      # movi_match_t

    @staticmethod
    def locate_matches_work_bytes(n_items):
        """movi_locate_matches_work_bytes: the bytes of d_work a device call over n_items items needs (host only)."""
        b = C.c_uint64(0)
        check(lib().movi_locate_matches_work_bytes(int(n_items), C.byref(b)))
        return int(b.value)

    def locate_matches_packed(self, bases, offs, items, max_occ, positions_cap=None, want_err=False):
        """movi_locate_matches_host -> (occ, first, positions, QueryStats[, item err, total, return code]); items: MATCH_DTYPE (or an
        (n, 3) integer array), ordered by read.  positions_cap None: room for a few positions per item, and a second call with room for
        the total where that is more."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        items = np.asarray(items)
        if items.dtype != self.MATCH_DTYPE:
            items = np.ascontiguousarray(items, np.uint32).reshape(-1, 3).view(self.MATCH_DTYPE).reshape(-1)
        items = np.ascontiguousarray(items)
        n, ni = offs.size - 1, items.size
        if positions_cap is None:                                 # a few positions per item first, then room for exactly the total
            occ, first, pos, st, err, total, rc = self.locate_matches_packed(bases, offs, items, max_occ, ni * 4 + 1024, want_err=True)
            if rc == -1 and total > pos.size:
                return self.locate_matches_packed(bases, offs, items, max_occ, total, want_err)
            if want_err:
                return occ, first, pos, st, err, total, rc
            check(rc)
            return occ, first, pos[:total], st
        occ = np.zeros(max(ni, 1), np.uint64)
        first = np.zeros(ni + 1, np.uint64)
        pos = np.zeros(max(int(positions_cap), 1), np.uint64)
        err = np.zeros(max(ni, 1), np.uint8)
        total = C.c_uint64(0)
        st = QueryStatsC()
        rc = lib().movi_locate_matches_host(self._h, bases.ctypes.data, offs.ctypes.data, n, items.ctypes.data, ni, int(max_occ),
                                            occ.ctypes.data, first.ctypes.data, pos.ctypes.data, int(positions_cap), C.byref(total),
                                            err.ctypes.data, C.byref(st))
        if want_err:
            return occ[:ni], first, pos[:int(positions_cap)], QueryStats(st), err[:ni], int(total.value), rc
        check(rc)
        return occ[:ni], first, pos[:int(total.value)], QueryStats(st)

    def locate_matches(self, reads, items, max_occ=100):
        """Per item (read, start, end), ordered by read: (occ, uint64 array of the first min(occ, max_occ) text positions of
        reads[read][start:end] in BWT order).  What `movi query --count --locate` / `--mem --locate` print."""
        bases, offs = _pack_reads(reads)
        occ, first, pos, _ = self.locate_matches_packed(bases, offs, items, max_occ)
        return [(int(occ[i]), pos[int(first[i]): int(first[i + 1])].copy()) for i in range(occ.size)]

    # -- Movi Color: colour tables and multi-class classification -------------------
    MC_DTYPE = np.dtype([("best", "<u2"), ("second", "<u2"), ("colors_count", "<u4"), ("sum_ml", "<u4"), ("best_count", "<u4"), ("second_count", "<u4"), ("reserved_", "<u4")])   # movi_mc_read_t
    DOC_NONE = 0xFFFF

    def build_colors(self, doc_offsets, doc_ids=None, stream=0):
        """movi_color_build: the colour tables from the document end offsets (and taxon ids), built on the device and attached."""
        offs = np.ascontiguousarray(doc_offsets, np.uint64)
        ids = np.ascontiguousarray(doc_ids, np.uint32) if doc_ids is not None else None
        check(lib().movi_color_build(self._h, offs.ctypes.data, ids.ctypes.data if ids is not None else None, offs.size,
                                     C.c_void_p(stream) if stream else None))

    def save_colors(self, path):
        """movi_color_save: the attached tables as the reference's doc_sets_flat.bin."""
        check(lib().movi_color_save(self._h, str(path).encode()))

    def load_colors(self, path, num_species):
        check(lib().movi_color_load(self._h, str(path).encode(), int(num_species)))

    def colors(self):
        """(flat_colors u16, flat offsets per run u64, num_species, to_taxon_id u32 -- empty after a load)."""
        fs, ns = C.c_uint64(0), C.c_uint32(0)
        check(lib().movi_color_get(self._h, C.byref(fs), None, 0, None, 0, C.byref(ns), None, 0))
        flat, inds, taxa = np.zeros(fs.value, np.uint16), np.zeros(self.desc.r, np.uint64), np.zeros(ns.value, np.uint32)
        check(lib().movi_color_get(self._h, None, flat.ctypes.data, flat.size, inds.ctypes.data, inds.size, None, None, 0))
        check(lib().movi_color_get(self._h, None, None, 0, None, 0, None, taxa.ctypes.data, taxa.size))
        return flat, inds, int(ns.value), taxa[:int(self.info("color_taxa"))]

    def multi_classify_packed(self, bases, offs, min_len=1, want_counts=True, want_pml=False, want_err=False):
        """movi_multi_classify_host -> (per-read records (MC_DTYPE), counter rows [n, num_species] or None, u16 PMLs or None,
        QueryStats[, err, rc])."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offs = np.ascontiguousarray(offs, np.uint64)
        n = offs.size - 1
        ns = C.c_uint32(0)
        check(lib().movi_color_get(self._h, None, None, 0, None, 0, C.byref(ns), None, 0))
        out = np.zeros(max(n, 1), self.MC_DTYPE)
        counts = np.zeros((max(n, 1), ns.value), np.uint32) if want_counts else None
        pml = np.zeros(max(bases.size, 1), np.uint16) if want_pml else None
        err = np.zeros(max(n, 1), np.uint8)
        st = QueryStatsC()
        rc = lib().movi_multi_classify_host(self._h, bases.ctypes.data, offs.ctypes.data, n, int(min_len), out.ctypes.data,
                                            counts.ctypes.data if want_counts else None, pml.ctypes.data if want_pml else None,
                                            err.ctypes.data, C.byref(st))
        res = (out[:n], counts[:n] if want_counts else None, pml[:bases.size] if want_pml else None, QueryStats(st))
        if want_err:
            return res + (err[:n], rc)
        check(rc)
        return res

    def multi_classify(self, reads, min_len=1):
        """Per read (best, second, colors_count, sum_ml, counter row)."""
        bases, offs = _pack_reads(reads)
        out, counts, _, _ = self.multi_classify_packed(bases, offs, min_len)
        return [(int(o["best"]), int(o["second"]), int(o["colors_count"]), int(o["sum_ml"]), counts[i]) for i, o in enumerate(out)]

    # -- device-pointer queries (bench / torch interop) ---------------------------
    def pml_device(self, d_bases, d_offs, n_reads, n_bases, d_out, d_err=0, stream=0, d_order=0):
        check(lib().movi_pml_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases,
                                    C.c_void_p(d_out), C.c_void_p(d_err) if d_err else None,
                                    C.c_void_p(d_order) if d_order else None,
                                    C.c_void_p(stream) if stream else None))

    def unpack_reads_device(self, d_packed, first_base, n_bases, d_out, d_exc_pos=0, d_exc_byte=0, n_exc=0, stream=0):
        """movi_reads_unpack_device on this handle's GPU: 2-bit packed reads -> one byte per base at d_out, for any *_device query."""
        check(lib().movi_reads_unpack_device(self.device, C.c_void_p(d_packed), int(first_base), int(n_bases),
                                             C.c_void_p(d_exc_pos) if d_exc_pos else None, C.c_void_p(d_exc_byte) if d_exc_byte else None,
                                             int(n_exc), C.c_void_p(d_out), C.c_void_p(stream) if stream else None))

    def pml_mask_device(self, d_bases, d_offs, n_reads, n_bases, d_words, first_base=0, d_err=0, stream=0, d_order=0):
        check(lib().movi_pml_mask_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases, int(first_base),
                                         C.c_void_p(d_words), C.c_void_p(d_err) if d_err else None,
                                         C.c_void_p(d_order) if d_order else None,
                                         C.c_void_p(stream) if stream else None))

    def pml_expand_device(self, d_words, d_offs, n_reads, n_bases, d_out, first_base=0, stream=0):
        check(lib().movi_pml_expand_device(self._h, C.c_void_p(d_words), C.c_void_p(d_offs), n_reads, n_bases, int(first_base),
                                           C.c_void_p(d_out), C.c_void_p(stream) if stream else None))

    def pml_classify_device(self, d_bases, d_offs, n_reads, n_bases, bin_width, max_value_thr, d_out, d_above,
                            d_below, d_sum, d_err=0, stream=0, d_order=0):
        """PML walk with Classifier::classify bins fused in; d_out = 0 writes no PML vector."""
        check(lib().movi_pml_classify_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases,
                                             int(bin_width), int(max_value_thr),
                                             C.c_void_p(d_out) if d_out else None, C.c_void_p(d_above),
                                             C.c_void_p(d_below), C.c_void_p(d_sum),
                                             C.c_void_p(d_err) if d_err else None,
                                             C.c_void_p(d_order) if d_order else None,
                                             C.c_void_p(stream) if stream else None))

    def zml_device(self, d_bases, d_offs, n_reads, n_bases, d_out, d_err=0, stream=0, d_order=0):
        check(lib().movi_zml_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases,
                                    C.c_void_p(d_out), C.c_void_p(d_err) if d_err else None,
                                    C.c_void_p(d_order) if d_order else None,
                                    C.c_void_p(stream) if stream else None))

    def count_device(self, d_bases, d_offs, n_reads, n_bases, d_matched, d_count, d_err=0, stream=0, d_order=0):
        check(lib().movi_count_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases,
                                      C.c_void_p(d_matched), C.c_void_p(d_count),
                                      C.c_void_p(d_err) if d_err else None,
                                      C.c_void_p(d_order) if d_order else None,
                                      C.c_void_p(stream) if stream else None))

    def mem_device(self, d_bases, d_offs, n_reads, n_bases, min_len, d_mems, d_n_mems, d_err=0, stream=0, d_order=0):
        """movi_mem_device: MEM j of read i at d_mems[offs[i] + j] (16 bytes each), j < d_n_mems[i]."""
        check(lib().movi_mem_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases, int(min_len),
                                    C.c_void_p(d_mems), C.c_void_p(d_n_mems),
                                    C.c_void_p(d_err) if d_err else None,
                                    C.c_void_p(d_order) if d_order else None,
                                    C.c_void_p(stream) if stream else None))

    def kmer_device(self, d_bases, d_offs, n_reads, n_bases, k, d_runs, d_n_runs, d_found=0, d_err=0, stream=0, d_order=0):
        """movi_kmer_device: run j of read i at d_runs[offs[i] + j] (8 bytes each), j < d_n_runs[i]; d_found[i] = found k-mers."""
        check(lib().movi_kmer_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases, int(k),
                                     C.c_void_p(d_runs), C.c_void_p(d_n_runs),
                                     C.c_void_p(d_found) if d_found else None,
                                     C.c_void_p(d_err) if d_err else None,
                                     C.c_void_p(d_order) if d_order else None,
                                     C.c_void_p(stream) if stream else None))

    def kmer_occ_device(self, d_bases, d_offs, n_reads, n_bases, k, d_occ, d_found=0, d_sum=0, d_err=0, stream=0):
        """movi_kmer_occ_device: d_occ[offs[i] + p] = occurrences of the k-mer at p of read i (u64, all n_bases slots written);
        d_found (u32), d_sum (u64), d_err (u8) per read, each optional."""
        check(lib().movi_kmer_occ_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases, int(k),
                                         C.c_void_p(d_occ),
                                         C.c_void_p(d_found) if d_found else None,
                                         C.c_void_p(d_sum) if d_sum else None,
                                         C.c_void_p(d_err) if d_err else None,
                                         C.c_void_p(stream) if stream else None))

    def locate_matches_device(self, d_bases, d_offs, n_reads, d_items, n_items, max_occ, d_occ, d_first, d_positions, positions_cap,
                              d_work, work_bytes, d_item_err=0, stream=0):
        """movi_locate_matches_device: d_occ[n_items] (u64), d_first[n_items + 1] (u64: exclusive prefix sum of min(occ, max_occ)),
        text positions of item i in d_positions[d_first[i] : d_first[i + 1]] below positions_cap; d_item_err (u8) optional."""
        check(lib().movi_locate_matches_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, C.c_void_p(d_items), n_items,
                                               int(max_occ), C.c_void_p(d_occ), C.c_void_p(d_first), C.c_void_p(d_positions),
                                               int(positions_cap), C.c_void_p(d_item_err) if d_item_err else None,
                                               C.c_void_p(d_work), int(work_bytes), C.c_void_p(stream) if stream else None))

    def locate_device(self, d_pos, n_items, stream=0):
        """movi_locate_device: packed positions in, suffix-array entries out, in place."""
        check(lib().movi_locate_device(self._h, C.c_void_p(d_pos), n_items, C.c_void_p(stream) if stream else None))

    def sa_entries_device(self, d_bases, d_offs, n_reads, n_bases, d_sa, d_pml=0, d_err=0, stream=0, d_order=0):
        check(lib().movi_sa_entries_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases,
                                           C.c_void_p(d_pml) if d_pml else None, C.c_void_p(d_sa),
                                           C.c_void_p(d_err) if d_err else None,
                                           C.c_void_p(d_order) if d_order else None,
                                           C.c_void_p(stream) if stream else None))

    def multi_classify_device(self, d_bases, d_offs, n_reads, n_bases, min_len, d_out, d_counts=0, d_pml=0, d_err=0, stream=0, d_order=0):
        """movi_multi_classify_device: d_out = n_reads 24-byte records; d_counts = 0 keeps the counters in the handle's scratch."""
        check(lib().movi_multi_classify_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offs), n_reads, n_bases, int(min_len),
                                               C.c_void_p(d_out), C.c_void_p(d_counts) if d_counts else None,
                                               C.c_void_p(d_pml) if d_pml else None, C.c_void_p(d_err) if d_err else None,
                                               C.c_void_p(d_order) if d_order else None,
                                               C.c_void_p(stream) if stream else None))

    PREPARE_PML, PREPARE_COUNT, PREPARE_ZML, PREPARE_SA, PREPARE_COLOR = 1, 2, 4, 8, 16

    def prepare(self, what=1 | 2 | 4, stream=0):
        """movi_index_prepare: build the handle's derived tables now (not inside the first query); returns their bytes."""
        n = C.c_uint64(0)
        check(lib().movi_index_prepare(self._h, int(what), C.c_void_p(stream) if stream else None, C.byref(n)))
        return int(n.value)

    def last_launch(self):
        """movi_last_launch: dict(kernel=..., variant=..., block_threads=..., waves_per_cu=..., segmented=..., idx64=...)."""
        li = LaunchInfoC()
        check(lib().movi_last_launch(self._h, C.byref(li)))
        return {"kernel": li.kernel.decode(), "variant": int(li.variant), "block_threads": int(li.block_threads),
                "waves_per_cu": int(li.waves_per_cu), "segmented": int(li.segmented), "idx64": int(li.idx64), "staged": int(li.staged), "ahead": int(li.ahead)}

    def info(self, key):
        """movi_index_info: bytes of the derived tables the handle holds, statistics their builders tallied."""
        v = C.c_double()
        check(lib().movi_index_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def last_stats(self, stream=0):
        st = QueryStatsC()
        check(lib().movi_last_stats(self._h, C.c_void_p(stream) if stream else None, C.byref(st)))
        return QueryStats(st)
