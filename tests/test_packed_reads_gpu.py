"""GPU suite (-m gpu): reads packed two bits per base (include/movi_hip.h, "2-bit packed reads").

  * the unpack kernels (movi_amd/csrc/movi_walk_pack.hip) against movi_reads_unpack_host, byte for byte with guard bytes around the output;
  * movi_reads_unpack_device + movi_pml_device against movi_pml_device on the ASCII bytes and the oracle, on every index type;
  * movi_pml_packed_host / movi_pml_mask_packed_host against movi_pml_host / movi_pml_mask_host word for word, through the
    synchronous and the overlapped path, chunk starts on all four phases of a packed byte;
  * what they refuse; one capture without a warm-up call; and what an ASCII call launches.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xEE
STAT_FIELDS = ("bases", "fast_forwards", "scans", "repositions", "errors", "lane_steps", "wave_steps", "segments", "rewalked")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def stats_tuple(st):
    return tuple(getattr(st, f) for f in STAT_FIELDS)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def concat(reads):
    lens = [len(r) for r in reads]
    offs = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    return np.frombuffer(b"".join(reads), np.uint8).copy(), offs


def take_log():
    from movi_amd._lib import lib
    need = C.c_size_t(0)
    lib().movi_launch_log(None, 0, C.byref(need))               # (switches the log on; clears it)


def read_log():
    from movi_amd._lib import lib
    buf = C.create_string_buffer(1 << 16)
    lib().movi_launch_log(buf, len(buf), None)
    return set(x for x in buf.value.decode().split("\n") if x)


@pytest.fixture(scope="module")
def ref(built_lib):
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


@pytest.fixture(scope="module")
def batch(ref):
    """200 mutated reads of 1 .. 1200 bp (substitutions, N, lower case) and the corner reads; ASCII and packed."""
    from movi_amd.engine import pack_reads
    rng = np.random.default_rng(4242)
    reads = []
    for _ in range(200):
        L = int(rng.integers(1, 1201))
        s = int(rng.integers(0, len(ref) - L))
        r = np.frombuffer(ref[s:s + L], np.uint8).copy()
        u = rng.random(L)
        sub, low = u < 0.02, (u >= 0.025) & (u < 0.03)
        r[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
        r[(u >= 0.02) & (u < 0.025)] = ord("N")
        r[low] = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, int(low.sum()))]
        reads.append(r.tobytes())
    reads += [b"", b"A", b"N", b"%", ref[500:700].lower(), bytes(rng.integers(128, 256, 150).astype(np.uint8))]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]                            # (the corner reads among the others, not at the end)
    bases, offs = concat(reads)
    packed, pos, byte = pack_reads(bases)
    assert pos.size > 300                                        # N, lower case, '%', bytes >= 128: the list is in use
    return {"reads": reads, "bases": bases, "offs": offs, "n": len(reads), "nb": int(bases.size), "packed": packed, "pos": pos, "byte": byte}


@pytest.fixture(scope="module")
def images(ref, golden_image):
    from oracle import build_index as B
    cache = {}

    def get(mode, sep):
        if (mode, sep) not in cache:
            cache[(mode, sep)] = golden_image(mode) if (not sep and mode in (6, 8)) else B.build_index_from_seqs([ref], mode, separators=bool(sep))
        return cache[(mode, sep)]
    return get


@pytest.fixture(scope="module")
def expected(batch, images):
    """The oracle's answer per index image, computed once."""
    from oracle.oracle import Oracle
    cache = {}

    def get(mode, sep):
        if (mode, sep) not in cache:
            cpu = Oracle(images(mode, sep))
            cache[(mode, sep)] = cpu.pml_batch(batch["bases"], batch["offs"], threads=8)
            cpu.close()
        return cache[(mode, sep)]
    return get


# ---- capture (first in this file: nothing has launched the unpack kernels before it) ------------------------------------

def test_capture_unpack_and_walk_without_warmup(batch, images, expected):
    """On a prepared handle, with no warm-up call of the unpack: movi_reads_unpack_device + movi_pml_device captured once in the
    default (global) mode, on a stream of the process's default queue budget; two replays, the second on other reads of the same
    shape, each give the oracle's vector."""
    import movi_amd
    import torch
    from movi_amd.engine import pack_reads
    from oracle.oracle import Oracle
    b = batch
    other = b["bases"].copy()                                    # same shape, other bytes: every read reversed in place
    for i in range(b["n"]):
        lo, hi = int(b["offs"][i]), int(b["offs"][i + 1])
        other[lo:hi] = other[lo:hi][::-1]
    cpu = Oracle(images(6, 0))
    exp2, ff2, sc2 = cpu.pml_batch(other, b["offs"], threads=8)
    cpu.close()
    packed2, pos2, byte2 = pack_reads(other)
    assert pos2.size == b["pos"].size                            # (reversal keeps the number of exceptions: one graph serves both)
    exp1, ff1, sc1 = expected(6, 0)
    SENT = 0x5A5A
    gpu = movi_amd.MoveIndex.from_image(images(6, 0))
    try:
        gpu.prepare()
        scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
        d_packed, d_pos, d_byte = _dev(b["packed"]), _dev(b["pos"].view(np.int64)), _dev(b["byte"])
        d_offs = _dev(b["offs"].view(np.int64))
        d_bases = torch.full((b["nb"],), GUARD, dtype=torch.uint8, device="cuda")
        out = torch.full((b["nb"],), SENT, dtype=torch.int16, device="cuda")
        err = torch.full((b["n"],), 0x77, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                gpu.unpack_reads_device(d_packed.data_ptr(), 0, b["nb"], d_bases.data_ptr(), d_pos.data_ptr(), d_byte.data_ptr(), b["pos"].size,
                                        stream=s.cuda_stream)
                gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), b["n"], b["nb"], out.data_ptr(), err.data_ptr(), s.cuda_stream)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint16) == SENT).all() and (d_bases.cpu().numpy() == GUARD).all()   # nothing ran at capture
        assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
        print("counters after the capture:", [hex(v) for v in stats_tuple(gpu.last_stats())])
        for want, ff, sc, src, pk, ps, by in ((exp1, ff1, sc1, b["bases"], b["packed"], b["pos"], b["byte"]), (exp2, ff2, sc2, other, packed2, pos2, byte2)):
            d_packed.copy_(torch.from_numpy(pk))
            d_pos.copy_(torch.from_numpy(ps.view(np.int64)))
            d_byte.copy_(torch.from_numpy(by))
            d_bases.fill_(GUARD)
            out.fill_(SENT)
            err.fill_(0x77)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert (d_bases.cpu().numpy() == src).all()
            assert (out.cpu().numpy().view(np.uint16) == want).all() and (err.cpu().numpy() == 0).all()
            st = gpu.last_stats()
            print("counters after a replay:", [hex(v) for v in stats_tuple(st)], "want", hex(ff), hex(sc))
            assert (st.fast_forwards, st.scans, st.errors) == (ff, sc, 0)
        assert gpu.info("device_scratch_bytes") == scratch0
    finally:
        gpu.close()


# ---- the unpack kernels against movi_reads_unpack_host ---------------------------------------------------------------------

N_BASES = (0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 4099)
BIG = 2 ** 33 + 1


@pytest.mark.parametrize("first_base", [0, 1, 2, 3, BIG])
def test_unpack_kernel_equals_host(built_lib, first_base):
    """Every length x output misalignment x exception placement.  first_base 2^33 + 1 is the 64-bit index path: the packed
    pointer handed over is 2^31 bytes below the small buffer, so that byte b >> 2 from it is the buffer's byte (b - 2^33) >> 2."""
    import torch
    from movi_amd._lib import check, lib
    from movi_amd.engine import pack_reads, unpack_reads
    L = lib()
    rng = np.random.default_rng(99 + (first_base & 3))
    small = first_base & 3 if first_base == BIG else first_base   # where the host packs: the same phase, a small buffer
    shift = first_base - small                                    # a multiple of four
    PRE, POST = 32, 48
    for n in N_BASES:
        for out_off in (0, 1, 7, 15):
            edge = 16 - out_off if out_off else 16               # the first base of the output's second 16-byte group
            places = {"none": [], "ends": sorted({0, n - 1}) if n else [], "edge": [j for j in (edge - 1, edge) if 0 <= j < n],
                      "all": list(range(n))}
            for name, where in places.items():
                x = ACGT[rng.integers(0, 4, n)].copy()
                x[where] = rng.choice(np.frombuffer(b"N%#acgt\x80\xff", np.uint8), len(where))
                packed, pos, byte = pack_reads(x, small)
                assert pos.tolist() == [small + j for j in where]
                want = unpack_reads(packed, small, n, pos, byte)
                assert (want == x).all()
                d_packed = _dev(packed if packed.size else np.zeros(1, np.uint8))
                d_pos = _dev((pos + np.uint64(shift)).view(np.int64)) if pos.size else None
                d_byte = _dev(byte) if pos.size else None
                d_out = torch.full((PRE + 16 + n + POST,), GUARD, dtype=torch.uint8, device="cuda")
                assert d_out.data_ptr() % 16 == 0
                at = PRE + out_off
                check(L.movi_reads_unpack_device(0, C.c_void_p(d_packed.data_ptr() - (shift >> 2)), first_base, n,
                                                 C.c_void_p(d_pos.data_ptr()) if pos.size else None,
                                                 C.c_void_p(d_byte.data_ptr()) if pos.size else None, pos.size,
                                                 C.c_void_p(d_out.data_ptr() + at), None))
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                tag = (first_base, n, out_off, name)
                assert (got[at:at + n] == want).all(), tag
                assert (got[:at] == GUARD).all() and (got[at + n:] == GUARD).all(), tag


# ---- movi_reads_unpack_device + movi_pml_device on every index type ------------------------------------------------------------

@pytest.mark.parametrize("mode,sep", [(6, 0), (8, 0), (7, 0), (6, 1), (8, 1), (7, 1)])
def test_unpacked_reads_walk_like_ascii_reads(batch, images, expected, mode, sep):
    import movi_amd
    import torch
    b = batch
    exp, ff, sc = expected(mode, sep)
    gpu = movi_amd.MoveIndex.from_image(images(mode, sep))
    try:
        d_offs = _dev(b["offs"].view(np.int64))
        d_ascii = _dev(b["bases"])
        d_packed, d_pos, d_byte = _dev(b["packed"]), _dev(b["pos"].view(np.int64)), _dev(b["byte"])
        d_bases = torch.full((b["nb"],), GUARD, dtype=torch.uint8, device="cuda")
        res = []
        for src in ("ascii", "packed"):
            out = torch.full((b["nb"],), 0x5A5A, dtype=torch.int16, device="cuda")
            err = torch.full((b["n"],), 0x77, dtype=torch.uint8, device="cuda")
            if src == "packed":
                gpu.unpack_reads_device(d_packed.data_ptr(), 0, b["nb"], d_bases.data_ptr(), d_pos.data_ptr(), d_byte.data_ptr(), b["pos"].size)
            gpu.pml_device((d_ascii if src == "ascii" else d_bases).data_ptr(), d_offs.data_ptr(), b["n"], b["nb"], out.data_ptr(), err.data_ptr())
            st = gpu.last_stats()
            res.append((out.cpu().numpy().view(np.uint16), err.cpu().numpy(), stats_tuple(st)))
        assert (d_bases.cpu().numpy() == b["bases"]).all()
        (pa, ea, sa), (pp, ep, sp) = res
        assert (pp == pa).all() and (ep == ea).all() and sp == sa
        assert (pp == exp).all() and (ep == 0).all() and (sp[1], sp[2], sp[4]) == (ff, sc, 0)
    finally:
        gpu.close()


# ---- the host entry points --------------------------------------------------------------------------------------------------

CHUNK_BASES = 9000


def chunk_starts(offs, target):
    """The cut of the overlapped path under "pipe_chunk_bases" (run_pipelined: as many reads as stay within `target` bases, at least one)."""
    starts, first, n = [], 0, offs.size - 1
    while first < n:
        starts.append(int(offs[first]))
        last = int(np.searchsorted(offs, offs[first] + np.uint64(target), side="right")) - 1
        first = min(max(last, first + 1), n)
    return starts


@pytest.mark.parametrize("pinned", [0, 1])
@pytest.mark.parametrize("overlap", [0, 1])
def test_packed_host_calls_equal_ascii_host_calls(batch, images, expected, overlap, pinned):
    import movi_amd
    from movi_amd.engine import mask_words, masks_of_pml, pack_reads, packed_bytes, pinned_empty
    b = batch
    exp, ff, sc = expected(6, 0)
    starts = chunk_starts(b["offs"], CHUNK_BASES)
    assert len(starts) >= 5 and {s & 3 for s in starts} == {0, 1, 2, 3}
    gpu = movi_amd.MoveIndex.from_image(images(6, 0))
    try:
        gpu.set_option("pipe_chunk_bases", CHUNK_BASES)
        gpu.set_option("host_overlap", overlap)
        alloc = pinned_empty if pinned else (lambda n, dt: np.zeros(n, dt))
        for lead in (0, 6):                                       # lead 6: a call whose h_offsets[0] is 6
            offs = b["offs"] + np.uint64(lead)
            bases = alloc(lead + b["nb"], np.uint8)
            bases[:lead] = ord("#")
            bases[lead:] = b["bases"]
            packed = alloc(packed_bytes(lead, b["nb"]), np.uint8)
            packed[:] = 0xFF if lead else 0                       # (bits of the bases before offsets[0] are nobody's)
            _, pos, byte = pack_reads(b["bases"], lead, packed=packed)
            assert (pos == b["pos"] + np.uint64(lead)).all()
            want = np.zeros(lead + b["nb"], np.uint16)
            want[lead:] = exp
            mwant, mvalid = masks_of_pml(want, offs)
            for host_masks in ((0, 1) if pinned and overlap else (0,)):   # 1: the vector through masks + host expansion
                gpu.set_option("host_masks", host_masks)
                out_a, out_p = alloc(lead + b["nb"], np.uint16), alloc(lead + b["nb"], np.uint16)
                out_a[:], out_p[:] = 0x5A5A, 0x5A5A
                _, st_a, err_a, rc_a = gpu.query_pml_packed(bases, offs, want_err=True, out=out_a)
                _, st_p, err_p, rc_p = gpu.query_pml_packed2(packed, pos, byte, offs, want_err=True, out=out_p)
                assert rc_a == 0 and rc_p == 0
                assert (out_p == out_a).all() and (err_p == err_a).all() and stats_tuple(st_p) == stats_tuple(st_a)
                assert (out_p[lead:] == exp).all() and (out_p[:lead] == 0x5A5A).all() and (err_p == 0).all()
                assert (st_p.bases, st_p.fast_forwards, st_p.scans, st_p.errors) == (b["nb"], ff, sc, 0)
            w_a, mst_a, merr_a, mrc_a = gpu.query_pml_mask_packed(bases, offs, want_err=True)
            w_p, mst_p, merr_p, mrc_p = gpu.query_pml_mask_packed2(packed, pos, byte, offs, want_err=True)
            assert mrc_a == 0 and mrc_p == 0 and w_p.size == mask_words(b["n"], b["nb"])
            assert (w_p[mvalid] == w_a[mvalid]).all() and (merr_p == merr_a).all() and stats_tuple(mst_p) == stats_tuple(mst_a)
            assert (w_p[mvalid] == mwant[mvalid]).all() and (mst_p.fast_forwards, mst_p.scans, mst_p.errors) == (ff, sc, 0)
    finally:
        gpu.close()


def test_refusals(batch, images):
    import movi_amd
    from movi_amd._lib import QueryStatsC, lib
    L = lib()
    b = batch
    gpu = movi_amd.MoveIndex.from_image(images(6, 0))
    try:
        offs = b["offs"] + np.uint64(8)
        packed = np.zeros((8 + b["nb"] + 3) >> 2, np.uint8)
        out = np.zeros(8 + b["nb"], np.uint16)
        words = np.zeros(b["nb"] // 32 + b["n"] + 2, np.uint32)
        byte = np.full(2, ord("N"), np.uint8)

        def both(packed_p, pos, byte_p, n_exc, offs_p=offs.ctypes.data, n=b["n"], out_p=out.ctypes.data, words_p=words.ctypes.data, stats=None):
            pos_p = pos.ctypes.data if pos is not None else None
            return (L.movi_pml_packed_host(gpu._h, packed_p, pos_p, byte_p, n_exc, offs_p, n, out_p, None, stats),
                    L.movi_pml_mask_packed_host(gpu._h, packed_p, pos_p, byte_p, n_exc, offs_p, n, words_p, None, stats))

        end = int(offs[-1])
        for bad in ([20, 19], [20, 20], [7, 20], [20, end]):       # descending, equal, below offsets[0], at offsets[n]
            assert both(packed.ctypes.data, np.array(bad, np.uint64), byte.ctypes.data, 2) == (-1, -1), bad
            assert b"ascending" in L.movi_last_error()
        assert both(None, None, None, 0) == (-1, -1) and b"NULL" in L.movi_last_error()
        assert both(packed.ctypes.data, None, byte.ctypes.data, 2) == (-1, -1) and b"NULL" in L.movi_last_error()
        assert both(packed.ctypes.data, np.array([20, 21], np.uint64), None, 2) == (-1, -1)
        assert both(packed.ctypes.data, None, None, 0, offs_p=None) == (-1, -1)
        assert both(packed.ctypes.data, None, None, 0, words_p=None)[1] == -1
        # n_reads 0 is accepted whatever the pointers, and the stats are zeroed
        st = QueryStatsC()
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        assert both(None, None, None, 0, offs_p=None, n=0, out_p=None, words_p=None, stats=C.byref(st)) == (0, 0)
        assert all(getattr(st, f) == 0 for f in STAT_FIELDS)
        # (and a list that is in order at the range's very ends is taken)
        good = np.array([8, end - 1], np.uint64)
        assert both(packed.ctypes.data, good, byte.ctypes.data, 2) == (0, 0)
    finally:
        gpu.close()


def test_ascii_host_call_launches_what_it_did(batch, images):
    """movi_launch_log: an ASCII movi_pml_host call launches its walk kernels and nothing of the packed path; the packed call
    launches the same walk kernels behind the two unpack kernels."""
    import movi_amd
    b = batch
    gpu = movi_amd.MoveIndex.from_image(images(6, 0))
    try:
        take_log()
        gpu.query_pml_packed(b["bases"], b["offs"])
        ascii_log = read_log()
        assert ascii_log and all(k.startswith("pml_kernel") for k in ascii_log), ascii_log
        gpu.query_pml_packed2(b["packed"], b["pos"], b["byte"], b["offs"])
        assert read_log() == ascii_log | {"unpack_reads_kernel", "unpack_exceptions_kernel"}
        gpu.query_pml_mask_packed(b["bases"], b["offs"])
        assert not any(k.startswith("unpack") for k in read_log())
    finally:
        gpu.close()
