"""2-bit packed reads, host side (no GPU): movi_reads_pack_host / movi_reads_unpack_host (movi_amd/csrc/movi_pack_host.cpp) against the
format include/movi_hip.h states -- base b in byte b >> 2 at bits 2 * (b & 3), A C G T = 0 1 2 3, every other byte code 0 plus an entry
(absolute position, byte) in the sparse exception list -- and the new entry points' place in the C-ABI."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

GUARD = 0xA5


def numpy_pack(x, first_base):
    """The format, restated in numpy: (packed bytes from byte 0 on, exc_pos, exc_byte)."""
    x = np.frombuffer(bytes(x), np.uint8)
    code = np.zeros(256, np.uint8)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    is_exc = ~np.isin(x, np.frombuffer(b"ACGT", np.uint8))
    b = first_base + np.arange(x.size, dtype=np.int64)
    packed = np.zeros((first_base + x.size + 3) >> 2, np.uint8)
    np.bitwise_or.at(packed, b >> 2, (code[x] << (2 * (b & 3))).astype(np.uint8))
    return packed, b[is_exc].astype(np.uint64), x[is_exc]


def inputs(rng, n):
    """What the issue lists: all 256 byte values; ACGT only; N at 0.1 % (at least one, so that short strings have one too)."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    with_n = acgt[rng.integers(0, 4, n)].copy()
    with_n[rng.random(n) < 0.001] = ord("N")
    if n:
        with_n[int(rng.integers(0, n))] = ord("N")
    return {"bytes": rng.integers(0, 256, n).astype(np.uint8), "acgt": acgt[rng.integers(0, 4, n)].copy(), "n": with_n}


def round_trip(x, first_base, threads):
    from movi_amd.engine import pack_reads, packed_bytes, unpack_reads
    packed, pos, byte = pack_reads(x, first_base, threads=threads)
    assert packed.size == packed_bytes(first_base, x.size) == (first_base + x.size + 3) >> 2
    want, wpos, wbyte = numpy_pack(x, first_base)
    assert (packed == want).all() and (pos == wpos).all() and (byte == wbyte).all()
    back = unpack_reads(packed, first_base, x.size, pos, byte, threads=threads)
    assert (back == x).all()


@pytest.mark.parametrize("threads", [1, 4])
def test_round_trip_every_length_and_phase(built_lib, threads):
    rng = np.random.default_rng(20)
    for n in range(0, 71):
        for first_base in range(0, 8):
            for x in inputs(rng, n).values():
                round_trip(x, first_base, threads)


@pytest.mark.parametrize("threads", [1, 4])
def test_round_trip_sliced_over_worker_threads(built_lib, threads):
    """Long enough (>= 2^16 bases per worker) for the slices aligned to four bases to go to threads of their own, and for the
    groups of 32 bases of the vector loop: with and without exceptions inside a group."""
    rng = np.random.default_rng(21)
    for n, first_base in ((4 * 65536 + 77, 0), (4 * 65536 + 131, 3), (5 * 65536 + 2, 6)):
        for x in inputs(rng, n).values():
            round_trip(x, first_base, threads)


def test_hand_written_case(built_lib):
    """ACGTN + acgt at first_base 3: base 3 = A in the top two bits of byte 0; C G T N in byte 1; a c g t in byte 2.  Every
    exception (N, a, c, g, t: bases 7 .. 11) has code 0 in the stream, and so have the padding bits."""
    from movi_amd.engine import pack_reads, unpack_reads
    packed, pos, byte = pack_reads(b"ACGTNacgt", 3)
    assert bytes(packed) == bytes([0b00000000, 0b00111001, 0b00000000])
    assert pos.tolist() == [7, 8, 9, 10, 11] and bytes(byte) == b"Nacgt"
    assert bytes(unpack_reads(packed, 3, 9, pos, byte)) == b"ACGTNacgt"
    # bits of the first byte that belong to earlier bases are kept, the last byte's unused bits are written 0
    buf = np.full(3, 0xFF, np.uint8)
    pack_reads(b"ACGTNacgt", 3, packed=buf)
    assert bytes(buf) == bytes([0b00111111, 0b00111001, 0b00000000])
    # appended batch by batch, a buffer is what one call would have written
    whole, _, _ = pack_reads(b"TTGCATGCAAGT", 0)
    parts = np.zeros(3, np.uint8)
    pack_reads(b"TTGCA", 0, packed=parts)
    pack_reads(b"TGCAAGT", 5, packed=parts)
    assert bytes(parts) == bytes(whole)


def test_capacity_one_too_small_touches_nothing_past_the_caps(built_lib):
    from movi_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(22)
    for n, threads in ((61, 1), (4 * 65536 + 9, 4)):
        x = inputs(rng, n)["bytes"]
        _, wpos, wbyte = numpy_pack(x, 5)
        need = int(wpos.size)
        assert need > 1
        cap = need - 1
        nbytes = (5 + n + 3) >> 2
        packed = np.full(nbytes + 16, GUARD, np.uint8)
        pos = np.full(cap + 4, 0xA5A5A5A5A5A5A5A5, np.uint64)
        byte = np.full(cap + 16, GUARD, np.uint8)
        got = C.c_uint64(0)
        rc = L.movi_reads_pack_host(x.ctypes.data, 5, n, packed.ctypes.data, pos.ctypes.data, byte.ctypes.data, cap, C.byref(got), threads)
        assert rc == -1 and got.value == need and b"exc_cap" in L.movi_last_error()
        assert (packed[nbytes:] == GUARD).all() and (pos[cap:] == 0xA5A5A5A5A5A5A5A5).all() and (byte[cap:] == GUARD).all()
        assert (pos[:cap] == wpos[:cap]).all() and (byte[:cap] == wbyte[:cap]).all()
        # with room for all of them: MOVI_OK, and still nothing past the buffers' ends
        pos = np.full(need + 4, 0xA5A5A5A5A5A5A5A5, np.uint64)
        byte = np.full(need + 16, GUARD, np.uint8)
        rc = L.movi_reads_pack_host(x.ctypes.data, 5, n, packed.ctypes.data, pos.ctypes.data, byte.ctypes.data, need, C.byref(got), threads)
        assert rc == 0 and got.value == need
        assert (packed[nbytes:] == GUARD).all() and (pos[need:] == 0xA5A5A5A5A5A5A5A5).all() and (byte[need:] == GUARD).all()


def test_unpack_refuses_a_bad_exception_list(built_lib):
    from movi_amd._lib import lib
    L = lib()
    packed, out = np.zeros(8, np.uint8), np.zeros(20, np.uint8)
    byte = np.full(2, ord("N"), np.uint8)
    for bad in ([9, 9], [9, 8], [3, 9], [9, 24]):                # equal, descending, before first_base, past the end
        pos = np.array(bad, np.uint64)
        assert L.movi_reads_unpack_host(packed.ctypes.data, 4, 20, pos.ctypes.data, byte.ctypes.data, 2, out.ctypes.data, 1) == -1
        assert b"ascending" in L.movi_last_error()
    pos = np.array([4, 23], np.uint64)
    assert L.movi_reads_unpack_host(packed.ctypes.data, 4, 20, pos.ctypes.data, byte.ctypes.data, 2, out.ctypes.data, 1) == 0
    assert bytes(out) == b"N" + b"A" * 18 + b"N"
    assert L.movi_reads_unpack_host(None, 0, 4, None, None, 0, out.ctypes.data, 1) == -1 and b"NULL" in L.movi_last_error()
    assert L.movi_reads_pack_host(None, 0, 4, packed.ctypes.data, None, None, 0, C.byref(C.c_uint64(0)), 1) == -1
    assert L.movi_reads_packed_bytes(0, 4, None) == -1
    assert L.movi_reads_packed_bytes(2 ** 64 - 2, 4, C.byref(C.c_uint64(0))) == -1


def test_abi_symbols(built_lib):
    """Every new entry point is in the header and in the ctypes table, and the query entry points refuse a NULL handle with
    MOVI_ERR_ARG (no handle exists without a device)."""
    from movi_amd._lib import SYMBOLS, lib
    import movi_amd.engine as E
    L = lib()
    new = ("movi_reads_packed_bytes", "movi_reads_pack_host", "movi_reads_unpack_host", "movi_reads_unpack_device",
           "movi_pml_packed_host", "movi_pml_mask_packed_host")
    assert all(n in SYMBOLS and hasattr(L, n) for n in new)
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    assert all(("int %s(" % n) in header for n in new) and "9 bytes" in header and "one exception per 36 bases" in header
    offs = np.array([0, 4], np.uint64)
    packed, out, words = np.zeros(1, np.uint8), np.zeros(4, np.uint16), np.zeros(2, np.uint32)
    assert L.movi_pml_packed_host(None, packed.ctypes.data, None, None, 0, offs.ctypes.data, 1, out.ctypes.data, None, None) == -1
    assert b"handle" in L.movi_last_error()
    assert L.movi_pml_mask_packed_host(None, packed.ctypes.data, None, None, 0, offs.ctypes.data, 1, words.ctypes.data, None, None) == -1
    assert b"handle" in L.movi_last_error()
    for name in ("pack_reads", "unpack_reads", "packed_bytes"):
        assert callable(getattr(E, name))
    for name in ("unpack_reads_device", "query_pml_packed2", "query_pml_mask_packed2"):
        assert callable(getattr(E.MoveIndex, name))
