"""GPU suite (-m gpu): the cells of (way down x overlapped or not x ASCII or packed reads x kind of call) of the *_host loop that no other
test runs, on the smallest batch that can still go wrong -- reads of 0, 1, 31, 32, 33 and about 150 bases, offsets[0] = 5 (so a chunk's
mask phase and the packed bytes two chunks share are non-trivial), "pipe_chunk_bases" 9 and 5000 (more chunks than the loop has slots):

  * a mixed call ("host_masks" 2: some chunks come down as the vector, the others as reset masks) on packed reads, overlapped;
  * a mixed call on page-locked buffers that "host_overlap" 0 sends down the synchronous loop, ASCII and packed;
  * a masks call ("host_masks" 1) on pageable packed reads (synchronous, expanded on the host);
  * a call without output (the vector stays on the device), overlapped and synchronous, ASCII and packed;
  * the mask words of movi_pml_mask_packed_host in the layout of movi_pml_mask_words, both loops.

Every vector is compared with the oracle's, stats.bases with the total, the counters with the oracle's."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
LEAD = 5


@pytest.fixture(scope="module")
def setup(built_lib, golden_image):
    import movi_amd
    from movi_amd.engine import masks_of_pml, pack_reads, packed_bytes, pinned_empty
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref = B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]
    rng = np.random.default_rng(77)
    reads = []
    for i in range(300):
        L = (0, 1, 31, 32, 33)[i % 5] if i % 5 == i // 5 % 5 else int(rng.integers(140, 161))      # 60 corner reads among 240 of ~150 bases
        s = int(rng.integers(0, len(ref) - 200))
        r = np.frombuffer(ref[s:s + L], np.uint8).copy()
        r[rng.random(L) < 0.03] = ord("N") if i % 7 == 0 else ord("C")
        reads.append(r.tobytes())
    lens = np.array([len(r) for r in reads], np.uint64)
    assert {0, 1, 31, 32, 33} <= set(lens.tolist()) and lens.sum() > 6 * 5000
    raw = np.frombuffer(b"".join(reads), np.uint8)
    offs0 = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    img = golden_image(6)
    cpu = Oracle(img)
    exp, ff, sc = cpu.pml_batch(raw, offs0, threads=4)
    cpu.close()
    offs, nb = offs0 + np.uint64(LEAD), int(raw.size)
    want = np.zeros(LEAD + nb, np.uint16)
    want[LEAD:] = exp
    mwant, mvalid = masks_of_pml(want, offs)

    def buffers(alloc):
        bases = alloc(LEAD + nb, np.uint8)
        bases[:LEAD] = ord("#")
        bases[LEAD:] = raw
        packed = alloc(packed_bytes(LEAD, nb), np.uint8)
        packed[:] = 0xFF                                           # (the bits of the bases before offsets[0] are nobody's)
        _, pos, byte = pack_reads(raw, LEAD, packed=packed)
        return bases, packed, pos, byte

    gpu = movi_amd.MoveIndex.from_image(img)
    yield dict(gpu=gpu, offs=offs, n=len(reads), nb=nb, want=want, ff=ff, sc=sc, mwant=mwant, mvalid=mvalid,
               pinned=buffers(pinned_empty) + (pinned_empty,), pageable=buffers(lambda n, dt: np.zeros(n, dt)) + ((lambda n, dt: np.zeros(n, dt)),))
    gpu.close()


# (name, buffers, "host_overlap", "host_masks" of the calls with a vector)
LOOPS = [("overlapped", "pinned", 1, (2,)), ("synchronous_page_locked", "pinned", 0, (2,)), ("synchronous_pageable", "pageable", 1, (1, 2))]


@pytest.mark.parametrize("chunk_bases", [9, 5000])
@pytest.mark.parametrize("loop", LOOPS, ids=[x[0] for x in LOOPS])
def test_uncovered_cells_equal_the_oracle(setup, loop, chunk_bases):
    from movi_amd._lib import QueryStatsC, lib
    from movi_amd.engine import mask_words
    s, gpu = setup, setup["gpu"]
    _, which, overlap, ways = loop
    bases, packed, pos, byte, alloc = s[which]
    offs, n, nb = s["offs"], s["n"], s["nb"]
    counters = lambda st: (st.bases, st.fast_forwards, st.scans, st.errors)
    gpu.set_option("pipe_chunk_bases", chunk_bases)
    gpu.set_option("host_overlap", overlap)
    gpu.set_option("host_mask_share", 50)
    try:
        for host_masks in ways:
            gpu.set_option("host_masks", host_masks)
            for src in ("ascii", "packed"):
                out = alloc(LEAD + nb, np.uint16)
                out[:] = 0x5A5A
                if src == "ascii":
                    _, st, err, rc = gpu.query_pml_packed(bases, offs, want_err=True, out=out)
                else:
                    _, st, err, rc = gpu.query_pml_packed2(packed, pos, byte, offs, want_err=True, out=out)
                assert rc == 0 and not err.any(), (host_masks, src)
                assert (out[LEAD:] == s["want"][LEAD:]).all() and (out[:LEAD] == 0x5A5A).all(), (host_masks, src)
                assert counters(st) == (nb, s["ff"], s["sc"], 0), (host_masks, src)
        gpu.set_option("host_masks", -1)
        # no output: the walk runs, error bytes and counters come back
        for src in ("ascii", "packed"):
            st, err = QueryStatsC(), np.full(n, 0x77, np.uint8)
            if src == "ascii":
                rc = lib().movi_pml_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, None, err.ctypes.data, C.byref(st))
            else:
                rc = lib().movi_pml_packed_host(gpu._h, packed.ctypes.data, pos.ctypes.data, byte.ctypes.data, pos.size, offs.ctypes.data, n, None,
                                                err.ctypes.data, C.byref(st))
            assert rc == 0 and not err.any() and counters(st) == (nb, s["ff"], s["sc"], 0), src
        # the masks themselves, where movi_pml_mask_words puts them
        words, st, err, rc = gpu.query_pml_mask_packed2(packed, pos, byte, offs, want_err=True)
        assert rc == 0 and not err.any() and counters(st) == (nb, s["ff"], s["sc"], 0)
        assert words.size == mask_words(n, nb) and (words[s["mvalid"]] == s["mwant"][s["mvalid"]]).all()
    finally:
        for key, value in (("pipe_chunk_bases", 0), ("host_overlap", 1), ("host_mask_share", 70), ("host_masks", -1)):
            gpu.set_option(key, value)
