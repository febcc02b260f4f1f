"""GPU suite (-m gpu): PARKED LANES of the mask walk ("park_lanes" option; DevIndex::park_at).  A wavefront of the reset-mask walk
(pml_kernel_flatp<..., RING = 2>) leaves its loop when at most T of its lanes still walk, parks their state in a queue in device
scratch and retires its other reads; a second launch of the same kernel resumes the parked reads 64 to a wavefront.  Whatever T,
the u16 vector, the mask words, the per-read error bytes and the fast-forward / scan / reposition counters must be what they are
without parking ("park_lanes" 0) and what the oracle says -- on the plain, the look-ahead and the deep rows, for reads around the
top-of-walk table's K, reads that roll through the staged stretch (a resumed lane stages again mid-read), illegal bases, failing
reads on a corrupt table, the routes on which the walk must not park (a vector that is not 16-byte aligned, a caller's read order)
and under a stream capture.  movi_index_info "parked_reads" keeps the cases from being vacuous."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_parity import mutated_reads, pack

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
MASK_KERNEL_DEEP = "pml_kernel_flatp<6, unsigned int, 0, 0, 0, 1, 2, 0, 2>"
THRESHOLDS = (1, 8, 32, 63)


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _ragged_reads(ref):
    """200 reads = three full wavefronts and one partial.  Reads 0 .. 63 are identical (a wavefront in which nothing can park); the
    other two full wavefronts and the partial one are ragged: lengths 1, <= 12 and exactly 13 (around the top-of-walk table), reads
    of 700 .. 1200 bases (longer than the 336 bases a lane stages: a resumed lane stages mid-read and rolls again), N, lower case
    and a byte >= 128."""
    rng = np.random.default_rng(20260)
    same = [ref[5000:5150]] * 64
    special = [b"A", b"C", ref[10:12], ref[100:107], ref[200:212], ref[300:313], ref[400:413], b"N", b"N" * 20,
               ref[500:560] + b"N" + ref[561:640], ref[700:800].lower(), ref[900:950] + b"\x80\xff" + ref[952:1000],
               b"acgtn" * 9, ref[1100:1113].lower()]
    long_reads = mutated_reads(rng, ref, 10, 700, 1200)
    body = mutated_reads(rng, ref, 136 - len(special) - len(long_reads), 20, 330)
    ragged = special + long_reads + body
    order = rng.permutation(len(ragged))
    reads = same + [ragged[i] for i in order]
    assert len(reads) == 200
    return reads


@pytest.fixture(scope="module")
def ragged(built_lib, golden_image):
    """The ragged batch on the golden index with the oracle's answers: computed once, shared, left unchanged."""
    from oracle.oracle import Oracle
    img = golden_image(6)
    reads = _ragged_reads(_ref())
    bases, offs = pack(reads)
    cpu = Oracle(img)
    exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
    cpu.close()
    return dict(img=img, reads=reads, bases=bases, offs=offs, n=len(reads), nb=int(bases.size), exp=exp, ff=ff, sc=sc)


def _rows(gpu, rows):
    """Force the table layout the walk runs on; returns what last_launch()["ahead"] must then say."""
    if rows == "plain":
        gpu.set_option("ahead_rows", 0)
        return 0
    if rows == "ahead":
        gpu.set_option("ahead_rows", 1)
        return 1
    gpu.set_option("deep_rows", 1)
    return 2


def _pml_device(gpu, d_bases, d_offs, n, nb, T, align=0, d_order=None, stream=0):
    """One movi_pml_device call at "park_lanes" T -> (vector, error bytes, stats, parked reads, park_lanes of the launch, kernel)."""
    import torch
    gpu.set_option("park_lanes", T)
    out = torch.full((nb + 8,), SENT, dtype=torch.int16, device="cuda")
    err = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr() + 2 * align, err.data_ptr(), stream,
                   d_order.data_ptr() if d_order is not None else 0)
    st = gpu.last_stats(stream)
    got = out.cpu().numpy().view(np.uint16)
    assert (got[:align] == SENT).all() and (got[align + nb:] == SENT).all()            # nothing outside the vector
    li = gpu.last_launch()
    return (got[align:align + nb].copy(), err.cpu().numpy().copy(), (st.fast_forwards, st.scans, st.repositions, st.errors),
            int(gpu.info("parked_reads")), int(gpu.info("park_lanes")), li["kernel"], li["ahead"])


@pytest.mark.parametrize("rows", ["plain", "ahead", "deep"])
def test_forced_thresholds_vs_off_and_oracle(ragged, rows):
    import movi_amd
    b = ragged
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare(gpu.PREPARE_PML)
        want_ahead = _rows(gpu, rows)
        gpu.set_option("pml_via_mask", 1)
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        v0, e0, s0, parked0, lanes0, kern0, ahead0 = _pml_device(gpu, d_bases, d_offs, b["n"], b["nb"], 0)
        assert ahead0 == want_ahead and kern0.endswith(", 2>"), (kern0, ahead0)
        if rows == "deep":
            assert kern0 == MASK_KERNEL_DEEP
        assert (parked0, lanes0) == (0, 0)
        assert (v0 == b["exp"]).all() and (e0 == 0).all() and s0[:2] == (b["ff"], b["sc"]) and s0[3] == 0
        for T in THRESHOLDS:
            v, e, s, parked, lanes, kern, ahead = _pml_device(gpu, d_bases, d_offs, b["n"], b["nb"], T)
            print("rows %s T %d: parked %d of %d reads" % (rows, T, parked, b["n"]))
            assert (kern, ahead, lanes) == (kern0, ahead0, T)
            assert (v == b["exp"]).all(), (rows, T, np.flatnonzero(v != b["exp"])[:8])
            assert (e == e0).all() and s == s0, (rows, T, s, s0)
            assert parked > 0, (rows, T)
            if T == 63:
                assert 2 * parked >= b["n"], (rows, parked)
        # a wavefront of identical reads: its lanes finish in the same iteration, whatever T
        for T in THRESHOLDS:
            v, e, s, parked, lanes, _, _ = _pml_device(gpu, d_bases, d_offs, 64, int(b["offs"][64]), T)
            assert lanes == T and parked == 0 and (v == b["exp"][:int(b["offs"][64])]).all() and (e == 0).all()
    finally:
        gpu.close()


def test_mask_words_with_a_phase(ragged):
    """movi_pml_mask_device at a first_base that is no multiple of 32: every word, written or not, as without parking."""
    import movi_amd
    import torch
    from movi_amd.engine import mask_words
    b = ragged
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare(gpu.PREPARE_PML)
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        first_base = 1000 * 32 + 13
        nw = mask_words(b["n"], b["nb"]) + 2
        got = {}
        for T in (0,) + THRESHOLDS:
            gpu.set_option("park_lanes", T)
            words = torch.full((nw,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
            err = torch.full((b["n"],), 0x77, dtype=torch.uint8, device="cuda")
            gpu.pml_mask_device(d_bases.data_ptr(), d_offs.data_ptr(), b["n"], b["nb"], words.data_ptr(), first_base, err.data_ptr())
            st = gpu.last_stats()
            assert gpu.last_launch()["kernel"].endswith(", 2>") and int(gpu.info("park_lanes")) == T
            parked = int(gpu.info("parked_reads"))
            assert (parked > 0) == (T > 0), (T, parked)
            got[T] = (words.cpu().numpy().copy(), err.cpu().numpy().copy(), (st.fast_forwards, st.scans, st.repositions, st.errors))
        assert (got[0][1] == 0).all() and got[0][2][:2] == (b["ff"], b["sc"])
        for T in THRESHOLDS:
            assert (got[T][0] == got[0][0]).all() and (got[T][1] == got[0][1]).all() and got[T][2] == got[0][2], T
    finally:
        gpu.close()


def test_routes_that_do_not_park(ragged):
    """A vector that is not 16-byte aligned and a caller's read order leave the fused route: whichever route the plan takes, the
    answers are the same and last_launch names the kernel it always named."""
    import movi_amd
    b = ragged
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare(gpu.PREPARE_PML)
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        order = np.random.default_rng(5).permutation(b["n"]).astype(np.uint32)
        d_order = _dev(order.view(np.int32))
        for T in (0, 8, 63):
            for align, d_ord in ((1, None), (3, None), (0, d_order)):
                v, e, s, parked, lanes, kern, ahead = _pml_device(gpu, d_bases, d_offs, b["n"], b["nb"], T, align=align, d_order=d_ord)
                assert kern == MASK_KERNEL_DEEP and ahead == 2                       # (the default policy on this index: deep rows, masks)
                assert (v == b["exp"]).all() and (e == 0).all() and s[:2] == (b["ff"], b["sc"]), (T, align)
                assert lanes == 0 and parked == 0, (T, align, lanes, parked)    # neither route is the fused one: nothing parks
    finally:
        gpu.close()


def test_failing_reads_that_were_parked(built_lib, golden_image):
    """A table with corrupt ids: reads whose walk throws.  Every wavefront starts with an empty read, so at T = 63 its loop never
    runs and EVERY other read of the batch is parked before its first step -- the failing ones included: same error codes, all-zero
    PMLs, same counters as without parking."""
    import movi_amd
    ref = _ref()
    img = bytearray(golden_image(6))
    _, _, off, _ = movi_amd.parse_index_image(bytes(img))
    rows = np.frombuffer(img, np.uint8, count=118209 * 8, offset=off).reshape(-1, 8).copy()
    rows[::97, 0:4] = 0xFF
    img[off: off + rows.size] = rows.tobytes()
    reads = mutated_reads(np.random.default_rng(9801), ref, 189, 20, 300)
    for i in (0, 64, 128):
        reads.insert(i, b"")
    bases, offs = pack(reads)
    n, nb = len(reads), int(bases.size)
    bad = movi_amd.MoveIndex.from_image(bytes(img))
    try:
        bad.prepare(bad.PREPARE_PML)
        bad.set_option("pml_via_mask", 1)
        d_bases, d_offs = _dev(bases), _dev(offs.view(np.int64))
        for rows_kind in ("plain", "deep"):
            _rows(bad, rows_kind)
            v0, e0, s0, parked0, _, kern0, _ = _pml_device(bad, d_bases, d_offs, n, nb, 0)
            assert parked0 == 0 and s0[3] > 0 and s0[3] == int((e0 != 0).sum())
            for i in np.flatnonzero(e0 != 0):
                assert (v0[int(offs[i]):int(offs[i + 1])] == 0).all()
            for T in (63, 8):
                v, e, s, parked, lanes, kern, _ = _pml_device(bad, d_bases, d_offs, n, nb, T)
                assert kern == kern0 and lanes == T
                assert (v == v0).all() and (e == e0).all() and s == s0, (rows_kind, T)
                if T == 63:
                    assert parked == n - 3, (rows_kind, parked)
                else:
                    assert parked > 0
    finally:
        bad.close()


def test_capture_without_warmup(ragged):
    """After prepare and the option, with no warm-up call: one movi_pml_device call captured in the default (global) mode allocates
    nothing, and two replays on different read bytes of the same shape each give the oracle's vector."""
    import movi_amd
    import torch
    from oracle.oracle import Oracle
    b = ragged
    other = np.array(b["bases"])                                   # same shape, other bytes: every read reversed in place
    for i in range(b["n"]):
        lo, hi = int(b["offs"][i]), int(b["offs"][i + 1])
        other[lo:hi] = other[lo:hi][::-1]
    cpu = Oracle(b["img"])
    exp2, ff2, sc2 = cpu.pml_batch(other, b["offs"], threads=4)
    cpu.close()
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare()
        gpu.set_option("park_lanes", 8)
        scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        out = torch.full((b["nb"],), SENT, dtype=torch.int16, device="cuda")
        err = torch.full((b["n"],), 0x77, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), b["n"], b["nb"], out.data_ptr(), err.data_ptr(), s.cuda_stream)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert gpu.last_launch()["kernel"] == MASK_KERNEL_DEEP and int(gpu.info("park_lanes")) == 8
        assert (out.cpu().numpy().view(np.uint16) == SENT).all()                  # nothing ran at capture
        assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
        for want, want_ff, want_sc, src in ((b["exp"], b["ff"], b["sc"], b["bases"]), (exp2, ff2, sc2, other)):
            d_bases.copy_(torch.from_numpy(np.array(src)))
            out.fill_(SENT)
            err.fill_(0x77)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert (out.cpu().numpy().view(np.uint16) == want).all() and (err.cpu().numpy() == 0).all()
            st = gpu.last_stats()
            assert (st.fast_forwards, st.scans, st.errors) == (want_ff, want_sc, 0)
            assert int(gpu.info("parked_reads")) > 0
        assert gpu.info("device_scratch_bytes") == scratch0
    finally:
        gpu.close()
