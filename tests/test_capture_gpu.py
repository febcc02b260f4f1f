"""GPU suite (-m gpu): the *_device entry points after movi_index_prepare keep their promise -- they allocate nothing, can be
captured into a HIP graph in the default (global) capture mode with no warm-up call, and the graphs replay to the oracle's answers --
and the reset-mask route of movi_pml_device holds at the edges where it could go wrong:

* a captured call whose mask words outgrow the reservation takes the packer route instead of allocating;
* a graph stays valid after a bigger uncaptured call has grown the mask words (the buffer it uses is retired, not freed);
* an output vector that is not 16-byte aligned, every first_base phase of the mask layout, a caller's d_read_order.

movi_index_info "device_scratch_bytes" makes "allocated nothing" exact.  Every graph is single-stream.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, classify_py
from test_gpu_parity import mutated_reads, pack

pytestmark = pytest.mark.gpu

SENT = 0x5A5A                      # sentinel of output vectors: every element a call writes differs from what it held


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _edge_reads(ref):
    return [b"", b"A", ref[100:131], ref[200:232], ref[300:333], b"N" * 40, b"N", ref[400:401] + b"N" * 31, ref[500:650]]


@pytest.fixture(scope="module")
def images(built_lib, golden_image):
    from oracle import build_index as B
    return {"mode6": golden_image(6), "mode8": golden_image(8),
            "separators": B.build_index_from_seqs([_ref()], 6, separators=True)}


def _fresh(img):
    import movi_amd
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.prepare()
    return gpu


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a))                     # (a copy: the packed reads are read-only buffers)
    return t.to(torch.device("cuda", 0)) if dtype is None else t.view(dtype).to(torch.device("cuda", 0))


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _short_batch(seed, n=1500):
    ref = _ref()
    reads = mutated_reads(np.random.default_rng(seed), ref, n, 1, 300) + _edge_reads(ref)
    return pack(reads)


def _capture(fn, stream):
    """fn() captured on `stream` in the default (global) mode; returns the graph (its capture must succeed)."""
    import torch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        try:
            fn()
        finally:
            g.capture_end()                                     # (a call that failed the capture still ends it)
    return g


@pytest.mark.parametrize("name", ["mode6", "mode8", "separators"])
def test_capture_without_warmup_in_global_mode(images, name):
    """A fresh prepared handle: one call of every *_device entry point captured with no warm-up call before it.  Nothing runs at
    capture, nothing is allocated (device_scratch_bytes and derived_bytes exact), two replays each give the oracle's vectors, masks,
    bins, counts and error bytes; movi_pml_device's default route is the fused-mask walk (RING = 2)."""
    import torch
    from movi_amd.engine import mask_words, masks_of_pml
    from oracle.oracle import Oracle
    img = images[name]
    cpu = Oracle(img)
    bases, offs = _short_batch({"mode6": 11, "mode8": 12, "separators": 13}[name])
    n, nb = offs.size - 1, int(bases.size)
    exp, _, _ = cpu.pml_batch(bases, offs, threads=4)
    expz = cpu.zml_batch(bases, offs, threads=4)
    em, ec = cpu.count_batch(bases, offs, threads=4)
    ew, valid = masks_of_pml(exp, offs)
    bw, thr = 40, 5
    ecls = [classify_py(exp[int(offs[i]):int(offs[i + 1])], thr, bw) if offs[i + 1] > offs[i] else None for i in range(n)]
    d_bases, d_offs = _dev(bases), _dev(offs.view(np.int64))
    gpu = _fresh(img)
    scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
    s = torch.cuda.Stream()
    vec = lambda: torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
    err = lambda: torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")

    def check_vec(out, e, want):
        assert (_u16(out) == want).all()
        assert (e.cpu().numpy() == 0).all()

    def check_untouched_vec(out, e):
        assert (_u16(out) == SENT).all() and (e.cpu().numpy() == 0x77).all()

    cases = []
    # movi_pml_device: default route, and the register packer ("pml_via_mask" 0)
    for via in (-1, 0):
        out, e = vec(), err()
        cases.append(("pml_device/%d" % via, via,
                      lambda out=out, e=e: gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), e.data_ptr(), s.cuda_stream),
                      lambda out=out, e=e: check_untouched_vec(out, e),
                      lambda out=out, e=e: check_vec(out, e, exp),
                      lambda out=out, e=e: (out.fill_(SENT), e.fill_(0x77))))
    # movi_pml_mask_device, movi_pml_expand_device (masks of the oracle's vector in)
    nw = mask_words(n, nb)
    words, we = torch.full((nw,), -1, dtype=torch.int32, device="cuda"), err()

    def check_words():
        got = words.cpu().numpy().view(np.uint32)
        assert (got[valid] == ew[valid]).all()
        assert (we.cpu().numpy() == 0).all()
    cases.append(("pml_mask_device", -1,
                  lambda: gpu.pml_mask_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, words.data_ptr(), 0, we.data_ptr(), s.cuda_stream),
                  lambda: (words.cpu().numpy() == -1).all() or pytest.fail("mask words written at capture"),
                  check_words, lambda: (words.fill_(-1), we.fill_(0x77))))
    d_ew, xout = _dev(ew.view(np.int32)), vec()
    cases.append(("pml_expand_device", -1,
                  lambda: gpu.pml_expand_device(d_ew.data_ptr(), d_offs.data_ptr(), n, nb, xout.data_ptr(), 0, s.cuda_stream),
                  lambda: (_u16(xout) == SENT).all() or pytest.fail("vector written at capture"),
                  lambda: (_u16(xout) == exp).all() or pytest.fail("expanded vector differs"), lambda: xout.fill_(SENT)))
    # movi_pml_classify_device: bins fused (with and without the vector) and the two-pass route ("classify_fused" 0, d_read_err)
    for fused, with_vec in ((1, True), (1, False), (0, True)):
        out, e = vec(), err()
        a = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        b = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        sm = torch.full((n,), -1, dtype=torch.int64, device="cuda")

        def check_cls(out=out, e=e, a=a, b=b, sm=sm, with_vec=with_vec):
            aa, bb, ss = a.cpu().numpy(), b.cpu().numpy(), sm.cpu().numpy()
            for i, c in enumerate(ecls):
                if c is None:
                    continue                                   # (an empty read has no bins: its entries are the caller's)
                _, avg, ea, eb = c
                assert (aa[i], bb[i]) == (ea, eb) and ss[i] == round(avg * (ea + eb)), (i, aa[i], bb[i], ss[i], c)
            assert (e.cpu().numpy() == 0).all()
            assert (_u16(out) == exp).all() if with_vec else (_u16(out) == SENT).all()

        def untouched_cls(out=out, e=e, a=a):
            assert (a.cpu().numpy() == -1).all() and (_u16(out) == SENT).all() and (e.cpu().numpy() == 0x77).all()
        cases.append(("pml_classify_device/%d/%d" % (fused, with_vec), fused,
                      lambda out=out, e=e, a=a, b=b, sm=sm, with_vec=with_vec: gpu.pml_classify_device(
                          d_bases.data_ptr(), d_offs.data_ptr(), n, nb, bw, thr, out.data_ptr() if with_vec else 0, a.data_ptr(),
                          b.data_ptr(), sm.data_ptr(), e.data_ptr(), s.cuda_stream),
                      untouched_cls, check_cls,
                      lambda out=out, e=e, a=a, b=b, sm=sm: (out.fill_(SENT), e.fill_(0x77), a.fill_(-1), b.fill_(-1), sm.fill_(-1))))
    # movi_count_device, movi_zml_device
    dm, dc, ce = torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((n,), -1, dtype=torch.int64, device="cuda"), err()

    def check_count():
        assert (dm.cpu().numpy().view(np.uint64) == em).all() and (dc.cpu().numpy().view(np.uint64) == ec).all()
        assert (ce.cpu().numpy() == 0).all()
    cases.append(("count_device", -1,
                  lambda: gpu.count_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, dm.data_ptr(), dc.data_ptr(), ce.data_ptr(), s.cuda_stream),
                  lambda: (dm.cpu().numpy() == -1).all() or pytest.fail("counts written at capture"),
                  check_count, lambda: (dm.fill_(-1), dc.fill_(-1), ce.fill_(0x77))))
    zout, ze = vec(), err()
    cases.append(("zml_device", -1,
                  lambda: gpu.zml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, zout.data_ptr(), ze.data_ptr(), s.cuda_stream),
                  lambda: check_untouched_vec(zout, ze), lambda: check_vec(zout, ze, expz),
                  lambda: (zout.fill_(SENT), ze.fill_(0x77))))
    try:
        for label, opt, call, untouched, check, reset in cases:
            if label.startswith("pml_device"):
                gpu.set_option("pml_via_mask", opt)
            if label.startswith("pml_classify_device"):
                gpu.set_option("classify_fused", opt)
            torch.cuda.synchronize()
            g = _capture(call, s)
            if label == "pml_device/-1":
                assert gpu.last_launch()["kernel"].endswith(", 2>"), gpu.last_launch()["kernel"]
            torch.cuda.synchronize()
            untouched()
            assert gpu.info("device_scratch_bytes") == scratch0, label
            assert gpu.info("derived_bytes") == derived0, label
            for _ in range(2):
                g.replay()
                torch.cuda.synchronize()
                check()
                reset()
                torch.cuda.synchronize()
            gpu.set_option("pml_via_mask", -1)
            gpu.set_option("classify_fused", -1)
        assert gpu.info("device_scratch_bytes") == scratch0
    finally:
        gpu.close()
        cpu.close()


@pytest.fixture(scope="module")
def big_batch(images):
    """A few thousand distinct short reads (edge lengths included) repeated into a batch whose mask words outgrow what
    movi_index_prepare reserves: the oracle runs on the distinct reads only and its vector is tiled."""
    import torch
    from movi_amd.engine import mask_words
    from oracle.oracle import Oracle
    img = images["mode6"]
    ref = _ref()
    reads = mutated_reads(np.random.default_rng(4242), ref, 3000, 1, 64) + _edge_reads(ref)
    bases, offs = pack(reads)
    cpu = Oracle(img)
    exp, _, _ = cpu.pml_batch(bases, offs, threads=4)
    cpu.close()
    gpu = _fresh(img)
    reserved = int(gpu.info("device_scratch_bytes"))           # (mask words only, right after the prepare call)
    gpu.close()
    tn, tb = offs.size - 1, int(bases.size)
    reps = 1
    while mask_words(tn * reps, tb * reps) * 4 <= reserved + (reserved >> 2):
        reps *= 2
    dev = torch.device("cuda", 0)
    d_bases = _dev(bases).repeat(reps)
    rel = torch.from_numpy(offs[:-1].view(np.int64).copy()).to(dev)
    d_offs = torch.cat([(rel.unsqueeze(0) + tb * torch.arange(reps, device=dev, dtype=torch.int64).unsqueeze(1)).reshape(-1),
                        torch.tensor([tb * reps], dtype=torch.int64, device=dev)])
    return dict(img=img, bases=bases, offs=offs, exp=exp, reps=reps, n=tn * reps, nb=tb * reps, d_bases=d_bases, d_offs=d_offs,
                reserved=reserved)


def _check_tiled(out, big):
    got = _u16(out).reshape(big["reps"], -1)
    assert (got == big["exp"][None, :]).all()


def test_capture_beyond_the_reservation_takes_the_packer(big_batch):
    """A captured movi_pml_device call whose mask words do not fit what the handle holds: no allocation (the capture succeeds in
    global mode, device_scratch_bytes unchanged), the packer walk (RING = 0) instead, the oracle's vector on replay."""
    import torch
    from movi_amd.engine import mask_words
    big = big_batch
    assert mask_words(big["n"], big["nb"]) * 4 > big["reserved"]
    gpu = _fresh(big["img"])
    try:
        scratch0 = gpu.info("device_scratch_bytes")
        out = torch.full((big["nb"],), SENT, dtype=torch.int16, device="cuda")
        e = torch.full((big["n"],), 0x77, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = _capture(lambda: gpu.pml_device(big["d_bases"].data_ptr(), big["d_offs"].data_ptr(), big["n"], big["nb"], out.data_ptr(),
                                            e.data_ptr(), s.cuda_stream), s)
        assert gpu.last_launch()["kernel"].endswith(", 0>"), gpu.last_launch()["kernel"]
        assert gpu.info("device_scratch_bytes") == scratch0
        torch.cuda.synchronize()
        assert int((out != SENT).sum().item()) == 0
        g.replay()
        torch.cuda.synchronize()
        _check_tiled(out, big)
        assert int(e.sum().item()) == 0
    finally:
        gpu.close()


def test_graph_replays_after_a_bigger_call_grew_the_masks(big_batch):
    """A graph captured over a small movi_pml_device call, then an uncaptured call more than 4x bigger on the same handle (it grows
    the mask words): the graph's buffer is retired, not freed -- device_scratch_bytes holds both -- and the replay still gives the
    oracle's vector."""
    import torch
    from movi_amd.engine import mask_words
    big = big_batch
    bases, offs, exp = big["bases"], big["offs"], big["exp"]
    n, nb = offs.size - 1, int(bases.size)
    assert big["nb"] >= 4 * nb
    gpu = _fresh(big["img"])
    try:
        scratch0 = gpu.info("device_scratch_bytes")
        d_bases, d_offs = _dev(bases), _dev(offs.view(np.int64))
        out = torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = _capture(lambda: gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), 0, s.cuda_stream), s)
        assert gpu.last_launch()["kernel"].endswith(", 2>")
        assert gpu.info("device_scratch_bytes") == scratch0
        bout = torch.full((big["nb"],), SENT, dtype=torch.int16, device="cuda")
        gpu.pml_device(big["d_bases"].data_ptr(), big["d_offs"].data_ptr(), big["n"], big["nb"], bout.data_ptr())
        assert gpu.last_launch()["kernel"].endswith(", 2>")
        torch.cuda.synchronize()
        _check_tiled(bout, big)
        del bout
        grown = gpu.info("device_scratch_bytes")
        assert grown >= scratch0 + mask_words(big["n"], big["nb"]) * 4   # the retired buffer and the new one
        for _ in range(2):
            out.fill_(SENT)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert (_u16(out) == exp).all()
        assert gpu.info("device_scratch_bytes") == grown
        gpu.set_option("release_scratch", 1)
        assert gpu.info("device_scratch_bytes") == 0
    finally:
        gpu.close()


@pytest.mark.parametrize("verdict", [0, 1])
def test_long_reads_capture_after_one_warmup(images, verdict):
    """Long reads with "seg_probe" 2 and the caller's verdict: one uncaptured warm-up call (it sizes the segment workspace, as the
    header documents), then captured movi_pml_device / movi_zml_device calls allocate nothing and replay to the oracle."""
    import torch
    from oracle.oracle import Oracle
    img = images["mode6"]
    cpu = Oracle(img)
    reads = mutated_reads(np.random.default_rng(700 + verdict), _ref(), 48, 4096, 6500)
    bases, offs = pack(reads)
    n, nb = offs.size - 1, int(bases.size)
    exp, _, _ = cpu.pml_batch(bases, offs, threads=4)
    expz = cpu.zml_batch(bases, offs, threads=4)
    d_bases, d_offs = _dev(bases), _dev(offs.view(np.int64))
    gpu = _fresh(img)
    gpu.set_option("seg_probe", 2)
    gpu.set_option("seg_verdict", verdict)
    s = torch.cuda.Stream()
    try:
        for fn, want in ((gpu.pml_device, exp), (gpu.zml_device, expz)):
            out = torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
            call = lambda fn=fn, out=out: fn(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), 0, s.cuda_stream)
            with torch.cuda.stream(s):
                call()                                          # warm-up
            torch.cuda.synchronize()
            assert (_u16(out) == want).all()
            assert gpu.last_launch()["segmented"] == verdict
            scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
            out.fill_(SENT)
            torch.cuda.synchronize()
            g = _capture(call, s)
            torch.cuda.synchronize()
            assert (_u16(out) == SENT).all()
            assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
            for _ in range(2):
                g.replay()
                torch.cuda.synchronize()
                assert (_u16(out) == want).all()
                out.fill_(SENT)
                torch.cuda.synchronize()
    finally:
        gpu.close()
        cpu.close()


@pytest.mark.parametrize("kind", ["short", "long"])
def test_unaligned_output_vector(images, kind):
    """movi_pml_device (default route) and movi_pml_expand_device into a vector 1 to 8 elements past a 16-byte boundary: the
    vector equals the oracle's and the sentinels before and after it are untouched."""
    import torch
    from movi_amd.engine import mask_words
    from oracle.oracle import Oracle
    img = images["mode6"]
    cpu = Oracle(img)
    ref = _ref()
    rng = np.random.default_rng(800 if kind == "short" else 801)
    reads = (mutated_reads(rng, ref, 1200, 1, 300) + _edge_reads(ref)) if kind == "short" else mutated_reads(rng, ref, 24, 2048, 3500)
    bases, offs = pack(reads)
    n, nb = offs.size - 1, int(bases.size)
    exp, _, _ = cpu.pml_batch(bases, offs, threads=4)
    d_bases, d_offs = _dev(bases), _dev(offs.view(np.int64))
    gpu = _fresh(img)
    pad = 64
    try:
        words = torch.zeros(mask_words(n, nb) + 1, dtype=torch.int32, device="cuda")
        gpu.pml_mask_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, words.data_ptr())
        for shift in range(1, 9):
            for entry in ("pml_device", "pml_expand_device"):
                buf = torch.full((nb + 2 * pad,), SENT, dtype=torch.int16, device="cuda")
                assert buf.data_ptr() % 16 == 0
                ptr = buf.data_ptr() + 2 * shift
                if entry == "pml_device":
                    gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, ptr)
                else:
                    gpu.pml_expand_device(words.data_ptr(), d_offs.data_ptr(), n, nb, ptr)
                torch.cuda.synchronize()
                got = _u16(buf)
                assert (got[:shift] == SENT).all() and (got[shift + nb:] == SENT).all(), (entry, shift)
                assert (got[shift:shift + nb] == exp).all(), (entry, shift)
    finally:
        gpu.close()
        cpu.close()


def test_every_first_base_phase(images):
    """movi_pml_mask_device and movi_pml_expand_device over a sub-batch at every first_base & 31 and at a first_base >= 2^32: the
    words' valid bits equal masks_of_pml of the oracle's vector at that phase, and the expansion gives the oracle's vector back."""
    import torch
    from movi_amd.engine import mask_words, masks_of_pml
    from oracle.oracle import Oracle
    img = images["mode6"]
    cpu = Oracle(img)
    bases, offs = _short_batch(900, n=700)
    n, nb = offs.size - 1, int(bases.size)
    exp, _, _ = cpu.pml_batch(bases, offs, threads=4)
    d_bases, d_offs = _dev(bases), _dev(offs.view(np.int64))
    gpu = _fresh(img)
    try:
        for fb in [(1 << 20) + p for p in range(32)] + [(1 << 32) + 13]:
            ew, valid = masks_of_pml(exp, offs, fb)
            nw = mask_words(n, nb, fb)
            assert nw == ew.size
            words = torch.full((nw,), -1, dtype=torch.int32, device="cuda")
            gpu.pml_mask_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, words.data_ptr(), fb)
            torch.cuda.synchronize()
            got = words.cpu().numpy().view(np.uint32)
            assert (got[valid] == ew[valid]).all(), fb
            out = torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
            gpu.pml_expand_device(words.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), fb)
            torch.cuda.synchronize()
            assert (_u16(out) == exp).all(), fb
    finally:
        gpu.close()
        cpu.close()


def test_read_order_on_the_mask_route(images):
    """A random d_read_order on movi_pml_device's default route and through movi_pml_mask_device: results indexed by read, the
    oracle's."""
    import torch
    from movi_amd.engine import mask_words, masks_of_pml
    from oracle.oracle import Oracle
    img = images["mode6"]
    cpu = Oracle(img)
    bases, offs = _short_batch(901)
    n, nb = offs.size - 1, int(bases.size)
    exp, _, _ = cpu.pml_batch(bases, offs, threads=4)
    ew, valid = masks_of_pml(exp, offs)
    order = np.random.default_rng(902).permutation(n).astype(np.uint32)
    d_bases, d_offs, d_order = _dev(bases), _dev(offs.view(np.int64)), _dev(order.view(np.int32))
    gpu = _fresh(img)
    try:
        out = torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
        gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), d_order=d_order.data_ptr())
        torch.cuda.synchronize()
        assert (_u16(out) == exp).all()
        words = torch.full((mask_words(n, nb),), -1, dtype=torch.int32, device="cuda")
        gpu.pml_mask_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, words.data_ptr(), d_order=d_order.data_ptr())
        torch.cuda.synchronize()
        assert (words.cpu().numpy().view(np.uint32)[valid] == ew[valid]).all()
    finally:
        gpu.close()
        cpu.close()
