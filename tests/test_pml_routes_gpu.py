"""GPU suite (-m gpu): the OUTPUT ROUTE of a PML call (plan_pml, movi_launch_policy.hpp), one call per route through every entry
point that can reach it.  The five routes -- the vector straight from the walk, reset masks native from the walk, masks packed from a
vector in scratch, the vector by fused expansion, the vector by the pml_expand_* kernels behind a native mask walk -- are forced by the
existing options ("pml_via_mask", "fused_expand", "block_threads" 256, "pml_variant" 1, "park_lanes" 2), an output pointer offset by 2
bytes and a read order, on a batch of short reads (130 reads of 0 .. 150 bases: two full wavefronts and a ragged third, read 0 empty,
read 1 of one base) and on the smallest batch of long reads the segment plan accepts (8 x 300 bases at "seg_len" 64, "seg_probe" 0).
Every call must give the oracle's answers and launch exactly what EXPECT says: (kernel, variant, block_threads, staged, ahead,
park_lanes, ff_skip, segmented) of movi_last_launch and the set of names in movi_launch_log.  The literals of EXPECT were recorded by
running this file's cases on the commit BEFORE the route moved into one planner: a call that changes kernel, template argument, block
or staging on any route fails here."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, classify_py
from test_gpu_parity import mutated_reads, pack

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
OPTIONS = dict(pml_via_mask=-1, fused_expand=1, block_threads=0, park_lanes=-1, pml_variant=-1, host_masks=-1, host_overlap=1,
               pipe_chunk_bases=0, seg_len=2048, seg_probe=1, classify_fused=-1)
LONG = dict(seg_len=64, seg_probe=0)
BW, THR = 40, 4

# (name, entry point, batch, options, output offset in u16 elements, with a read order)
CASES = [
    # ---- short reads
    ("device/default", "device", "short", {}, 0, False),                                   # fused expansion
    ("device/via1", "device", "short", dict(pml_via_mask=1), 0, False),
    ("device/via0", "device", "short", dict(pml_via_mask=0), 0, False),                    # the vector straight from the walk
    ("device/offset2", "device", "short", {}, 1, False),                                   # expand kernels behind the mask walk
    ("device/order", "device", "short", {}, 0, True),
    ("device/unfused", "device", "short", dict(fused_expand=0), 0, False),
    ("device/bt256", "device", "short", dict(block_threads=256), 0, False),                # the walk cannot write masks: the plain vector
    ("device/bt256/via1", "device", "short", dict(block_threads=256, pml_via_mask=1), 0, False),   # forced, cannot: the plain vector
    ("device/variant1/via1", "device", "short", dict(pml_variant=1, pml_via_mask=1), 0, False),
    ("device/park2", "device", "short", dict(park_lanes=2), 0, False),
    ("device/park2/offset2", "device", "short", dict(park_lanes=2), 1, False),             # not the fused route: nothing parks
    ("device/park2/order", "device", "short", dict(park_lanes=2), 0, True),
    ("device/park2/via0", "device", "short", dict(park_lanes=2, pml_via_mask=0), 0, False),
    ("mask/default", "mask", "short", {}, 0, False),                                       # masks native from the walk
    ("mask/order", "mask", "short", {}, 0, True),
    ("mask/park2", "mask", "short", dict(park_lanes=2), 0, False),
    ("mask/park2/order", "mask", "short", dict(park_lanes=2), 0, True),
    ("mask/bt256", "mask", "short", dict(block_threads=256), 0, False),                    # masks packed from a vector in scratch
    ("mask/variant1", "mask", "short", dict(pml_variant=1), 0, False),
    ("host/default", "host", "short", {}, 0, False),
    ("host/via0", "host", "short", dict(pml_via_mask=0), 0, False),
    ("host/via1/bt256", "host", "short", dict(pml_via_mask=1, block_threads=256), 0, False),
    ("host/masks", "host", "short", dict(host_masks=1), 0, False),                         # masks down, expanded on the host
    ("host/masks/variant1", "host", "short", dict(host_masks=1, pml_variant=1), 0, False),
    ("host/park2", "host", "short", dict(park_lanes=2), 0, False),
    ("overlapped/default", "overlapped", "short", {}, 0, False),
    ("overlapped/via0", "overlapped", "short", dict(pml_via_mask=0), 0, False),
    ("overlapped/masks", "overlapped", "short", dict(host_masks=1), 0, False),
    ("overlapped/masks/bt256", "overlapped", "short", dict(host_masks=1, block_threads=256), 0, False),
    ("classify/default", "classify", "short", {}, 0, False),                               # bins fused: the vector from the walk
    ("classify/two_pass", "classify", "short", dict(classify_fused=0), 0, False),          # an ordinary PML call, then the pass
    ("classify/two_pass/via1", "classify", "short", dict(classify_fused=0, pml_via_mask=1), 0, False),
    # ---- long reads: the segment plan gets the first say
    ("device/long", "device", "long", LONG, 0, False),
    ("device/long/via1", "device", "long", dict(LONG, pml_via_mask=1), 0, False),          # falls back to the plain vector, segmented
    ("device/long/order", "device", "long", LONG, 0, True),                                # a read order: one lane per read, masks
    ("device/long/variant1", "device", "long", dict(LONG, pml_variant=1), 0, False),
    ("mask/long", "mask", "long", LONG, 0, False),                                         # segmented into scratch, then packed
    ("mask/long/order", "mask", "long", LONG, 0, True),
    ("host/long", "host", "long", LONG, 0, False),
    ("host/long/masks", "host", "long", dict(LONG, host_masks=1), 0, False),
    ("overlapped/long", "overlapped", "long", LONG, 0, False),
    ("classify/long", "classify", "long", LONG, 0, False),
    ("classify/long/two_pass", "classify", "long", dict(LONG, classify_fused=0), 0, False),
]


def _walk(args):
    return "pml_kernel_flatp<6, unsigned int, %s>" % args


# The launches the cases were recorded to make: (movi_last_launch tuple, names in movi_launch_log).  On the golden index after
# movi_index_prepare the default walk runs on the deep rows (ahead 2) with 336 staged bases and the fast-forward skip.
MASK_WALK, VECTOR_WALK, BINS_WALK = _walk("0, 0, 0, 1, 2, 0, 2"), _walk("0, 0, 0, 1, 2, 0, 0"), _walk("1, 0, 0, 1, 2, 0, 0")
UNSTAGED_WALK, SEG_K1, SEG_K3 = _walk("0, 0, 0, 0, 0, 0, 0"), _walk("0, 0, 1, 1, 1, 0, 1"), _walk("0, 0, 2, 1, 1, 0, 1")
MASKS = ((MASK_WALK, 14, 64, 336, 2, 0, 1, 0), {MASK_WALK})
MASKS_PARKED = ((MASK_WALK, 14, 64, 336, 2, 2, 1, 0), {MASK_WALK})
VECTOR = ((VECTOR_WALK, 14, 64, 336, 2, 0, 1, 0), {VECTOR_WALK})
BINS = ((BINS_WALK, 14, 64, 336, 2, 0, 1, 0), {BINS_WALK})
BLOCK256 = ((UNSTAGED_WALK, 14, 256, 0, 0, 0, 0, 0), {UNSTAGED_WALK})
VARIANT1 = (("pml_kernel<6, 1, 0>", 1, 64, 0, 0, 0, 0, 0), set())         # (the launch log names walk kernels only)
SEGMENTED = ((SEG_K1, 14, 64, 336, 1, 0, 0, 1), {SEG_K1, SEG_K3})
# (MASKS stands for the fused expansion -- device/default -- and for the expand kernels behind the walk -- offset2, order, unfused -- alike:
# the log names walk kernels only and no info key says which of the two ran, so here only the results tell them apart -- with park_lanes 2,
# also the parked tuple, which the fused route alone gives; tests/golden/launch_route_table.txt pins vector_fused against vector_expand.)
EXPECT = {
    "device/default": MASKS, "device/via1": MASKS, "device/via0": VECTOR, "device/offset2": MASKS, "device/order": MASKS,
    "device/unfused": MASKS, "device/bt256": BLOCK256, "device/bt256/via1": BLOCK256, "device/variant1/via1": VARIANT1,
    "device/park2": MASKS_PARKED, "device/park2/offset2": MASKS, "device/park2/order": MASKS, "device/park2/via0": VECTOR,
    "mask/default": MASKS, "mask/order": MASKS, "mask/park2": MASKS_PARKED, "mask/park2/order": MASKS_PARKED, "mask/bt256": BLOCK256,
    "mask/variant1": VARIANT1,
    "host/default": MASKS, "host/via0": VECTOR, "host/via1/bt256": BLOCK256, "host/masks": MASKS, "host/masks/variant1": VARIANT1,
    "host/park2": MASKS,                                                   # (the host path lends no park queue)
    "overlapped/default": MASKS, "overlapped/via0": VECTOR, "overlapped/masks": MASKS, "overlapped/masks/bt256": BLOCK256,
    "classify/default": BINS, "classify/two_pass": VECTOR, "classify/two_pass/via1": VECTOR,
    "device/long": SEGMENTED, "device/long/via1": SEGMENTED, "device/long/order": MASKS, "device/long/variant1": VARIANT1,
    "mask/long": SEGMENTED, "mask/long/order": MASKS, "host/long": SEGMENTED, "host/long/masks": SEGMENTED, "overlapped/long": SEGMENTED,
    "classify/long": SEGMENTED, "classify/long/two_pass": SEGMENTED,
}


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _log_on():
    from movi_amd._lib import lib
    need = C.c_size_t(0)
    lib().movi_launch_log(None, 0, C.byref(need))                # (switches the log on; clears it)


def _log():
    from movi_amd._lib import lib
    buf = C.create_string_buffer(1 << 16)
    lib().movi_launch_log(buf, len(buf), None)
    return frozenset(x for x in buf.value.decode().split("\n") if x)


def _chunks(offs, target):
    """Chunks of the overlapped path under "pipe_chunk_bases" (run_pipelined: as many reads as stay within `target` bases, at least one)."""
    k, first, n = 0, 0, offs.size - 1
    while first < n:
        last = int(np.searchsorted(offs, offs[first] + np.uint64(target), side="right")) - 1
        first = min(max(last, first + 1), n)
        k += 1
    return k


@pytest.fixture(scope="module")
def world(built_lib, golden_image):
    """The handle, the two batches and the oracle's answers: made once, shared by every case, left unchanged."""
    import movi_amd
    from movi_amd.engine import masks_of_pml
    from oracle import build_index as B
    from oracle.oracle import Oracle
    img = golden_image(6)
    ref = B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]
    rng = np.random.default_rng(41)
    short = [b"", ref[777:778]] + mutated_reads(rng, ref, 128, 20, 151)
    long_reads = mutated_reads(rng, ref, 8, 300, 301)
    assert len(short) == 130 and all(len(r) == 300 for r in long_reads)
    cpu = Oracle(img)
    batches = {}
    for name, reads in (("short", short), ("long", long_reads)):
        bases, offs = pack(reads)
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
        words, valid = masks_of_pml(exp, offs)
        n, nb = len(reads), int(bases.size)
        order = np.random.default_rng(5).permutation(n).astype(np.uint32)
        bins = [classify_py(exp[int(offs[i]):int(offs[i + 1])], THR, BW) if offs[i + 1] > offs[i] else None for i in range(n)]
        pb, po = movi_amd.pinned_empty(nb, np.uint8), movi_amd.pinned_empty(nb, np.uint16)
        pb[:] = bases
        batches[name] = dict(bases=np.array(bases), offs=offs, n=n, nb=nb, exp=exp, ff=ff, sc=sc, words=words, valid=valid, bins=bins,
                             d_bases=_dev(bases), d_offs=_dev(offs.view(np.int64)), d_order=_dev(order.view(np.int32)), pb=pb, po=po,
                             chunk_bases=nb // 3 + int(np.diff(offs.astype(np.int64)).max()))
        assert _chunks(offs, batches[name]["chunk_bases"]) == 3
    cpu.close()
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.prepare(gpu.PREPARE_PML)
    yield gpu, batches
    gpu.close()


def run_case(gpu, b, entry, opts, align, ordered):
    """One call: its results against the oracle's -> (the launch tuple, the names in the launch log)."""
    import torch
    for k, v in dict(OPTIONS, **opts).items():
        gpu.set_option(k, v)
    n, nb = b["n"], b["nb"]
    d_order = b["d_order"].data_ptr() if ordered else 0
    err = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    _log_on()
    if entry in ("device", "classify"):
        out = torch.full((nb + 8,), SENT, dtype=torch.int16, device="cuda")
        if entry == "device":
            gpu.pml_device(b["d_bases"].data_ptr(), b["d_offs"].data_ptr(), n, nb, out.data_ptr() + 2 * align, err.data_ptr(), 0, d_order)
        else:
            above, below = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
            sums = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            gpu.pml_classify_device(b["d_bases"].data_ptr(), b["d_offs"].data_ptr(), n, nb, BW, THR, out.data_ptr(), above.data_ptr(),
                                    below.data_ptr(), sums.data_ptr(), err.data_ptr(), 0, d_order)
        st = gpu.last_stats()
        got = out.cpu().numpy().view(np.uint16)
        assert (got[:align] == SENT).all() and (got[align + nb:] == SENT).all()            # nothing outside the vector
        assert (got[align:align + nb] == b["exp"]).all(), np.flatnonzero(got[align:align + nb] != b["exp"])[:8]
        if entry == "classify":
            aa, bb, ss = above.cpu().numpy(), below.cpu().numpy(), sums.cpu().numpy()
            for i, c in enumerate(b["bins"]):
                if c is not None:                                  # (an empty read has no bins: its entries are the caller's)
                    assert (aa[i], bb[i]) == (c[2], c[3]) and ss[i] == round(c[1] * (c[2] + c[3])), (i, aa[i], bb[i], ss[i], c)
        assert (err.cpu().numpy() == 0).all()
    elif entry == "mask":
        from movi_amd.engine import mask_words
        words = torch.full((mask_words(n, nb) + 2,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
        gpu.pml_mask_device(b["d_bases"].data_ptr(), b["d_offs"].data_ptr(), n, nb, words.data_ptr(), 0, err.data_ptr(), 0, d_order)
        st = gpu.last_stats()
        got = words.cpu().numpy().view(np.uint32)
        assert (got[:-2][b["valid"]] == b["words"][b["valid"]]).all() and (got[-2:] == 0x3C3C3C3C).all()
        assert (err.cpu().numpy() == 0).all()
    else:
        if entry == "overlapped":                                  # page-locked reads and vector, three chunks
            gpu.set_option("pipe_chunk_bases", b["chunk_bases"])
            bases, out = b["pb"], b["po"]
        else:                                                      # pageable buffers: the synchronous path
            bases, out = b["bases"], np.zeros(nb, np.uint16)
        out[:] = SENT
        _, st, herr, rc = gpu.query_pml_packed(bases, b["offs"], want_err=True, out=out)
        assert rc == 0 and (out == b["exp"]).all() and not herr.any()
        assert st.bases == nb
    assert (st.fast_forwards, st.scans, st.errors) == (b["ff"], b["sc"], 0)
    li = gpu.last_launch()
    return ((li["kernel"], li["variant"], li["block_threads"], li["staged"], li["ahead"], int(gpu.info("park_lanes")), int(gpu.info("ff_skip")),
             li["segmented"]), _log())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_route(world, case):
    gpu, batches = world
    name, entry, batch, opts, align, ordered = case
    launch, names = run_case(gpu, batches[batch], entry, opts, align, ordered)
    print(name, launch, sorted(names))
    assert (launch, names) == (EXPECT[name][0], frozenset(EXPECT[name][1]))
