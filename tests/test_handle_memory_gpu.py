"""GPU suite (-m gpu): a handle that has used every kind of buffer it owns gives the device back what it took.

One create -> use -> close() cycle loads the code objects and fills the runtime's own pools; a second one is measured with
torch.cuda.mem_get_info() around it.  The cycle uses the derived tables of movi_index_prepare, the mask words and the park queue of
movi_pml_device (a captured call marks them, a growth retires them), the synchronous staging, the pipeline slots of an overlapped
movi_pml_host call, the count query's tables, a sampled suffix array and colour tables with their counter scratch.

The sizes are chosen against the resolution of mem_get_info -- megabytes -- not against any workload: a leaked block of each class
must show.  Mask words for 2^28 / 2^30 bases are 90 / 430 MB, the staging of 2^24 bases and reads is 16 - 70 MB per buffer, four
pipeline slots stage a chunk of 4.9 M bases each (5.5 MB of reads, 11 MB of results), the park queue is 4 MB, and the derived tables
of the golden index (two 256 MB lookup tables) are the largest of all.  (Blocks of less than 1 MB -- a slot's offsets, error bytes
and counters -- come out of the runtime's own pool and do not move mem_get_info at all: they are beyond this test.)

Measured on an MI355X (profiles/handle_buffers.txt), three runs of this body per library: on the parent commit's library the second
cycle kept 2 097 152, 0 and 0 bytes (PARENT_DIFF_BYTES: the largest), on this commit's 0, 0 and 2 097 152 -- a granule of the
runtime's own pool that comes and goes with either.  Free memory moves in granules of 2 MiB: hipMalloc of 4 x 1 MiB, 4 x (1 MiB + 1),
4 x 3 MiB and 4 x 16 MiB took 4, 6, 16 and 64 MiB, anything below 1 MiB took nothing (GRANULE_BYTES).  The margin is their sum,
4 MiB: less than the smallest block above.
"""
import numpy as np
import pytest

from test_capture_gpu import SENT, _capture, _dev, _short_batch, _u16

pytestmark = pytest.mark.gpu

PARENT_DIFF_BYTES = 2 << 20        # what the second cycle kept on the parent commit
GRANULE_BYTES = 2 << 20            # one allocation granule of the runtime, as observed
HOST_BASES, READ_LEN, CHECKED_READS = 1 << 24, 150, 2000


def _cycle(img, stream, short, dev, host, want):
    """create -> use every kind of buffer -> close(); the caller's device and host arrays are the same in every cycle"""
    import movi_amd
    bases, offs = short
    n, nb = offs.size - 1, int(bases.size)
    d_bases, d_offs, out = dev
    cpu_short, cpu_host, cpu_count = want
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.prepare()
    # a captured call marks the mask words (and the park queue, once there is one) as used by a graph: their growth retires them
    call = lambda: gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), 0, stream.cuda_stream)
    g = _capture(call, stream)
    out.fill_(SENT)
    g.replay()
    stream.synchronize()
    assert (_u16(out) == cpu_short).all()
    gpu.set_option("park_lanes", 8)
    held = gpu.info("device_scratch_bytes")
    gpu.set_option("reserve_device_masks", 1 << 30)
    assert gpu.info("device_scratch_bytes") > held + (1 << 27)          # the new words, and the old ones still held
    for key in ("reserve_host_bases", "reserve_host_results", "reserve_host_reads"):
        gpu.set_option(key, 1 << 24)
    assert gpu.info("host_staging_bytes") >= 3 * (1 << 24)
    # midway: everything the calls hold goes, and the handle stays usable
    del g
    gpu.set_option("release_scratch", 1)
    assert gpu.info("device_scratch_bytes") == 0 and gpu.info("host_staging_bytes") == 0
    gpu.set_option("reserve_device_masks", 1 << 28)
    g = _capture(call, stream)                                          # (marks the new words: the growth below retires tens of MB)
    out.fill_(SENT)
    g.replay()
    stream.synchronize()
    assert (_u16(out) == cpu_short).all()
    gpu.set_option("reserve_device_masks", 1 << 30)
    for key in ("reserve_host_bases", "reserve_host_results", "reserve_host_reads"):
        gpu.set_option(key, 1 << 24)
    # one overlapped host call: page-locked reads and result vector, the vector itself comes down; several slots hold staging
    h_bases, h_offs, h_out = host
    gpu.set_option("host_masks", 0)
    h_out[:] = SENT
    got, st = gpu.query_pml_packed(h_bases, h_offs, out=h_out)
    assert st.bases == h_bases.size
    assert (got[:CHECKED_READS * READ_LEN] == cpu_host).all()
    matched, count, _ = gpu.query_count_packed(h_bases[:CHECKED_READS * READ_LEN], h_offs[:CHECKED_READS + 1])
    assert (matched == cpu_count[0]).all() and (count == cpu_count[1]).all()
    gpu.build_ssa(64)
    length = gpu.desc.length
    gpu.build_colors([(length - 1) // 2, length - 1])
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]) for i in range(8)]
    assert len(gpu.multi_classify(reads)) == 8
    assert gpu.info("derived_bytes") > (256 << 20) and gpu.info("device_scratch_bytes") > (1 << 27) and gpu.info("host_staging_bytes") > (1 << 24)
    del g
    gpu.close()


def test_close_returns_device_memory(built_lib, golden_image):
    import torch
    from movi_amd.engine import pinned_empty
    from oracle.oracle import Oracle
    img = golden_image(6)
    cpu = Oracle(img)
    short = _short_batch(71)
    cpu_short = cpu.pml_batch(short[0], short[1], threads=4)[0]
    rng = np.random.default_rng(72)
    n_reads = HOST_BASES // READ_LEN
    h_bases = pinned_empty(n_reads * READ_LEN, np.uint8)
    h_bases[:] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, h_bases.size)]
    h_offs = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(READ_LEN)
    host = (h_bases, h_offs, pinned_empty(h_bases.size, np.uint16))
    head = (h_bases[:CHECKED_READS * READ_LEN], h_offs[:CHECKED_READS + 1])
    want = (cpu_short, cpu.pml_batch(head[0], head[1], threads=4)[0], cpu.count_batch(head[0], head[1], threads=4))
    dev = (_dev(short[0]), _dev(short[1].view(np.int64)), torch.full((int(short[0].size),), SENT, dtype=torch.int16, device="cuda"))
    stream = torch.cuda.Stream()
    _cycle(img, stream, short, dev, host, want)                         # code objects, the runtime's pools
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    _cycle(img, stream, short, dev, host, want)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("handle memory: free before %d, after %d, kept %d bytes (margin %d)" % (before, after, before - after, PARENT_DIFF_BYTES + GRANULE_BYTES))
    assert after >= before - (PARENT_DIFF_BYTES + GRANULE_BYTES)
