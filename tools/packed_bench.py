"""2-bit packed reads against ASCII reads through the C-ABI host entry points, side by side from one process (profiles/packed_reads.txt):
the parent-equivalent ASCII calls (their spread is the noise floor), the packed calls on pre-packed input, the packed calls with the pack
time included, the packer alone, the unpack kernels per chunk -- and the legs a call is made of (upload, walk, mask download, host
expansion), each timed on its own, so that the file can name the term that bounds each call.

usage: python tools/packed_bench.py [--out profiles/packed_reads.txt] [--big-rows 1000000000 | --no-big] [--reps 5]
The c2 batch (1 M x 150 bp on the pangenome index) comes from bench.py's cache; the 1 B-row table is tools/synth's, if the device has room."""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import movi_amd
from movi_amd._lib import QueryStatsC, check, lib
from movi_amd.engine import expand_masks_host, mask_words, pack_reads, packed_bytes, pinned_empty

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps):
    fn()                                                       # warm-up: staging, page-locked blocks, derived tables
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def rate_line(name, ts, nb):
    r = sorted(nb / t / 1e9 for t in ts)
    say("   %-58s median %6.2f  min %6.2f  max %6.2f Gbases/s  (spread %.1f %%; %s ms)" %
        (name, r[len(r) // 2], r[0], r[-1], 100 * (r[-1] - r[0]) / r[len(r) // 2], " ".join("%.2f" % (t * 1e3) for t in ts)))
    return r[len(r) // 2], r[0], r[-1]


def gpu_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def run(tag, ix, bases, offs, reps):
    n, nb = offs.size - 1, int(bases.size)
    say("== %s: %d reads, %d bases" % (tag, n, nb))
    L = lib()
    st = QueryStatsC()
    err = np.zeros(n, np.uint8)
    out = np.ones(nb, np.uint16)                               # pageable and touched: movi_pml_host's default route brings masks down and expands them here
    words = np.zeros(mask_words(n, nb), np.uint32)
    words2 = np.zeros_like(words)
    pb = pinned_empty(nb, np.uint8)
    pb[:] = bases
    pk = pinned_empty(packed_bytes(0, nb), np.uint8)
    pk[:] = 0
    _, pos, byte = pack_reads(bases, 0, packed=pk)
    say("   packed: %d bytes + %d exceptions (%d bytes) = %.3f of the ASCII bytes" % (pk.size, pos.size, 9 * pos.size, (pk.size + 9 * pos.size) / nb))
    ascii_pml = lambda: check(L.movi_pml_host(ix._h, pb.ctypes.data, offs.ctypes.data, n, out.ctypes.data, err.ctypes.data, C.byref(st)))
    ascii_mask = lambda: check(L.movi_pml_mask_host(ix._h, pb.ctypes.data, offs.ctypes.data, n, words.ctypes.data, err.ctypes.data, C.byref(st)))
    packed_pml = lambda: check(L.movi_pml_packed_host(ix._h, pk.ctypes.data, pos.ctypes.data, byte.ctypes.data, pos.size, offs.ctypes.data, n,
                                                      out.ctypes.data, err.ctypes.data, C.byref(st)))
    packed_mask = lambda: check(L.movi_pml_mask_packed_host(ix._h, pk.ctypes.data, pos.ctypes.data, byte.ctypes.data, pos.size, offs.ctypes.data, n,
                                                            words2.ctypes.data, err.ctypes.data, C.byref(st)))
    cap = max(int(pos.size), 1)
    epos, ebyte, got = np.zeros(cap, np.uint64), np.zeros(cap, np.uint8), C.c_uint64(0)

    def pack_only(threads=0):
        check(L.movi_reads_pack_host(bases.ctypes.data, 0, nb, pk.ctypes.data, epos.ctypes.data, ebyte.ctypes.data, cap, C.byref(got), threads))

    def pack_then(call):
        def f():
            pack_only()
            call()
        return f
    say(" -- the calls (page-locked reads; %d repeats after a warm-up call; ASCII first and last: drift shows as a difference between the two)" % reps)
    a_pml = rate_line("movi_pml_host (ASCII, the parent's call)", timed(ascii_pml, reps), nb)
    a_mask = rate_line("movi_pml_mask_host (ASCII, the parent's call)", timed(ascii_mask, reps), nb)
    p_pml = rate_line("movi_pml_packed_host, pre-packed", timed(packed_pml, reps), nb)
    want = out.copy()
    p_mask = rate_line("movi_pml_mask_packed_host, pre-packed", timed(packed_mask, reps), nb)
    rate_line("movi_pml_packed_host, pack time included", timed(pack_then(packed_pml), reps), nb)
    rate_line("movi_pml_mask_packed_host, pack time included", timed(pack_then(packed_mask), reps), nb)
    a_pml2 = rate_line("movi_pml_host (ASCII) again", timed(ascii_pml, reps), nb)
    a_mask2 = rate_line("movi_pml_mask_host (ASCII) again", timed(ascii_mask, reps), nb)
    assert (out == want).all() and (expand_masks_host(words2, offs) == want).all(), "packed and ASCII results differ"   # (gap words are unspecified: compared expanded)
    say(" -- the packer alone (movi_reads_pack_host, pageable ASCII in, page-locked packed out)")
    for threads in (1, 4, 12):
        ts = timed(lambda: pack_only(threads), reps)
        say("   %2d threads: best %.2f ms = %.2f GB/s of ASCII bytes" % (threads, min(ts) * 1e3, nb / min(ts) / 1e9))
    say(" -- the legs of a call, each on its own")
    d_pk, d_bases = torch.empty(pk.size, dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")
    t_pk, t_pb = torch.from_numpy(pk), torch.from_numpy(pb)
    up_packed = gpu_ms(lambda: d_pk.copy_(t_pk, non_blocking=True))
    up_ascii = gpu_ms(lambda: d_bases.copy_(t_pb, non_blocking=True))
    d_pos = torch.from_numpy(pos.view(np.int64).copy()).cuda() if pos.size else None
    d_byte = torch.from_numpy(byte.copy()).cuda() if pos.size else None
    unpack_all = gpu_ms(lambda: ix.unpack_reads_device(d_pk.data_ptr(), 0, nb, d_bases.data_ptr(), d_pos.data_ptr() if pos.size else 0,
                                                       d_byte.data_ptr() if pos.size else 0, pos.size))
    chunk = nb // 16                                           # the mask calls cut a batch into sixteen chunks
    unpack_chunk = gpu_ms(lambda: ix.unpack_reads_device(d_pk.data_ptr(), 0, chunk, d_bases.data_ptr(), 0, 0, 0))
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_words = torch.empty(words.size, dtype=torch.int32, device="cuda")
    walk = gpu_ms(lambda: ix.pml_mask_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, d_words.data_ptr()))
    pw = pinned_empty(words.size, np.uint32)
    t_pw = torch.from_numpy(pw.view(np.int32))
    down_masks = gpu_ms(lambda: t_pw.copy_(d_words, non_blocking=True))
    ex = min(timed(lambda: expand_masks_host(words, offs, out=out), reps)) * 1e3
    say("   upload, ASCII   %7.3f ms = %5.1f GB/s = %6.1f Gbases/s" % (up_ascii, nb / up_ascii / 1e6, nb / up_ascii / 1e6))
    say("   upload, packed  %7.3f ms = %5.1f GB/s = %6.1f Gbases/s" % (up_packed, pk.size / up_packed / 1e6, nb / up_packed / 1e6))
    say("   unpack kernels  %7.3f ms whole batch = %6.1f Gbases/s; one chunk of %d bases: %.3f ms (HIP events)" % (unpack_all, nb / unpack_all / 1e6, chunk, unpack_chunk))
    say("   mask walk       %7.3f ms = %6.1f Gbases/s (movi_pml_mask_device, reads on the device)" % (walk, nb / walk / 1e6))
    say("   mask download   %7.3f ms = %6.1f Gbases/s" % (down_masks, nb / down_masks / 1e6))
    say("   host expansion  %7.3f ms = %6.1f Gbases/s (movi_pml_expand_host, default threads, the whole batch at once)" % (ex, nb / ex / 1e6))
    legs_mask = {"upload": up_packed, "walk": walk + unpack_all, "mask download": down_masks}
    legs_pml = dict(legs_mask, **{"host expansion": ex})
    legs_ascii = {"upload": up_ascii, "walk": walk, "mask download": down_masks}
    say(" -- verdict")
    noise = max(a_mask[2], a_mask2[2]) - min(a_mask[1], a_mask2[1])
    say("   masks only: packed %.2f against ASCII %.2f / %.2f Gbases/s (medians); the ASCII calls' spread over both blocks is %.2f: %s" %
        (p_mask[0], a_mask[0], a_mask2[0], noise, "NOT slower than the ASCII call beyond the spread" if p_mask[0] >= min(a_mask[0], a_mask2[0]) - noise
         else "SLOWER than the ASCII call by more than the spread"))
    say("   vector:     packed %.2f against ASCII %.2f / %.2f Gbases/s (medians)" % (p_pml[0], a_pml[0], a_pml2[0]))
    for name, legs, med in (("movi_pml_mask_host (ASCII)", legs_ascii, a_mask[0]), ("movi_pml_host (ASCII)", dict(legs_ascii, **{"host expansion": ex}), a_pml[0]),
                            ("movi_pml_mask_packed_host", legs_mask, p_mask[0]), ("movi_pml_packed_host", legs_pml, p_pml[0])):
        k = max(legs, key=legs.get)
        call_ms = nb / med / 1e6
        say("   %-28s %.2f ms per call; longest leg: %s, %.2f ms = a ceiling of %.1f Gbases/s; %.2f ms of the call are not that leg (the pipeline's fill and drain, "
            "sixteen chunks' launches, walks of a sixteenth of the batch)" % (name, call_ms, k, legs[k], nb / legs[k] / 1e6, call_ms - legs[k]))
    say()
    del pb, pk, pw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_reads.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big-rows", type=int, default=1_000_000_000)
    ap.add_argument("--no-big", action="store_true")
    args = ap.parse_args()
    import bench
    from tools import synth
    say("tools/packed_bench.py on %s" % torch.cuda.get_device_name(0))
    idx_dir, reads_file = bench.prepare_inputs("c2")
    wl = bench.WORKLOADS["c2"]
    bases = np.fromfile(reads_file, np.uint8)[: wl["reads"] * wl["read_len"]]
    offs = np.arange(wl["reads"] + 1, dtype=np.uint64) * np.uint64(wl["read_len"])
    ix = movi_amd.MoveIndex.load(idx_dir)
    run("c2 (pangenome index, %d rows)" % ix.desc.r, ix, bases, offs, args.reps)
    ix.close()
    free = torch.cuda.mem_get_info()[0]
    if not args.no_big and free > 40 * args.big_rows:          # rows (8 B) + look-ahead copy (16 B) + staging, with room to spare
        six = synth.synth_index(args.big_rows, mode=6, seed=1)
        ix = movi_amd.MoveIndex.from_image(six.image())
        bases, offs = synth.synth_reads(six, 1_000_000, 150, seed=2, sub_rate=0.01, n_rate=0.001)
        run("synthetic table, %d rows" % args.big_rows, ix, bases, offs, args.reps)
        ix.close()
    else:
        say("== the %d-row table: not run (%s)" % (args.big_rows, "--no-big" if args.no_big else "%.1f GB free on the device" % (free / 1e9)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
