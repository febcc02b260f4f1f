"""GPU suite (-m gpu): k-mer occurrences (movi_kmer_occ_host / movi_kmer_occ_device, `movi query --kmer-occ`) against the contract
of include/movi_hip.h, restated on the oracle's count query in tests/kmer_occ_ref.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_fastx
from test_gpu_parity import mutated_reads, pack
from test_kernel_coverage_gpu import read_log, take_log
from test_kmer_gpu import SHAPES, _edge_reads, _ref
import kmer_occ_ref
import odd_texts

pytestmark = pytest.mark.gpu

KS = (1, 5, 12, 13, 31, 200)
ODD_KS = (5, 12, 31)
MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
ERR_BIT = np.uint64(1 << 63)


def _reads():
    ref = _ref()
    return mutated_reads(np.random.default_rng(616), ref, 600, 1, 400) + _edge_reads(ref)


@pytest.fixture(scope="module")
def texts(built_lib):
    """{separators: {mode: index image}} over ref.fasta: the six index types, plus 6 and 8 with --separators."""
    from oracle import build_index as B
    ref = _ref()
    out = {}
    for sep, modes in ((False, (6, 8, 7, 3, 2, 5)), (True, (6, 8))):
        bwt, thr = B.bwt_and_thresholds(B.clean_text([ref], separators=sep))
        out[sep] = {mode: B.serialize(B.build_rows(bwt, thr, mode)) for mode in modes}
    return out


@pytest.fixture(scope="module")
def expected(texts):
    """{separators: (reads, {k: occ arrays per read})} from the oracle on the mode-6 image of each text; computed once, left unchanged."""
    from oracle.oracle import Oracle
    reads = _reads()
    out = {}
    for sep, imgs in texts.items():
        o = Oracle(imgs[6])
        out[sep] = (reads, {k: kmer_occ_ref.occ(o, reads, k) for k in KS})
        o.close()
    return out


def slots(reads, occ):
    """The contract's layout: one u64 per base -- a read's occ values, then zeros for its other slots -- with found and sum per read."""
    full = np.concatenate([np.concatenate([o, np.zeros(len(r) - len(o), np.uint64)]) for r, o in zip(reads, occ)] + [np.zeros(0, np.uint64)])
    fs = [kmer_occ_ref.found_sum(o) for o in occ]
    return full, np.array([f for f, _ in fs], np.uint32), np.array([s for _, s in fs], np.uint64)


def device_occ(gpu, reads, k, stream=None, bufs=None):
    """movi_kmer_occ_device on torch buffers pre-filled with 0x5A -> (occ per slot, found, sum, err)."""
    import torch
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(bases) if nb else np.zeros(1, np.uint8)).to(dev)
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    docc = torch.full((max(nb, 1) * 8,), 0x5A, dtype=torch.uint8, device=dev)
    df = torch.full((n * 4,), 0x5A, dtype=torch.uint8, device=dev)
    ds = torch.full((n * 8,), 0x5A, dtype=torch.uint8, device=dev)
    de = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    gpu.kmer_occ_device(db.data_ptr(), do.data_ptr(), n, nb, k, docc.data_ptr(), df.data_ptr(), ds.data_ptr(), de.data_ptr())
    torch.cuda.synchronize()
    return (docc.cpu().numpy().view(np.uint64)[:nb], df.cpu().numpy().view(np.uint32), ds.cpu().numpy().view(np.uint64), de.cpu().numpy())


def check_both_forms(gpu, reads, occ, k, tag):
    """Device and host forms against the restatement: every slot, found, sum, no error."""
    full, found, total = slots(reads, occ)
    got, gf, gs, ge = device_occ(gpu, reads, k)
    assert (got == full).all() and (gf == found).all() and (gs == total).all() and (ge == 0).all(), ("device", tag, k)
    bases, offs = pack(reads)
    hocc, hf, hs, st, he, rc = gpu.query_kmer_occ_packed(bases, offs, k, want_err=True)
    assert rc == 0 and (hocc == full).all() and (hf == found).all() and (hs == total).all() and (he == 0).all(), ("host", tag, k)
    assert st.errors == 0 and st.bases == len(bases)


@pytest.mark.parametrize("sep,mode", SHAPES)
def test_occ_vs_restatement(texts, expected, sep, mode):
    import movi_amd
    reads, exp = expected[sep]
    gpu = movi_amd.MoveIndex.from_image(texts[sep][mode])
    for k in KS:
        check_both_forms(gpu, reads, exp[k], k, (sep, mode))
        assert gpu.last_launch()["kernel"].startswith("kmer_occ_kernel<%d, " % (3 if mode in (3, 2) else 6))
    per_read = gpu.query_kmer_occ(reads, 31)
    assert len(per_read) == len(reads)
    for (f, s, o), w in zip(per_read, exp[31]):
        assert o.dtype == np.uint64 and o.shape == w.shape and (o == w).all() and (f, s) == kmer_occ_ref.found_sum(w)
    assert sum(kmer_occ_ref.found_sum(o)[0] for o in exp[31]) > 10000        # the cases are not vacuous
    assert any(int(o.max()) > 1 for o in exp[5] if o.size)
    gpu.close()


@pytest.fixture(scope="module")
def odd_expected():
    """(kind, sep) -> (reads, {k: occ per read}) from the oracle on the mode-6 image."""
    from oracle.oracle import Oracle
    done = {}

    def get(kind, sep):
        if (kind, sep) not in done:
            reads = list(odd_texts.reads_of(kind))
            o = Oracle(odd_texts.fields(kind, sep, 6)[1])
            done[(kind, sep)] = (reads, {k: kmer_occ_ref.occ(o, reads, k) for k in ODD_KS})
            o.close()
        return done[(kind, sep)]
    return get


@pytest.mark.parametrize("kind", odd_texts.KINDS)
@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("mode", [6, 3])
def test_occ_on_odd_texts(built_lib, odd_expected, kind, sep, mode):
    import movi_amd
    reads, exp = odd_expected(kind, sep)
    gpu = movi_amd.MoveIndex.from_image(odd_texts.fields(kind, sep, mode)[1])
    for k in ODD_KS:
        check_both_forms(gpu, reads, exp[k], k, (kind, sep, mode))
    top = max(int(o.max()) for k in ODD_KS for o in exp[k] if o.size)
    if kind in ("poly", "tandem"):
        assert top > 2047                                     # counts beyond a run's length: the interval spans rows
    if kind == "pangenome":
        assert top >= 24
    gpu.close()


def test_table_too_small_for_windows(built_lib):
    """Fewer than 8 rows: the interval step runs row by row (shrink_interval_rows)."""
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle
    seqs = [b"AAAAAAAACCCCCCCC"]
    reads = [b"AAAACCCC", b"CCCCAAAA", b"GGGGTTTT", b"AAAAGGGG", b"ACGT", b"AANAA", b"", b"A", b"GGGGGGGGGTTTTTTTTT", b"AAAAAAAACCCCCCCCGGGGGGGGTTTTTTTT"]
    for mode in (6, 3):
        img = B.build_index_from_seqs(seqs, mode)
        gpu = movi_amd.MoveIndex.from_image(img)
        assert gpu.desc.r < 8
        o = Oracle(img)
        some = 0
        for k in (1, 2, 3, 5, 8):
            exp = kmer_occ_ref.occ(o, reads, k)
            check_both_forms(gpu, reads, exp, k, mode)
            some += sum(kmer_occ_ref.found_sum(x)[0] for x in exp)
        assert some > 30
        o.close()
        gpu.close()


def built_occ_kernels():
    """Demangled names of the kmer_occ_kernel instantiations in the library's gfx950 code object."""
    import movi_amd
    data = open(movi_amd.lib_path(), "rb").read()
    names, pos = set(), 0
    tmp = "/tmp/movi_occcov_co_%d.o" % os.getpid()
    while True:
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", pos)
        if i < 0:
            break
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, ts = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + ts].decode()
            p += ts
            if "gfx950" in triple and size:
                open(tmp, "wb").write(data[i + off:i + off + size])
                syms = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-sW", tmp], capture_output=True, check=True).stdout.decode()
                mangled = [ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "kmer_occ_kernel" in ln]
                dem = subprocess.run(["c++filt"], input="\n".join(mangled).encode(), capture_output=True, check=True).stdout.decode()
                for ln in dem.splitlines():
                    k = ln.strip()
                    if k.startswith("void movi::"):
                        k = k[len("void movi::"):]
                    names.add(k.split(">(")[0] + ">")
        pos = i + 24
    if os.path.exists(tmp):
        os.remove(tmp)
    return names


def test_options_change_nothing_and_every_kernel_runs(texts, expected):
    import movi_amd
    built = built_occ_kernels()
    assert len(built) == 4, sorted(built)
    reads, exp = expected[False]
    take_log()
    occupancy = {}
    for mode in (6, 3):
        for idx64 in (0, 1):
            gpu = movi_amd.MoveIndex.from_image(texts[False][mode])
            gpu.set_option("idx64", idx64)
            for K in (0, 6, 12):
                gpu.set_option("ftab_k", K)
                for k in (5, 12, 31):
                    check_both_forms(gpu, reads, exp[k], k, (mode, idx64, K))
                    got = device_occ(gpu, reads, k)[0]
                    st = gpu.last_stats()
                    assert (got == slots(reads, exp[k])[0]).all()
                    assert 0 < st.lane_steps <= 64 * st.wave_steps, (mode, idx64, K, k)
                    occupancy[(mode, idx64, K, k)] = round(st.lane_steps / (64.0 * st.wave_steps), 3)
            li = gpu.last_launch()
            assert li["idx64"] == idx64 and li["kernel"] == "kmer_occ_kernel<%d, %s>" % (mode, "unsigned long" if idx64 else "unsigned int")
            gpu.close()
    print("occupancy of the strided lists (mode, idx64, K, k):", occupancy)
    seen = read_log()
    assert {k for k in seen if "kmer_occ_kernel" in k} == built


def test_equals_the_count_query_on_the_kmers_as_reads(texts):
    """Without the oracle: every 31-mer of the reads through movi_count_device as a read of its own."""
    import torch
    import movi_amd
    k, reads = 31, _reads()
    gpu = movi_amd.MoveIndex.from_image(texts[True][6])
    kb, ko, per = kmer_occ_ref.kmers(reads, k)
    n = len(ko) - 1
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(kb)).to(dev), torch.from_numpy(ko.view(np.int64).copy()).to(dev)
    dm = torch.zeros(n, dtype=torch.int64, device=dev)
    dc = torch.zeros(n, dtype=torch.int64, device=dev)
    gpu.count_device(db.data_ptr(), do.data_ptr(), n, int(ko[-1]), dm.data_ptr(), dc.data_ptr())
    torch.cuda.synchronize()
    matched, count = dm.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint64)
    vals = np.where(matched == np.uint64(k), count, np.uint64(0)).astype(np.uint64)
    want, j = [], 0
    for c in per:
        want.append(vals[j:j + c])
        j += c
    assert n > 50000 and np.count_nonzero(vals) > 10000
    check_both_forms(gpu, reads, want, k, "count")
    gpu.close()


def test_capture_without_warmup(texts, expected):
    import torch
    import movi_amd
    reads, exp = expected[True]
    full, found, total = slots(reads, exp[31])
    gpu = movi_amd.MoveIndex.from_image(texts[True][6])
    gpu.prepare(gpu.PREPARE_COUNT)
    scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(bases)).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    docc = torch.full((nb,), -1, dtype=torch.int64, device=dev)
    df = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ds = torch.full((n,), -1, dtype=torch.int64, device=dev)
    de = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            gpu.kmer_occ_device(db.data_ptr(), do.data_ptr(), n, nb, 31, docc.data_ptr(), df.data_ptr(), ds.data_ptr(), de.data_ptr(),
                                stream=s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert (docc.cpu().numpy() == -1).all() and (df.cpu().numpy() == -1).all()         # nothing ran at capture
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    for _ in range(2):
        docc.fill_(-1)
        df.fill_(-1)
        ds.fill_(-1)
        de.fill_(0x77)
        g.replay()
        torch.cuda.synchronize()
        assert (docc.cpu().numpy().view(np.uint64) == full).all()
        assert (df.cpu().numpy().view(np.uint32) == found).all() and (ds.cpu().numpy().view(np.uint64) == total).all()
        assert (de.cpu().numpy() == 0).all()
    del g
    got, gf, gs, ge = device_occ(gpu, reads, 31)                                       # the eager result
    assert (got == full).all() and (gf == found).all() and (gs == total).all() and (ge == 0).all()
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    gpu.close()


def test_host_in_several_chunks(texts, expected):
    """"pipe_chunk_bases" 3000: some forty chunks through the handle's staging, the answers the same; offsets that do not start at 0."""
    import movi_amd
    reads, exp = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    gpu.set_option("pipe_chunk_bases", 3000)
    bases, offs = pack(reads)
    for k in (12, 31):
        full, found, total = slots(reads, exp[k])
        hocc, hf, hs, st, he, rc = gpu.query_kmer_occ_packed(bases, offs, k, want_err=True)
        assert rc == 0 and (hocc == full).all() and (hf == found).all() and (hs == total).all() and (he == 0).all()
        assert st.bases == len(bases) and st.lane_steps > 0
    # the reads from read 7 on: h_occ is laid out relative to h_offsets[0]
    first = int(offs[7])
    hocc, hf, hs, st, he, rc = gpu.query_kmer_occ_packed(bases, offs[7:], 31, want_err=True)
    full, found, total = slots(reads, exp[31])
    assert rc == 0 and (hocc == full[first:]).all() and (hf == found[7:]).all() and (hs == total[7:]).all() and st.bases == len(bases) - first
    gpu.set_option("pipe_chunk_bases", 0)
    gpu.close()


def test_argument_errors(texts, expected):
    import torch
    import movi_amd
    from movi_amd._lib import lib
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    bases, offs = pack([b"ACGTACGT"])
    occ = np.zeros(8, np.uint64)
    L = lib()
    assert L.movi_kmer_occ_host(gpu._h, bases.ctypes.data, offs.ctypes.data, 1, 0, occ.ctypes.data, None, None, None, None) == -1   # k = 0
    assert b"at least 1" in L.movi_last_error()
    assert L.movi_kmer_occ_host(gpu._h, bases.ctypes.data, offs.ctypes.data, 1, 5, None, None, None, None, None) == -1              # no h_occ
    assert L.movi_kmer_occ_host(gpu._h, None, offs.ctypes.data, 1, 5, occ.ctypes.data, None, None, None, None) == -1
    assert L.movi_kmer_occ_host(gpu._h, bases.ctypes.data, None, 1, 5, occ.ctypes.data, None, None, None, None) == -1
    assert L.movi_kmer_occ_device(gpu._h, None, None, 1, 8, 0, None, None, None, None, None) == -1
    assert L.movi_kmer_occ_device(gpu._h, None, None, 1, 8, 5, None, None, None, None, None) == -1                                   # NULL buffers
    assert L.movi_kmer_occ_device(gpu._h, None, None, 0, 0, 5, None, None, None, None, None) == 0                                    # no reads: nothing to do
    # n_bases != offsets[n_reads].  The offsets live on the device, so the call cannot refuse it; it stays inside [0, n_bases): slots
    # at and past n_bases are not touched, a read that reaches past n_bases reports 0xFF and no k-mer, the reads before it are answered
    reads, exp = expected[False]
    reads, occs = reads[:40], exp[12][:40]
    full, found, total = slots(reads, occs)
    b40, o40 = pack(reads)
    n, nb = len(reads), int(o40[-1])
    cut = int(o40[30]) + 3                                                    # inside read 30 (or at its end, if it is short)
    inside = [i for i in range(n) if int(o40[i + 1]) <= cut]
    outside = [i for i in range(n) if int(o40[i + 1]) > cut]
    assert len(inside) >= 25 and outside and sum(found[i] for i in inside) > 0
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(b40)).to(dev), torch.from_numpy(o40.view(np.int64).copy()).to(dev)
    docc = torch.full((nb,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    df = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ds = torch.full((n,), -1, dtype=torch.int64, device=dev)
    de = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
    gpu.kmer_occ_device(db.data_ptr(), do.data_ptr(), n, cut, 12, docc.data_ptr(), df.data_ptr(), ds.data_ptr(), de.data_ptr())
    torch.cuda.synchronize()
    got, gf, gs, ge = docc.cpu().numpy().view(np.uint64), df.cpu().numpy().view(np.uint32), ds.cpu().numpy().view(np.uint64), de.cpu().numpy()
    assert (got[cut:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    last_in = int(o40[inside[-1] + 1])
    assert (got[:last_in] == full[:last_in]).all() and (got[last_in:cut] == 0).all()
    assert (ge[inside] == 0).all() and (gf[inside] == found[inside]).all() and (gs[inside] == total[inside]).all()
    assert (ge[outside] == 0xFF).all() and (gf[outside] == 0).all() and (gs[outside] == 0).all()
    gpu.close()


def test_corrupt_table(texts, expected):
    """One row's destination id set to r + 5: a k-mer whose search takes an LF step from that row becomes an error slot, every other
    slot is answered, the call returns; the host form reports MOVI_ERR_INVARIANT."""
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle, OracleError
    ref = _ref()
    reads, exp = expected[False]
    t0, k = 10000, 31
    probe = ref[t0:t0 + k]
    reads = list(reads) + [probe]
    good = Oracle(texts[False][6])
    occ = exp[k] + kmer_occ_ref.occ(good, [probe], k)
    good.close()
    assert int(occ[-1][0]) >= 1
    # the row that holds the BWT position of the suffix at t0 + 11: an end of the probe's interval stands there after 20 bases
    text = B.clean_text([ref], separators=False)
    assert bytes(text[t0:t0 + k]) == probe
    sa = np.asarray(B.suffix_array(text))
    p = int(np.flatnonzero(sa == t0 + 11)[0])
    img = bytearray(texts[False][6])
    desc, _, off, _ = movi_amd.parse_index_image(bytes(img))
    rows = np.frombuffer(img, np.uint8, count=desc.r * 8, offset=off).reshape(-1, 8).copy()
    lens = rows.view(np.uint32).reshape(-1, 2)[:, 1] & 0x7FF
    j = int(np.searchsorted(np.cumsum(lens.astype(np.int64)), p, "right"))
    rows[j, 0:4] = np.frombuffer(struct.pack("<I", desc.r + 5), np.uint8)
    img[off: off + rows.size] = rows.tobytes()
    o = Oracle(bytes(img))                                                    # the premise, on the CPU: the reference throws on the probe
    with pytest.raises(OracleError):
        o.count_batch(*pack([probe]))
    o.close()
    bad = movi_amd.MoveIndex.from_image(bytes(img))
    full, found, total = slots(reads, occ)
    got, gf, gs, ge = device_occ(bad, reads, k)                               # the call returns
    st = bad.last_stats()
    is_err = (got & ERR_BIT) != 0
    assert is_err.any() and ((got == full) | is_err).all()
    assert st.errors == int(is_err.sum())
    assert set(np.unique(got[is_err] & np.uint64(0xFF))) <= {1, 2} and ((got[is_err] | np.uint64(0xFF)) == np.uint64(2 ** 64 - 1)).all()
    _, offs = pack(reads)
    hit = np.array([is_err[int(offs[i]):int(offs[i + 1])].any() for i in range(len(reads))])
    assert hit[-1]                                                            # the probe itself
    assert (ge[hit] != 0).all() and (gf[hit] == 0).all() and (gs[hit] == 0).all()
    assert (ge[~hit] == 0).all() and (gf[~hit] == found[~hit]).all() and (gs[~hit] == total[~hit]).all()
    bases, offs = pack(reads)
    hocc, hf, hs, hst, he, rc = bad.query_kmer_occ_packed(bases, offs, k, want_err=True)
    assert rc == -6 and hst.errors == st.errors and (hocc == got).all() and (he == ge).all() and (hf == gf).all() and (hs == gs).all()
    bad.close()


def _write_fastq(path, ids, reads):
    with open(path, "wb") as f:
        for i, r in zip(ids, reads):
            f.write(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


@pytest.mark.parametrize("sep", [False, True])
def test_cli(built_lib, tmp_path, sep):
    from oracle.oracle import Oracle
    idx = tmp_path / "idx"
    r = subprocess.run([MOVI, "build", "-i", str(idx), "-f", os.path.join(GOLDEN, "ref.fasta"), "--type", "regular-thresholds"] +
                       (["--separators"] if sep else []), capture_output=True)
    assert r.returncode == 0, r.stderr
    o = Oracle((idx / "index.movi").read_bytes())
    recs = read_fastx(os.path.join(GOLDEN, "sample.fastq"))
    ids = [i.encode() if isinstance(i, str) else i for i, _ in recs]
    reads = [s for _, s in recs]
    more = [x for x in mutated_reads(np.random.default_rng(99), _ref(), 200, 1, 400) if x]
    ids += [b"m%d" % i for i in range(len(more))]
    reads += more
    fq = str(tmp_path / "reads.fq")
    _write_fastq(fq, ids, reads)

    def lines(rs, k):
        occ = kmer_occ_ref.occ(o, rs, k)
        txt = b"".join(kmer_occ_ref.line(i, len(x), k, v) for i, x, v in zip(ids, rs, occ))
        f = sum(kmer_occ_ref.found_sum(v)[0] for v in occ)
        s = sum(kmer_occ_ref.found_sum(v)[1] for v in occ)
        return txt, b"Number of kmers found in the index:\t%d\nSum of the counts of found k-mers:\t%d\n" % (f, s)

    base = [MOVI, "query", "-i", str(idx), "-r", fq, "--kmer-occ"]
    for kargs, k in (([], 31), (["-k", "12"], 12)):
        want, summary = lines(reads, k)
        assert want.count(b"\n") == len(reads) and b"\t0/0\t0\t\n" in lines([b"ACGT"], 31)[0]
        r = subprocess.run(base + kargs + ["-o", str(tmp_path / "o")], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / ("o.kmer_occ.%d" % k)).read_bytes() == want
        assert r.stdout == summary
        r = subprocess.run(base + kargs + ["--stdout", "--ftab-k", "8"], capture_output=True)
        assert r.returncode == 0 and r.stdout == want and summary in r.stderr, r.stderr
        r = subprocess.run(base + kargs + ["--no-output", "-o", str(tmp_path / "none")], capture_output=True)
        assert r.returncode == 0 and r.stdout == summary and not (tmp_path / ("none.kmer_occ.%d" % k)).exists(), r.stderr
    rev = [x[::-1] for x in reads]
    want, summary = lines(rev, 12)
    r = subprocess.run(base + ["-k", "12", "--reverse", "--stdout"], capture_output=True)
    assert r.returncode == 0 and r.stdout == want and summary in r.stderr, r.stderr
    # --gpus N shards each chunk of reads over N handles (MOVI_SHARE_GPU=1: every logical GPU is device 0): the same bytes
    want, summary = lines(reads, 12)
    r = subprocess.run(base + ["-k", "12", "--stdout", "--gpus", "3"], capture_output=True, env=dict(os.environ, MOVI_SHARE_GPU="1"))
    assert r.returncode == 0 and r.stdout == want and summary in r.stderr, r.stderr
    o.close()
