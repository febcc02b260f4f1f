"""GPU suite (-m gpu): k-mer presence (movi_kmer_host / movi_kmer_device, `movi query --kmer`) against the contract of
include/movi_hip.h, restated on the oracle's backward search in tests/kmer_ref.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_fastx
from test_gpu_parity import mutated_reads, pack
from test_kernel_coverage_gpu import read_log, take_log
import kmer_ref

pytestmark = pytest.mark.gpu

KS = (1, 5, 12, 13, 31, 200)
MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
SHAPES = [(False, 6), (False, 8), (False, 7), (False, 3), (False, 2), (False, 5), (True, 6), (True, 8)]


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _edge_reads(ref):
    out = [b"", ref[100:101], b"N" * 40, b"%", ref[1000:6000], ref[2000:2100] + b"N" + ref[2101:2200],
           ref[3000:3100].lower() + ref[3100:3200], ref[4000:4040] + b"%" + ref[4041:4100]]
    for k in KS:
        out += [ref[300:300 + k - 1], ref[400:400 + k], ref[500:500 + k + 1]]
    return out


def _reads():
    ref = _ref()
    return ([s for _, s in read_fastx(os.path.join(GOLDEN, "sample.fastq"))] +
            mutated_reads(np.random.default_rng(616), ref, 2000, 1, 400) + _edge_reads(ref))


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
    """{separators: (reads, {k: (found, runs) per read})} from the oracle on the mode-6 image of each text."""
    from oracle.oracle import Oracle
    reads = _reads()
    out = {}
    for sep, imgs in texts.items():
        o = Oracle(imgs[6])
        exp, _ = kmer_ref.restate(o, reads, KS)
        o.close()
        out[sep] = (reads, exp)
    return out


def _unpack(runs, n_runs, found, offs, n):
    return [(int(found[i]), [(int(x["start"]), int(x["count"])) for x in runs[int(offs[i]):int(offs[i]) + int(n_runs[i])]])
            for i in range(n)]


def device_kmers(gpu, reads, k, order=None, with_err=False):
    """movi_kmer_device on torch buffers -> (found, runs) per read (and the error bytes)."""
    import torch
    from movi_amd.engine import KMER_RUN_DTYPE
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(bases) if nb else np.zeros(1, np.uint8)).to(dev)
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dr = torch.full((max(nb, 1) * 8,), 0x5A, dtype=torch.uint8, device=dev)
    dn = torch.full((n,), -1, dtype=torch.int32, device=dev)
    df = torch.full((n,), -1, dtype=torch.int32, device=dev)
    de = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
    dord = torch.from_numpy(np.asarray(order, np.int32)).to(dev) if order is not None else None
    gpu.kmer_device(db.data_ptr(), do.data_ptr(), n, nb, k, dr.data_ptr(), dn.data_ptr(), df.data_ptr(), de.data_ptr(),
                    d_order=dord.data_ptr() if dord is not None else 0)
    torch.cuda.synchronize()
    out = _unpack(dr.cpu().numpy().view(KMER_RUN_DTYPE), dn.cpu().numpy().view(np.uint32), df.cpu().numpy().view(np.uint32), offs, n)
    return (out, de.cpu().numpy()) if with_err else out


def _check(want):
    """The restatement itself: found = sum of the counts, at most max(0, m - k + 1) runs (what the device layout relies on)."""
    for found, runs in want:
        assert found == sum(c for _, c in runs)


@pytest.mark.parametrize("sep,mode", SHAPES)
def test_kmers_vs_restatement(texts, expected, sep, mode):
    import movi_amd
    reads, exp = expected[sep]
    gpu = movi_amd.MoveIndex.from_image(texts[sep][mode])
    total = 0
    for k in KS:
        want = exp[k]
        _check(want)
        for r, (_, runs) in zip(reads, want):
            assert len(runs) <= max(0, len(r) - k + 1)
        got = gpu.query_kmers(reads, k)
        assert got == want, (mode, sep, k)
        got, err = device_kmers(gpu, reads, k, with_err=True)
        assert got == want and (err == 0).all(), (mode, sep, k)
        total += sum(f for f, _ in want)
    assert total > 100000                                     # the cases are not vacuous
    assert gpu.last_launch()["kernel"].startswith("kmer_kernel<%d, " % (3 if mode in (3, 2) else 6))
    gpu.close()


def test_table_and_lookahead_change_nothing(texts, expected):
    import movi_amd
    reads, exp = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    steps = {}
    for K in (0, 6, 12):
        gpu.set_option("ftab_k", K)
        for la in (-1, 3, 0, 2):
            gpu.set_option("kmer_lookahead", la)
            for k in (1, 5, 12, 13, 31):
                assert gpu.query_kmers(reads, k) == exp[k], (K, la, k)
                assert device_kmers(gpu, reads, k) == exp[k], (K, la, k)
                st = gpu.last_stats()
                assert st.lane_steps > 0 and st.wave_steps > 0 and st.lane_steps <= 64 * st.wave_steps
                steps[(K, la, k)] = st.lane_steps
    print("lane steps (K, lookahead, k):", steps)
    gpu.close()


def test_read_order(texts, expected):
    import movi_amd
    reads, exp = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    perm = np.random.default_rng(3).permutation(len(reads))
    for k in (12, 31):
        got, err = device_kmers(gpu, reads, k, order=perm, with_err=True)
        assert got == exp[k] and (err == 0).all()
    gpu.close()


def test_table_too_small_for_windows(built_lib):
    """Fewer than 8 rows: the interval step runs row by row (shrink_interval_rows)."""
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle
    seqs = [b"AAAAAAAACCCCCCCC"]
    for mode in (6, 3):
        img = B.build_index_from_seqs(seqs, mode)
        gpu = movi_amd.MoveIndex.from_image(img)
        assert gpu.desc.r < 8
        o = Oracle(img)
        reads = [b"AAAACCCC", b"CCCCAAAA", b"GGGGTTTT", b"AAAAGGGG", b"ACGT", b"AANAA", b"", b"A", b"GGGGGGGGGTTTTTTTTT", b"AAAAAAAACCCCCCCCGGGGGGGGTTTTTTTT"]
        exp, _ = kmer_ref.restate(o, reads, (1, 2, 3, 5, 8))
        for k in (1, 2, 3, 5, 8):
            for la in (3, 0):
                gpu.set_option("kmer_lookahead", la)
                assert gpu.query_kmers(reads, k) == exp[k], (mode, k, la)
                assert device_kmers(gpu, reads, k) == exp[k], (mode, k, la)
        assert sum(f for f, _ in exp[3]) > 10
        o.close()
        gpu.close()


def test_argument_errors(texts):
    import movi_amd
    from movi_amd._lib import lib
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    bases, offs = pack([b"ACGTACGT"])
    nr, found, total = np.zeros(1, np.uint32), np.zeros(1, np.uint32), C.c_uint64(0)
    runs = np.zeros(8, np.uint64)
    rc = lib().movi_kmer_host(gpu._h, bases.ctypes.data, offs.ctypes.data, 1, 0, nr.ctypes.data, found.ctypes.data, runs.ctypes.data, 8,
                              C.byref(total), None)
    assert rc == -1                                           # k = 0: MOVI_ERR_ARG
    rc = lib().movi_kmer_device(gpu._h, None, None, 1, 8, 0, None, None, None, None, None, None)
    assert rc == -1
    rc = lib().movi_kmer_device(gpu._h, None, None, 1, 8, 5, None, None, None, None, None, None)
    assert rc == -1                                           # NULL buffers
    with pytest.raises(movi_amd.MoviError):
        gpu.set_option("kmer_lookahead", 1)
    with pytest.raises(movi_amd.MoviError):
        gpu.set_option("kmer_lookahead", -2)
    gpu.close()


def test_capture_without_warmup(texts, expected):
    import torch
    import movi_amd
    from movi_amd.engine import KMER_RUN_DTYPE
    reads, exp = expected[True]
    gpu = movi_amd.MoveIndex.from_image(texts[True][6])
    gpu.prepare(gpu.PREPARE_COUNT)
    scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(bases)).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dr = torch.zeros(nb * 8, dtype=torch.uint8, device=dev)
    dn = torch.full((n,), -1, dtype=torch.int32, device=dev)
    df = torch.full((n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            gpu.kmer_device(db.data_ptr(), do.data_ptr(), n, nb, 31, dr.data_ptr(), dn.data_ptr(), df.data_ptr(), stream=s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert (dn.cpu().numpy() == -1).all()                             # nothing ran at capture
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    for _ in range(2):
        dn.fill_(-1)
        df.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = _unpack(dr.cpu().numpy().view(KMER_RUN_DTYPE), dn.cpu().numpy().view(np.uint32), df.cpu().numpy().view(np.uint32), offs, n)
        assert got == exp[31]
    del g
    assert device_kmers(gpu, reads, 31) == exp[31]                    # the eager result
    gpu.close()


def built_kmer_kernels():
    import movi_amd
    data = open(movi_amd.lib_path(), "rb").read()
    names, pos = set(), 0
    tmp = "/tmp/movi_kmercov_co_%d.o" % os.getpid()
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
                mangled = [ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "kmer_kernel" in ln]
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


def test_every_kmer_kernel_is_reachable(texts, expected):
    import movi_amd
    built = built_kmer_kernels()
    assert len(built) == 4, sorted(built)
    reads, exp = expected[False]
    take_log()
    for mode in (6, 3):
        for idx64 in (0, 1):
            gpu = movi_amd.MoveIndex.from_image(texts[False][mode])
            gpu.set_option("idx64", idx64)
            for k in (12, 31):
                assert gpu.query_kmers(reads, k) == exp[k], (mode, idx64, k)
                assert device_kmers(gpu, reads, k) == exp[k], (mode, idx64, k)
            li = gpu.last_launch()
            assert li["idx64"] == idx64 and li["kernel"] == "kmer_kernel<%d, %s>" % (mode, "unsigned long" if idx64 else "unsigned int")
            gpu.close()
    seen = read_log()
    assert {k for k in seen if "kmer_kernel" in k} == built


def test_host_cap_too_small(texts, expected):
    import movi_amd
    from movi_amd._lib import QueryStatsC, lib
    from movi_amd.engine import KMER_RUN_DTYPE
    reads, exp = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    bases, offs = pack(reads)
    n = len(reads)
    want_n = np.array([len(runs) for _, runs in exp[12]], np.uint32)
    want_f = np.array([f for f, _ in exp[12]], np.uint32)
    cap = int(want_n.sum()) - 1
    nr, found = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    runs = np.zeros(cap, KMER_RUN_DTYPE)
    total = C.c_uint64(0)
    rc = lib().movi_kmer_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, 12, nr.ctypes.data, found.ctypes.data, runs.ctypes.data, cap,
                              C.byref(total), C.byref(QueryStatsC()))
    assert rc == -1 and total.value == want_n.sum() and (nr == want_n).all() and (found == want_f).all()
    nr2, found2, runs2, st, rc2 = gpu.query_kmers_packed(bases, offs, 12, want_rc=True)
    assert rc2 == 0 and len(runs2) == want_n.sum() and st.lane_steps > 0
    gpu.close()


@pytest.fixture(scope="module")
def tile(texts):
    """A small batch of short reads (mean length < 128, so that 2^25 bases hold more than 2^18 reads and the host loop cuts there), one
    with an illegal base and one shorter than k among them, and its k-mers at k = 13 from the oracle."""
    from oracle.oracle import Oracle
    k, ref = 13, _ref()
    reads = [r for r in _reads() if len(r) <= 120][:300] + [ref[2000:2050] + b"N" + ref[2051:2100], ref[300:300 + k - 1]]
    o = Oracle(texts[False][6])
    exp, _ = kmer_ref.restate(o, reads, (k,))
    o.close()
    return k, reads, exp[k]


@pytest.mark.parametrize("K", [0, 12])
def test_host_two_chunks(texts, tile, K):
    """movi_kmer_host on just over 2^25 bases -- the tile repeated -- takes two chunks: the second chunk's runs follow the first's."""
    import movi_amd
    from movi_amd._lib import QueryStatsC, lib
    from movi_amd.engine import KMER_RUN_DTYPE
    k, reads, want = tile
    tb, toffs = pack(reads)
    tnb = int(toffs[-1])
    copies = (1 << 25) // tnb + 2                             # past 2^25 + one copy
    bases = np.tile(np.asarray(tb), copies)
    offs = np.concatenate([(toffs[:-1].astype(np.uint64) + np.uint64(c * tnb)) for c in range(copies)] + [np.array([copies * tnb], np.uint64)])
    n = len(reads) * copies
    assert (1 << 25) + tnb < copies * tnb <= (1 << 25) + 2 * tnb
    assert np.searchsorted(offs, 1 << 25, "right") - 1 >= 1 << 18          # the first chunk ends at 2^25 bases, not at 2^27
    want_n = np.tile(np.array([len(runs) for _, runs in want], np.uint32), copies)
    want_f = np.tile(np.array([f for f, _ in want], np.uint32), copies)
    want_runs = np.tile(np.array([r for _, runs in want for r in runs], KMER_RUN_DTYPE), copies)
    assert len(want_runs) > len(reads)
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    gpu.set_option("ftab_k", K)
    nr, found = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    runs = np.zeros(len(want_runs), KMER_RUN_DTYPE)
    total, st = C.c_uint64(0), QueryStatsC()
    rc = lib().movi_kmer_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, k, nr.ctypes.data, found.ctypes.data, runs.ctypes.data,
                              len(runs), C.byref(total), C.byref(st))
    assert rc == 0 and total.value == len(want_runs) and st.bases == copies * tnb
    assert (nr == want_n).all() and (found == want_f).all()
    assert (runs == want_runs).all()
    nr[:] = 0
    found[:] = 0
    rc = lib().movi_kmer_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, k, nr.ctypes.data, found.ctypes.data, runs.ctypes.data,
                              len(runs) - 1, C.byref(total), C.byref(st))
    assert rc == -1 and total.value == len(want_runs) and (nr == want_n).all() and (found == want_f).all()
    assert ("%d runs found, runs_cap is %d" % (len(want_runs), len(runs) - 1)).encode() in lib().movi_last_error()
    gpu.close()


def _kmer_lines(ids, reads, oracle, k):
    exp, _ = kmer_ref.restate(oracle, reads, (k,))
    return b"".join(kmer_ref.line(i, len(r), k, f, runs) for i, r, (f, runs) in zip(ids, reads, exp[k]))


def test_cli(texts, tmp_path):
    from oracle.oracle import Oracle
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(texts[False][6])
    o = Oracle(texts[False][6])
    ref = _ref()
    fq = os.path.join(GOLDEN, "sample.fastq")
    fa = tmp_path / "n.fa"
    seqs = [ref[100:300], ref[500:560] + b"NNN" + ref[600:700], b"ACGTN" * 10, ref[900:1000].lower() + ref[1000:1100], ref[50:60],
            ref[1200:1300] + b"T" + ref[1301:1500]]
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    for path in (fq, str(fa)):
        recs = read_fastx(path)
        ids, reads = [i.encode() if isinstance(i, str) else i for i, _ in recs], [s for _, s in recs]
        for kargs, k in (([], 31), (["-k", "12"], 12)):
            want = _kmer_lines(ids, reads, o, k)
            assert want.count(b"\n") == len(reads)
            for ftab in ([], ["--ftab-k", "8"]):
                out = tmp_path / "o"
                base = ["query", "-i", str(idx), "--kmer"] + kargs + ftab
                r = subprocess.run([MOVI] + base + ["-r", path, "-o", str(out)], capture_output=True)
                assert r.returncode == 0, r.stderr
                assert (tmp_path / ("o.kmers.%d" % k)).read_bytes() == want
                r = subprocess.run([MOVI] + base + ["-r", path, "--stdout"], capture_output=True)
                assert r.returncode == 0 and r.stdout == want, r.stderr
    # the reference's prefix rule without -o: <reads>.<index type>.kmers.<k>
    fa2 = tmp_path / "m.fa"
    fa2.write_bytes(fa.read_bytes())
    r = subprocess.run([MOVI, "query", "-i", str(idx), "--kmer", "-k", "12", "-r", str(fa2)], capture_output=True)
    assert r.returncode == 0, r.stderr
    made = [p.name for p in tmp_path.iterdir() if p.name.startswith("m.fa.")]
    assert len(made) == 1 and made[0].endswith(".kmers.12"), made
    recs = read_fastx(str(fa))
    ids, reads = [i.encode() if isinstance(i, str) else i for i, _ in recs], [s for _, s in recs]
    assert (tmp_path / made[0]).read_bytes() == _kmer_lines(ids, reads, o, 12)
    r = subprocess.run([MOVI, "query", "-i", str(idx), "--kmer", "-r", str(fa), "--no-output", "-o", str(tmp_path / "none")], capture_output=True)
    assert r.returncode == 0 and not (tmp_path / "none.kmers.31").exists()
    # --gpus N shards each chunk of reads over N handles (MOVI_SHARE_GPU=1: every logical GPU is device 0): the same bytes
    recs = read_fastx(fq)
    ids, reads = [i.encode() if isinstance(i, str) else i for i, _ in recs], [s for _, s in recs]
    r = subprocess.run([MOVI, "query", "-i", str(idx), "--kmer", "-k", "12", "-r", fq, "--stdout", "--gpus", "3"], capture_output=True,
                       env=dict(os.environ, MOVI_SHARE_GPU="1"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == _kmer_lines(ids, reads, o, 12)
    o.close()


def test_cli_more_runs_than_the_first_guess(texts, tmp_path):
    """The command gives a shard's runs room for 8 per read and one per 16 bases first, and calls again with room for exactly what the
    first call found.  Six random reads of 200 bases at -k 8 (about every other 8-mer is in the text: 578 runs by the restatement) against
    a first guess of 6 * 8 + 1200 / 16 = 123 (two shards: 3 * 8 + 600 / 16 = 61 each), so the bytes below come from the second call."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(7)
    seqs = [bytes(rng.choice(list(b"ACGT"), 200).astype(np.uint8)) for _ in range(6)]
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(texts[False][6])
    fa = tmp_path / "q.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    o = Oracle(texts[False][6])
    exp, _ = kmer_ref.restate(o, seqs, (8,))
    per_read = [len(runs) for _, runs in exp[8]]
    assert sum(per_read) > 6 * 8 + 1200 // 16 and min(sum(per_read[:3]), sum(per_read[3:])) > 3 * 8 + 600 // 16
    want = _kmer_lines([b"r%d" % i for i in range(6)], seqs, o, 8)
    for extra, env in (([], {}), (["--gpus", "2"], {"MOVI_SHARE_GPU": "1"})):
        r = subprocess.run([MOVI, "query", "-i", str(idx), "--kmer", "-k", "8", "-r", str(fa), "--stdout"] + extra,
                           capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == want, (extra, r.stderr)
    o.close()
