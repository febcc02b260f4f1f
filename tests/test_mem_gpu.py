"""GPU suite (-m gpu): MEM finding (movi_mem_host / movi_mem_device, `movi query --mem`) against the contract of
include/movi_hip.h, restated on the oracle's backward search in tests/mem_ref.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_fastx
from test_gpu_parity import mutated_reads, pack
from test_kernel_coverage_gpu import read_log, take_log
import mem_ref

pytestmark = pytest.mark.gpu

LS = (0, 1, 5, 12, 25, 31, 200)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _edge_reads(ref):
    out = [b"", ref[100:101], b"N" * 40, ref[1000:6000]]
    for Lp in (1, 5, 12, 25, 31, 200):
        out += [ref[300:300 + Lp - 1], ref[400:400 + Lp]]
    return out


def _reads():
    ref = _ref()
    return ([s for _, s in read_fastx(os.path.join(GOLDEN, "sample.fastq"))] +
            mutated_reads(np.random.default_rng(515), ref, 2000, 1, 400) + _edge_reads(ref))


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
    """{separators: (reads, {L: mems per read}, arrays)} from the oracle on the mode-6 image of each text."""
    from oracle.oracle import Oracle
    import movi_amd
    reads = _reads()
    out = {}
    for sep, imgs in texts.items():
        desc, _, _, _ = movi_amd.parse_index_image(imgs[6])
        o = Oracle(imgs[6])
        exp, arr = mem_ref.restate(o, reads, desc.code_of, LS)
        o.close()
        out[sep] = (reads, exp, arr, desc.code_of)
    return out


def device_mems(gpu, reads, L, order=None, with_err=False):
    """movi_mem_device on torch buffers -> list of (start, end, count) per read (and the error bytes)."""
    import torch
    from movi_amd.engine import MEM_DTYPE
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(bases) if nb else np.zeros(1, np.uint8)).to(dev)
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dm = torch.full((max(nb, 1) * 16,), 0x5A, dtype=torch.uint8, device=dev)
    dn = torch.full((n,), -1, dtype=torch.int32, device=dev)
    de = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
    dord = torch.from_numpy(np.asarray(order, np.int32)).to(dev) if order is not None else None
    gpu.mem_device(db.data_ptr(), do.data_ptr(), n, nb, L, dm.data_ptr(), dn.data_ptr(), de.data_ptr(),
                   d_order=dord.data_ptr() if dord is not None else 0)
    torch.cuda.synchronize()
    mems = dm.cpu().numpy().view(MEM_DTYPE)
    nm = dn.cpu().numpy().view(np.uint32)
    out = [[(int(x["start"]), int(x["end"]), int(x["count"])) for x in mems[int(offs[i]):int(offs[i]) + int(nm[i])]]
           for i in range(n)]
    return (out, de.cpu().numpy()) if with_err else out


@pytest.mark.parametrize("sep,mode", [(False, 6), (False, 8), (False, 7), (False, 3), (False, 2), (False, 5), (True, 6), (True, 8)])
def test_mems_vs_restatement(texts, expected, sep, mode):
    import movi_amd
    reads, exp, arr, _ = expected[sep]
    gpu = movi_amd.MoveIndex.from_image(texts[sep][mode])
    for L in LS:
        want = exp[L]
        assert want == [mem_ref.mems_set(fw, cnt, len(r), L) for r, (bw, fw, cnt) in zip(reads, arr)], L   # closed text
        got = gpu.query_mems(reads, L)
        assert got == want, (mode, sep, L)
        assert device_mems(gpu, reads, L) == want, (mode, sep, L)
    assert gpu.last_launch()["kernel"].startswith("mem_kernel<%d, " % (3 if mode in (3, 2) else 6))
    gpu.close()


def test_interval_table_changes_nothing(texts, expected):
    import movi_amd
    reads, exp, _, _ = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    for K in (0, 8, 12):
        gpu.set_option("ftab_k", K)
        for L in (1, 5, 12, 25):
            assert gpu.query_mems(reads, L) == exp[L], (K, L)
    gpu.close()


def test_text_not_closed_under_rc(built_lib):
    """8 synthetic genomes, no separators: the junctions of the records are not rc-symmetric; still the header's loop."""
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle
    rng = np.random.default_rng(8181)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(rng.integers(500, 3000))).astype(np.uint8)) for _ in range(8)]
    img = B.build_index_from_seqs(seqs, 6)
    t = bytes(B.clean_text(seqs)[:-1])
    reads = mutated_reads(rng, t, 600, 1, 300)
    ends = np.cumsum([2 * len(s) for s in seqs])[:-1]
    reads += [t[e - 40:e + 40] for e in ends] + [t[e - 40:e + 40].translate(COMP)[::-1] for e in ends]
    gpu = movi_amd.MoveIndex.from_image(img)
    o = Oracle(img)
    exp, _ = mem_ref.restate(o, reads, gpu.desc.code_of, (1, 5, 12, 25))
    for L in (1, 5, 12, 25):
        assert gpu.query_mems(reads, L) == exp[L], L
        assert device_mems(gpu, reads, L) == exp[L], L
    o.close()
    gpu.close()


def test_read_order_errors_and_corrupt_rows(texts, expected):
    import movi_amd
    reads, exp, _, _ = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    perm = np.random.default_rng(3).permutation(len(reads))
    got, err = device_mems(gpu, reads, 12, order=perm, with_err=True)
    assert got == exp[12] and (err == 0).all()
    gpu.close()
    # a corrupted row table (as in tests/test_top_of_walk_gpu.py): MOVI_ERR_INVARIANT, per-read codes, no MEMs for those reads
    img = bytearray(texts[False][6])
    desc, _, off, _ = movi_amd.parse_index_image(bytes(img))
    rows = np.frombuffer(img, np.uint8, count=desc.r * 8, offset=off).reshape(-1, 8).copy()
    rng = np.random.default_rng(8600)
    rows[rng.choice(desc.r, desc.r // 4, replace=False), 0:4] = 0xFF
    img[off: off + rows.size] = rows.tobytes()
    bad = movi_amd.MoveIndex.from_image(bytes(img))
    bases, offs = pack(reads)
    nm, mems, st, e, rc = bad.query_mems_packed(bases, offs, 12, want_err=True)
    assert rc == -6 and st.errors > 50 and (e != 0).sum() == st.errors
    assert (nm[e != 0] == 0).all() and set(np.unique(e[e != 0])) <= {1, 2}
    dgot, derr = device_mems(bad, reads, 12, with_err=True)
    assert (derr == e).all() and all(not dgot[i] for i in np.nonzero(e)[0])
    bad.close()


def test_capture_without_warmup(texts, expected):
    import torch
    import movi_amd
    from movi_amd.engine import MEM_DTYPE
    reads, exp, _, _ = expected[True]
    gpu = movi_amd.MoveIndex.from_image(texts[True][6])
    gpu.prepare(gpu.PREPARE_COUNT)
    scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(bases)).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dm = torch.zeros(nb * 16, dtype=torch.uint8, device=dev)
    dn = torch.full((n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            gpu.mem_device(db.data_ptr(), do.data_ptr(), n, nb, 25, dm.data_ptr(), dn.data_ptr(), stream=s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert (dn.cpu().numpy() == -1).all()                             # nothing ran at capture
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    for _ in range(2):
        dn.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        mems, nm = dm.cpu().numpy().view(MEM_DTYPE), dn.cpu().numpy().view(np.uint32)
        got = [[(int(x["start"]), int(x["end"]), int(x["count"])) for x in mems[int(offs[i]):int(offs[i]) + int(nm[i])]]
               for i in range(n)]
        assert got == exp[25]
    del g
    gpu.close()


def built_mem_kernels():
    import movi_amd
    data = open(movi_amd.lib_path(), "rb").read()
    names, pos = set(), 0
    tmp = "/tmp/movi_memcov_co_%d.o" % os.getpid()
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
                mangled = [ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "mem_kernel" in ln]
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


def test_every_mem_kernel_is_reachable(texts, expected):
    import movi_amd
    built = built_mem_kernels()
    assert len(built) == 4, sorted(built)
    reads, exp, _, _ = expected[False]
    seen = set()
    take_log()
    for mode in (6, 3):
        for idx64 in (0, 1):
            gpu = movi_amd.MoveIndex.from_image(texts[False][mode])
            gpu.set_option("idx64", idx64)
            assert gpu.query_mems(reads, 25) == exp[25], (mode, idx64)
            li = gpu.last_launch()
            assert li["idx64"] == idx64 and li["kernel"] == "mem_kernel<%d, %s>" % (mode, "unsigned long" if idx64 else "unsigned int")
            gpu.close()
    seen = read_log()
    assert {k for k in seen if "mem_kernel" in k} == built


def test_host_cap_too_small(texts, expected):
    import ctypes as C
    import movi_amd
    from movi_amd._lib import QueryStatsC, lib
    from movi_amd.engine import MEM_DTYPE
    reads, exp, _, _ = expected[False]
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    bases, offs = pack(reads)
    n = len(reads)
    want_n = np.array([len(x) for x in exp[12]], np.uint32)
    cap = int(want_n.sum()) - 1
    nm = np.zeros(n, np.uint32)
    mems = np.zeros(cap, MEM_DTYPE)
    total = C.c_uint64(0)
    rc = lib().movi_mem_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, 12, nm.ctypes.data, mems.ctypes.data, cap,
                             C.byref(total), None, C.byref(QueryStatsC()))
    assert rc == -1 and total.value == want_n.sum() and (nm == want_n).all()
    gpu.close()


@pytest.fixture(scope="module")
def tile(texts):
    """A small batch of short reads (mean length < 128, so that 2^25 bases hold more than 2^18 reads and the host loop cuts there), one
    with an illegal base and one shorter than L among them, and its MEMs at L = 25 from the oracle."""
    from oracle.oracle import Oracle
    import movi_amd
    L, ref = 25, _ref()
    reads = [r for r in _reads() if len(r) <= 120][:300] + [ref[2000:2050] + b"N" + ref[2051:2100], ref[300:300 + L - 1]]
    desc, _, _, _ = movi_amd.parse_index_image(texts[False][6])
    o = Oracle(texts[False][6])
    exp, _ = mem_ref.restate(o, reads, desc.code_of, (L,))
    o.close()
    return L, reads, exp[L]


@pytest.mark.parametrize("K", [0, 12])
def test_host_two_chunks(texts, tile, K):
    """movi_mem_host on just over 2^25 bases -- the tile repeated -- takes two chunks: the second chunk's MEMs follow the first's."""
    import ctypes as C
    import movi_amd
    from movi_amd._lib import QueryStatsC, lib
    from movi_amd.engine import MEM_DTYPE
    L, reads, want = tile
    tb, toffs = pack(reads)
    tnb = int(toffs[-1])
    copies = (1 << 25) // tnb + 2                             # past 2^25 + one copy
    bases = np.tile(np.asarray(tb), copies)
    offs = np.concatenate([(toffs[:-1].astype(np.uint64) + np.uint64(c * tnb)) for c in range(copies)] + [np.array([copies * tnb], np.uint64)])
    n = len(reads) * copies
    assert (1 << 25) + tnb < copies * tnb <= (1 << 25) + 2 * tnb
    assert np.searchsorted(offs, 1 << 25, "right") - 1 >= 1 << 18          # the first chunk ends at 2^25 bases, not at 2^27
    want_n = np.tile(np.array([len(x) for x in want], np.uint32), copies)
    want_mems = np.tile(np.array([m for x in want for m in x], MEM_DTYPE), copies)
    assert len(want_mems) > len(reads)
    gpu = movi_amd.MoveIndex.from_image(texts[False][6])
    gpu.set_option("ftab_k", K)
    nm = np.zeros(n, np.uint32)
    mems = np.zeros(len(want_mems), MEM_DTYPE)
    total, st = C.c_uint64(0), QueryStatsC()
    rc = lib().movi_mem_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, L, nm.ctypes.data, mems.ctypes.data, len(mems),
                             C.byref(total), None, C.byref(st))
    assert rc == 0 and total.value == len(want_mems) and st.bases == copies * tnb
    assert (nm == want_n).all()
    assert (mems == want_mems).all()
    nm[:] = 0
    rc = lib().movi_mem_host(gpu._h, bases.ctypes.data, offs.ctypes.data, n, L, nm.ctypes.data, mems.ctypes.data, len(mems) - 1,
                             C.byref(total), None, C.byref(st))
    assert rc == -1 and total.value == len(want_mems) and (nm == want_n).all()
    assert ("%d MEMs found, mems_cap is %d" % (len(want_mems), len(mems) - 1)).encode() in lib().movi_last_error()
    gpu.close()


def _mem_lines(ids, reads, oracle, code_of, L):
    exp, _ = mem_ref.restate(oracle, reads, code_of, (L,))
    return b"".join(b"%s\t%d\t%d\t%d\n" % (i, s, e, c & 0xFFFF) for i, ms in zip(ids, exp[L]) for s, e, c in ms)


def test_cli(texts, tmp_path):
    import movi_amd
    from oracle.oracle import Oracle
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(texts[False][6])
    o = Oracle(texts[False][6])
    code_of = movi_amd.parse_index_image(texts[False][6])[0].code_of
    ref = _ref()
    fq = os.path.join(GOLDEN, "sample.fastq")
    fa = tmp_path / "n.fa"
    seqs = [ref[100:300], ref[500:560] + b"NNN" + ref[600:700], b"ACGTN" * 10, ref[900:1000].lower() + ref[1000:1100]]
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    # (sample.fastq's reads are not drawn from ref.fasta: no MEM reaches 20 bases, 35 reach 12)
    for path, L in ((fq, 20), (fq, 12), (str(fa), 20)):
        recs = read_fastx(path)
        ids, reads = [i.encode() if isinstance(i, str) else i for i, _ in recs], [s for _, s in recs]
        want = _mem_lines(ids, reads, o, code_of, L)
        assert want or (path == fq and L == 20)
        out = tmp_path / "o"
        base = ["query", "-i", str(idx), "--mem", "--ftab-k", "12", "-l", str(L)]
        r = subprocess.run([MOVI] + base + ["-r", path, "-o", str(out)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.mems").read_bytes() == want
        r = subprocess.run([MOVI] + base + ["-r", path, "--stdout"], capture_output=True)
        assert r.returncode == 0 and r.stdout == want, r.stderr
    # --reverse and --ignore-illegal-chars 1 are applied before the search
    recs = read_fastx(str(fa))
    ids = [i.encode() if isinstance(i, str) else i for i, _ in recs]
    rev = [s[::-1] for _, s in recs]
    r = subprocess.run([MOVI] + base + ["-r", str(fa), "--stdout", "--reverse"], capture_output=True)
    assert r.returncode == 0 and r.stdout == _mem_lines(ids, rev, o, code_of, 20), r.stderr
    subst = [bytes(c if code_of[c] != 0xFF else ord("A") for c in s) for _, s in recs]
    r = subprocess.run([MOVI] + base + ["-r", str(fa), "--stdout", "--ignore-illegal-chars", "1"], capture_output=True)
    assert r.returncode == 0 and r.stdout == _mem_lines(ids, subst, o, code_of, 20), r.stderr
    r = subprocess.run([MOVI] + base + ["-r", str(fa), "--no-output", "-o", str(tmp_path / "none")], capture_output=True)
    assert r.returncode == 0 and not (tmp_path / "none.mems").exists()
    o.close()


def _cli_setup(texts, tmp_path, seqs):
    import movi_amd
    from oracle.oracle import Oracle
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(texts[False][6])
    fa = tmp_path / "q.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    return idx, fa, Oracle(texts[False][6]), movi_amd.parse_index_image(texts[False][6])[0].code_of


def test_cli_shards(texts, tmp_path):
    """--gpus 3 shards each chunk of reads over three handles (MOVI_SHARE_GPU=1: every logical GPU is device 0) and puts the shards' MEMs
    back in read order: the same bytes as one GPU, from the restatement."""
    ref = _ref()
    seqs = [ref[100:300], ref[500:560] + b"NNN" + ref[600:700], b"ACGTN" * 10, ref[900:1000].lower() + ref[1000:1100], ref[50:60],
            ref[1200:1300] + b"T" + ref[1301:1500], ref[3000:3400]]
    idx, fa, o, code_of = _cli_setup(texts, tmp_path, seqs)
    want = _mem_lines([b"r%d" % i for i in range(len(seqs))], seqs, o, code_of, 20)
    assert want.count(b"\n") >= 5                                 # five of the reads hold 60 bases of the text or more: every shard has MEMs
    for extra, env in (([], {}), (["--gpus", "3"], {"MOVI_SHARE_GPU": "1"})):
        r = subprocess.run([MOVI, "query", "-i", str(idx), "--mem", "--ftab-k", "12", "-l", "20", "-r", str(fa), "--stdout"] + extra,
                           capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == want, (extra, r.stderr)
    o.close()


def test_cli_more_mems_than_the_first_guess(texts, tmp_path):
    """The command gives a shard's MEMs room for 8 per read and one per 16 bases first, and calls again with room for exactly what the
    first call found.  Six random reads of 200 bases at -l 4 hold 675 MEMs against a first guess of 6 * 8 + 1200 / 16 = 123 (two shards:
    3 * 8 + 600 / 16 = 61 each), so the bytes below come from the second call."""
    rng = np.random.default_rng(7)
    seqs = [bytes(rng.choice(list(b"ACGT"), 200).astype(np.uint8)) for _ in range(6)]
    idx, fa, o, code_of = _cli_setup(texts, tmp_path, seqs)
    exp, _ = mem_ref.restate(o, seqs, code_of, (4,))
    per_read = [len(ms) for ms in exp[4]]
    assert sum(per_read) > 6 * 8 + 1200 // 16 and min(sum(per_read[:3]), sum(per_read[3:])) > 3 * 8 + 600 // 16
    want = _mem_lines([b"r%d" % i for i in range(6)], seqs, o, code_of, 4)
    assert want.count(b"\n") == sum(per_read)
    for extra, env in (([], {}), (["--gpus", "2"], {"MOVI_SHARE_GPU": "1"})):
        r = subprocess.run([MOVI, "query", "-i", str(idx), "--mem", "--ftab-k", "12", "-l", "4", "-r", str(fa), "--stdout"] + extra,
                           capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == want, (extra, r.stderr)
    o.close()


def test_count_beyond_u16(built_lib, tmp_path):
    """A MEM that occurs more than 65535 times: the ABI returns occ, the file prints occ mod 2^16 (mem_t::count is a uint16_t)."""
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle
    rng = np.random.default_rng(99)
    g = bytes(rng.choice(list(b"ACGT"), 300).astype(np.uint8))
    seqs = [g + b"A" * 70000 + g[::-1]]
    img = B.build_index_from_seqs(seqs, 6)
    gpu = movi_amd.MoveIndex.from_image(img)
    o = Oracle(img)
    reads = [b"A", b"AA", b"CAAAT"]
    exp, _ = mem_ref.restate(o, reads, gpu.desc.code_of, (1,))
    got = gpu.query_mems(reads, 1)
    assert got == exp[1] and got[0][0][2] > 65535
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(img)
    fa = tmp_path / "a.fa"
    fa.write_bytes(b"".join(b">q%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", str(fa), "--mem", "--ftab-k", "12", "-l", "1", "--stdout"],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    want = b"".join(b"q%d\t%d\t%d\t%d\n" % (i, s, e, c % 65536) for i, ms in enumerate(got) for s, e, c in ms)
    assert r.stdout == want
    o.close()
    gpu.close()
