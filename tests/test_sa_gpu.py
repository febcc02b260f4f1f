"""GPU suite (-m gpu): locate -- the sampled suffix array built on the device (movi_ssa_build), ssa.movi, movi_locate_device,
movi_sa_entries_host / _device and `movi build-SA` / `movi query --sa-entries` -- against tests/sa_ref.py: the suffix array of the text
and the restatement of query_pml's positions, which is itself held to the oracle's PMLs."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_fastx
from test_gpu_parity import mutated_reads, pack
from test_kernel_coverage_gpu import read_log, take_log
import sa_ref

pytestmark = pytest.mark.gpu

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
MODES = (6, 8, 7, 3, 2, 5)


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


@pytest.fixture(scope="module")
def texts(built_lib):
    """{separators: (SA, {mode: (build_rows fields, index image)})} over ref.fasta."""
    from oracle import build_index as B
    out = {}
    for sep in (False, True):
        t = B.clean_text([_ref()], separators=sep)
        bwt, thr = B.bwt_and_thresholds(t)
        SA = B.suffix_array(t)
        per = {}
        for mode in MODES:
            f = B.build_rows(bwt, thr, mode)
            per[mode] = (f, B.serialize(f))
        out[sep] = (SA, per)
    return out


def rates_of(n):
    return (1, 2, 7, 100, n + 13)


def check_locate_everything(gpu, f, SA, rate, tmp_path):
    """build_ssa at `rate`: ssa(), the saved file and locate of all n positions against sa_ref."""
    n = f["n"]
    gpu.build_ssa(rate)
    got_rate, got = gpu.ssa()
    assert got_rate == rate and (got == sa_ref.samples(SA, rate)).all(), rate
    path = str(tmp_path / ("ssa_%d_%d.movi" % (f["mode"], rate)))
    gpu.save_ssa(path)
    assert open(path, "rb").read() == sa_ref.ssa_bytes(f, SA, rate) and not os.path.exists(path + ".tmp"), rate
    rows, offs = sa_ref.all_positions(f)
    want = sa_ref.entries(SA, rate)
    loc = gpu.locate(rows, offs)
    assert (loc == want).all(), rate
    assert gpu.last_launch()["kernel"].startswith("locate_kernel<%d, " % (3 if f["mode"] in (3, 2) else 6))
    return bool((want >= n).any())                           # some walks passed text position 0 and report entry + n


@pytest.mark.parametrize("sep,mode", [(sep, m) for sep in (False, True) for m in MODES])
def test_exhaustive_locate(texts, tmp_path, sep, mode):
    import movi_amd
    SA, per = texts[sep]
    f, img = per[mode]
    gpu = movi_amd.MoveIndex.from_image(img)
    derived0 = gpu.info("derived_bytes")
    wraps = {}
    for rate in rates_of(f["n"]):
        wraps[rate] = check_locate_everything(gpu, f, SA, rate, tmp_path)
        assert gpu.info("locate_bytes") == f["r"] * 16 + (f["n"] // rate + 1) * 8
        assert gpu.info("derived_bytes") == derived0 + gpu.info("locate_bytes")
    # rate 1 samples everything, so no walk passes text position 0. A rate beyond n samples only BWT position 0 (value n - 1), so every
    # walk but the one that starts there does. In between, the walks from below the lowest sample do.
    assert not wraps[1] and wraps[f["n"] + 13] and (wraps[2] or wraps[7] or wraps[100])
    assert gpu.last_stats().errors == 0
    gpu.close()


def test_multi_genome_text(built_lib, tmp_path):
    """The 8-genome text of test_mem_gpu.py::test_text_not_closed_under_rc.
    (Independent genomes: repetitive texts -- a pangenome, long runs, tandem repeats -- are in tests/test_odd_texts_gpu.py.)"""
    import movi_amd
    from oracle import build_index as B
    rng = np.random.default_rng(8181)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(rng.integers(500, 3000))).astype(np.uint8)) for _ in range(8)]
    f, SA = sa_ref.text_fields(seqs, 6)
    gpu = movi_amd.MoveIndex.from_image(B.serialize(f))
    check_locate_everything(gpu, f, SA, 100, tmp_path)
    gpu.close()


def _reads():
    ref = _ref()
    fq = [s for _, s in read_fastx(os.path.join(GOLDEN, "sample.fastq"))]
    return fq[:100] + mutated_reads(np.random.default_rng(616), ref, 190, 1, 300) + [b"", ref[100:101], b"N" * 40, ref[1000:6000]]


@pytest.fixture(scope="module")
def read_cases(texts):
    """{(sep, mode): (reads, expected entries per read at rate 100, oracle PMLs per read)}"""
    from oracle.oracle import Oracle
    reads = _reads()
    out = {}
    for sep in (False, True):
        SA, per = texts[sep]
        for mode in (6, 8, 7):
            f, img = per[mode]
            o = Oracle(img)
            out[(sep, mode)] = (reads, sa_ref.read_entries(f, o, SA, 100, reads), [np.asarray(o.pml(r)) for r in reads])
            o.close()
    return out


def device_entries(gpu, reads, order=None, want_pml=True):
    import torch
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(bases)).to(dev)
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dsa = torch.full((nb,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    dp = torch.full((nb,), 0x5A5A, dtype=torch.int16, device=dev)
    de = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
    dord = torch.from_numpy(np.asarray(order, np.int32)).to(dev) if order is not None else None
    gpu.sa_entries_device(db.data_ptr(), do.data_ptr(), n, nb, dsa.data_ptr(), d_pml=dp.data_ptr() if want_pml else 0, d_err=de.data_ptr(),
                          d_order=dord.data_ptr() if dord is not None else 0)
    torch.cuda.synchronize()
    return dsa.cpu().numpy().view(np.uint64), dp.cpu().numpy().view(np.uint16), de.cpu().numpy(), offs


@pytest.mark.parametrize("sep,mode", [(False, 6), (False, 8), (False, 7), (True, 6), (True, 8), (True, 7)])
def test_per_base_entries(texts, read_cases, sep, mode):
    import movi_amd
    reads, want, pmls = read_cases[(sep, mode)]
    gpu = movi_amd.MoveIndex.from_image(texts[sep][1][mode][1])
    gpu.build_ssa(100)
    got = gpu.query_sa_entries(reads)
    assert all((g == w).all() for g, w in zip(got, want))
    bases, offs = pack(reads)
    sa, pml, st = gpu.query_sa_entries_packed(bases, offs)
    wsa, wpml = np.concatenate(want), np.concatenate(pmls).astype(np.uint16)
    assert (sa == wsa).all() and (pml == wpml).all() and st.errors == 0 and st.bases == len(bases)
    dsa, dpml, derr, _ = device_entries(gpu, reads)
    assert (dsa == wsa).all() and (dpml == wpml).all() and (derr == 0).all()
    perm = np.random.default_rng(3).permutation(len(reads))
    dsa, _, derr, _ = device_entries(gpu, reads, order=perm, want_pml=False)
    assert (dsa == wsa).all() and (derr == 0).all()
    assert gpu.last_launch()["kernel"].startswith("locate_kernel<6, ")
    gpu.close()


def built_sa_kernels():
    import movi_amd
    data = open(movi_amd.lib_path(), "rb").read()
    names, pos = set(), 0
    tmp = "/tmp/movi_sacov_co_%d.o" % os.getpid()
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
                mangled = [ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and ("locate_kernel" in ln or "sa_pos_kernel" in ln)]
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


def test_both_index_widths(texts, read_cases, tmp_path):
    import movi_amd
    built = built_sa_kernels()
    assert len(built) == 6, sorted(built)
    SA, per = texts[False]
    reads, want, _ = read_cases[(False, 6)]
    take_log()
    for mode in (6, 3):
        f, img = per[mode]
        for idx64 in (0, 1):
            T = "unsigned long" if idx64 else "unsigned int"
            gpu = movi_amd.MoveIndex.from_image(img)
            gpu.set_option("idx64", idx64)
            check_locate_everything(gpu, f, SA, 7, tmp_path)
            li = gpu.last_launch()
            assert li["idx64"] == idx64 and li["kernel"] == "locate_kernel<%d, %s>" % (mode, T)
            if mode == 6:
                gpu.build_ssa(100)
                got = gpu.query_sa_entries(reads)
                assert all((g == w).all() for g, w in zip(got, want))
            gpu.close()
    seen = read_log()
    assert {k for k in seen if "locate_kernel" in k or "sa_pos_kernel" in k} == built


def test_capture_without_warmup(texts, read_cases):
    import torch
    import movi_amd
    reads, want, pmls = read_cases[(True, 6)]
    gpu = movi_amd.MoveIndex.from_image(texts[True][1][6][1])
    gpu.build_ssa(100)
    gpu.prepare(gpu.PREPARE_SA)
    scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(bases)).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dsa = torch.full((nb,), -7, dtype=torch.int64, device=dev)
    dp = torch.zeros(nb, dtype=torch.int16, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            gpu.sa_entries_device(db.data_ptr(), do.data_ptr(), n, nb, dsa.data_ptr(), d_pml=dp.data_ptr(), stream=s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert (dsa.cpu().numpy() == -7).all()                            # nothing ran at capture
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    for _ in range(2):
        dsa.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert (dsa.cpu().numpy().view(np.uint64) == np.concatenate(want)).all()
        assert (dp.cpu().numpy().view(np.uint16) == np.concatenate(pmls).astype(np.uint16)).all()
    del g
    gpu.close()


def test_host_two_chunks(texts, read_cases):
    """movi_sa_entries_host on just over 2^28 bases -- a tile of short reads repeated -- takes two chunks of the host loop."""
    import movi_amd
    allreads, allwant, _ = read_cases[(False, 6)]
    keep = [i for i, r in enumerate(allreads) if 0 < len(r) <= 300][:250]
    reads, want = [allreads[i] for i in keep], np.concatenate([allwant[i] for i in keep])
    tb, toffs = pack(reads)
    tnb = int(toffs[-1])
    copies = (1 << 28) // tnb + 2
    bases = np.tile(np.asarray(tb), copies)
    offs = np.concatenate([(toffs[:-1].astype(np.uint64) + np.uint64(c * tnb)) for c in range(copies)] + [np.array([copies * tnb], np.uint64)])
    assert (1 << 28) + tnb < copies * tnb <= (1 << 28) + 2 * tnb
    assert np.searchsorted(offs, 1 << 28, "right") - 1 >= 1 << 18          # the first chunk ends at 2^28 bases
    gpu = movi_amd.MoveIndex.from_image(texts[False][1][6][1])
    gpu.build_ssa(100)
    sa, _, st = gpu.query_sa_entries_packed(bases, offs, want_pml=False)
    assert st.bases == copies * tnb and st.errors == 0
    assert (sa.reshape(copies, tnb) == want[None, :]).all()
    gpu.close()


def test_load_round_trip_and_refusals(texts, read_cases, tmp_path):
    import movi_amd
    SA, per = texts[False]
    f, img = per[6]
    reads, want, _ = read_cases[(False, 6)]
    gpu = movi_amd.MoveIndex.from_image(img)
    bases, offs = pack(reads)
    # no sampled suffix array attached: MOVI_ERR_ARG, the message names build-SA
    for call in (lambda: gpu.query_sa_entries(reads), lambda: gpu.locate([0], [0]), lambda: gpu.ssa(), lambda: gpu.prepare(gpu.PREPARE_SA),
                 lambda: device_entries(gpu, reads)):
        with pytest.raises(movi_amd.MoviError) as e:
            call()
        assert e.value.code == -1 and "build-SA" in str(e.value)
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.load_ssa(str(tmp_path / "missing.movi"))
    assert e.value.code == -3 and "build-SA" in str(e.value)
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.build_ssa((1 << 24) + 1)
    assert e.value.code == -1
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.build_ssa(0)
    assert e.value.code == -1
    # round trip through the expected bytes (not through a file this engine wrote)
    good = tmp_path / "ssa.movi"
    good.write_bytes(sa_ref.ssa_bytes(f, SA, 100))
    gpu.load_ssa(str(good))
    assert gpu.ssa()[0] == 100 and (gpu.ssa()[1] == sa_ref.samples(SA, 100)).all()
    got = gpu.query_sa_entries(reads)
    assert all((g == w).all() for g, w in zip(got, want))
    # a wrong trailing r, a truncated file
    raw = bytearray(good.read_bytes())
    pos_r = 16 + 8 * (f["n"] // 100 + 1)
    raw[pos_r:pos_r + 8] = struct.pack("<Q", f["r"] + 1)
    (tmp_path / "bad_r.movi").write_bytes(bytes(raw))
    (tmp_path / "short.movi").write_bytes(good.read_bytes()[:100])
    (tmp_path / "no_all_p.movi").write_bytes(good.read_bytes()[:pos_r + 8])   # ends right after the trailing r
    for name in ("bad_r.movi", "short.movi", "no_all_p.movi"):
        with pytest.raises(movi_amd.MoviError) as e:
            gpu.load_ssa(str(tmp_path / name))
        assert e.value.code == -2, name
    assert all((g == w).all() for g, w in zip(gpu.query_sa_entries(reads), want))      # the attached array is still the good one
    # positions that are not positions of the table
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.locate([f["r"]], [0])
    assert e.value.code == -6
    gpu.close()
    # a corrupted row table (the corruption of test_mem_gpu.py::test_read_order_errors_and_corrupt_rows): MOVI_ERR_INVARIANT, and the calls return
    bad_img = bytearray(img)
    desc, _, off, _ = movi_amd.parse_index_image(bytes(bad_img))
    rows = np.frombuffer(bad_img, np.uint8, count=desc.r * 8, offset=off).reshape(-1, 8).copy()
    rng = np.random.default_rng(8600)
    rows[rng.choice(desc.r, desc.r // 4, replace=False), 0:4] = 0xFF
    bad_img[off: off + rows.size] = rows.tobytes()
    bad = movi_amd.MoveIndex.from_image(bytes(bad_img))
    with pytest.raises(movi_amd.MoviError) as e:
        bad.build_ssa(100)
    assert e.value.code == -6
    with pytest.raises(movi_amd.MoviError) as e:
        bad.ssa()
    assert e.value.code == -1                                               # nothing stays attached
    bad.load_ssa(str(good))
    sa, pml, st, err, rc = bad.query_sa_entries_packed(bases, offs, want_err=True)
    assert rc == -6 and st.errors > 50 and (err != 0).sum() > 0 and set(np.unique(err[err != 0])) <= {1, 2}
    for i in np.nonzero(err)[0]:
        assert (sa[int(offs[i]):int(offs[i + 1])] == np.uint64(bad.POS_NONE)).all()
    bad.close()


def pml_file_ids(raw):
    """The read ids of a PML .bpf file in record order: a 12-byte header (byte 7 = bits per value), then per read u16 id length, the id,
    u64 count, count values."""
    width, pos, ids = raw[7] // 8, 12, []
    while pos < len(raw):
        idl = struct.unpack_from("<H", raw, pos)[0]
        ids.append(raw[pos + 2: pos + 2 + idl])
        cnt = struct.unpack_from("<Q", raw, pos + 2 + idl)[0]
        pos += 2 + idl + 8 + cnt * width
    assert pos == len(raw)
    return ids


def test_cli(texts, tmp_path):
    from oracle.oracle import Oracle
    SA, per = texts[False]
    f, img = per[6]
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(img)
    ref = _ref()
    fq = os.path.join(GOLDEN, "sample.fastq")
    fa = tmp_path / "n.fa"
    seqs = [ref[100:300], ref[500:560] + b"NNN" + ref[600:700], b"ACGTN" * 10, ref[900:1000].lower() + ref[1000:1100]]
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    # --sa-entries before build-SA: the missing ssa.movi is named
    r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", fq, "--sa-entries", "-o", str(tmp_path / "x")], capture_output=True)
    assert r.returncode == 1 and b"build-SA" in r.stderr
    o = Oracle(img)
    for rate, extra in ((100, []), (7, ["--sample-rate", "7"])):
        r = subprocess.run([MOVI, "build-SA", "-i", str(idx)] + extra, capture_output=True)
        assert r.returncode == 0, r.stderr
        assert (idx / "ssa.movi").read_bytes() == sa_ref.ssa_bytes(f, SA, rate)
        for path in (fq, str(fa)):
            recs = read_fastx(path)
            ids, reads = [i.encode() if isinstance(i, str) else i for i, _ in recs], [s for _, s in recs]
            per_read = sa_ref.read_entries(f, o, SA, rate, reads)
            want = sa_ref.sa_entries_file(ids, per_read)
            plain, out = tmp_path / "plain", tmp_path / "o"
            r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", path, "-o", str(plain), "-n"], capture_output=True)
            assert r.returncode == 0, r.stderr
            r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", path, "-o", str(out), "-n", "--sa-entries"], capture_output=True)
            assert r.returncode == 0, r.stderr
            assert (tmp_path / "o.pml.sa_entries.bpf").read_bytes() == want
            assert (tmp_path / "o.pml.bpf").read_bytes() == (tmp_path / "plain.pml.bpf").read_bytes()
            # the strand scheduler's record order (no -n): the same records in the PML file's order
            r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", path, "-o", str(tmp_path / "p"), "--sa-entries"], capture_output=True)
            assert r.returncode == 0, r.stderr
            r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", path, "-o", str(tmp_path / "pp")], capture_output=True)
            assert (tmp_path / "p.pml.bpf").read_bytes() == (tmp_path / "pp.pml.bpf").read_bytes()
            order = pml_file_ids((tmp_path / "p.pml.bpf").read_bytes())
            assert sorted(order) == sorted(ids) and len(set(ids)) == len(ids)
            by_id = dict(zip(ids, per_read))
            assert (tmp_path / "p.pml.sa_entries.bpf").read_bytes() == sa_ref.sa_entries_file(order, [by_id[i] for i in order])
            r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", path, "-o", str(tmp_path / "none"), "--sa-entries", "--no-output"], capture_output=True)
            assert r.returncode == 0 and not (tmp_path / "none.pml.sa_entries.bpf").exists() and not (tmp_path / "none.pml.bpf").exists()
    o.close()
