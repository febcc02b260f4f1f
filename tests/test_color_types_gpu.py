"""GPU suite (-m gpu): Movi Color on every index type it accepts, against tests/color_ref.py (the references themselves are held to a
brute force in tests/test_color_types_cpu.py, which also defines the texts):

  * the builder on the six types with and without separators -- color_walk_kernel<6, ...> on the thresholds types and on `sampled`,
    <3, ...> on `regular` and `blocked`, both index widths --, and with document offsets that do not end at n - 1;
  * the scorer on the three thresholds types with and without separators, min_len 0 / 1 / 5 / 255, through the host entry, the device
    entry with the caller's counters and with the handle's scratch in chunks;
  * a match of 100 000 bases: sum_ml wraps, the PMLs clamp;
  * reads that hit one of the reference's throws on a table with corrupt rows, and the builder on that table;
  * every colour kernel in the shipped code object is launched here;
  * `movi build --type blocked-thresholds --separators --color`, `movi color` on a `regular` index."""
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT
from test_color_gpu import check_records, device_call
from test_gpu_parity import pack
from test_kernel_coverage_gpu import read_log, take_log
from test_color_types_cpu import (LONG1_LEN, LONG1_SUM, MODES, THRESHOLD_MODES, corrupt_image, corrupt_reads, expected_scores,
                                  expected_tables, long1, long1_reads, long1_scores, odd_lasts, odd_offsets, reads_of, small4, small4_seqs,
                                  text_of)
import color_ref
import sa_ref

pytestmark = pytest.mark.gpu

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
NONE = color_ref.NONE
# The resident layout a type is expanded to, which is the builder's instantiation: `regular` keeps its 12-bit lengths and `blocked` is
# expanded to them (layout 3); `sampled`, like the three thresholds types, is expanded to regular-thresholds rows (layout 6, all threshold
# bits zero) -- as tests/test_sa_gpu.py pins for locate_kernel.
WALK = {6: 6, 8: 6, 7: 6, 5: 6, 3: 3, 2: 3}
WIDTH = ("unsigned int", "unsigned long")
SEEN = set()                                                    # the colour kernels this file's runs launched (movi_launch_log)


@pytest.fixture(scope="module", autouse=True)
def launch_log():
    take_log()
    yield


def note_launches():
    SEEN.update(k for k in read_log() if k.startswith("color_"))


def check_tables(gpu, want, tmp_path, tag):
    flat, inds, ns, taxa = want
    gflat, ginds, gns, gtaxa = gpu.colors()
    assert gns == ns and list(gtaxa) == taxa, tag
    assert len(gflat) == len(flat) and (gflat == flat).all() and (ginds == inds).all(), tag
    path = str(tmp_path / ("doc_sets_%s.bin" % tag))
    gpu.save_colors(path)
    assert open(path, "rb").read() == color_ref.flat_file(flat, inds) and not os.path.exists(path + ".tmp")
    assert gpu.info("color_bytes") == 2 * len(flat) + 8 * len(inds)


def refuses_for_thresholds(gpu):
    """Both entries of the scorer on a type without thresholds: MOVI_ERR_ARG, before anything is read."""
    import movi_amd
    for call in (lambda: gpu.multi_classify([b"ACGT"]), lambda: gpu.multi_classify_device(0, 0, 1, 4, 1, 0)):
        with pytest.raises(movi_amd.MoviError) as e:
            call()
        assert e.value.code == -1 and "needs thresholds" in str(e.value)


BUILDER_CASES = [("small4", m, s) for m in MODES for s in (False, True)] + [("poly", 6, True), ("poly", 8, True), ("poly", 3, True)]


@pytest.mark.parametrize("name,mode,sep", BUILDER_CASES)
def test_builder_on_every_type(name, mode, sep, tmp_path):
    import movi_amd
    _, f, img, _, offsets, doc_ids = text_of(name, mode, sep)
    want = expected_tables(name, mode, sep)
    assert len(want[1]) == f["r"] and f["sep"] == int(sep)
    # none attached: a sampled suffix array is built at the default rate and stays
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    assert gpu.ssa()[0] == 100 and gpu.info("color_chunks") == 1
    assert gpu.last_launch()["kernel"] == "color_walk_kernel<%d, unsigned int>" % WALK[mode]
    check_tables(gpu, want, tmp_path, "none")
    if mode not in THRESHOLD_MODES:
        refuses_for_thresholds(gpu)
        check_tables(gpu, want, tmp_path, "still")               # the tables stay attached
    if name == "small4" and mode == 6:                           # a last document that ends early / beyond the text
        for last in odd_lasts(f["n"]):
            gpu.build_colors(odd_offsets(offsets, last), doc_ids)
            check_tables(gpu, expected_tables(name, mode, sep, last), tmp_path, "last%d" % last)
    gpu.close()
    # rate 7 attached, the chunk budget forced small: several chunks, the same tables; 64-bit row indexes
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_ssa(7)
    gpu.set_option("color_chunk_keys", max(64, f["n"] // 3))
    gpu.set_option("idx64", 1)
    gpu.build_colors(offsets, doc_ids)
    assert gpu.ssa()[0] == 7 and gpu.info("color_chunks") >= 2
    assert gpu.last_launch()["kernel"] == "color_walk_kernel<%d, unsigned long>" % WALK[mode] and gpu.last_launch()["idx64"] == 1
    check_tables(gpu, want, tmp_path, "rate7")
    if mode not in THRESHOLD_MODES:
        refuses_for_thresholds(gpu)
    gpu.close()
    note_launches()


SCORING_CASES = [("small4", m, s) for m in THRESHOLD_MODES for s in (False, True)] + [("poly", 6, True)]


@pytest.mark.parametrize("name,mode,sep", SCORING_CASES)
def test_scoring_on_every_thresholds_type(name, mode, sep):
    import movi_amd
    from oracle.oracle import Oracle
    _, f, img, _, offsets, doc_ids = text_of(name, mode, sep)
    reads = reads_of(name, sep)
    ns = expected_tables(name, mode, sep)[2]
    # what the reads must hold, by the restatement, before the device runs: no best document; a runner-up; a lead that changes hands
    one = expected_scores(name, mode, sep, 1)
    assert any(w[0] == NONE for w, _ in one) and any(w[1] != NONE for w, _ in one) and any(ch > 0 for _, ch in one)
    assert len(reads) > 128 and {0, 1, 2, 63, 64, 65, 300} <= {len(r) for r in reads}
    assert not sep or sum(b"%" in r for r in reads) >= 2
    o = Oracle(img)
    pml = np.concatenate([np.asarray(o.pml(r)) for r in reads]).astype(np.uint16)
    o.close()
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    bases, offs = pack(reads)
    for min_len in (0, 1, 5, 255):
        want = [w for w, _ in expected_scores(name, mode, sep, min_len)]
        out, counts, gp, st = gpu.multi_classify_packed(bases, offs, min_len, want_pml=True)
        check_records(out, counts, want)
        assert (gp == pml).all() and st.errors == 0 and st.bases == len(bases), min_len
        out, counts, gp, err = device_call(gpu, reads, min_len, True, ns)
        check_records(out, counts, want)
        assert (gp == pml).all() and (err == 0).all(), min_len
    assert gpu.last_launch()["kernel"] == "color_kernel<6, unsigned int>"
    # the counters in the handle's scratch, a few reads per chunk; a permuted read order; 64-bit row indexes
    want = [w for w, _ in one]
    gpu.set_option("color_scratch_bytes", 4 * ns * 7)
    gpu.set_option("release_scratch", 1)
    perm = np.random.default_rng(3).permutation(len(reads))
    out, _, gp, err = device_call(gpu, reads, 1, False, ns, order=perm)
    check_records(out, None, want)
    assert (gp == pml).all() and (err == 0).all()
    assert gpu.info("device_scratch_bytes") <= 4 * ns * 7 * 9 // 8 + 64
    gpu.set_option("idx64", 1)
    out, counts, gp, st = gpu.multi_classify_packed(bases, offs, 1, want_pml=True)
    check_records(out, counts, want)
    assert (gp == pml).all() and gpu.last_launch()["kernel"] == "color_kernel<6, unsigned long>"
    gpu.close()
    note_launches()


def test_long_match_wraps_the_sum_and_clamps_the_pml():
    """long1's 100 000-base document, read as a whole beside ~70 short reads: the match length passes 65535 (the PML written is
    clamped, the length carried is not) and the sum of the match lengths passes 2^32 (a uint32_t there too).
    One lane walks the 100 000 bases base by base while its wavefront's other lanes have long finished."""
    import movi_amd
    _, f, img, _, offsets, doc_ids = long1()
    reads, at = long1_reads()
    ns = expected_tables("long1", 6, False)[2]
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    bases, offs = pack(reads)
    b0 = int(offs[at])
    clamped = np.minimum(np.arange(1, LONG1_LEN + 1), 65535).astype(np.uint16)
    for min_len in (1, 255):
        want = long1_scores(min_len)
        assert want[at][3] == LONG1_SUM
        t0 = time.perf_counter()
        out, counts, gp, st = gpu.multi_classify_packed(bases, offs, min_len, want_pml=True)
        print("long1: movi_multi_classify_host, min_len %d: %.3f s" % (min_len, time.perf_counter() - t0))
        check_records(out, counts, want)
        assert int(out[at]["sum_ml"]) == LONG1_SUM and int(out[at]["colors_count"]) == LONG1_LEN - min_len
        assert (gp[b0: b0 + LONG1_LEN] == clamped).all() and int(gp[b0 + LONG1_LEN - 1]) == 65535 and st.errors == 0
    want = long1_scores(1)
    out, counts, gp, err = device_call(gpu, reads, 1, True, ns)
    check_records(out, counts, want)
    assert (gp[b0: b0 + LONG1_LEN] == clamped).all() and (err == 0).all()
    gpu.close()
    note_launches()


def test_failed_reads_and_the_builder_on_corrupt_rows(tmp_path):
    """A table in which every 97th destination id is beyond r (the corruption of tests/test_deep_rows_gpu.py): a read whose walk takes
    an LF step from such a row hits LF_move's throw (src/move_structure.cpp:63-65).  The set of failing reads and their codes are the
    plain PML walk's on the same handle; a failed read reports no document, zero counters, all-zero PMLs; every other read walks the
    rows of the intact table and scores as there.  The builder refuses the table."""
    import movi_amd
    from oracle.oracle import Oracle, OracleError
    _, f, img, _, offsets, doc_ids = small4(6, False)
    flat, inds, ns, _ = expected_tables("small4", 6, False)
    good = movi_amd.MoveIndex.from_image(img)
    good.build_colors(offsets, doc_ids)
    path = str(tmp_path / "doc_sets_flat.bin")
    good.save_colors(path)
    bad_img = corrupt_image(img)
    bad = movi_amd.MoveIndex.from_image(bad_img)
    bad.load_colors(path, ns)
    reads = corrupt_reads()
    bases, offs = pack(reads)
    n = len(reads)
    # the reference: the plain PML walk on the same handle
    bad.set_option("ahead_rows", 0)
    epml, est, eerr, erc = bad.query_pml_packed(bases, offs, want_err=True)
    failed = np.asarray(eerr) != 0
    assert erc == -6 and est.errors == int(failed.sum())
    assert not epml[np.repeat(failed, [len(r) for r in reads])].any()           # (a failed read: all-zero PMLs there too)
    assert n // 10 <= int(failed.sum()) <= n - n // 10, int(failed.sum())       # both populations: at least a tenth of the batch
    # the premise, on the CPU: a walk that takes no LF step from a corrupted row reads the same rows -- the same PMLs on both images
    o_good, o_bad = Oracle(img), Oracle(bad_img)
    codes = sa_ref.code_table(f)
    want = []
    for rd, fl in zip(reads, failed):
        if fl:
            with pytest.raises(OracleError):
                o_bad.pml(rd)
            want.append((NONE, NONE, 0, 0, [0] * ns))
        else:
            assert (o_bad.pml(rd) == o_good.pml(rd)).all()
            want.append(color_ref.score(f, o_good, rd, flat, inds, ns, 1, codes))
    wpml = np.concatenate([np.zeros(len(rd), np.uint16) if fl else np.asarray(o_good.pml(rd)) for rd, fl in zip(reads, failed)])
    o_good.close()
    o_bad.close()
    assert any(w[0] != NONE for w in want) and any(w[1] != NONE for w in want)

    def check(out, counts, gp, err):
        check_records(out, counts, want)
        assert list(err) == list(eerr)
        assert gp is None or ((gp == wpml).all() and (gp == epml).all())
        for o, fl in zip(out, failed):
            if fl:
                assert (int(o["best"]), int(o["second"]), int(o["best_count"]), int(o["second_count"]), int(o["colors_count"]), int(o["sum_ml"])) == (NONE, NONE, 0, 0, 0, 0)
        if counts is not None:
            assert not counts[failed].any()

    out, counts, gp, st, err, rc = bad.multi_classify_packed(bases, offs, 1, want_pml=True, want_err=True)
    assert rc == erc and st.errors == int(failed.sum())
    check(out, counts, gp, err)
    # the device entry: the caller's counter rows, pre-filled with a sentinel by device_call
    out, counts, gp, err = device_call(bad, reads, 1, True, ns)
    check(out, counts, gp, err)
    assert bad.last_stats().errors == int(failed.sum())
    # ... and the handle's scratch, five reads per chunk, in a permuted order: a failed read's zeroing stays in its own row
    bad.set_option("color_scratch_bytes", 4 * ns * 5)
    bad.set_option("release_scratch", 1)
    out, _, gp, err = device_call(bad, reads, 1, False, ns, order=np.random.default_rng(5).permutation(n))
    check(out, None, gp, err)
    # the builder on the corrupt table: MOVI_ERR_INVARIANT (from the sampled suffix array's builder or from the colour walk), never a
    # wrong table -- and no table, the loaded one included, stays attached
    with pytest.raises(movi_amd.MoviError) as e:
        bad.build_colors(offsets, doc_ids)
    assert e.value.code == -6
    with pytest.raises(movi_amd.MoviError) as e:
        bad.colors()
    assert e.value.code == -1 and "no colour tables" in str(e.value)
    bad.close()
    # a fresh intact handle in the same process builds the right tables
    fresh = movi_amd.MoveIndex.from_image(img)
    fresh.build_colors(offsets, doc_ids)
    check_tables(fresh, expected_tables("small4", 6, False), tmp_path, "fresh")
    fresh.close()
    good.close()
    note_launches()


def built_color_kernels():
    import struct
    import movi_amd
    data = open(movi_amd.lib_path(), "rb").read()
    names, pos = set(), 0
    tmp = "/tmp/movi_colcov_co_%d.o" % os.getpid()
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
                mangled = [ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and ("color_walk_kernel" in ln or "color_kernel" in ln)]
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


def test_every_colour_kernel_is_reachable(tmp_path):
    """The colour kernels in the shipped gfx950 code object are the ones the launch log names over this file's runs: 4 color_walk_kernel
    + 2 color_kernel.  (The launches below make the test stand by itself; each one is held to color_ref.)"""
    import movi_amd
    built = built_color_kernels()
    expected = {"color_walk_kernel<%d, %s>" % (k, t) for k in (6, 3) for t in WIDTH} | {"color_kernel<6, %s>" % t for t in WIDTH}
    assert built == expected, sorted(built)
    for mode in (6, 3):
        _, f, img, _, offsets, doc_ids = small4(mode, False)
        for idx64 in (0, 1):
            gpu = movi_amd.MoveIndex.from_image(img)
            gpu.set_option("idx64", idx64)
            gpu.build_colors(offsets, doc_ids)
            assert gpu.last_launch()["kernel"] == "color_walk_kernel<%d, %s>" % (mode, WIDTH[idx64])
            check_tables(gpu, expected_tables("small4", mode, False), tmp_path, "m%d_%d" % (mode, idx64))
            if mode == 6:
                reads = reads_of("small4", False)[:70]
                bases, offs = pack(reads)
                out, counts, _, st = gpu.multi_classify_packed(bases, offs, 1)
                check_records(out, counts, [w for w, _ in expected_scores("small4", 6, False, 1)][:70])
                assert gpu.last_launch()["kernel"] == "color_kernel<6, %s>" % WIDTH[idx64] and st.errors == 0
            gpu.close()
    note_launches()
    assert SEEN == built, (sorted(SEEN - built), sorted(built - SEEN))


def test_cli_on_blocked_thresholds_with_separators_and_on_regular(tmp_path):
    """`movi build --type blocked-thresholds --separators --color` and `movi query --multi-classify` on it (the documents numbered
    1 .. 4: a FASTA names no taxa); `movi color` on a `regular` index, which `--multi-classify` then refuses."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    seqs, f, img, SA, offsets, _ = small4(8, True)
    flat, inds, ns, taxa = color_ref.tables(f, SA, offsets, None)
    assert ns == 4 and taxa == [1, 2, 3, 4]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    d = tmp_path / "idx"
    r = subprocess.run([MOVI, "build", "-i", str(d), "-f", str(fa), "--type", "blocked-thresholds", "--separators", "--color"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (d / "index.movi").read_bytes() == img
    assert (d / "ref.fa.doc_offsets").read_text().split() == [str(x) for x in offsets]
    assert (d / "doc_sets_flat.bin").read_bytes() == color_ref.flat_file(flat, inds)
    reads = reads_of("small4", True)
    o = Oracle(img)
    codes = sa_ref.code_table(f)
    scores = [color_ref.score(f, o, rd, flat, inds, ns, 1, codes) for rd in reads]
    o.close()
    rf = tmp_path / "reads.fa"
    rf.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads) if len(s)))
    r = subprocess.run([MOVI, "query", "-i", str(d), "-r", str(rf), "--multi-classify", "-n", "--stdout"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split(b"\n")[:-1] == [color_ref.mls_line(b"r%d" % i, len(rd), s, taxa) for i, (rd, s) in enumerate(zip(reads, scores)) if len(rd)]
    # `movi color` on a `regular` index: the tables of its own rows; no scoring without thresholds
    _, f3, img3, _, offsets3, doc_ids3 = small4(3, False)
    flat3, inds3, _, _ = expected_tables("small4", 3, False)
    d3 = tmp_path / "regular"
    d3.mkdir()
    (d3 / "index.movi").write_bytes(img3)
    (d3 / "ref.fa.doc_offsets").write_text("".join("%d\n" % x for x in offsets3))
    (d3 / "ref.fa.doc_ids").write_text(" ".join(str(x) for x in doc_ids3) + "\n")
    r = subprocess.run([MOVI, "color", "-i", str(d3)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (d3 / "doc_sets_flat.bin").read_bytes() == color_ref.flat_file(flat3, inds3)
    r = subprocess.run([MOVI, "query", "-i", str(d3), "-r", str(rf), "--multi-classify", "-n", "--stdout"], capture_output=True)
    assert r.returncode == 1 and b"needs thresholds" in r.stderr and r.stdout == b"", r.stderr
