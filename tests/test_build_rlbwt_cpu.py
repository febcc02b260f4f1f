"""CPU suite: index.movi from a run-length BWT -- `movi rlbwt`, `tools/build_index --emit-rlbwt`, the command line and the input checks
of `movi build --preprocessed` (every one is made before any device call, so it is reported on a machine without a GPU), and the
new ABI symbol.  The builder itself: tests/test_build_rlbwt_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import build_index as B

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
TOOL = os.path.join(ROOT, "tools", "build_index")


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


@pytest.fixture(scope="module")
def tool():
    src = TOOL + ".cpp"
    if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", TOOL, src])
    return TOOL


def rle(bwt):
    """(heads, lens) of the maximal runs of a uint8 array."""
    bwt = np.asarray(bwt, np.uint8)
    starts = np.flatnonzero(np.concatenate(([True], bwt[1:] != bwt[:-1])))
    return bwt[starts], np.diff(np.concatenate((starts, [bwt.size]))).astype(np.uint64)


def five(values):
    """5-byte little-endian values, as .len and .thr_pos hold them."""
    return np.asarray(values, "<u8").view(np.uint8).reshape(-1, 8)[:, :5].tobytes()


def unfive(data):
    a = np.zeros((len(data) // 5, 8), np.uint8)
    a[:, :5] = np.frombuffer(data, np.uint8).reshape(-1, 5)
    return a.view("<u8").ravel()


def write_rlbwt(prefix, heads, lens, thr=None):
    """PREFIX.bwt.heads / .bwt.len (/ .thr_pos) the way `movi rlbwt` and pfp-thresholds leave them."""
    with open(prefix + ".bwt.heads", "wb") as f:
        f.write(np.asarray(heads, np.uint8).tobytes())
    with open(prefix + ".bwt.len", "wb") as f:
        f.write(five(lens))
    if thr is not None:
        with open(prefix + ".thr_pos", "wb") as f:
            f.write(five(thr))


def _golden_bwt():
    ref = B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]
    return B.bwt_and_thresholds(B.clean_text([ref]))[0]


RLBWT_CASES = {
    "golden": _golden_bwt,
    "single_run": lambda: np.full(37, ord("G"), np.uint8),
    "last_run_of_one": lambda: np.frombuffer(b"AAAC\x00CCGGGTTA", np.uint8),
    "run_of_70000": lambda: np.concatenate((np.frombuffer(b"CA", np.uint8), np.full(70000, ord("T"), np.uint8), np.frombuffer(b"\x00GG", np.uint8))),
}


@pytest.mark.parametrize("case", sorted(RLBWT_CASES))
def test_rlbwt_files(built_lib, tmp_path, case):
    bwt = RLBWT_CASES[case]()
    path = str(tmp_path / "ref.bwt")
    bwt.tofile(path)
    r = run(["rlbwt", "--bwt-file", path])
    assert r.returncode == 0, r.stderr
    heads, lens = rle(bwt)
    assert open(path + ".heads", "rb").read() == heads.tobytes()
    assert open(path + ".len", "rb").read() == five(lens)
    assert (unfive(five(lens)) == lens).all() and (case != "run_of_70000" or lens.max() == 70000)


def test_rlbwt_errors(built_lib, tmp_path):
    missing = str(tmp_path / "nothing.bwt")
    r = run(["rlbwt", "--bwt-file", missing])
    assert r.returncode == 1 and b"[build_rlbwt] Failed to open the BWT file: " + missing.encode() in r.stderr
    assert not os.path.exists(missing + ".heads") and not os.path.exists(missing + ".len")
    r = run(["rlbwt"])                                              # src/movi_parser.cpp:440-446
    assert r.returncode == 1 and b"Please specify one bwt file." in r.stderr
    assert b"not part of the MI355X engine" not in r.stderr


def test_emit_rlbwt(tool, tmp_path):
    rng = np.random.default_rng(77)
    base = bytes(rng.choice(list(b"ACGT"), 700).astype(np.uint8))
    seqs = [base * 3 + bytes(rng.choice(list(b"ACGT"), 400).astype(np.uint8)), base[100:600] + b"A" * 2500 + base[:50]]
    fa = tmp_path / "s.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    prefix = str(tmp_path / "ref")
    for mode in (6, 2):
        plain, emitted = str(tmp_path / ("plain%d" % mode)), str(tmp_path / ("emit%d" % mode))
        subprocess.check_call([tool, "fasta", str(fa), str(mode), plain], stderr=subprocess.DEVNULL)
        subprocess.check_call([tool, "fasta", str(fa), str(mode), emitted, "--emit-rlbwt", prefix], stderr=subprocess.DEVNULL)
        assert open(os.path.join(plain, "index.movi"), "rb").read() == open(os.path.join(emitted, "index.movi"), "rb").read()
        bwt, thr = B.bwt_and_thresholds(B.clean_text(seqs))
        heads = np.frombuffer(open(prefix + ".bwt.heads", "rb").read(), np.uint8)
        lens = unfive(open(prefix + ".bwt.len", "rb").read())
        assert (np.repeat(heads, lens.astype(np.int64)) == bwt).all() and (heads[1:] != heads[:-1]).all()
        assert (unfive(open(prefix + ".thr_pos", "rb").read()) == thr.astype(np.uint64)).all()
        for ext in (".bwt.heads", ".bwt.len", ".thr_pos"):
            os.remove(prefix + ext)
    # the option in front of the positional arguments, with separators
    out = str(tmp_path / "sep")
    subprocess.check_call([tool, "--emit-rlbwt", prefix, "fasta", str(fa), "8", out, "separators"], stderr=subprocess.DEVNULL)
    bwt, thr = B.bwt_and_thresholds(B.clean_text(seqs, separators=True))
    heads, lens = rle(bwt)
    assert open(prefix + ".bwt.heads", "rb").read() == heads.tobytes() and open(prefix + ".bwt.len", "rb").read() == five(lens)
    assert open(prefix + ".thr_pos", "rb").read() == five(thr)


# A small valid table: "$" run in the middle, thresholds within the text
HEADS = np.frombuffer(b"ACGT\x00ACGT", np.uint8)
LENS = np.array([3, 2, 4, 1, 1, 2, 5, 1, 3], np.uint64)
THR = np.array([0, 0, 0, 0, 0, 4, 6, 12, 15], np.uint64)


def _pre(tmp_path, heads=HEADS, lens=LENS, thr=THR, typ="regular-thresholds", extra=()):
    prefix = str(tmp_path / "ref")
    write_rlbwt(prefix, heads, lens, thr)
    return prefix, run(["build", "-i", str(tmp_path / "idx"), "-f", prefix, "--preprocessed", "--type", typ] + list(extra))


def test_preprocessed_input_checks(built_lib, tmp_path):
    """Return code 1, the file named, and no device touched: the same lines on a machine with and without a GPU."""
    def refused(r, path, *words):
        assert r.returncode == 1, r.stderr
        assert path.encode() in r.stderr and all(w in r.stderr for w in words), r.stderr
        assert b"Error parsing command line" not in r.stderr and not os.path.exists(str(tmp_path / "idx" / "index.movi"))
    # missing files, with the reference's words
    prefix = str(tmp_path / "ref")
    r = run(["build", "-i", str(tmp_path / "idx"), "-f", prefix, "--preprocessed"])
    refused(r, prefix + ".bwt.heads", b"[build] Failed to open the heads file: ")
    write_rlbwt(prefix, HEADS, LENS)
    os.remove(prefix + ".bwt.len")
    r = run(["build", "-i", str(tmp_path / "idx"), "-f", prefix, "--preprocessed"])
    refused(r, prefix + ".bwt.len", b"[build] Failed to open the len file: ")
    write_rlbwt(prefix, HEADS, LENS)
    r = run(["build", "-i", str(tmp_path / "idx"), "-f", prefix, "--preprocessed"])
    refused(r, prefix + ".thr_pos", b"[read_thresholds] open() file ", b" failed")
    # counts and sizes
    p, r = _pre(tmp_path, lens=LENS[:-1])
    refused(r, p + ".bwt.len", b"8 lengths", b"9 run heads")
    p = prefix                                                      # (written, then spoilt, before it is run)
    write_rlbwt(p, HEADS, LENS, THR)
    with open(p + ".bwt.len", "ab") as f:
        f.write(b"\x01\x00")
    r = run(["build", "-i", str(tmp_path / "idx"), "-f", p, "--preprocessed"])
    refused(r, p + ".bwt.len", b"not a multiple of 5")
    write_rlbwt(p, HEADS, LENS, THR)
    with open(p + ".thr_pos", "ab") as f:
        f.write(b"\x01")
    r = run(["build", "-i", str(tmp_path / "idx"), "-f", p, "--preprocessed"])
    refused(r, p + ".thr_pos", b"not a multiple of 5")
    p, r = _pre(tmp_path, thr=THR[:-2])
    refused(r, p + ".thr_pos", b"7 thresholds", b"9 run heads")
    # contents
    bad = LENS.copy(); bad[6] = 0
    p, r = _pre(tmp_path, lens=bad)
    refused(r, p + ".bwt.len", b"run 6 has length zero")
    p, r = _pre(tmp_path, heads=np.frombuffer(b"ACGTCACGT", np.uint8))
    refused(r, p + ".bwt.heads", b"terminator", b"appears 0 times")
    p, r = _pre(tmp_path, heads=np.frombuffer(b"ACGT\x00AC\x00T", np.uint8))
    refused(r, p + ".bwt.heads", b"terminator", b"appears 2 times")
    bad = LENS.copy(); bad[4] = 2
    p, r = _pre(tmp_path, lens=bad)
    refused(r, p + ".bwt.heads", b"terminator", b"appears 2 times")
    p, r = _pre(tmp_path, heads=np.frombuffer(b"ACGT\x00AAGT", np.uint8))
    refused(r, p + ".bwt.heads", b"runs 5 and 6 have the same head")
    bad = THR.copy(); bad[7] = int(LENS.sum()) + 1
    p, r = _pre(tmp_path, thr=bad)
    refused(r, p + ".thr_pos", b"threshold 7", b"greater than the text's length 22")
    p, r = _pre(tmp_path, heads=np.frombuffer(b"ACGT\x00ANGT", np.uint8))
    refused(r, p + ".bwt.heads", b"alphabet has 5 symbols: only DNA (<= 4) and separator ('%' + ACGT) indexes are supported")
    # Sound input goes on to the device step: without a GPU it ends there with the engine's message, with one it builds the index.
    def passed_the_checks(r, *absent):
        assert r.returncode in (0, 1) and all(w not in r.stderr for w in absent), r.stderr
        if r.returncode == 1:
            assert b"Error: building the index on the GPU: " in r.stderr, r.stderr
        else:
            assert b"index.movi" in r.stderr and os.path.getsize(str(tmp_path / "idx" / "index.movi")) > 2215
    p, r = _pre(tmp_path, heads=np.frombuffer(b"%CGT\x00%CGT", np.uint8))          # four symbols led by '%': plain DNA scope
    passed_the_checks(r, b"alphabet has")
    # the types without thresholds do not open REF.thr_pos: a bad one is not reported
    p, r = _pre(tmp_path, thr=THR[:-2], typ="regular")
    passed_the_checks(r, b".thr_pos")
    bad = THR.copy(); bad[7] = 1000
    p, r = _pre(tmp_path, thr=bad, typ="sampled")
    passed_the_checks(r, b".thr_pos")


def test_preprocessed_command_line(built_lib, tmp_path):
    r = run(["build", "-i", "x", "-f", "y", "--preprocessed", "--color"])
    assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"--color cannot be combined with --preprocessed" in r.stderr
    r = run(["build", "-i", "x", "--preprocessed"])
    assert r.returncode == 1 and b"Please specify the reference fasta file." in r.stderr
    r = run(["build", "-i", "x", "-f", "y", "--preprocessed", "--type", "nonsense"])
    assert r.returncode == 1 and b"index type 'nonsense' is not supported" in r.stderr
    r = run(["--help"])
    text = r.stdout + r.stderr
    assert b"movi build -i DIR -f REF --preprocessed" in text and b"movi rlbwt --bwt-file FILE" in text
    r = run(["inspect"])
    assert r.returncode == 1 and b"not part of the MI355X engine" in r.stderr and b"rlbwt" in r.stderr


def test_abi_symbol(built_lib):
    from movi_amd._lib import SYMBOLS, lib
    import movi_amd
    L = lib()
    assert "movi_build_from_rlbwt" in SYMBOLS and hasattr(L, "movi_build_from_rlbwt") and callable(movi_amd.build_image)
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    assert "int movi_build_from_rlbwt(int device, uint32_t mode, const uint8_t *h_heads, const uint64_t *h_lens, const uint64_t *h_thr" in header
    img, nbytes = C.c_void_p(1), C.c_size_t(1)
    h, l, t = HEADS.copy(), LENS.copy(), THR.copy()
    args = lambda **kw: [kw.get("device", 0), kw.get("mode", 6), kw.get("h", h.ctypes.data), kw.get("l", l.ctypes.data),
                         kw.get("t", t.ctypes.data), h.size, kw.get("img", C.byref(img)), kw.get("nb", C.byref(nbytes))]
    for kw in ({"h": None}, {"l": None}, {"t": None}, {"img": None}, {"nb": None}):
        assert L.movi_build_from_rlbwt(*args(**kw)) == -1 and L.movi_last_error(), kw
    assert img.value is None and nbytes.value == 0                                  # a refused call leaves no image
    assert L.movi_build_from_rlbwt(*args(mode=4)) == -1 and b"unsupported mode" in L.movi_last_error()
    # the checks of the arrays come before the device: MOVI_ERR_ARG here, whatever the machine holds
    l[2] = 0
    assert L.movi_build_from_rlbwt(*args()) == -1 and b"h_lens: run 2 has length zero" in L.movi_last_error()
