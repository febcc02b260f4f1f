"""CPU suite: `movi build --gpu-build` and movi_rlbwt_from_text / movi_build_from_text up to the first device call -- the host refusals
(each made before any device call, so they are reported on a machine without a GPU), the plan's memory formula, the command line and
the new ABI symbols.  The builder itself: tests/test_build_text_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
TYPES = ("regular-thresholds", "blocked-thresholds", "sampled-thresholds", "regular", "blocked", "sampled")
MAX_CHARS = 2 ** 32 - 2 ** 20


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


def rlbwt_call(L, text_ptr, n, opts=None):
    from movi_amd._lib import TextBuildStatsC
    heads, lens, thr, r, st = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1), C.c_uint64(7), TextBuildStatsC()
    rc = L.movi_rlbwt_from_text(0, text_ptr, n, opts, C.byref(heads), C.byref(lens), C.byref(thr), C.byref(r), C.byref(st))
    return rc, L.movi_last_error(), (heads.value, lens.value, thr.value, r.value)


def image_call(L, text_ptr, n, mode=6):
    img, nbytes = C.c_void_p(1), C.c_size_t(1)
    rc = L.movi_build_from_text(0, mode, text_ptr, n, None, C.byref(img), C.byref(nbytes), None)
    return rc, L.movi_last_error(), (img.value, nbytes.value)


def test_host_refusals(built_lib):
    """MOVI_ERR_ARG with the argument in the message and NULL outputs: a NULL pointer, n = 0, a byte 0 with its position, a text longer
    than the limit (refused by its length alone: the bytes are not read)."""
    from movi_amd._lib import lib
    L = lib()
    text = np.frombuffer(b"ACGTACGTTT", np.uint8).copy()
    zero = text.copy()
    zero[6] = 0
    for call, empty in ((rlbwt_call, (None, None, None, 0)), (image_call, (None, 0))):
        rc, msg, out = call(L, None, 10)
        assert rc == -1 and msg == b"h_text is NULL" and out == empty
        rc, msg, out = call(L, text.ctypes.data, 0)
        assert rc == -1 and msg.startswith(b"n is 0") and out == empty
        rc, msg, out = call(L, zero.ctypes.data, 10)
        assert rc == -1 and b"h_text holds a byte 0 at position 6" in msg and out == empty
        rc, msg, out = call(L, text.ctypes.data, MAX_CHARS + 1)
        assert rc == -1 and b"n is %d" % (MAX_CHARS + 1) in msg and b"limit of %d characters" % MAX_CHARS in msg and out == empty
    # ... and the output pointers, each by its name
    st = None
    assert L.movi_rlbwt_from_text(0, text.ctypes.data, 10, None, None, None, None, None, st) == -1 and L.movi_last_error() == b"h_heads is NULL"
    img = C.c_void_p()
    assert L.movi_build_from_text(0, 6, text.ctypes.data, 10, None, C.byref(img), None, None) == -1 and L.movi_last_error() == b"image_bytes is NULL"
    nbytes = C.c_size_t()
    assert L.movi_build_from_text(0, 4, text.ctypes.data, 10, None, C.byref(img), C.byref(nbytes), None) == -1
    assert b"mode 4 is not supported" in L.movi_last_error()


def test_limit_in_the_header():
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    assert "#define MOVI_TEXT_MAX_CHARS %dull" % MAX_CHARS in header


# n -> bytes, by hand from the parts movi_text.hpp lists, with N = n + 1:
#   text ((N + 7) & ~7) + 16 | ranks 4 N | keys 16 (N + 2) | suffixes 8 N | bitmap N / 8 + 8 | scratch min(N, 2^30) + 32 MiB | counters 64
PLAN = {
    1: 24 + 8 + 64 + 16 + 8 + 2 + 33554432 + 64,                                       # N = 2
    159840: 159864 + 639364 + 2557488 + 1278728 + 19988 + 159841 + 33554432 + 64,           # the golden text, N = 159841
    2 ** 31 + 2 ** 26: 2214592536 + 8858370052 + 35433480240 + 17716740104 + 276824072 + 1073741824 + 33554432 + 64,      # N = 2214592513
    MAX_CHARS: 4293918744 + 17175674884 + 68702699568 + 34351349768 + 536739848 + 1073741824 + 33554432 + 64,      # N = 4293918721
}


@pytest.mark.parametrize("n", sorted(PLAN))
def test_memory_formula(built_lib, n):
    import movi_amd
    assert movi_amd.text_device_bytes(n) == PLAN[n]
    if n > 1000:
        assert 29.1 < (PLAN[n] - (32 << 20)) / (n + 1) < 30.2      # 29.1 bytes per character and the sort's scratch, one more at most


def test_memory_formula_refuses_what_the_builder_refuses(built_lib):
    import movi_amd
    for n in (0, MAX_CHARS + 1):
        with pytest.raises(movi_amd.MoviError) as e:
            movi_amd.text_device_bytes(n)
        assert e.value.code == -1


def test_command_line(built_lib, tmp_path):
    r = run(["build", "-i", "x", "-f", "y", "--gpu-build", "--preprocessed"])
    assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"--gpu-build cannot be combined with --preprocessed" in r.stderr
    r = run(["build", "-i", "x", "-f", "y", "--verify"])
    assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"--verify belongs to --gpu-build" in r.stderr
    r = run(["build", "-i", "x", "-f", "y", "--keep"])
    assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"--keep belongs to --gpu-build" in r.stderr
    r = run(["build", "-i", "x", "-f", "y", "--keep", "--preprocessed"])
    assert r.returncode == 1 and b"--keep belongs to --gpu-build" in r.stderr
    # accepted with every type (and with the flags that go with it): the command gets as far as the FASTA, which is not there
    missing = str(tmp_path / "nothing.fasta")
    for typ in TYPES:
        r = run(["build", "-i", str(tmp_path / "out"), "-f", missing, "--gpu-build", "--type", typ, "--verify", "--keep", "--separators", "--color"])
        assert r.returncode == 1 and b"Error parsing command line" not in r.stderr and b"cannot open " + missing.encode() in r.stderr
    r = run(["build", "-i", "x", "-f", missing, "--gpu-build", "--type", "nonsense"])
    assert r.returncode == 1 and b"index type 'nonsense' is not supported" in r.stderr
    # a FASTA without a record is refused before any device call
    empty = tmp_path / "empty.fasta"
    empty.write_bytes(b"no header line\n")
    r = run(["build", "-i", str(tmp_path / "out"), "-f", str(empty), "--gpu-build"])
    assert r.returncode == 1 and b"no sequence in " + str(empty).encode() in r.stderr
    assert not os.path.exists(str(tmp_path / "out"))


def test_usage_mentions_the_flag(built_lib):
    r = run(["--help"])
    text = r.stdout + r.stderr
    assert b"--gpu-build" in text and b"--verify" in text and b"--keep" in text


def test_new_symbols(built_lib):
    from movi_amd._lib import SYMBOLS, TextBuildOptsC, TextBuildStatsC, lib
    L = lib()
    new = ("movi_rlbwt_from_text", "movi_build_from_text", "movi_text_device_bytes")
    assert all(n in SYMBOLS and hasattr(L, n) for n in new)
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    assert all(n + "(" in header for n in new)
    assert C.sizeof(TextBuildOptsC) == 40 and C.sizeof(TextBuildStatsC) == 80       # the header's structs, field for field
    import movi_amd
    assert callable(movi_amd.rlbwt_from_text) and callable(movi_amd.build_image_from_text)
