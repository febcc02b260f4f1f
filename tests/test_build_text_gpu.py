"""GPU suite (-m gpu): the run-length BWT, the thresholds and index.movi built on the GPU from a text (movi_rlbwt_from_text,
movi_build_from_text, `movi build --gpu-build`).  Heads, lengths and thresholds are compared for equality with rle(bwt) and thr of
oracle/build_index.py bwt_and_thresholds, images with serialize(build_rows(...)) -- or, through the command line, with what `movi build`
without the flag and tools/build_index write for the same FASTA."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import build_index as B
import odd_texts
from test_build_rlbwt_cpu import MOVI, rle, tool  # noqa: F401  (tool: fixture)
from test_build_rlbwt_gpu import KAT, MODES, golden_table, same

pytestmark = pytest.mark.gpu

REF_FASTA = os.path.join(GOLDEN, "ref.fasta")


def with_terminator(text):
    return np.concatenate((np.frombuffer(bytes(text), np.uint8), np.zeros(1, np.uint8)))


@functools.lru_cache(maxsize=None)
def golden_text(separators):
    return B.clean_text([B.read_fasta(REF_FASTA)[0][1]], separators=separators)


@functools.lru_cache(maxsize=None)
def golden_image(mode, separators):
    bwt, thr = golden_table(separators)
    return B.serialize(B.build_rows(bwt, thr, mode))


@functools.lru_cache(maxsize=None)
def long_a():
    """One record of A * 70 000 and 50 random bases: with its reverse complement N = 140 101, and the suffixes inside the A's (and the
    T's) share up to 69 999 characters and more -- an LCP beyond 16 bits, and doubling rounds up to 131 072 compared characters."""
    rng = np.random.default_rng(70000)
    t = B.clean_text([b"A" * 70000 + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 50)])])
    return (t,) + tuple(B.bwt_and_thresholds(t))


@functools.lru_cache(maxsize=None)
def odd(kind, separators=False):
    bwt, thr, _ = odd_texts.table(kind, separators)
    return B.clean_text(odd_texts.odd_text(kind), separators=separators), bwt, thr


def arrays(t, **opts):
    """The GPU's arrays for the text t (terminator included, as the oracle takes it)."""
    import movi_amd
    assert t[-1] == 0
    return movi_amd.rlbwt_from_text(t[:-1], **opts)


def check_arrays(t, bwt, thr, **opts):
    heads, lens, got_thr, st = arrays(t, **opts)
    want_heads, want_lens = rle(bwt)
    assert st.n_positions == t.size and st.original_r == want_heads.size == heads.size
    assert (heads == want_heads).all()
    assert (lens == want_lens).all()
    bad = np.flatnonzero(got_thr != np.asarray(thr, np.uint64))
    assert bad.size == 0, "thresholds differ at %d runs, first at run %d: %d, expected %d" % (bad.size, bad[0], got_thr[bad[0]], thr[bad[0]])
    assert st.rounds >= 1 and 0 < st.device_bytes
    return st


# ------------------------------------------------------------------------------------------------ the golden text
@pytest.mark.parametrize("separators", [False, True])
def test_golden_arrays(built_lib, separators):
    import movi_amd
    t = golden_text(separators)
    st = check_arrays(t, *golden_table(separators))
    assert st.device_bytes <= movi_amd.text_device_bytes(t.size - 1)         # the plan's formula bounds what was held
    assert st.verified == 0


@pytest.mark.parametrize("separators", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_golden_images(built_lib, mode, separators):
    import movi_amd
    img = movi_amd.build_image_from_text(golden_text(separators)[:-1], mode)
    assert len(img) == KAT[(mode, separators)]
    assert same(img, golden_image(mode, separators))
    if not separators and mode in (6, 8):
        name = {6: "index_regular-thresholds", 8: "index_blocked-thresholds"}[mode]
        assert img == open(os.path.join(GOLDEN, name, "index.movi"), "rb").read()


# ------------------------------------------------------------------------------------------------ awkward texts
@pytest.mark.parametrize("kind,separators", [(k, False) for k in odd_texts.KINDS] + [("poly", True), ("tandem", True)])
def test_odd_arrays(built_lib, kind, separators):
    check_arrays(*odd(kind, separators))


@pytest.mark.parametrize("kind,separators,mode", [(k, False, m) for k in odd_texts.KINDS for m in (6, 8, 7, 3)] +
                         [(k, True, m) for k in ("poly", "tandem") for m in (6, 8, 7, 3)])
def test_odd_images(built_lib, kind, separators, mode):
    import movi_amd
    t = odd(kind, separators)[0]
    assert same(movi_amd.build_image_from_text(t[:-1], mode), odd_texts.fields(kind, separators, mode)[1])


def test_repeat_longer_than_16_bits(built_lib):
    t, bwt, thr = long_a()
    assert t.size == 140101
    st = check_arrays(t, bwt, thr)
    # the A's share 69 999 characters or one more: settled once 131 072 are compared, not at 65 536 -- rounds compare 8, 16, 32, ...
    assert st.rounds == 15


@pytest.mark.parametrize("text", ["tandem", "long_a"])
def test_chunk_edges(built_lib, text):
    """A lane's chunk of the LCP pass of 1, 7 and 64 positions and the default: the same arrays, the oracle's."""
    t, bwt, thr = odd("tandem") if text == "tandem" else long_a()
    first = None
    for chunk in (1, 7, 64, 0):
        check_arrays(t, bwt, thr, lcp_chunk=chunk)
        got = arrays(t, lcp_chunk=chunk)[:3]
        if first is None:
            first = got
        assert all((a == b).all() for a, b in zip(first, got))


# ------------------------------------------------------------------------------------------------ tiny texts, wide alphabets
@pytest.mark.parametrize("record", [b"A", b"AC", b"ACG", b"AAAA"])
def test_tiny_texts(built_lib, record):
    t = B.clean_text([record])
    bwt, thr = B.bwt_and_thresholds(t)
    check_arrays(t, bwt, thr)
    if record == b"AAAA":                                            # AAAATTTT$
        heads, lens, got, _ = arrays(t)
        assert np.repeat(heads, lens.astype(np.int64)).tobytes() == b"T\x00AAATTTA" and got.tolist() == [0, 0, 0, 1, 5]
    for mode in (6, 3):
        import movi_amd
        assert same(movi_amd.build_image_from_text(t[:-1], mode), B.serialize(B.build_rows(bwt, thr, mode)))


def test_every_byte_value(built_lib):
    """Bytes 1 .. 255 are characters of the array builder (the DNA scope is the table builder's check): all of them once, then a random
    tail over all of them and a repeat of the whole."""
    rng = np.random.default_rng(255)
    body = np.concatenate((np.arange(1, 256), rng.integers(1, 256, 1500), rng.integers(1, 4, 300))).astype(np.uint8)
    t = with_terminator(np.concatenate((body, body[100:900], body)).tobytes())
    bwt, thr = B.bwt_and_thresholds(t)
    st = check_arrays(t, bwt, thr)
    assert np.unique(rle(bwt)[0]).size == 256
    import movi_amd
    with pytest.raises(movi_amd.MoviError) as e:                     # ... and the table builder says so
        movi_amd.build_image_from_text(t[:-1], 6)
    assert e.value.code == -1 and "alphabet has 255 symbols" in str(e.value)
    assert st.original_r > 255


# ------------------------------------------------------------------------------------------------ options
@pytest.mark.parametrize("text", ["golden", "tandem"])
def test_verify(built_lib, text):
    t, bwt, thr = (golden_text(False),) + tuple(golden_table(False)) if text == "golden" else odd("tandem")
    st = check_arrays(t, bwt, thr, verify=True)
    assert st.verified == 1
    import movi_amd
    assert st.device_bytes <= movi_amd.text_device_bytes(t.size - 1)         # with the verifier's bitmap too
    stats = []
    assert same(movi_amd.build_image_from_text(t[:-1], 3, verify=True, stats=stats),       # without thresholds: the suffix array alone
                golden_image(3, False) if text == "golden" else odd_texts.fields("tandem", False, 3)[1])
    assert stats[0].verified == 1 and stats[0].seconds["lcp"] == 0 and stats[0].seconds["thresholds"] == 0


def test_memory_refusal(built_lib):
    """max_device_bytes below the plan: refused before the first allocation, both figures in the message, outputs NULL."""
    import movi_amd
    from movi_amd._lib import TextBuildOptsC, lib
    L = lib()
    t = np.ascontiguousarray(golden_text(False)[:-1])
    need = movi_amd.text_device_bytes(t.size)
    opts = TextBuildOptsC(max_device_bytes=1 << 20)
    heads, lens, thr, r = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1), C.c_uint64(7)
    rc = L.movi_rlbwt_from_text(0, t.ctypes.data, t.size, C.byref(opts), C.byref(heads), C.byref(lens), C.byref(thr), C.byref(r), None)
    msg = L.movi_last_error()
    assert rc == -1 and (heads.value, lens.value, thr.value, r.value) == (None, None, None, 0)
    assert b"needs %d device bytes" % need in msg and b"1048576 are allowed (max_device_bytes)" in msg
    img, nbytes = C.c_void_p(1), C.c_size_t(1)
    rc = L.movi_build_from_text(0, 6, t.ctypes.data, t.size, C.byref(opts), C.byref(img), C.byref(nbytes), None)
    assert rc == -1 and (img.value, nbytes.value) == (None, 0) and b"needs %d device bytes" % need in L.movi_last_error()
    opts = TextBuildOptsC(max_device_bytes=need)                     # exactly the plan: built
    rc = L.movi_build_from_text(0, 6, t.ctypes.data, t.size, C.byref(opts), C.byref(img), C.byref(nbytes), None)
    assert rc == 0 and nbytes.value == KAT[(6, False)]
    assert L.movi_host_free(img) == 0


# ------------------------------------------------------------------------------------------------ the command line
def movi(args):
    r = subprocess.run([MOVI] + args, capture_output=True)
    assert r.returncode == 0, r.stderr
    return r.stderr


def index_of(d):
    return open(os.path.join(str(d), "index.movi"), "rb").read()


@pytest.mark.parametrize("typ,extra", [("regular-thresholds", []), ("blocked-thresholds", []), ("regular-thresholds", ["--separators"])])
def test_cli_same_index_as_the_cpu_constructor(built_lib, tmp_path, typ, extra):
    movi(["build", "-i", str(tmp_path / "cpu"), "-f", REF_FASTA, "--type", typ] + extra)
    err = movi(["build", "-i", str(tmp_path / "gpu"), "-f", REF_FASTA, "--type", typ, "--gpu-build", "--verify"] + extra)
    assert same(index_of(tmp_path / "gpu"), index_of(tmp_path / "cpu"))
    n = golden_text(bool(extra)).size - 1
    assert b"built on the GPU: %d characters, " % n in err and b" BWT runs, " in err and b" doubling rounds, verified; seconds: upload " in err
    assert b"suffix sort " in err and b"LCP " in err and b"thresholds " in err


@pytest.fixture(scope="module")
def three_records(tmp_path_factory):
    d = tmp_path_factory.mktemp("three")
    fa = d / "three.fasta"
    fa.write_bytes(b"".join(b">genome%d some words\n%s\n" % (i, s) for i, s in enumerate(odd_texts.odd_text("pangenome")[:3])))
    return d, str(fa)


def test_cli_three_records_and_color(built_lib, three_records):
    d, fa = three_records
    movi(["build", "-i", str(d / "cpu"), "-f", fa, "--color"])
    movi(["build", "-i", str(d / "gpu"), "-f", fa, "--color", "--gpu-build"])
    assert same(index_of(d / "gpu"), index_of(d / "cpu"))
    offs = open(str(d / "gpu" / "ref.fa.doc_offsets"), "rb").read()
    assert offs == open(str(d / "cpu" / "ref.fa.doc_offsets"), "rb").read() and offs == b"12000\n24000\n36000\n"


def test_cli_keep_and_preprocessed(built_lib, tool, three_records, tmp_path):
    d, fa = three_records
    mine = str(tmp_path / "three.fasta")
    shutil.copy(fa, mine)
    movi(["build", "-i", str(tmp_path / "gpu8"), "-f", mine, "--gpu-build", "--keep", "--type", "blocked-thresholds"])
    prefix = str(tmp_path / "tool")
    subprocess.check_call([tool, "fasta", fa, "8", str(tmp_path / "tool8"), "--emit-rlbwt", prefix], stderr=subprocess.DEVNULL)
    for ext in (".bwt.heads", ".bwt.len", ".thr_pos"):
        assert open(mine + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    assert same(index_of(tmp_path / "gpu8"), index_of(tmp_path / "tool8"))
    # another type from the kept files, without sorting again -- and the same one once more
    for typ, mode in (("blocked-thresholds", 8), ("sampled-thresholds", 7), ("regular", 3)):
        movi(["build", "-i", str(tmp_path / ("pre%d" % mode)), "-f", mine, "--preprocessed", "--type", typ])
        movi(["build", "-i", str(tmp_path / ("gpu%d" % mode)), "-f", mine, "--gpu-build", "--type", typ])
        assert same(index_of(tmp_path / ("pre%d" % mode)), index_of(tmp_path / ("gpu%d" % mode)))
