"""GPU suite (-m gpu): index.movi built on the GPU from a run-length BWT (movi_build_from_rlbwt, `movi build --preprocessed`).
Every comparison is byte equality of the whole image with oracle/build_index.py: serialize(build_rows(bwt, thr, mode)) -- or, for the
2 M-row table, with the index.movi tools/build_index wrote for the same text.  One case cannot be held to that oracle: see
test_block_size_halves."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import build_index as B
import odd_texts
from test_build_rlbwt_cpu import MOVI, TOOL, rle, tool, write_rlbwt  # noqa: F401  (tool: fixture)

pytestmark = pytest.mark.gpu

MODES = (6, 3, 8, 2, 7, 5)


def gpu_image(bwt, thr, mode):
    import movi_amd
    heads, lens = rle(bwt)
    return movi_amd.build_image(heads, lens, np.asarray(thr, np.uint64) if mode in B.THRESHOLD_MODES else None, mode)


def same(got, want):
    """Byte equality, with the first difference in the message instead of two images."""
    if got == want:
        return True
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    k = min(a.size, b.size)
    d = np.flatnonzero(a[:k] != b[:k])
    raise AssertionError("images differ: %d vs %d bytes, first difference at byte %s" % (a.size, b.size, int(d[0]) if d.size else "-"))


def check(bwt, thr, mode):
    f = B.build_rows(np.asarray(bwt, np.uint8), np.asarray(thr, np.int64), mode)
    assert same(gpu_image(bwt, thr, mode), B.serialize(f))
    return f


@functools.lru_cache(maxsize=None)
def golden_table(separators):
    ref = B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]
    return B.bwt_and_thresholds(B.clean_text([ref], separators=separators))


# the index sizes of the reference's known answers (tests/test_build.cpp of the reference), by (mode, separators)
KAT = {(6, False): 948119, (8, False): 711733, (7, False): 475326, (5, False): 437006, (3, False): 871479, (2, False): 654253,
       (6, True): 948232, (8, True): 711854, (7, True): 505009, (5, True): 464203, (3, True): 871496, (2, True): 654280}


@pytest.mark.parametrize("separators", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_golden_text(built_lib, mode, separators):
    bwt, thr = golden_table(separators)
    img = gpu_image(bwt, thr, mode)
    assert len(img) == KAT[(mode, separators)]
    assert same(img, B.serialize(B.build_rows(bwt, thr, mode)))
    if not separators and mode in (6, 8):
        name = {6: "index_regular-thresholds", 8: "index_blocked-thresholds"}[mode]
        assert img == open(os.path.join(GOLDEN, name, "index.movi"), "rb").read()


@pytest.mark.parametrize("kind,separators,mode", [(k, False, m) for k in odd_texts.KINDS for m in MODES] +
                         [(k, True, m) for k in ("poly", "tandem") for m in (6, 8, 7)])
def test_odd_texts(built_lib, kind, separators, mode):
    bwt, thr, _ = odd_texts.table(kind, separators)
    f, want = odd_texts.fields(kind, separators, mode)
    assert same(gpu_image(bwt, thr, mode), want)
    if kind == "poly":
        assert f["r"] > len(rle(bwt)[0]) and int(f["lens"].max()) == B.MAX_RUN[mode]      # runs split at MAX_RUN_LENGTH
    if kind == "two_letters":
        assert len(f["alphabet"]) == 2


def expand(runs):
    """[(byte, length)] -> the BWT as uint8."""
    return np.concatenate([np.full(n, c if isinstance(c, int) else ord(c), np.uint8) for c, n in runs])


def starts_of(runs):
    return np.concatenate(([0], np.cumsum([n for _, n in runs])))[:-1]


@pytest.mark.parametrize("mode", MODES)
def test_hand_made_thresholds(built_lib, mode):
    """Corners a text rarely gives.  Any threshold from 0 to n is a legal split point for build_rows."""
    runs = [("A", 5), ("C", 3000), ("G", 7), ("A", 5000), ("T", 2), (0, 1), ("C", 40), ("G", 4100), ("A", 1), ("T", 600)]
    st = starts_of(runs)
    n = int(sum(k for _, k in runs))
    thr = np.zeros(len(runs), np.int64)
    thr[1] = st[3]                      # equal to a run start
    thr[2] = thr[4] = st[3] + 1500      # two runs with one threshold, in the middle of a run longer than every MAX_RUN_LENGTH
    thr[3] = st[1] + B.MAX_RUN[mode]    # exactly where a piece of the C run ends anyway
    thr[6] = st[7] + 4099               # one character before a run's end
    thr[7] = n                          # the text's length: no split
    thr[8] = st[5]                      # the terminator's row
    thr[9] = st[7] + 1                  # one character into a run
    f = check(expand(runs), thr, mode)
    if mode in B.THRESHOLD_MODES:       # the pieces restart at the split: A(5000) is cut at 1500, and in pieces of MAX_RUN_LENGTH from there
        p, m = f["all_p"].tolist(), B.MAX_RUN[mode]
        assert st[3] + 1500 in p and st[3] + 1500 + m in p and st[3] + (1500 // m + 1) * m not in p


TERMINATOR_PLACES = {
    "before_A": [("C", 3), (0, 1), ("A", 4), ("G", 2), ("T", 3), ("C", 2)],
    "after_A": [("C", 3), ("A", 4), (0, 1), ("G", 2), ("T", 3), ("A", 2)],
    "between_A": [("G", 3), ("A", 4), (0, 1), ("A", 2), ("T", 3), ("C", 2)],
    "first": [(0, 1), ("A", 4), ("C", 2), ("G", 2), ("T", 3), ("A", 2)],
    "last": [("T", 2), ("A", 4), ("C", 2), ("G", 2), ("T", 3), ("A", 2), (0, 1)],
    "first_separators": [(0, 1), ("%", 2), ("A", 4), ("C", 2), ("%", 1), ("G", 2), ("T", 3), ("A", 2)],
    "last_separators": [("%", 1), ("T", 2), ("A", 4), ("%", 2), ("C", 2), ("G", 2), ("T", 3), ("A", 2), (0, 1)],
    "after_separator": [("A", 2), ("%", 3), (0, 1), ("%", 1), ("C", 2), ("G", 2), ("T", 3)],
}


@pytest.mark.parametrize("place", sorted(TERMINATOR_PLACES))
@pytest.mark.parametrize("mode", MODES)
def test_terminator_places(built_lib, mode, place):
    runs = TERMINATOR_PLACES[place]
    st = starts_of(runs)
    rng = np.random.default_rng(len(place))
    for thr in (np.zeros(len(runs), np.int64), st[rng.integers(0, len(runs), len(runs))], rng.integers(0, int(st[-1]) + 1, len(runs))):
        check(expand(runs), thr, mode)


def singles(k, letters=b"AT", first=0):
    """k runs of length 1 over `letters` in turn."""
    return [(letters[(first + i) % len(letters)], 1) for i in range(k)]


@pytest.mark.parametrize("mode", (7, 5))
@pytest.mark.parametrize("r", (39, 40, 41, 20 * 300 - 1, 20 * 300, 20 * 300 + 1))
def test_rows_around_a_tally_checkpoint(built_lib, mode, r):
    """r a multiple of the checkpoint distance: the table has an entry no checkpoint fills (it stays 0) before the last one."""
    runs = singles(r // 2) + [(0, 1)] + singles(r - r // 2 - 1, b"CAGT")
    f = check(expand(runs), np.zeros(len(runs), np.int64), mode)
    assert f["r"] == r and f["tally_ids"].shape[1] == r // 20 + 2


@pytest.mark.parametrize("mode,block", [(8, 1 << 20), (2, 1 << 22)])
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_rows_around_a_block_boundary(built_lib, mode, block, delta):
    """r = the blocked block size and one row either side, over two letters (build_rows walks the rows in Python)."""
    r = block + delta
    heads = np.tile(np.frombuffer(b"AT", np.uint8), r // 2 + 1)[:r].copy()
    heads[r // 3] = 0                                            # (its neighbours are one letter, but not each other's)
    f = check(heads, np.zeros(r, np.int64), mode)
    assert f["r"] == r and f["id_blocks"].shape[1] == (2 if delta == 1 else 1) and f["block_size"] == block


def _rows_of(img, mode):
    """(u16 row words, the bytes after the rows) of a mode 6 / 8 image over a 4-symbol alphabet."""
    off = 48 + 96 + 8 + 2048 + 8 + 4 + 3
    r = int(np.frombuffer(img, "<u8", 1, 24)[0])
    words = {6: 4, 8: 3}[mode]
    return np.frombuffer(img, "<u2", r * words, off).reshape(r, words).astype(np.int64), img[off + r * words * 2:]


def test_block_size_halves(built_lib):
    """A table on which the blocked block size must halve: within one block of 2^20 rows the ids of C advance by more than the
    22 bits a row keeps, within each half by less.  oracle/build_index.py compute_blocked_ids cannot be the reference here: it halves
    the bound together with the block size, and then no round after a failed one can pass (a block whose distance exceeds
    4 b - 1 holds a half whose distance exceeds 2 b - 1), so it ends in a division by zero on this and on every such table.  The
    reference sets the bound anew in every round (src/move_structure_build.cpp:956); that rule is restated below and the blocked
    table is held to the regular-thresholds table of the same input, which test_golden_text and the others hold to the oracle:
    no run is longer than either type's MAX_RUN_LENGTH, so the two have the same rows."""
    half = 9 << 19                                               # a 2^19 boundary inside the block [4 * 2^20, 5 * 2^20)
    k = 2600
    heads = np.concatenate((np.frombuffer(b"A\x00", np.uint8), np.tile(np.frombuffer(b"GT", np.uint8), (half - 2 * k - 2) // 2),
                            np.tile(np.frombuffer(b"CG", np.uint8), 2 * k), np.frombuffer(b"T", np.uint8)))
    lens = np.ones(heads.size, np.uint64)
    lens[heads == ord("C")] = 1023
    thr = np.zeros(heads.size, np.uint64)
    import movi_amd
    img6, img8 = movi_amd.build_image(heads, lens, thr, 6), movi_amd.build_image(heads, lens, thr, 8)
    w6, _ = _rows_of(img6, 6)
    w8, tail = _rows_of(img8, 8)
    r = heads.size
    assert w6.shape[0] == r and w8.shape[0] == r
    pid = w6[:, 0] | (w6[:, 1] << 16) | ((w6[:, 3] >> 12) << 32)
    code, end = w6[:, 2] >> 13, 1
    # the reference's rule on the regular table's ids
    u = np.frombuffer(tail, "<u8", 4 + 4 + 1 + 20, 0)
    assert u[:3].tolist() == [0, 0, 0] and u[3] == 4 and u[8] == 5
    first_runs = u[19:24].astype(np.int64)
    adj = pid - first_runs[code + 1]
    block, fits = 1 << 20, False
    while not fits:
        nb = (r + block - 1) // block
        ck = np.zeros((4, nb), np.int64)
        for a in range(4):
            idx = np.flatnonzero((code == a) & (np.arange(r) != end))
            at = np.searchsorted(idx, np.arange(nb) * block, side="left")
            ck[a] = np.where(at > 0, adj[idx[np.maximum(at - 1, 0)]], 0)
        blocked = adj - ck[code, np.arange(r) // block]
        blocked[end] = 0
        fits = blocked.max() <= (1 << 22) - 1
        if not fits:
            block //= 2
    assert block == 1 << 19                                      # it halved, once
    nb8 = int(np.frombuffer(tail, "<u8", 1, 29 * 8)[0])
    assert nb8 == nb and int(np.frombuffer(tail, "<u8", 1, 30 * 8 + nb * 16)[0]) == block
    assert (np.frombuffer(tail, "<u4", 4 * nb, 30 * 8).reshape(4, nb) == ck).all()
    assert ((w8[:, 0] | ((w8[:, 1] >> 10) << 16)) == blocked).all()
    # ... and everything else in the rows is the regular table's
    assert ((w8[:, 1] & 0x3FF) == (w6[:, 2] & 0x7FF)).all() and ((w8[:, 2] & 0x3FF) == (w6[:, 3] & 0x7FF)).all()
    assert (((w8[:, 2] >> 10) & 7) == code).all()
    assert ((w8[:, 2] >> 13) == (((w6[:, 3] >> 11) & 1) | (((w6[:, 2] >> 11) & 1) << 1) | (((w6[:, 2] >> 12) & 1) << 2))).all()
    head = 48 + 96 + 8 + 2048 + 8 + 4 + 3
    assert img8[:7] == img6[:7] and img8[7] == 8 and img8[8:head] == img6[8:head]


@pytest.fixture(scope="module")
def big_table(tool, tmp_path_factory):
    """A synthetic pangenome of about 2 M rows: its run-length BWT files, and the directory of the tool's own indexes."""
    d = tmp_path_factory.mktemp("rlbwt2m")
    prefix = str(d / "ref")
    subprocess.check_call([tool, "pangenome", "700000", "2", "0.25", "11", "6", str(d / "tool6"), "2000", "120", "0.02", "--emit-rlbwt", prefix],
                          stderr=subprocess.DEVNULL)
    return d, prefix


@pytest.mark.parametrize("mode,typ", [(6, "regular-thresholds"), (8, "blocked-thresholds"), (7, "sampled-thresholds")])
def test_two_million_rows_through_the_cli(built_lib, tool, big_table, mode, typ):
    d, prefix = big_table
    want_dir = str(d / ("tool%d" % mode))
    if mode != 6:
        subprocess.check_call([tool, "pangenome", "700000", "2", "0.25", "11", str(mode), want_dir], stderr=subprocess.DEVNULL)
    out = str(d / ("gpu%d" % mode))
    r = subprocess.run([MOVI, "build", "-i", out, "-f", prefix, "--preprocessed", "--type", typ], capture_output=True)
    assert r.returncode == 0, r.stderr
    got, want = open(os.path.join(out, "index.movi"), "rb").read(), open(os.path.join(want_dir, "index.movi"), "rb").read()
    assert 1_500_000 < int(np.frombuffer(want, "<u8", 1, 24)[0]) < 3_000_000
    assert same(got, want)
    if mode == 6:                                                # the built index answers a PML batch like the oracle
        import movi_amd
        from oracle.oracle import Oracle
        gpu, cpu = movi_amd.MoveIndex.load(out), Oracle(want)
        bases = np.fromfile(str(d / "tool6" / "reads.bin"), np.uint8)
        offs = np.arange(2001, dtype=np.uint64) * np.uint64(120)
        pml, _ = gpu.query_pml_packed(bases, offs)
        assert (pml == cpu.pml_batch(bases, offs, threads=4)[0]).all()
        gpu.close()
        cpu.close()


def test_malformed_arrays_are_refused(built_lib):
    """Straight through the C-ABI: MOVI_ERR_ARG with the reason, no image -- refusals by the host checks, not faults."""
    from movi_amd._lib import lib
    L = lib()
    heads0 = np.frombuffer(b"ACGT\x00ACGT", np.uint8)
    lens0 = np.array([3, 2, 4, 1, 1, 2, 5, 1, 3], np.uint64)
    thr0 = np.array([0, 0, 0, 0, 0, 4, 6, 12, 15], np.uint64)

    def call(heads, lens, thr, mode=6):
        img, nbytes = C.c_void_p(1), C.c_size_t(1)
        rc = L.movi_build_from_rlbwt(0, mode, heads.ctypes.data, lens.ctypes.data, thr.ctypes.data, heads.size, C.byref(img), C.byref(nbytes))
        return rc, L.movi_last_error(), img.value, nbytes.value

    bad = lens0.copy(); bad[3] = 0
    assert call(heads0, bad, thr0) == (-1, b"h_lens: run 3 has length zero", None, 0)
    bad = thr0.copy(); bad[8] = 23
    rc, msg, img, nb = call(heads0, lens0, bad)
    assert (rc, img, nb) == (-1, None, 0) and b"h_thr: threshold 8 is 23, greater than the text's length 22" in msg
    rc, msg, img, nb = call(np.frombuffer(b"ACGT\x00AC\x00T", np.uint8).copy(), lens0, thr0)
    assert (rc, img, nb) == (-1, None, 0) and b"h_heads: the terminator (byte 0) appears 2 times" in msg
    rc, msg, img, nb = call(np.frombuffer(b"ACGT\x00ACCT", np.uint8).copy(), lens0, thr0)
    assert (rc, img, nb) == (-1, None, 0) and b"h_heads: runs 6 and 7 have the same head" in msg
    # the same arrays, sound: an image
    rc, msg, img, nb = call(heads0.copy(), lens0, thr0)
    assert rc == 0 and img and nb > 2215
    assert C.string_at(img, nb) == B.serialize(B.build_rows(np.repeat(heads0, lens0.astype(np.int64)), thr0.astype(np.int64), 6))
    assert L.movi_host_free(C.c_void_p(img)) == 0
