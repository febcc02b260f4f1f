"""CPU suite: the locate-matches contract of include/movi_hip.h (movi_locate_matches_device) -- its brute force over the text
(tests/locate_ref.py) against the suffix array's own slices, the `movi query --locate` / `--max-occ` command line, its plan, its two
line writers, and the three symbols in the header, the library and the engine."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import locate_ref

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")

SMALL_TEXTS = [
    ([b"ACGTACGTTTGACCA"], False),
    ([b"ACGTACGTTTGACCA"], True),
    ([b"AAAAAAAAAAAAAAAAAAAAAAAA"], False),
    ([b"ATATATATATATTTATATAATATAT", b"GGGATATCC"], False),            # two records: X may span the junctions
    ([b"ATATATATATATTTATATAATATAT", b"GGGATATCC"], True),
    ([bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, 150)])], False),
]


def sa_slice(T, SA, X):
    """The suffix array's entries whose suffixes start with X, in suffix-array order: found by comparing every suffix."""
    return np.array([int(t) for t in SA if T[int(t):int(t) + len(X)] == X], np.uint64)


@pytest.mark.parametrize("case", range(len(SMALL_TEXTS)))
def test_hits_are_the_suffix_array_slice(case):
    seqs, sep = SMALL_TEXTS[case]
    tx = locate_ref.Text(seqs, separators=sep)
    assert tx.n <= 400 and tx.T[-1] == 0 and sorted(tx.SA.tolist()) == list(range(tx.n))
    body = tx.T[:-1]
    xs = {body[a:a + l] for a in range(len(body)) for l in (1, 2, 3, 5, 9) if a + l <= len(body)}
    xs |= {b"A", b"C", b"G", b"T", b"ACGTACGTACGTACGTA", b"GGGGGGG", body[:12], body[-7:]}
    some = many = 0
    for X in sorted(xs):
        got = tx.hits(X)
        if any(c not in locate_ref.LEGAL for c in X):            # (a substring of a --separators text that holds '%')
            assert got.size == 0, X
            continue
        want = sa_slice(tx.T, tx.SA, X)
        assert got.dtype == np.uint64 and got.shape == want.shape and (got == want).all(), X
        # the slice is contiguous in the suffix array: the hits are an interval of BWT positions, listed upwards
        if got.size:
            ranks = [tx.ISA[int(t)] for t in got]
            assert ranks == list(range(ranks[0], ranks[0] + len(ranks))), X
        some += got.size > 0
        many += got.size > 1
    assert some > 10 and many > 3
    assert 0 in tx.hits(body[:12]).tolist()                      # t = 0 is a hit of T's first bytes


def test_junctions_count_without_separators_only():
    seqs = [b"ATATATATATATTTATATAATATAT", b"GGGATATCC"]
    plain, sep = locate_ref.Text(seqs, False), locate_ref.Text(seqs, True)
    first_len = len(seqs[0])
    X = plain.T[first_len - 3:first_len + 3]                     # the end of record 0 and the start of its reverse complement
    assert first_len - 3 in plain.hits(X).tolist()
    assert b"%" in sep.T and sep.hits(X).size < plain.hits(X).size


def test_illegal_bases_have_no_hits():
    tx = locate_ref.Text([b"ACGTACGTTTGACCA"], separators=True)
    assert b"%" in tx.T and tx.T.find(b"A%") >= 0
    for X in (b"N", b"ACNGT", b"A%", b"%", b"acgt", b"", b"ACG\x00"):
        assert tx.hits(X).size == 0, X
    exp = tx.expect([b"ACGTNACGT"], [(0, 0, 4), (0, 2, 6), (0, 5, 9)], 2)
    assert [(o, l) for o, l, _ in exp] == [(4, 2), (0, 0), (4, 2)]         # ACGT: twice forward, twice in the reverse complement
    occ, first, pos = locate_ref.flat(exp)
    assert occ.tolist() == [4, 0, 4] and first.tolist() == [0, 2, 2, 4] and pos.size == 4


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


def test_command_line(built_lib):
    q = ["query", "-i", "/nonexistent/index", "-r", "/nonexistent/reads.fq"]
    for extra in (["--count", "--locate"], ["--count", "--locate", "--max-occ", "1"], ["--count", "--locate", "--max-occ", "4294967295"],
                  ["--mem", "--ftab-k", "8", "--locate", "--max-occ", "3"], ["--count", "--locate", "--stdout"],
                  ["--count", "--locate", "--no-output"], ["--count", "--locate", "--reverse", "--gpus", "2", "--ignore-illegal-chars", "1"]):
        r = run(q + extra)
        assert r.returncode == 1 and b"Error parsing command line" not in r.stderr, extra
        assert b"build-SA" in r.stderr, extra                     # the missing ssa.movi is reported as --sa-entries reports it
    for extra in (["--locate"], ["--pml", "--locate"], ["--zml", "--locate"], ["--kmer", "--locate"], ["--kmer-occ", "--locate"],
                  ["--sa-entries", "--locate"], ["--multi-classify", "-o", "x", "--locate"]):
        r = run(q + extra)
        assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"--locate" in r.stderr and b"--count or --mem" in r.stderr, extra
    for extra in (["--classify"], ["--filter"], ["--logs"]):
        r = run(q + ["--mem", "--ftab-k", "8", "--locate"] + extra)
        assert r.returncode == 1 and b"Error parsing command line" in r.stderr, extra
        assert b"cannot be combined with --classify, --filter or --logs" in r.stderr, extra
    r = run(q + ["--count", "--locate", "--logs"])
    assert r.returncode == 1 and b"--locate cannot be combined with --classify, --filter or --logs" in r.stderr
    r = run(q + ["--count", "--max-occ", "5"])
    assert r.returncode == 1 and b"--max-occ belongs to --locate" in r.stderr
    for bad in ("0", "4294967296", "-1", "x", "1.5", "", "99999999999999999999999"):
        r = run(q + ["--count", "--locate", "--max-occ", bad])
        assert r.returncode == 1 and b"--max-occ must be between 1 and 4294967295" in r.stderr, bad
    r = run(q + ["--count", "--sa-entries"])                      # unchanged: --sa-entries is the PML walk's
    assert r.returncode == 1 and b"--sa-entries reports the positions of the PML walk" in r.stderr
    text = run(["--help"])
    text = text.stdout + text.stderr
    assert b"--locate [--max-occ N]" in text and b".matches.locs" in text and b".mems.locs" in text


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locplan") / "query_kind_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "query_kind_driver.cpp")])
    return exe


def test_plan(plan_driver):
    def plan(line):
        out = subprocess.run([plan_driver], input=("query -i idx -r reads.fq " + line + "\n").encode(), capture_output=True, check=True).stdout.decode()
        return dict(f.split("=", 1) for f in out.split()) if not out.startswith("rejected") else out
    # the ordinary query's plan with the suffix array prepared beside the count tables (MOVI_PREPARE_COUNT | MOVI_PREPARE_SA = 10)
    for line, kind, matches in (("--count", "count", ".count.matches"), ("--mem --ftab-k 8", "mem", ".mems")):
        a, b = plan(line), plan(line + " --locate")
        assert a["kind"] == b["kind"] == kind and a["prepare"] == "2" and b["prepare"] == "10"
        assert a["matches"] == b["matches"] == matches
        assert {k: v for k, v in a.items() if k != "prepare"} == {k: v for k, v in b.items() if k != "prepare"}
        assert plan(line + " --locate --max-occ 7") == b
        assert plan(line + " --locate --stdout")["open_files"] == "0" and plan(line + " --locate --no-output")["open_files"] == "0"
    assert plan("--pml --locate").startswith("rejected: --locate reports the text positions of count or MEM hits")
    assert plan("--count --max-occ 3").startswith("rejected: --max-occ belongs to --locate")
    assert plan("--count --locate --max-occ 0").startswith("rejected: --max-occ must be between")


@pytest.fixture(scope="module")
def line_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locline") / "locs_line_driver")
    host = os.path.join(ROOT, "movi_amd", "host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "locs_line_driver.cpp"),
                           os.path.join(host, "output.cpp"), os.path.join(host, "options.cpp"), os.path.join(host, "reads.cpp"), "-lpthread"])
    return exe


@pytest.mark.parametrize("kind,rid,a,b,occ,pos,want", [
    ("count", b"r1", 150, 31, 3, [7, 0, 70000], b"r1\t31/150\t3\t3\t7,0,70000\n"),
    ("count", b"capped", 40, 40, 2 ** 40 + 5, [2 ** 40 - 1], b"capped\t40/40\t1099511627781\t1\t1099511627775\n"),    # occ in full 64 bits
    ("count", b"none", 12, 0, 0, [], b"none\t0/12\t0\t0\t\n"),                              # matched = 0: occ = listed = 0, an empty list
    ("count", b"empty", 0, 0, 0, [], b"empty\t0/0\t0\t0\t\n"),
    ("mem", b"m", 5, 36, 70000, [1, 2], b"m\t5\t36\t70000\t2\t1,2\n"),                       # not the u16 of .mems
    ("mem", b"m0", 0, 1, 0, [], b"m0\t0\t1\t0\t0\t\n"),
    ("mem", b"big", 0, 25, 2 ** 63 + 1, [2 ** 63], b"big\t0\t25\t9223372036854775809\t1\t9223372036854775808\n"),
])
def test_line_writers(line_driver, kind, rid, a, b, occ, pos, want):
    got = subprocess.run([line_driver, kind, rid.decode(), str(a), str(b), str(occ)] + [str(p) for p in pos], capture_output=True, check=True).stdout
    assert got == want
    if kind == "count":
        assert locate_ref.count_line(rid, b, a, occ, pos) == want
    else:
        assert locate_ref.mem_line(rid, a, b, occ, pos) == want


def test_symbols_in_header_library_and_engine(built_lib):
    import ctypes as C
    import movi_amd
    from movi_amd._lib import SYMBOLS, lib
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    L = lib()
    for name in ("movi_locate_matches_work_bytes", "movi_locate_matches_device", "movi_locate_matches_host"):
        assert ("int %s(" % name) in header and name in SYMBOLS and getattr(L, name) is not None
    assert "typedef struct movi_match { uint32_t read, start, end; } movi_match_t;" in header
    assert "there is none" in header                              # the note on the reference
    for meth in ("locate_matches_device", "locate_matches", "locate_matches_packed", "locate_matches_work_bytes"):
        assert callable(getattr(movi_amd.MoveIndex, meth))
    assert movi_amd.MoveIndex.MATCH_DTYPE.itemsize == 12
    # the work area: host only, grows with the items, refuses what one device scan cannot index
    b = C.c_uint64(0)
    sizes = []
    for n in (0, 1, 1000, 70000, 2 ** 31 - 2):
        assert L.movi_locate_matches_work_bytes(n, C.byref(b)) == 0
        sizes.append(b.value)
        assert b.value >= 24 * n + 8 * (n + 1) and b.value % 256 == 0
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert L.movi_locate_matches_work_bytes(2 ** 31 - 1, C.byref(b)) == -1 and b"2^31" in L.movi_last_error()
    assert L.movi_locate_matches_work_bytes(5, None) == -1
    assert movi_amd.MoveIndex.locate_matches_work_bytes(1000) == sizes[2]


def test_argument_errors_without_a_handle(built_lib):
    from movi_amd._lib import lib
    L = lib()
    buf = np.zeros(16, np.uint64)
    p = buf.ctypes.data
    assert L.movi_locate_matches_device(None, p, p, 1, p, 1, 5, p, p, p, 4, None, p, 1 << 20, None) == -1
    assert b"NULL" in L.movi_last_error()
    assert L.movi_locate_matches_host(None, p, p, 1, p, 1, 5, p, p, p, 4, None, None, None) == -1
    assert b"NULL" in L.movi_last_error()
