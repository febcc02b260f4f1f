"""CPU suite: locate -- the command lines of `movi build-SA` and `movi query --sa-entries`, the new ABI symbols, the writer of
.sa_entries.bpf, and tests/sa_ref.py's own formulas against literal LF walks (get_SA_entries, find_sampled_SA_entries) on a small text."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sa_ref

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


def test_command_lines(built_lib, tmp_path):
    # build-SA: the errors of src/movi_parser.cpp:308-317
    r = run(["build-SA"])
    assert r.returncode == 1 and b"Please specify the index directory file." in r.stderr
    r = run(["build-SA", "-i", "a", "-i", "b"])
    assert r.returncode == 1 and b"Please specify the index directory file." in r.stderr
    r = run(["build-SA", "-i", "x", "--sample-rate", "abc"])
    assert r.returncode == 1 and b"failed to parse for option 'sample-rate'" in r.stderr
    for bad in ("0", "-3", str((1 << 24) + 1)):
        r = run(["build-SA", "-i", "x", "--sample-rate", bad])
        assert r.returncode == 1 and b"Error parsing command line" in r.stderr, bad
    r = run(["build-SA", "-i", "x", "--sample-rate"])
    assert r.returncode == 1 and b"missing an argument" in r.stderr
    r = run(["build-SA", "-i", "/nonexistent/index"])               # a command now: it fails on the index (or the device), not as unknown
    assert r.returncode == 1 and b"not part of the MI355X engine" not in r.stderr and b"Error parsing command line" not in r.stderr
    # --sa-entries is a query flag now; with another query type it is a usage error (the reference opens an empty file there)
    for other in ("--zml", "--count", "--kmer"):
        r = run(["query", "-i", "x", "-r", "y", "--sa-entries", other])
        assert r.returncode == 1 and b"--sa-entries" in r.stderr and b"cannot be combined" in r.stderr, other
    r = run(["query", "-i", "x", "-r", "y", "--sa-entries", "--mem", "--ftab-k", "8"])
    assert r.returncode == 1 and b"--sa-entries" in r.stderr and b"cannot be combined" in r.stderr
    for extra in ("--classify", "--filter", "--logs"):
        r = run(["query", "-i", "x", "-r", "y", "--sa-entries", extra])
        assert r.returncode == 1 and b"--sa-entries cannot be combined" in r.stderr, extra
    r = run(["query", "-i", "x", "-r", "y", "--zml", "--sa-entries", "--pml"])   # the last query type wins: PML
    assert r.returncode == 1 and b"Error parsing command line" not in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--sa-entries", "--sample-rate", "7"])      # the rate comes from ssa.movi
    assert r.returncode == 1 and b"--sample-rate belongs to build-SA" in r.stderr
    # a missing ssa.movi: the reference's hint
    idx = tmp_path / "idx"
    idx.mkdir()
    r = run(["query", "-i", str(idx), "-r", "y", "--sa-entries"])
    assert r.returncode == 1 and b"not supported" not in r.stderr
    assert b"Failed to open sampled SA entries file at " + str(idx).encode() + b"/ssa.movi" in r.stderr and b"build-SA" in r.stderr
    for bad in ("--kmer-count", "--rpml"):
        r = run(["query", "-i", "x", "-r", "y", bad])
        assert r.returncode == 1 and b"not supported" in r.stderr, bad
    r = run(["--help"])
    assert b"build-SA -i DIR [--sample-rate N]" in r.stdout + r.stderr and b"--sa-entries" in r.stdout + r.stderr


def test_abi_symbols(built_lib):
    """Every new entry point is bound, refuses a NULL handle with MOVI_ERR_ARG and leaves a message (no handle exists without a
    device: movi_index_create fails with MOVI_ERR_NO_DEVICE / MOVI_ERR_HIP there, tests/test_abi_cpu.py)."""
    from movi_amd._lib import SYMBOLS, lib
    L = lib()
    new = ("movi_ssa_build", "movi_ssa_save", "movi_ssa_load", "movi_ssa_get", "movi_locate_device", "movi_sa_entries_device",
           "movi_sa_entries_host")
    assert all(n in SYMBOLS and hasattr(L, n) for n in new)
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    assert all(("int %s(" % n) in header for n in new) and "#define MOVI_PREPARE_SA 8u" in header and "MOVI_POS_PACK" in header
    assert L.movi_ssa_build(None, 100, None) == -1 and L.movi_last_error()
    assert L.movi_ssa_save(None, b"x") == -1 and L.movi_ssa_load(None, b"x") == -1
    assert L.movi_ssa_get(None, None, None, 0, None) == -1
    assert L.movi_locate_device(None, None, 0, None) == -1
    assert L.movi_sa_entries_device(None, None, None, 0, 0, None, None, None, None, None) == -1
    assert L.movi_sa_entries_host(None, None, None, 0, None, None, None, None) == -1
    assert L.movi_index_prepare(None, 8, None, None) == -1


@pytest.fixture(scope="module")
def record_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sarec") / "sa_record_driver")
    host = os.path.join(ROOT, "movi_amd", "host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "sa_record_driver.cpp"),
                           os.path.join(host, "output.cpp"), os.path.join(host, "options.cpp"), os.path.join(host, "reads.cpp"), "-lpthread"])
    return exe


@pytest.mark.parametrize("rid,entries", [(b"r1", [5, 0, (1 << 40) + 3]), (b"empty", []), (b"x" * 300, [18446744073709551615]), (b"one", [7])])
def test_sa_record_writer(record_driver, rid, entries):
    got = subprocess.run([record_driver, rid.decode()] + [str(e) for e in entries], capture_output=True, check=True).stdout
    want = struct.pack("<H", len(rid)) + rid + struct.pack("<Q", len(entries)) + b"".join(struct.pack("<Q", e) for e in entries)
    assert got == want
    assert sa_ref.sa_entries_file([rid], [np.array(entries, np.uint64)]) == want


@pytest.mark.parametrize("sep", [False, True])
def test_formula_equals_the_literal_walks(sep):
    """entry() and samples() against get_SA_entries / find_sampled_SA_entries walked literally over the build_rows fields."""
    rng = np.random.default_rng(31 + sep)
    seqs = [bytes(rng.choice(list(b"ACGT"), 90).astype(np.uint8)), bytes(rng.choice(list(b"AC"), 60).astype(np.uint8))]
    f, SA = sa_ref.text_fields(seqs, 6, separators=sep)
    n = f["n"]
    assert 300 <= n <= 310 and sorted(SA) == list(range(n))
    rows, offs = sa_ref.all_positions(f)
    wrapped = 0
    for rate in (1, 2, 7, n, n + 5):
        smp = sa_ref.lf_walk_samples(f, rate)
        assert (smp == sa_ref.samples(SA, rate)).all() and len(smp) == n // rate + 1, rate
        if n % rate == 0:
            assert smp[-1] == 0
        want = sa_ref.entries(SA, rate)
        got = [sa_ref.lf_walk_entry(f, smp, rate, int(r), int(o)) for r, o in zip(rows, offs)]
        assert got == [int(x) for x in want], rate
        wrapped += int((want >= n).sum())
        assert sa_ref.ssa_bytes(f, SA, rate)[:16] == struct.pack("<QQ", rate, n // rate + 1)
        assert len(sa_ref.ssa_bytes(f, SA, rate)) == 8 * (3 + n // rate + 1 + f["r"])
    assert wrapped > 0


def test_position_restatement_is_pinned_to_the_oracle(built_lib):
    """walk() reproduces Oracle.pml on mutated reads with illegal bases (positions() asserts it), for the three thresholds layouts."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    from test_gpu_parity import mutated_reads
    rng = np.random.default_rng(5)
    seqs = [bytes(rng.choice(list(b"ACGT"), 4000).astype(np.uint8))]
    t = bytes(B.clean_text(seqs)[:-1])
    reads = mutated_reads(rng, t, 60, 1, 200) + [b"", b"N" * 9, t[10:11]]
    for sep in (False, True):
        for mode in (6, 8, 7):
            f, SA = sa_ref.text_fields(seqs, mode, separators=sep)
            o = Oracle(B.serialize(f))
            pos = sa_ref.positions(f, o, reads)
            assert [len(p[0]) for p in pos] == [len(r) for r in reads]
            assert all((0 <= p[1]).all() and (p[1] < np.asarray(f["lens"])[p[0]]).all() for p in pos if len(p[0]))
            o.close()
