"""CPU suite: the k-mer occurrence contract of include/movi_hip.h (movi_kmer_occ_device) -- its restatement on the oracle's count
query (tests/kmer_occ_ref.py) against a dictionary of the text's k-mers, its `found` against the k-mer presence restatement, the
`movi query --kmer-occ` command line, its plan and its line writer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import kmer_occ_ref
import kmer_ref
import odd_texts
from test_gpu_parity import mutated_reads
from test_kmer_gpu import _edge_reads

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
KS = (1, 5, 12, 13, 31, 200)
ODD_KS = (5, 12, 31)


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def ref_reads():
    ref = _ref()
    return mutated_reads(np.random.default_rng(616), ref, 600, 1, 400) + _edge_reads(ref)


def _text(seqs, sep):
    from oracle import build_index as B
    return bytes(B.clean_text(seqs, separators=sep)[:-1])


@pytest.fixture(scope="module")
def ref_restated():
    """{separators: (reads, text, {k: occ per read})} on ref.fasta, from the oracle on the mode-6 image."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref, reads, out = _ref(), ref_reads(), {}
    for sep in (False, True):
        o = Oracle(B.build_index_from_seqs([ref], 6, separators=sep))
        out[sep] = (reads, _text([ref], sep), {k: kmer_occ_ref.occ(o, reads, k) for k in KS})
        o.close()
    return out


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint64 and g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


@pytest.mark.parametrize("sep", [False, True])
def test_restatement_equals_brute_force(ref_restated, sep):
    reads, text, occ = ref_restated[sep]
    assert any(b"N" in r[p:p + 12] for r in reads for p in range(len(r) - 11))        # some k-mer holds an illegal base
    ones = 0
    for k in KS:
        want = kmer_occ_ref.brute(text, reads, k)
        assert _same(occ[k], want), k
        assert sum(int(np.count_nonzero(o)) for o in want) > 0, k
        ones += sum(int((o == 1).sum()) for o in want)
        for r, o in zip(reads, want):
            assert len(o) == max(0, len(r) - k + 1)
    assert ones > 1000


def test_separators_change_the_sums(ref_restated):
    """The text with separators holds the reverse complement too: the k = 5 sums differ, so the two cases are two cases."""
    sums = [sum(int(o.sum(dtype=np.uint64)) for o in ref_restated[sep][2][5]) for sep in (False, True)]
    assert sums[0] != sums[1] and min(sums) > 0


@pytest.mark.parametrize("kind", odd_texts.KINDS)
def test_restatement_on_odd_texts(kind):
    from oracle.oracle import Oracle
    reads = list(odd_texts.reads_of(kind))
    o = Oracle(odd_texts.fields(kind, False, 6)[1])
    text = _text(odd_texts.odd_text(kind), False)
    top = 0
    for k in ODD_KS:
        got, want = kmer_occ_ref.occ(o, reads, k), kmer_occ_ref.brute(text, reads, k)
        assert _same(got, want), (kind, k)
        top = max([top] + [int(x.max()) for x in want if x.size])
    o.close()
    if kind in ("poly", "tandem"):
        assert top > 2047                                     # beyond what one run holds: the count spans rows
    if kind == "two_letters":
        w31 = kmer_occ_ref.brute(text, reads, 31)
        assert {int(v) for x in w31 for v in x} == {0, 1}


def test_found_equals_the_presence_query(ref_restated):
    from oracle import build_index as B
    from oracle.oracle import Oracle
    reads, _, occ = ref_restated[False]
    o = Oracle(B.build_index_from_seqs([_ref()], 6))
    pres, _ = kmer_ref.restate(o, reads, KS)
    o.close()
    for k in KS:
        assert [kmer_occ_ref.found_sum(x)[0] for x in occ[k]] == [f for f, _ in pres[k]], k


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


def test_command_line(built_lib):
    for extra in ([], ["-k", "12"], ["--ftab-k", "8"], ["--stdout"], ["--no-output"], ["--kmer"]):
        r = run(["query", "-i", "/nonexistent/index", "-r", "/nonexistent/reads.fq", "--kmer-occ"] + extra)
        assert r.returncode == 1 and b"not supported" not in r.stderr and b"Error parsing command line" not in r.stderr, extra
    for extra in (["--classify"], ["--filter"], ["--logs"], ["--sa-entries"], ["--multi-classify", "-o", "x"]):
        r = run(["query", "-i", "x", "-r", "y", "--kmer-occ"] + extra)
        assert r.returncode == 1 and b"--kmer-occ cannot be combined" in r.stderr, extra
    r = run(["query", "-i", "x", "-r", "y", "--kmer-occ", "-k", "0"])
    assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"at least 1" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--kmer-occ", "--kmer-count"])
    assert r.returncode == 1 and b"--kmer-count is not supported" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--kmer-occ", "--mem"])
    assert r.returncode == 1 and b"MEM finding requires ftab" in r.stderr
    for other in ("--count", "--zml", "--pml"):
        r = run(["query", "-i", "x", "-r", "y", "--kmer-occ", "-k", "0", other])    # (-k 0 is an error of the k-mer queries only)
        assert r.returncode == 1 and b"Error parsing command line" not in r.stderr, other
    r = run(["--help"])
    text = r.stdout + r.stderr
    assert b"--kmer-occ [-k K]" in text and b"--kmer [-k K]" in text and b"--kmer-count, --rpml: not supported" in text


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("occplan") / "query_kind_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "query_kind_driver.cpp")])
    return exe


def test_plan(plan_driver):
    def plan(line):
        out = subprocess.run([plan_driver], input=("query -i idx -r reads.fq " + line + "\n").encode(), capture_output=True, check=True).stdout.decode()
        return dict(f.split("=", 1) for f in out.split()) if not out.startswith("rejected") else out
    for line, files, suffix in (("--kmer-occ", "1", ".kmer_occ.31"), ("--kmer-occ --stdout", "0", "-"), ("--kmer-occ --no-output", "0", "-"),
                                ("--kmer --kmer-occ -k 12", "1", ".kmer_occ.12")):
        p = plan(line)
        assert p["kind"] == "kmer_occ" and p["prepare"] == "2" and p["open_files"] == files and p["matches"] == suffix, line
        assert p["result_vector"] == p["to_bpf"] == p["verdict_only"] == p["walk_only"] == "0" and p["bpf"] == p["sa"] == p["report"] == "-"
    assert plan("--kmer-occ --count") == plan("--count") and plan("--count")["kind"] == "count"
    assert plan("--kmer")["kind"] == "kmer" and plan("--kmer")["matches"] == ".kmers.31"
    assert plan("--kmer-occ --logs").startswith("rejected: --kmer-occ cannot be combined")


@pytest.fixture(scope="module")
def line_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("occline") / "kmer_occ_line_driver")
    host = os.path.join(ROOT, "movi_amd", "host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "kmer_occ_line_driver.cpp"),
                           os.path.join(host, "output.cpp"), os.path.join(host, "options.cpp"), os.path.join(host, "reads.cpp"), "-lpthread"])
    return exe


@pytest.mark.parametrize("rid,m,k,occ,want", [
    (b"r1", 6, 3, [3, 0, 70000, 1], b"r1\t3/4\t70004\t3,0,70000,1\n"),
    (b"big", 3, 3, [2 ** 40 + 5], b"big\t1/1\t1099511627781\t1099511627781\n"),
    (b"none", 5, 2, [0, 0, 0, 0], b"none\t0/4\t0\t0,0,0,0\n"),
    (b"short", 10, 31, [], b"short\t0/0\t0\t\n"),                                            # m < k: all = 0, an empty list
    (b"empty", 0, 1, [], b"empty\t0/0\t0\t\n"),
    (b"exact", 31, 31, [7], b"exact\t1/1\t7\t7\n"),
])
def test_line_writer(line_driver, rid, m, k, occ, want):
    o = np.array(occ, np.uint64)
    f, s = kmer_occ_ref.found_sum(o)
    slots = [int(v) for v in o] + [0] * (m - len(occ))                                       # the engine's layout: one slot per base
    got = subprocess.run([line_driver, rid.decode(), str(m), str(k), str(f), str(s)] + [str(v) for v in slots], capture_output=True, check=True).stdout
    assert got == want
    assert kmer_occ_ref.line(rid, m, k, o) == want


def test_argument_errors_without_a_handle(built_lib):
    from movi_amd._lib import lib
    L = lib()
    buf = np.zeros(8, np.uint64)
    for k in (0, 5):
        assert L.movi_kmer_occ_host(None, buf.ctypes.data, buf.ctypes.data, 1, k, buf.ctypes.data, None, None, None, None) == -1
        assert b"NULL" in L.movi_last_error()
        assert L.movi_kmer_occ_device(None, buf.ctypes.data, buf.ctypes.data, 1, 8, k, buf.ctypes.data, None, None, None, None) == -1
        assert b"NULL" in L.movi_last_error()
