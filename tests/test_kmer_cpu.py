"""CPU suite: the k-mer contract of include/movi_hip.h (movi_kmer_device) -- its restatement on the oracle's backward search
(tests/kmer_ref.py) against brute-force substring search on tiny texts, the header's loop against a transcription of the
reference's control flow, the `movi query --kmer` command line and the k-mer line writer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import kmer_ref
from test_mem_cpu import COMP, tiny_reads

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
KS = (1, 2, 3, 5, 8, 13)


def _case(case):
    """(text as the index sees it, separators, the sequences, rc) of the four index shapes of tests/test_mem_cpu.py."""
    rng = np.random.default_rng({"closed": 21, "closed_sep": 22, "single": 23, "open": 24}[case])
    g = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    if case == "closed":
        base = g(120)
        seqs, sep, rc = [base + base.translate(COMP)[::-1]], False, False
    elif case == "closed_sep":
        seqs, sep, rc = [g(90), g(70)], True, True
    elif case == "single":
        seqs, sep, rc = [g(150)], False, True
    else:
        seqs, sep, rc = [g(60), g(50), g(40)], False, True
    return rng, seqs, sep, rc


def _code_of(sep):
    code_of = bytearray([0xFF] * 256)
    for i, c in enumerate(b"%ACGT" if sep else b"ACGT"):
        if c != ord("%"):
            code_of[c] = i
    return code_of


@pytest.mark.parametrize("case", ["closed", "closed_sep", "single", "open"])
def test_restatement_equals_brute_force(case):
    from oracle import build_index as B
    from oracle.oracle import Oracle
    rng, seqs, sep, rc = _case(case)
    text = bytes(B.clean_text(seqs, rc=rc, separators=sep)[:-1])
    o = Oracle(B.build_index_from_seqs(seqs, 6, rc=rc, separators=sep))
    code_of = _code_of(sep)
    genome = text.replace(b"%", b"")
    reads = tiny_reads(rng, genome, 80)
    reads += [genome[5:5 + k + d] for k in KS for d in (-1, 0, 1) if k + d > 0]          # shorter than k, exactly k, k + 1
    arr = kmer_ref.bw_arrays(o, reads)
    some = 0
    for r, bw in zip(reads, arr):
        m = len(r)
        legal = [code_of[c] != 0xFF for c in r]
        for k in KS:
            found, runs = kmer_ref.kmers_loop(bw, m, k)
            want = {p for p in range(m - k + 1) if all(legal[p:p + k]) and r[p:p + k] in text}
            got = [p for s, c in runs for p in range(s, s + c)]
            assert len(got) == len(set(got)) == found and set(got) == want, (r, k)       # disjoint, cover exactly the found set
            assert [s for s, _ in runs] == sorted((s for s, _ in runs), reverse=True)
            for s, c in runs:
                e = s + c + k - 2                                                         # the run's last k-mer ends at e
                assert c >= 1 and s == e - bw[e] + 1, (r, k)
            some += found
    assert some > 1000
    o.close()


def test_reference_control_flow_equals_the_loop():
    """The transcription of the reference's walk (look-ahead, ftab try, initialize_skipped) gives the header's loop wherever it
    is defined; it is undefined (out-of-bounds reads, a search from an illegal or absent base) on at most 15 % of the cases."""
    rng = np.random.default_rng(77)
    legal = lambda c: c in b"ACGT"
    n_def = n_undef = with_n = restarts = 0
    for _ in range(1500):
        text = bytes(rng.choice(list(b"ACGT"), int(rng.choice([40, 200, 1000]))).astype(np.uint8))
        m = int(rng.integers(1, 61))
        s = int(rng.integers(0, max(0, len(text) - m) + 1))
        R = bytearray(text[s:s + m])
        for i in range(len(R)):
            u = rng.random()
            if u < 0.06:
                R[i] = b"ACGT"[int(rng.integers(0, 4))]
            elif u < 0.09:
                R[i] = ord("N")
        R = bytes(R)
        if not R:
            continue
        bw = []
        for e in range(len(R)):
            l = 0
            while l < e + 1 and legal(R[e - l]) and R[e - l:e + 1] in text:
                l += 1
            bw.append(l)
        occ = lambda x: x in text
        for k in (2, 3, 5, 8, 13):
            want = kmer_ref.kmers_loop(bw, len(R), k)
            for fk in (0, 2, 3, 5):
                if fk >= k:
                    continue
                got = kmer_ref.literal(occ, legal, R, k, fk)
                if got is None:
                    n_undef += 1
                    continue
                n_def += 1
                assert got == want, (text, R, k, fk)
                with_n += b"N" in R
                runs = want[1]
                restarts += any(a[0] + k - 2 == b[0] + b[1] + k - 2 for a, b in zip(runs, runs[1:]))   # next run ends at L + k - 2
    assert n_def > 10000 and n_undef <= 0.15 * (n_def + n_undef), (n_def, n_undef)
    assert with_n > 0 and restarts > 0


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


def test_kmer_command_line(built_lib):
    # --kmer is a query now: against a missing index it fails for that reason, not as unsupported
    for extra in ([], ["-k", "12"], ["--ftab-k", "8"]):
        r = run(["query", "-i", "/nonexistent/index", "-r", "/nonexistent/reads.fq", "--kmer"] + extra)
        assert r.returncode == 1 and b"not supported" not in r.stderr and b"Error parsing command line" not in r.stderr, extra
    for bad in ("--kmer-count", "--rpml"):
        r = run(["query", "-i", "x", "-r", "y", bad])
        assert r.returncode == 1 and b"not supported" in r.stderr, bad
    r = run(["query", "-i", "x", "-r", "y", "--kmer", "--kmer-count"])
    assert r.returncode == 1 and b"not supported" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--kmer", "-k", "abc"])
    assert r.returncode == 1 and b"failed to parse for option 'k-length'" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--kmer", "-k", "0"])
    assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"at least 1" in r.stderr
    for extra in (["--classify"], ["--filter"], ["--logs"]):
        r = run(["query", "-i", "x", "-r", "y", "--kmer"] + extra)
        assert r.returncode == 1 and b"--kmer cannot be combined" in r.stderr, extra
    # set_kmer comes before set_mem / set_count / set_zml / set_pml (movi_parser.cpp:350-355): the later one is the query
    r = run(["query", "-i", "x", "-r", "y", "--kmer", "--mem"])
    assert r.returncode == 1 and b"MEM finding requires ftab" in r.stderr
    for other in ("--count", "--zml", "--pml"):
        r = run(["query", "-i", "x", "-r", "y", "--kmer", "-k", "0", other])        # (-k 0 is an error of the k-mer query only)
        assert r.returncode == 1 and b"Error parsing command line" not in r.stderr, other
    r = run(["query", "-i", "x", "-r", "y", "--kmer", "--count", "--classify"])
    assert r.returncode == 1 and b"--classify needs PML or ZML" in r.stderr
    r = run(["--help"])
    assert b"--kmer [-k K]" in r.stdout + r.stderr and b"--kmer-count, --rpml: not supported" in r.stdout + r.stderr


@pytest.fixture(scope="module")
def line_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kmerline") / "kmer_line_driver")
    host = os.path.join(ROOT, "movi_amd", "host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "kmer_line_driver.cpp"),
                           os.path.join(host, "output.cpp"), os.path.join(host, "options.cpp"), os.path.join(host, "reads.cpp"), "-lpthread"])
    return exe


@pytest.mark.parametrize("rid,m,k,found,runs,want", [
    (b"r1", 150, 31, 100, [(60, 60), (0, 40)], b"r1\t100/120\t60:60 0:40 \n"),               # every pair followed by a space
    (b"r2", 150, 31, 0, [], b"r2\t0/120\t\n"),                                                # empty third field
    (b"short", 10, 31, 0, [], b"short\t0/18446744073709551596\t\n"),                          # m < k: the wrapped all
    (b"empty", 0, 1, 0, [], b"empty\t0/0\t\n"),
    (b"exact", 31, 31, 1, [(0, 1)], b"exact\t1/1\t0:1 \n"),
])
def test_kmer_line_writer(line_driver, rid, m, k, found, runs, want):
    args = [line_driver, rid.decode(), str(m), str(k), str(found)] + [str(x) for r in runs for x in r]
    got = subprocess.run(args, capture_output=True, check=True).stdout
    assert got == want
    assert kmer_ref.line(rid, m, k, found, runs) == want
