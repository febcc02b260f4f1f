"""CPU suite: the MEM contract of include/movi_hip.h (movi_mem_device) -- its restatement on the oracle's backward search
(tests/mem_ref.py) against brute-force substring search on tiny texts, and the `movi query --mem` command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import mem_ref

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def occ(text, x):
    """Occurrences of x in text, overlapping ones included."""
    n, i = 0, text.find(x)
    while i >= 0:
        n += 1
        i = text.find(x, i + 1)
    return n


def brute_arrays(text, read, legal):
    m = len(read)
    bw, fw, cnt = [0] * m, [0] * m, [0] * m
    for e in range(m):
        l = 0
        while l < e + 1 and legal[e - l] and occ(text, read[e - l:e + 1]) > 0:
            l += 1
        bw[e] = l
    for s in range(m):
        l = 0
        while s + l < m and legal[s + l] and occ(text, read[s:s + l + 1].translate(COMP)[::-1]) > 0:
            l += 1
        fw[s] = l
        cnt[s] = occ(text, read[s:s + l].translate(COMP)[::-1]) if l else 0
    return bw, fw, cnt


def tiny_reads(rng, genome, n):
    reads = []
    for _ in range(n):
        L = int(rng.integers(1, 40))
        s = int(rng.integers(0, max(1, len(genome) - L)))
        r = bytearray(genome[s:s + L])
        if rng.random() < 0.5:
            r = bytearray(bytes(r).translate(COMP)[::-1])
        for k in range(len(r)):
            u = rng.random()
            if u < 0.08:
                r[k] = b"ACGT"[rng.integers(0, 4)]
            elif u < 0.11:
                r[k] = ord("N")
            elif u < 0.13:
                r[k] = ord("acgt"[rng.integers(0, 4)])
            elif u < 0.14:
                r[k] = ord("%")
        reads.append(bytes(r))
    return reads + [b"", b"A", b"N", b"%", b"ACGTNACGT", genome[:30]]


@pytest.mark.parametrize("case", ["closed", "closed_sep", "single", "open"])
def test_restatement_equals_brute_force(case):
    from oracle import build_index as B
    from oracle.oracle import Oracle
    rng = np.random.default_rng({"closed": 11, "closed_sep": 12, "single": 13, "open": 14}[case])
    g = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    if case == "closed":                      # a random genome plus its rc as ONE record: rc-closed
        base = g(120)
        seqs, sep, rc = [base + base.translate(COMP)[::-1]], False, False
    elif case == "closed_sep":
        seqs, sep, rc = [g(90), g(70)], True, True
    elif case == "single":
        seqs, sep, rc = [g(150)], False, True
    else:                                     # several records, no separators: record junctions are not rc-symmetric
        seqs, sep, rc = [g(60), g(50), g(40)], False, True
    t = B.clean_text(seqs, rc=rc, separators=sep)
    text = bytes(t[:-1])
    img = B.build_index_from_seqs(seqs, 6, rc=rc, separators=sep)
    o = Oracle(img)
    code_of = bytearray([0xFF] * 256)
    for i, c in enumerate(b"%ACGT" if sep else b"ACGT"):
        if c != ord("%"):
            code_of[c] = i
    reads = tiny_reads(rng, text.replace(b"%", b""), 60)
    arr = mem_ref.arrays(o, reads, code_of)
    closed = case != "open"
    for r, (bw, fw, cnt) in zip(reads, arr):
        legal = [code_of[c] != 0xFF for c in r]
        assert (bw, fw, cnt) == brute_arrays(text, r, legal), r
        for L in (0, 1, 2, 3, 5, 8, 13):
            loop = mem_ref.mems_loop(bw, fw, cnt, len(r), L)
            if closed:
                assert loop == mem_ref.mems_set(fw, cnt, len(r), L), (r, L)
            for s, e, c in loop:
                assert e - s >= max(L, 1) and c == occ(text, r[s:e].translate(COMP)[::-1]) > 0
                assert all(code_of[x] != 0xFF for x in r[s:e])
    o.close()


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


def test_mem_command_line(built_lib):
    # --mem --ftab-k K is a MEM query now: against a missing index it fails for that reason, not as unsupported
    r = run(["query", "-i", "/nonexistent/index", "-r", "/nonexistent/reads.fq", "--mem", "--ftab-k", "12"])
    assert r.returncode == 1 and b"not supported" not in r.stderr and b"Error parsing command line" not in r.stderr
    r = run(["query", "-i", "/nonexistent/index", "-r", "/nonexistent/reads.fq", "--mem", "--ftab-k", "12", "-l", "20"])
    assert r.returncode == 1 and b"not supported" not in r.stderr and b"Error parsing command line" not in r.stderr
    # --mem without --ftab-k: the reference's message (src/movi.cpp:240-241)
    r = run(["query", "-i", "x", "-r", "y", "--mem"])
    assert r.returncode == 1 and b"not supported" in r.stderr and b"MEM finding requires ftab" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--mem", "--ftab-k", "0"])
    assert r.returncode == 1 and b"MEM finding requires ftab" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--mem", "--ftab-k", "12", "-l", "abc"])
    assert r.returncode == 1 and b"failed to parse for option 'min-mem-length'" in r.stderr
    for extra in (["--classify"], ["--filter"], ["--logs"]):
        r = run(["query", "-i", "x", "-r", "y", "--mem", "--ftab-k", "12"] + extra)
        assert r.returncode == 1 and b"--mem cannot be combined" in r.stderr, extra
    # set_mem comes before set_count / set_zml / set_pml (movi_parser.cpp:352-355): --mem --count is a count query
    for other in ("--count", "--zml", "--pml"):
        r = run(["query", "-i", "x", "-r", "y", "--mem", other])
        assert r.returncode == 1 and b"MEM finding" not in r.stderr and b"Error parsing command line" not in r.stderr, other
    # --ftab-k is accepted for every query; --multi-ftab stays refused
    r = run(["query", "-i", "x", "-r", "y", "--count", "--ftab-k", "8"])
    assert r.returncode == 1 and b"not supported" not in r.stderr and b"Error parsing command line" not in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--mem", "--ftab-k", "8", "--multi-ftab"])
    assert r.returncode == 1 and b"not supported" in r.stderr
    r = run(["--help"])
    assert b"--mem --ftab-k K" in r.stdout + r.stderr
