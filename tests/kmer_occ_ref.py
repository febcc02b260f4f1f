"""The k-mer occurrence contract of include/movi_hip.h (movi_kmer_occ_device), restated on the oracle's count query.

occ[p] of a read = the `count` Oracle.count_batch reports for P[p .. p+k) as a read of its own where its `matched` is k, else 0.
`brute` is the same number from a dictionary of the text's k-mers; `line` is the line of `movi query --kmer-occ`."""
from collections import Counter

import numpy as np


def kmers(reads, k):
    """Every k-mer of every read, packed for count_batch: (bases, offsets, number of k-mers per read)."""
    parts, per = [], []
    for r in reads:
        a = np.frombuffer(bytes(r), np.uint8)
        n = max(0, a.size - k + 1)
        per.append(n)
        if n:
            parts.append(np.lib.stride_tricks.sliding_window_view(a, k).reshape(-1))
    bases = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    offs = np.arange(sum(per) + 1, dtype=np.uint64) * np.uint64(k)
    return bases, offs, per


def occ(oracle, reads, k):
    """Per read: the uint64 array of its max(0, m - k + 1) occurrence counts."""
    bases, offs, per = kmers(reads, k)
    if offs.size > 1:
        matched, count = oracle.count_batch(bases, offs, threads=4)
        vals = np.where(matched == np.uint64(k), count, np.uint64(0)).astype(np.uint64)
    else:
        vals = np.zeros(0, np.uint64)
    out, j = [], 0
    for n in per:
        out.append(vals[j:j + n])
        j += n
    return out


def found_sum(o):
    return int(np.count_nonzero(o)), int(o.sum(dtype=np.uint64)) if o.size else 0


def brute(text, reads, k, legal=b"ACGT"):
    """The same from a Counter over the text's k-mers (text: bytes, as the index sees it without its terminator)."""
    table = Counter(text[i:i + k] for i in range(len(text) - k + 1))
    ok = set(legal)
    out = []
    for r in reads:
        r = bytes(r)
        out.append(np.array([table.get(r[p:p + k], 0) if all(c in ok for c in r[p:p + k]) else 0 for p in range(max(0, len(r) - k + 1))],
                            np.uint64))
    return out


def line(rid, m, k, o):
    """`id <TAB> found/all <TAB> sum <TAB> occ[0],occ[1],... <LF>`, all = max(0, m - k + 1)."""
    f, s = found_sum(o)
    assert len(o) == max(0, m - k + 1)
    return b"%s\t%d/%d\t%d\t%s\n" % (rid, f, len(o), s, b",".join(b"%d" % int(v) for v in o))
