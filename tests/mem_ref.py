"""The MEM contract of include/movi_hip.h (movi_mem_device), restated on the oracle's backward search.

bw[e]  = longest legal suffix of P[0..e] that occurs in the text: Oracle.count_batch over the prefixes P[0..e] (`matched`);
fw[s]  = longest legal P[s..s+l) whose reverse complement occurs, cnt[s] its occurrences: Oracle.count_batch over
         rc(P[s..m)) with illegal bytes mapped to N first (`matched`, `count`).
Then the search loop of the header (query_mem_bml, /root/reference/src/mem_finder.cpp:27-103) runs over those arrays."""
import numpy as np

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _packed(seqs):
    lens = np.fromiter((len(s) for s in seqs), np.uint64, len(seqs))
    offs = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    return np.frombuffer(b"".join(seqs), np.uint8) if seqs else np.zeros(0, np.uint8), offs


def arrays(oracle, reads, code_of):
    """Per read: (bw, fw, cnt) as int lists."""
    code = np.frombuffer(bytes(code_of), np.uint8)
    pre, suf = [], []
    for r in reads:
        r = bytes(r)
        a = np.frombuffer(r, np.uint8)
        clean = np.where(code[a] == 0xFF, ord("N"), a).astype(np.uint8).tobytes() if len(r) else b""
        rc = clean.translate(COMP)[::-1]
        m = len(r)
        pre += [r[:e + 1] for e in range(m)]
        suf += [rc[:m - s] for s in range(m)]            # rc(P[s..m)) = the first m - s bytes of rc(P)
    out = []
    if pre:
        bwm, _ = oracle.count_batch(*_packed(pre), threads=4)
        fwm, fwc = oracle.count_batch(*_packed(suf), threads=4)
    k = 0
    for r in reads:
        m = len(r)
        out.append(([int(x) for x in bwm[k:k + m]] if m else [], [int(x) for x in fwm[k:k + m]] if m else [],
                    [int(x) for x in fwc[k:k + m]] if m else []))
        k += m
    return out


def mems_loop(bw, fw, cnt, m, L):
    """The header's search loop."""
    Lp = max(L, 1)
    out, pos = [], 0
    while pos + Lp <= m:
        w = pos + Lp - 1
        if bw[w] < Lp:
            pos = w - bw[w] + 1
            continue
        if fw[pos] < Lp:
            pos += 1
            continue
        e = pos + fw[pos]
        out.append((pos, e, cnt[pos]))
        if e == m:
            break
        pos = max(pos + 1, e - bw[e] + 1)
    return out


def mems_set(fw, cnt, m, L):
    """The closed-text form: every MEM of length >= L', by increasing start."""
    Lp = max(L, 1)
    return [(s, s + fw[s], cnt[s]) for s in range(m) if fw[s] >= Lp and (s == 0 or fw[s - 1] <= fw[s])]


def restate(oracle, reads, code_of, Ls):
    """{L: [list of (start, end, count) per read]} for every L in Ls, plus the arrays."""
    arr = arrays(oracle, reads, code_of)
    return {L: [mems_loop(bw, fw, cnt, len(r), L) for r, (bw, fw, cnt) in zip(reads, arr)] for L in Ls}, arr
