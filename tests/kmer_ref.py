"""The k-mer contract of include/movi_hip.h (movi_kmer_device), restated on the oracle's backward search.

bw[e] = longest legal suffix of P[0..e] that occurs in the text: Oracle.count_batch over the prefixes P[0..e] (`matched`), the
array tests/mem_ref.py defines.  Then the header's greedy loop runs over it.  `literal` is a transcription of the control flow
of the reference's query_all_kmers / query_kmers_from (src/sequitur.cpp:257-421, the non-count branch: the
look-ahead with step = k / 3, the ftab try, initialize_skipped, the max_length break) over an "occurs" predicate; it returns
None on the reads where the reference is undefined (header: deviations 1 and 2)."""
import mem_ref


def bw_arrays(oracle, reads):
    """Per read: bw as an int list."""
    pre = []
    for r in reads:
        r = bytes(r)
        pre += [r[:e + 1] for e in range(len(r))]
    if pre:
        bwm, _ = oracle.count_batch(*mem_ref._packed(pre), threads=4)
    out, k = [], 0
    for r in reads:
        m = len(r)
        out.append([int(x) for x in bwm[k:k + m]] if m else [])
        k += m
    return out


def kmers_loop(bw, m, k):
    """The header's loop: (found, [(start, count), ...]) -- runs by decreasing start."""
    assert k >= 1
    out, found, e = [], 0, m - 1
    while e >= k - 1:
        if bw[e] < k:
            e -= 1
            continue
        L = e - bw[e] + 1
        out.append((L, bw[e] - k + 1))
        found += bw[e] - k + 1
        e = L + k - 2
    return found, out


def restate(oracle, reads, ks):
    """{k: [(found, runs) per read]} for every k in ks, plus the bw arrays."""
    arr = bw_arrays(oracle, reads)
    return {k: [kmers_loop(bw, len(r), k) for r, bw in zip(reads, arr)] for k in ks}, arr


def line(rid, m, k, found, runs):
    """output_kmers, src/utils.cpp:258-266: all = m - k + 1 in 64-bit unsigned arithmetic."""
    return b"%s\t%d/%d\t%s\n" % (rid, found, (m - k + 1) % (1 << 64), b"".join(b"%d:%d " % (s, c) for s, c in runs))


def literal(occ, legal, R, k, fk):
    """The reference's control flow on read R (bytes): occ(x) = x occurs in the text, legal(byte) = check_alphabet.
    (found, runs), or None where the reference reads out of bounds or searches from an illegal / absent base."""
    out, found = [], 0
    m = len(R)
    pos = m - 1

    def init(p):                      # initialize_backward_search + try_ftab: (leftmost matched position, match length so far)
        if fk > 1 and p >= fk - 1:
            s = R[p - fk + 1:p + 1]
            if all(legal(c) for c in s) and occ(s):
                return p - fk + 1, fk - 1
        return p, 0

    def bsearch(p_left, p_right, maxlen, saved):    # backward_search: extend left while P[p-1 .. p_right] occurs
        p = p_left
        while p > 0:
            if not legal(R[p - 1]) or not occ(R[p - 1:p_right + 1]):
                break
            p -= 1
            if saved - p > maxlen:
                break
        return p

    def look(p, step):
        pa = p - step
        if not legal(R[pa]):
            return None
        l, ml = init(pa)
        if not occ(R[l:pa + 1]):
            return None
        q = bsearch(l, pa, k - step - ml, l)
        return (p - q) >= k - 1

    while pos >= 0 and not legal(R[pos]):
        pos -= 1
    if pos < 0:
        return None
    step = k // 3
    if k - step < fk:
        step = k - fk - 1
    while pos >= k - 1:
        r = look(pos, step) if pos >= k - 1 + step else True
        if r is None:
            return None
        if pos >= k - 1 + step and not r:
            pos = pos - step - 1
        else:
            saved = pos
            while True:                # initialize_skipped
                l, ml = init(pos)
                if ml == 0 and fk > 1:
                    pos -= 1
                    saved = pos
                if not (ml == 0 and pos >= k - 1 and fk > 1):
                    break
            if pos < 0 or not legal(R[pos]):
                return None
            if not occ(R[l:pos + 1]):
                return None
            q = bsearch(l if ml else pos, saved, 1 << 30, saved)
            if saved - q >= k - 1:
                f = saved - q - k + 2
                pos = q + k - 2
                out.append((pos + 2 - k, f))
                found += f
            else:
                pos = saved - 1
        while pos >= 0 and not legal(R[pos]):
            pos -= 1
        if pos < 0:
            return None
    return found, out
