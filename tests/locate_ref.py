"""The locate-matches contract of include/movi_hip.h (movi_locate_matches_device), stated on the indexed text itself: the reference
has no such mode, so this is a brute force over T = oracle.build_index.clean_text(...) and its suffix array.

  hits(T, ISA, X)          every t with T[t : t + |X|] == X (overlapping occurrences, bytes.find), sorted by ISA[t] -- the rank of the
                           suffix T[t:], that is, BWT order; none if X holds a byte that is no legal base (N, the separator '%', ...);
  Text(seqs, separators)   T, SA and ISA of the text `movi build [--separators]` indexes, with hits() cached per X;
  Text.expect(reads, items, max_occ)   per item (read, start, end): (occ, listed, positions) with listed = min(occ, max_occ);
  flat(expected)           the device layout: occ[n], first[n + 1] (exclusive prefix sum of listed), the positions end to end;
  count_line / mem_line    the lines of <prefix>.matches.locs and <prefix>.mems.locs."""
import numpy as np

from oracle import build_index as B

LEGAL = frozenset(b"ACGT")


def hits(T, ISA, X):
    """Text positions of X in `T` (bytes, terminator included) by increasing ISA."""
    X = bytes(X)
    if not X or any(c not in LEGAL for c in X):
        return np.zeros(0, np.uint64)
    out, t = [], T.find(X)
    while t >= 0:
        out.append(t)
        t = T.find(X, t + 1)
    out.sort(key=lambda p: ISA[p])
    return np.array(out, np.uint64)


class Text:
    def __init__(self, seqs, separators=False, SA=None):
        t = B.clean_text(seqs, separators=separators)
        self.T = bytes(t)
        self.n = len(self.T)
        self.SA = np.asarray(SA if SA is not None else B.suffix_array(t), np.int64)
        isa = np.empty(self.n, np.int64)
        isa[self.SA] = np.arange(self.n)
        self.ISA = isa.tolist()
        self._cache = {}

    def hits(self, X):
        X = bytes(X)
        if X not in self._cache:
            self._cache[X] = hits(self.T, self.ISA, X)
        return self._cache[X]

    def expect(self, reads, items, max_occ):
        out = []
        for r, s, e in items:
            h = self.hits(reads[r][s:e])
            listed = min(len(h), max_occ)
            out.append((len(h), listed, h[:listed]))
        return out


def flat(expected):
    occ = np.array([o for o, _, _ in expected], np.uint64)
    first = np.zeros(len(expected) + 1, np.uint64)
    first[1:] = np.cumsum([l for _, l, _ in expected], dtype=np.uint64) if expected else 0
    pos = np.concatenate([p for _, _, p in expected] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    return occ, first, pos


def _tail(occ, pos):
    return b"%d\t%d\t%s\n" % (occ, len(pos), b",".join(b"%d" % int(p) for p in pos))


def count_line(rid, matched, length, occ, pos):
    """`id <TAB> matched/len <TAB> occ <TAB> listed <TAB> p,p,... <LF>` (a read with matched = 0: occ = listed = 0, the last field empty)."""
    return b"%s\t%d/%d\t" % (rid, matched, length) + _tail(occ, pos)


def mem_line(rid, start, end, occ, pos):
    """`id <TAB> start <TAB> end <TAB> occ <TAB> listed <TAB> p,p,... <LF>`."""
    return b"%s\t%d\t%d\t" % (rid, start, end) + _tail(occ, pos)
