"""rlbwt_ref.py -- TEST INFRASTRUCTURE: oracle/build_index.py build_rows restated on runs instead of characters.

build_rows_rl(heads, lens, thr, mode) returns the dict build_rows(bwt, thr, mode) returns for the expanded text, so that
B.serialize() writes it -- without ever holding the text, and without a Python loop over rows: a table that describes 2^33
characters is a few thousand runs and a few million rows.  Everything is int64 numpy.  It restates build_rows and, through it, the
reference's src/move_structure_build.cpp (line numbers as in oracle/build_index.py); it shares nothing with the GPU builder.
tests/test_rlbwt_ref_cpu.py holds it to build_rows byte for byte on every text small enough for build_rows.

big_table(n_target, separators) makes the run-length tables of texts of 2^31, 2^32 and 2^33 characters that
tests/test_build_big_text_gpu.py builds on the GPU; test_rlbwt_ref_cpu.py pins what they must contain."""
import functools
import os

import numpy as np

from conftest import GOLDEN
from oracle import build_index as B


def build_rows_rl(heads, lens, thr, mode):
    assert mode in (2, 3, 5, 6, 7, 8)
    heads = np.asarray(heads, np.uint8)
    run_len = np.asarray(lens).astype(np.int64)
    original_r = heads.size
    assert run_len.size == original_r and (run_len > 0).all() and (heads[1:] != heads[:-1]).all()
    maxrun = B.MAX_RUN[mode]
    with_thr = mode in B.THRESHOLD_MODES
    # --- detect_move_row_boundaries (:328-396): the hard boundaries are the run starts, and with thresholds every distinct
    # threshold below n (fill_bits_by_thresholds :733-746; a threshold of n sets the bit behind the text: no split)
    run_start = np.cumsum(run_len) - run_len
    n = int(run_len.sum())
    if with_thr:
        thr = np.asarray(thr).astype(np.int64)
        assert thr.size == original_r and thr.min() >= 0 and thr.max() <= n
        seg = np.union1d(run_start, thr[thr < n])
    else:
        seg = run_start
    seg_len = np.diff(np.concatenate((seg, [n])))
    # pieces of MAX_RUN_LENGTH (:380-385)
    pieces = (seg_len + maxrun - 1) // maxrun
    row_seg = np.repeat(np.arange(seg.size), pieces)
    first_of_seg = np.cumsum(pieces) - pieces
    all_p = seg[row_seg] + (np.arange(row_seg.size) - first_of_seg[row_seg]) * maxrun
    del row_seg
    r = all_p.size
    row_len = np.diff(np.concatenate((all_p, [n])))
    row_run = np.searchsorted(run_start, all_p, side="right") - 1
    row_head = heads[row_run]
    # --- build_alphabet (:428-447): exact integer sums of the runs' lengths
    alphamap = np.full(256, 256, np.uint64)
    alphabet, counts = [], []
    for ch in range(1, 256):
        cnt = int(run_len[heads == ch].sum())
        if cnt:
            alphamap[ch] = len(alphabet)
            alphabet.append(ch)
            counts.append(cnt)
    sigma = len(alphabet)
    sep = 1 if (sigma == 5 and alphabet[0] == B.SEPARATOR) else 0
    assert 1 <= sigma <= 4 or sep
    assert int(run_len[heads == 0].sum()) == 1, "exactly one terminator"
    code = alphamap[row_head].astype(np.int64)
    code[row_head == 0] = 0
    end_bwt_idx = int(np.flatnonzero(row_head == 0)[0])
    is_end = np.arange(r) == end_bwt_idx
    # --- find_run_heads_information (:74-121) + LF_heads
    C = 1 + np.cumsum(counts) - np.asarray(counts, np.int64)
    lf = np.zeros(r, np.int64)
    for a in range(sigma):
        m = (code == a) & ~is_end
        cl = np.where(m, row_len, 0)
        lf[m] = C[a] + (np.cumsum(cl) - cl)[m]
    # --- build_move_rows (:449-692)
    pp_id = np.searchsorted(all_p, lf, side="right") - 1
    offset = lf - all_p[pp_id]
    assert offset.max() <= maxrun and row_len.max() <= maxrun
    # --- find_base_interval_data (:694-731)
    first_runs, first_offsets, last_runs, last_offsets = [0], [0], [0], [0]
    char_count = 1
    for a in range(sigma):
        lr, lo = last_runs[-1], last_offsets[-1]
        if lo + 1 >= row_len[lr]:
            first_runs.append(lr + 1); first_offsets.append(0)
        else:
            first_runs.append(lr); first_offsets.append(lo + 1)
        char_count += counts[a]
        occ_rank = int(np.searchsorted(all_p, char_count, side="left"))
        last_runs.append(occ_rank - 1)
        last_offsets.append(char_count - int(all_p[occ_rank - 1]) - 1)
    # --- compute_thresholds (:807-935).  The walk goes from the last row up to row 1 and remembers, per character, the threshold of
    # the run it saw last: for a row and a character j other than its own that is the run of the nearest row below with code j
    # (the terminator's row counts as code 0), and n when there is none.
    thr_bits = np.zeros((r, 3), np.int64)
    end_thr = [0, 0, 0, 0]
    sep_thr, sep_map = [], {}
    if with_thr:
        walked = np.arange(r) >= 1                               # row 0 is not walked
        of_sep = (code == 0) if sep else np.zeros(r, bool)       # the rows of '%', and the terminator's
        sep_rows = np.flatnonzero(of_sep & walked)[::-1]         # descending, as the walk appends them
        sep_vals = np.zeros((sep_rows.size, 4), np.int64)
        plain = walked & ~is_end & ~of_sep
        for j in range(sep, sigma):                              # no threshold is kept for the separator (:849-852)
            of_j = np.flatnonzero(code == j)
            below = np.searchsorted(of_j, np.arange(r), side="right")
            found = below < of_j.size
            cur = np.full(r, n, np.int64)
            cur[found] = thr[row_run[of_j[below[found]]]]
            val = np.clip(cur - all_p, 0, row_len)               # len when cur >= p + len, 0 when cur <= p, cur - p inside the row
            if end_bwt_idx >= 1 and j != 0:                      # (the terminator's own code is 0)
                end_thr[j - sep] = int(val[end_bwt_idx])
            if sep:
                sep_vals[:, j - 1] = np.where(sep_rows == end_bwt_idx, 0, val[sep_rows])   # the terminator's own entry stays zero
            rows = np.flatnonzero(plain & (code != j))
            assert ((val[rows] == 0) | (val[rows] == row_len[rows])).all(), "threshold strictly inside a row: rows must be split at thresholds"
            thr_bits[rows, B.ALPHAMAP_3[code[rows] - sep, j - sep]] = val[rows] != 0
        if sep:
            sep_thr = sep_vals.tolist()
            sep_map = {int(i): k for k, i in enumerate(sep_rows.tolist())}
            if code[0] == 0:                                     # :917-920
                sep_map[0] = len(sep_thr)
                sep_thr.append([0, 0, 0, 0])
    out = dict(mode=mode, n=n, r=r, original_r=original_r, end_bwt_idx=end_bwt_idx,
               alphamap=alphamap, alphabet=bytes(alphabet), counts=counts,
               first_runs=first_runs, first_offsets=first_offsets,
               last_runs=last_runs, last_offsets=last_offsets, end_thr=end_thr,
               lens=row_len, offset=offset, code=code, pp_id=pp_id, thr_bits=thr_bits, all_p=all_p,
               sep=sep, sep_thr=sep_thr, sep_map=sep_map, lf=lf, run_start=run_start)
    if mode in (8, 2):
        out.update(B.compute_blocked_ids(pp_id, code, end_bwt_idx, first_runs, sigma, mode))
    if mode in (5, 7):
        out.update(tally_ids_rl(pp_id, code, end_bwt_idx, sigma))
    return out


def tally_ids_rl(pp_id, code, end_bwt_idx, sigma, checkpoints=B.TALLY_CHECKPOINTS):
    """compute_tally_ids without the walk: at checkpoint row i the id of the latest row <= i of each character (the terminator's row is
    no row of any), the id of the character's first row where there is none yet, and the final ids in one extra last entry.  With r a
    multiple of the distance the entry before the last is filled by nothing and stays 0."""
    r = pp_id.size
    n_ck = r // checkpoints + 2
    tally = np.zeros((sigma, n_ck), np.int64)
    at = np.arange(0, r, checkpoints)
    not_end = np.arange(r) != end_bwt_idx
    for a in range(sigma):
        of_a = np.flatnonzero((code == a) & not_end)
        if of_a.size == 0:
            tally[a, :at.size] = r
            tally[a, n_ck - 1] = r
            continue
        k = np.searchsorted(of_a, at, side="right")
        tally[a, :at.size] = pp_id[of_a[np.maximum(k - 1, 0)]]
        tally[a, n_ck - 1] = pp_id[of_a[-1]]
    return dict(tally_ids=tally, tally_checkpoints=checkpoints)


def rle(bwt):
    """(heads, lens) of the maximal runs of a uint8 array."""
    bwt = np.asarray(bwt, np.uint8)
    starts = np.flatnonzero(np.concatenate(([True], bwt[1:] != bwt[:-1])))
    return bwt[starts], np.diff(np.concatenate((starts, [bwt.size]))).astype(np.int64)


BIG_RUNS = 6000
BIG_N = {"2^31": (1 << 31) + 54321, "2^32": (1 << 32) + 54321, "2^33": (1 << 33) + 777}     # the big tables' text lengths


@functools.lru_cache(maxsize=None)
def _golden_runs(separators):
    ref = B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]
    return rle(B.bwt_and_thresholds(B.clean_text([ref], separators=separators))[0])


@functools.lru_cache(maxsize=None)
def big_table(n_target, separators=False):
    """(heads uint8, lens int64, thr int64, edge) of a text of n_target characters: the first 6000 maximal runs of the golden BWT, one
    terminator run of length 1 put between two of them, and all the rest of the text in one run of A near the top: the first before
    which every letter has a run (the second run of A; with a giant run of millions of rows above the first row of some letter, every
    backward-search step for that letter from the whole text scans all of them, in the oracle as on the GPU).  All rows but a few lie
    behind that run, past `edge` (2^31 for the smallest table, 2^32 for the others), and the C / G / T rows' LF targets lie there
    too.  A quarter of the thresholds are uniform over [0, n] -- almost all of those fall into the giant run -- a quarter uniform over
    what lies behind it, half are positions behind it where no run starts (a split there is a row boundary that only the thresholds
    make), and ten are set to the values either side of the edge, of n and of the giant run's ends.  The same table on every call:
    nobody writes to it."""
    gh, gl = _golden_runs(separators)
    k = BIG_RUNS // 2
    assert not (gh[:BIG_RUNS] == 0).any()
    heads = np.concatenate((gh[:k], [0], gh[k:BIG_RUNS])).astype(np.uint8)
    lens = np.concatenate((gl[:k], [1], gl[k:BIG_RUNS])).astype(np.int64)
    letters = set(heads.tolist()) - {0}
    giant = next(k for k in np.flatnonzero(heads == ord("A")).tolist() if set(heads[:k].tolist()) >= letters)
    lens[giant] += n_target - int(lens.sum())
    n = int(lens.sum())
    edge = (1 << 31) if n_target < (1 << 32) else (1 << 32)
    start = np.cumsum(lens) - lens
    behind = int(start[giant] + lens[giant])
    assert n == n_target and behind > edge + 1
    rng = np.random.default_rng(n_target % 1000003 + int(separators))
    R = heads.size
    inside = np.setdiff1d(np.arange(behind, n), start)           # behind the giant run, and no run's start
    thr = inside[rng.integers(0, inside.size, R)]
    kind = rng.integers(0, 4, R)
    thr[kind == 0] = rng.integers(0, n + 1, int((kind == 0).sum()))
    thr[kind == 1] = rng.integers(behind, n + 1, int((kind == 1).sum()))
    at = rng.choice(R, 10, replace=False)
    thr[at] = [edge - 1, edge, edge + 1, n - 1, n, 0, behind, behind - 1, behind + 1, int(start[giant])]
    for a in (heads, lens, thr):
        a.setflags(write=False)
    return heads, lens, thr, edge


@functools.lru_cache(maxsize=None)
def big_fields(n_target, separators, mode):
    """(build_rows_rl fields, image) of big_table(n_target, separators) in `mode`, computed once per process."""
    heads, lens, thr, _ = big_table(n_target, separators)
    f = build_rows_rl(heads, lens, thr, mode)
    return f, B.serialize(f)
