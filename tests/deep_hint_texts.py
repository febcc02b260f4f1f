"""Run sequences for the tests of the deep rows' reposition hints (tests/test_deep_hints_gpu.py, tests/test_deep_fields_cpu.py), and the
builder's hint rule restated in Python.

A table here is a run-length BWT given run by run (one row per run): A and C alternate, and every `period` rows a G and a T take two rows'
place, so that from the rows in between the nearest G or T lies any number of rows beyond the window's edge from 1 up to period - 3, in
either direction, and the two directions' distances add up to period - 2 or so.  The terminator sits in the middle, where every letter has runs on both sides.  The direction of a row's scan for a letter is
the row's threshold bit, which the tests set themselves (`choose_directions`), so that a table holds exactly the distances a case is about.
`end`: the terminator's row where the codes come from a built table (its row has a letter code of its own there and takes no hints).
"""
import numpy as np

A, C, G, T, END = 0, 1, 2, 3, 4
LETTER = {A: ord("A"), C: ord("C"), G: ord("G"), T: ord("T"), END: 0}


def run_heads(period, periods):
    """Codes of the rows: G at rows 1 + k * period, T at the row behind each, the terminator in the middle, A / C alternating elsewhere.
    r = period * periods + 3: a G and a T in the first window and in the last (rows r - 2, r - 1); period must be no multiple of 3, so that
    the windows' edges take every place between two Gs."""
    assert period % 3 != 0
    r = period * periods + 3
    out, ac = [], 0
    for t in range(r):
        if t % period == 1:
            out.append(G)
        elif t % period == 2:
            out.append(T)
        else:
            out.append(A if ac % 2 == 0 else C)
            ac += 1
    mid = (r // 2) // 3 * 3 + 1
    while out[mid] in (G, T):
        mid += 1
    out[mid] = END
    return np.array(out, np.int64)


def slot_letter(c, k):
    """The letter whose threshold slot of a row of letter c is k (alphamap_3: a - (a > c))."""
    return k if k < c else k + 1


def beyond_edge(codes, i, a, down):
    """Rows beyond the edge of row i's three-row window at which the nearest row of letter a lies in the direction given:
    0 = inside the window, None = nowhere."""
    r, wb = len(codes), (i // 3) * 3
    if down:
        for t in range(i + 1, r):
            if codes[t] == a:
                return max(0, t - (wb + 2))
    else:
        for t in range(i - 1, -1, -1):
            if codes[t] == a:
                return max(0, wb - t)
    return None


def hint_of(codes, i, a, down, reach):
    """deep_hint_of (movi_deep_fields.hpp) restated: 1 .. reach, or 0 = inside the window, further, or nowhere."""
    d = beyond_edge(codes, i, a, down)
    return d if d is not None and 1 <= d <= reach else 0


def choose_directions(codes, rule, seed=1, end=None):
    """Per row and threshold slot: 1 = the scan goes up (threshold bit set), 0 = down.  Only directions in which the letter has a run are
    chosen, so no scan fails.  rule "any": at random; "avoid_4_15": a direction whose distance beyond the edge is not 4 .. 15 (in the
    window, up to 3, or 16 and more) -- a table on which 4-bit hints say nothing that 2-bit hints do not."""
    rng = np.random.default_rng(seed)
    r = len(codes)
    up = np.zeros((r, 3), np.int64)
    for i in range(r):
        c = int(codes[i])
        if c == END or i == end:
            continue
        for k in range(3):
            a = slot_letter(c, k)
            if a > 3:
                continue
            opts = [(d, beyond_edge(codes, i, a, d)) for d in (True, False)]
            opts = [(d, e) for d, e in opts if e is not None]
            assert opts, (i, a)
            if rule == "avoid_4_15":
                good = [(d, e) for d, e in opts if not 4 <= e <= 15]
                assert good, (i, a, opts)
                opts = good
            down = opts[int(rng.integers(0, len(opts)))][0]
            up[i, k] = 0 if down else 1
    return up


def distances(codes, up, end=None):
    """{(direction, distance beyond the edge): [(row, slot, target row)]} over every row and slot, in the direction its bit gives."""
    out = {}
    for i in range(len(codes)):
        c = int(codes[i])
        if c == END or i == end:
            continue
        for k in range(3):
            a = slot_letter(c, k)
            if a > 3:
                continue
            down = up[i, k] == 0
            e = beyond_edge(codes, i, a, down)
            if e:
                wb = (i // 3) * 3
                out.setdefault(("down" if down else "up", e), []).append((i, k, wb + 2 + e if down else wb - e))
    return out
