"""CPU suite: the chain rows' field map, the rule that says which look-ahead entries are valid, and the builder's hint rule for windows of
two rows (movi_amd/csrc/movi_chain_fields.hpp) through tests/host/chain_fields_driver.cpp, a stand-alone program compiled with
-fsanitize=address,undefined and run directly: what chain_rows_kernel packs is what the walk's readers unpack, for every extreme of every
field and for random rows; an entry whose target is no row, or is the '$' row, or whose own id is no row, is invalid (c = 7, n = 0) and
so is everything behind it, at each depth; and chain_hint_of gives what the rule says at both edges of the table."""
import os
import subprocess

import numpy as np
import pytest

import deep_hint_texts as D
from conftest import ROOT

NOT_A_ROW = (1 << 28) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chainfields") / "chain_fields_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "chain_fields_driver.cpp")])
    return exe


def test_round_trip_of_every_field_at_its_extremes(driver):
    out = subprocess.run([driver, "roundtrip", "20261", "200000"], capture_output=True, check=True).stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) == 6 * (6 * 4 * 4 * 4 * 4) + 200000


def _fields(driver, rows, end_row):
    feed = "%d %d\n" % (len(rows), end_row) + "".join("%d %d %d %d %d\n" % tuple(w) for w in rows)
    out = subprocess.run([driver, "fields"], input=feed.encode(), capture_output=True, check=True).stdout.decode()
    got = []
    for ln in out.splitlines():
        g = [[int(x) for x in part.split()] for part in ln.split("|")]
        got.append(dict(j=g[0], c=g[1][0], n=g[1][1], off=g[1][2], thr=g[1][3], e=[tuple(g[2]), tuple(g[3]), tuple(g[4])], nj4=g[5][0]))
    return got


def _rule(rows, end_row, i):
    """The header's rule restated: ids, entries (c, n, off) of j1 .. j3 and n(j4)."""
    r = len(rows)
    j, e, nj4, ok, at = [NOT_A_ROW] * 4, [(7, 0, 0)] * 3, 0, True, rows[i][0]
    for t in range(4):
        if at >= r:
            break
        j[t] = at
        nid, n, off, c, _ = rows[at]
        ok = ok and at != end_row
        if t == 3:
            nj4 = n if ok else 0
            break
        ok = ok and nid < r
        if ok:
            e[t] = (c, n, off)
        at = nid
    return j, e, nj4


def test_invalid_entries_at_each_depth(driver):
    """A ring of 11 rows i -> i + 1 (odd r: the last window is padded); then one id at a time is made "no row" -- r, the 28-bit
    all-ones value, 2^32 - 1 and 2^28 + 5, which cut to 28 bits would be row 5 -- and the '$' row is put at every place of the ring."""
    r = 11
    base = [[(i + 1) % r, 2 + i, 1 + i, i % 4, i % 8] for i in range(r)]
    got = _fields(driver, base, r)                              # (no '$' row among the rows)
    assert len(got) == 12
    for i in range(r):
        assert got[i]["j"] == [(i + d) % r for d in (1, 2, 3, 4)]
        assert got[i]["e"] == [((i + d) % r % 4, 2 + (i + d) % r, 1 + (i + d) % r) for d in (1, 2, 3)]
        assert (got[i]["c"], got[i]["n"], got[i]["off"], got[i]["thr"], got[i]["nj4"]) == (i % 4, 2 + i, 1 + i, i % 8, 2 + (i + 4) % r)
    assert got[11] == dict(j=[NOT_A_ROW] * 4, c=7, n=0, off=0, thr=0, e=[(7, 0, 0)] * 3, nj4=0)        # the padding row
    for bad_id in (r, NOT_A_ROW, 0xFFFFFFFF, (1 << 28) + 5):
        rows = [list(w) for w in base]
        rows[6][0] = bad_id                                     # row 6 points nowhere
        got = _fields(driver, rows, r)
        for i in range(r):
            assert (got[i]["j"], got[i]["e"], got[i]["nj4"]) == _rule(rows, r, i), (bad_id, i)
        assert got[6]["j"] == [NOT_A_ROW] * 4 and got[6]["e"] == [(7, 0, 0)] * 3 and got[6]["nj4"] == 0          # depth 0: no LF target
        assert got[5]["j"] == [6] + [NOT_A_ROW] * 3 and got[5]["e"] == [(7, 0, 0)] * 3                            # depth 1: j1's id is no row
        assert got[4]["j"] == [5, 6] + [NOT_A_ROW] * 2 and got[4]["e"][0] == (1, 7, 6) and got[4]["e"][1:] == [(7, 0, 0)] * 2
        assert got[3]["j"] == [4, 5, 6, NOT_A_ROW] and got[3]["e"][:2] == [(0, 6, 5), (1, 7, 6)] and got[3]["e"][2] == (7, 0, 0) and got[3]["nj4"] == 0
        assert got[2]["j"] == [3, 4, 5, 6] and got[2]["e"] == [(3, 5, 4), (0, 6, 5), (1, 7, 6)] and got[2]["nj4"] == 8   # n(j4) is known: row 6 is a row
    for end in range(r):                                        # the '$' row at each depth: the entry is invalid, and everything behind it
        got = _fields(driver, base, end)
        for i in range(r):
            j, e, nj4 = _rule(base, end, i)
            assert (got[i]["j"], got[i]["e"], got[i]["nj4"]) == (j, e, nj4), (end, i)
            depth = (end - i) % r                               # the '$' row is j<depth> of row i
            assert got[i]["j"] == [(i + d) % r for d in (1, 2, 3, 4)]          # ids are ids: the row behind '$' is still a row
            for d in (1, 2, 3):
                assert (got[i]["e"][d - 1] == (7, 0, 0)) == (1 <= depth <= d), (end, i, d)
            assert (got[i]["nj4"] == 0) == (1 <= depth <= 4), (end, i)


def _beyond_edge2(codes, i, a, down):
    r, wb = len(codes), i & ~1
    rng = range(i + 1, r) if down else range(i - 1, -1, -1)
    for t in rng:
        if codes[t] == a:
            return max(0, t - (wb + 1)) if down else max(0, wb - t)
    return None


@pytest.mark.parametrize("period,periods", [(19, 12), (38, 8), (7, 2), (4, 2), (5, 1)])
def test_hint_rule_for_windows_of_two_rows(driver, period, periods):
    """deep_hint_texts' run sequences: targets 1 .. 15 rows beyond a two-row window's edge are hinted, 16 and more are not, in both
    directions; at both edges of the table (targets in the first window going up, in the last going down; rows r - 1 and 0 as targets)."""
    codes = D.run_heads(period, periods)
    up = D.choose_directions(codes, "any", seed=period)
    r = len(codes)
    feed = "%d\n%s\n%s\n" % (r, " ".join(map(str, codes)), "\n".join(" ".join(map(str, row)) for row in up))
    seen = set()
    for reach in (15, 3):
        out = subprocess.run([driver, "hints", str(reach)], input=feed.encode(), capture_output=True, check=True).stdout.decode()
        got = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
        assert len(got) == r
        for i in range(r):
            c = int(codes[i])
            for k in range(3):
                a = D.slot_letter(c, k)
                if c == D.END or a > 3:
                    assert got[i][k] == 0
                    continue
                down = up[i, k] == 0
                e = _beyond_edge2(codes, i, a, down)
                want = e if e is not None and 1 <= e <= reach else 0
                assert got[i][k] == want, (period, reach, i, k, e)
                if want and reach == 15:
                    wb = i & ~1
                    t = wb + 1 + want if down else wb - want
                    assert 0 <= t < r and codes[t] == a
                    seen.add(("first" if t < 2 else "last" if t >= ((r - 1) & ~1) else "mid", want))
                if e is not None and reach == 15:
                    seen.add(("dist", e))
    if period == 19:
        assert {("dist", 15), ("dist", 16), ("dist", 1)} <= seen
        assert any(w == "first" for w, _ in seen) and any(w == "last" for w, _ in seen)
