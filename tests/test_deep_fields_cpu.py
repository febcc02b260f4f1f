"""CPU suite: the deep rows' two field maps and the builder's hint rule (movi_amd/csrc/movi_deep_fields.hpp) through
tests/host/deep_fields_driver.cpp, compiled with -fsanitize=address,undefined: what deep_rows_kernel packs is what the walk's readers
unpack, for every extreme of every field and for random rows; tables of up to 2^26 - 1 rows take narrow ids when 4-bit hints are asked
for and every other table the wide ones; and deep_hint_of on the run sequences of tests/deep_hint_texts.py -- targets exactly 3, 4, 15
and 16 rows beyond a window's edge, in the first and the last window -- gives what the rule says, at reach 3 and at reach 15."""
import os
import subprocess

import pytest

import deep_hint_texts as D
from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deepfields") / "deep_fields_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "deep_fields_driver.cpp")])
    return exe


def test_round_trip_of_both_maps(driver):
    out = subprocess.run([driver, "roundtrip", "20261", "200000"], capture_output=True, check=True).stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) == 2 * (7 ** 3 * 5 * 4 + 200000)


def test_map_by_row_count(driver):
    cases = [(8, 4), (8, 2), (8, -1), ((1 << 26) - 2, 4), ((1 << 26) - 1, 4), (1 << 26, 4), ((1 << 26) + 1, 4), ((1 << 28) - 2, 4),
             ((1 << 26) - 1, 2), (1 << 26, 2)]
    out = subprocess.run([driver, "map"], input="".join("%d %d\n" % c for c in cases).encode(), capture_output=True, check=True).stdout.decode()
    got = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
    narrow, wide = (26, (1 << 26) - 1, 4, 6), (28, (1 << 28) - 1, 2, 2)
    want = [narrow if (bits == 4 and r <= (1 << 26) - 1) else wide for r, bits in cases]
    assert got == want
    assert got[4] == narrow and got[5] == wide               # the last table with narrow ids, the first without
    for id_bits, id_mask, hint_bits, j3_shift in (narrow, wide):
        assert id_mask == (1 << id_bits) - 1 and j3_shift == 3 * hint_bits - (32 - id_bits) and 3 * hint_bits + id_bits <= 32 + j3_shift


@pytest.mark.parametrize("period,periods,rule", [(19, 12, "any"), (38, 8, "avoid_4_15"), (7, 2, "any"), (4, 2, "any")])
def test_hint_rule_on_the_constructed_tables(driver, period, periods, rule):
    codes = D.run_heads(period, periods)
    up = D.choose_directions(codes, rule, seed=period)
    dist = D.distances(codes, up)
    r = len(codes)
    if period == 19:
        last_win = (r - 1) // 3 * 3
        for way in ("up", "down"):
            for e in (3, 4, 15, 16):
                assert dist.get((way, e)), (way, e)
        far = [x for (way, e), v in dist.items() if 4 <= e <= 15 for x in v]
        assert any(t < 3 for _, _, t in far) and any(t >= last_win for _, _, t in far)
    if rule == "avoid_4_15":
        assert not any(4 <= e <= 15 for _, e in dist) and dist.get(("up", 16)) and dist.get(("down", 16))
    feed = "%d\n%s\n%s\n" % (r, " ".join(map(str, codes)), "\n".join(" ".join(map(str, row)) for row in up))
    for reach in (3, 15):
        out = subprocess.run([driver, "hints", str(reach)], input=feed.encode(), capture_output=True, check=True).stdout.decode()
        got = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
        assert len(got) == r
        for i in range(r):
            c = int(codes[i])
            for k in range(3):
                a = D.slot_letter(c, k)
                want = D.hint_of(codes, i, a, up[i, k] == 0, reach) if c != D.END and a <= 3 else 0
                assert got[i][k] == want, (reach, i, k, got[i], want)
                if got[i][k]:                                # never beyond the table, never past row 0 or row r - 1
                    wb = (i // 3) * 3
                    t = wb + 2 + got[i][k] if up[i, k] == 0 else wb - got[i][k]
                    assert 0 <= t <= r - 1 and codes[t] == a
    if rule == "avoid_4_15":                                 # a table on which 4-bit hints say nothing that 2-bit hints do not
        assert all(D.hint_of(codes, i, D.slot_letter(int(codes[i]), k), up[i, k] == 0, 15) ==
                   D.hint_of(codes, i, D.slot_letter(int(codes[i]), k), up[i, k] == 0, 3)
                   for i in range(r) if codes[i] != D.END for k in range(3) if D.slot_letter(int(codes[i]), k) <= 3)
