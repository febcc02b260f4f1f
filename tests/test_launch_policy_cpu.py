"""CPU suite: the launch policy (movi_amd/csrc/movi_launch_policy.hpp: plan_pml, plan_pml_seg, plan_zml, plan_count, call_seg_len, the
segment-eligibility predicates) through tests/host/launch_policy_driver.cpp.  tests/golden/launch_policy_table.txt varies one input at
a time around the defaults and crosses the options that interact; beside every case it holds what the launchers computed BEFORE the
policy moved into the header (recorded from that commit's plan_pml and from its launchers' own expressions;
tools/launch_policy_cases.py writes the table and says how), so a launch that changes kernel, block, dynamic LDS or staging for any of
these inputs shows here, without a GPU."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

TABLE = open(os.path.join(GOLDEN, "launch_policy_table.txt")).read().splitlines()
FIELDS = TABLE[0].split()[1:]                                     # the driver's 28 inputs ...
DEFAULTS = dict(zip(FIELDS, map(int, TABLE[1].split()[1:])))      # ... and the values a case leaves unsaid


def feed(**kw):
    assert set(kw) <= set(FIELDS), kw
    return " ".join(str(dict(DEFAULTS, **kw)[f]) for f in FIELDS) + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launchpolicy") / "launch_policy_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "launch_policy_driver.cpp")])
    return exe


def plans(driver, **kw):
    out = subprocess.run([driver], input=feed(**kw).encode(), capture_output=True, check=True).stdout
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.decode().splitlines()}


def test_plans_equal_the_recorded_launches(driver):
    assert len(FIELDS) == 28 and len(DEFAULTS) == 28
    rows = [ln.split(" => ") for ln in TABLE[2:]]
    cases = [{k: int(v) for k, v in (kv.split("=") for kv in left.split())} for left, _ in rows]
    got = subprocess.run([driver], input="".join(feed(**c) for c in cases).encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(rows) >= 400 and len(got) == 4 * len(rows)
    bad = [(left, " | ".join(got[4 * i:4 * i + 4]), want) for i, (left, want) in enumerate(rows) if " | ".join(got[4 * i:4 * i + 4]) != want]
    assert not bad, (len(bad), bad[:5])


def test_routes_equal_the_recorded_launches(driver):
    """tests/golden/launch_route_table.txt: the route of a PML call (plan_pml) -- where its results leave the walk, the scratch it needs,
    the parked lanes and their second grid, hint_w, ff_skip, the walk kernel's selectors -- beside what the launcher and the C ABI's four
    layers derived around the plan BEFORE the route moved into the header (tools/launch_policy_cases.py says how it was recorded, and
    marks the two columns the one planner changes on purpose)."""
    table = open(os.path.join(GOLDEN, "launch_route_table.txt")).read().splitlines()
    fields, defaults = table[0].split()[1:], [int(x) for x in table[1].split()[1:]]
    assert len(fields) == 36 and len(defaults) == 36 and fields[:28] == FIELDS
    rows = [ln.split(" => ") for ln in table[2:] if not ln.startswith("#")]
    cases = [dict(zip(fields, defaults), **{k: int(v) for k, v in (kv.split("=") for kv in left.split())}) for left, _ in rows]
    text = "".join(" ".join(str(c[f]) for f in fields) + "\n" for c in cases)
    got = subprocess.run([driver, "route"], input=text.encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(rows) >= 300 and len(got) == len(rows)
    assert {want.split()[1] for _, want in rows} == {"vector", "mask_native", "mask_from_tmp", "vector_fused", "vector_expand", "invalid"}
    bad = [(left, g, want) for (left, want), g in zip(rows, got) if g != want]
    assert not bad, (len(bad), bad[:5])


def test_occupancy_caps_by_hand(driver):
    # A cap of bpc blocks per CU pads every block to dyn_lds + 1 KiB (static LDS and granule) so that bpc of them fill the CU's 160 KiB
    # and bpc + 1 do not; a lane stages dyn_lds / 64 bases, rounded down to 16.
    #   kCapWaves 7:       163840 / 7 = 23405 -> 22 KiB - 1 KiB = 21504 B, 336 bases
    #   kCapWavesAhead 9:  163840 / 9 = 18204 -> 17 KiB - 1 KiB = 16384 B, 256 bases
    #   kCapWavesDeep 13:  163840 / 13 = 12603 -> 12 KiB - 1 KiB = 11264 B, 176 bases
    plain = dict(rows2=0, hints=0, rows2_count=0, rows3=0)
    for tables, bpc, dyn, staged in ((plain, 7, 21504, 336), (dict(plain, rows2=1, hints=1), 9, 16384, 256),
                                     (dict(plain, rows2=1, hints=1, rows3=1), 13, 11264, 176)):
        v, bt, wpc, dyn_lds, stage_lds = plans(driver, **tables)["pml"][:5]
        assert (v, bt, wpc, dyn_lds, stage_lds) == (14, 64, bpc, dyn, staged), (tables, v, bt, wpc, dyn_lds, stage_lds)
        assert bpc * (dyn_lds + 1024) <= 163840 < (bpc + 1) * (dyn_lds + 1024)
        assert stage_lds == dyn_lds // 64 and stage_lds % 16 == 0
    # the ZML parse and the count query stage in kZmlStageBytes = 10 KiB of their own: 160 bases per lane
    p = plans(driver, **plain)
    assert p["zml"][:5] == [1, 64, 0, 10240, 160] and p["count"][:5] == [1, 64, 0, 10240, 160]
