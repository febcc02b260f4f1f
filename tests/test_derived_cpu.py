"""CPU suite: which derived tables a handle holds (movi_amd/csrc/movi_derived.hpp: ensure_pml_tables, ensure_count_tables,
request_table, on_prepare) through tests/host/derived_driver.cpp, compiled with -fsanitize=address,undefined, on a scripted device.
tests/golden/derived_table.txt varies one input at a time around the golden index on an idle MI355X and crosses what interacts; beside
every case it holds what movi_abi.hip did BEFORE the rules moved into the header -- in five places, between its HIP calls
(tools/derived_cases.py writes the table and says how it was recorded) -- so a table that is built, dropped, declined, retried or given
up at another moment for these inputs shows here, without a GPU and without starving one of memory."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

TABLE = open(os.path.join(GOLDEN, "derived_table.txt")).read().splitlines()
FIELDS = TABLE[0].split()[1:]
DEFAULTS = dict(zip(FIELDS, TABLE[1].split()[1:]))
GIB = 1 << 30
HELD = "kmer ftab ahead deep ckpt rows2_count deep_width".split()
POLICY = "kmer_auto ftab_auto ahead_auto deep_auto deep_hint_bits ahead_retry_in count_declined_ahead ahead_tallied ahead_no_ff prepared".split()
CV0 = "S count_variant 0 "


def feed(script, **kw):
    assert set(kw) <= set(FIELDS), kw
    return " ".join(str(dict(DEFAULTS, **kw)[f]) for f in FIELDS) + " : " + script + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("derived") / "derived_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "derived_driver.cpp")])
    return exe


def parse(line):
    """A driver line: ([(step, device call)], what the handle holds by name, the policy's fields by name)."""
    trace, held, policy = line.split(" | ")
    calls = []
    for t in [] if trace == "-" else trace.split():              # "1:drop ahead 2:kmer 12" -> (1, "drop_ahead"), (2, "kmer_12")
        if ":" in t:
            calls.append((int(t.split(":")[0]), t.split(":")[1]))
        else:
            calls[-1] = (calls[-1][0], calls[-1][1] + "_" + t)
    h, p = held.split(), policy.split()
    assert h[0] == "held" and p[0] == "policy" and len(h) == 1 + len(HELD) and len(p) == 1 + len(POLICY), line
    return calls, dict(zip(HELD, map(int, h[1:]))), dict(zip(POLICY, [float(x) if "." in x else int(x) for x in p[1:]]))


def run(driver, script, **kw):
    return parse(subprocess.run([driver], input=feed(script, **kw).encode(), capture_output=True, check=True).stdout.decode().strip())


def names(calls):
    return [c for _, c in calls]


def test_rules_equal_the_recorded_decisions(driver):
    rows = [ln.split(" => ") for ln in TABLE[2:]]
    cases = [(dict(kv.split("=") for kv in left.split(":")[0].split()), left.split(":")[1].strip()) for left, _ in rows]
    got = subprocess.run([driver], input="".join(feed(s, **c) for c, s in cases).encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(rows) >= 600 and len(got) == len(rows)
    bad = [(left, g, want) for (left, want), g in zip(rows, got) if g != want]
    assert not bad, (len(bad), bad[:3])


def test_the_table_names_both_outcomes_of_every_branch():
    rec = [(dict(DEFAULTS, **dict(kv.split("=") for kv in left.split(":")[0].split())), left.split(":")[1].strip()) + parse(want)
           for left, want in (ln.split(" => ") for ln in TABLE[2:])]

    def some(pred):
        return any(pred(c, s, calls, held, pol) for c, s, calls, held, pol in rec)

    # eligibility: every value the rules tell apart, and every build-now option both built and refused
    assert {c["kmode"] for c, *_ in rec} == {"6", "3", "7"} and {c["dna"] for c, *_ in rec} == {"0", "1"}
    assert {7, 8, 48 << 20, (48 << 20) + 1, (1 << 28) - 2, (1 << 28) - 1, (1 << 26) - 1, 1 << 26} <= {int(c["r"]) for c, *_ in rec}
    for key, t in (("kmer_k", "kmer"), ("ftab_k", "ftab"), ("ahead_rows", "ahead"), ("deep_rows", "deep")):
        for want in (0, 1):
            assert some(lambda c, s, calls, held, pol: s.startswith("S " + key) and len(s.split()) == 3 and s.split()[2] != "0" and held[t] == want and
                        ("refused" in names(calls)) == (want == 0) and c["fail_mask"] == "0"), (key, want)
    # the deep rows by themselves: up to kDeepAutoRows rows and no further; the statistic at 0.67 and just below it
    assert some(lambda c, s, calls, held, pol: s == "P" and int(c["r"]) == 48 << 20 and held["deep"] == 1)
    assert some(lambda c, s, calls, held, pol: s == "P" and int(c["r"]) == (48 << 20) + 1 and held["deep"] == 0 and pol["deep_auto"] == 1)
    for full, want in (("0.67", 1), ("0.6699", 0)):
        assert some(lambda c, s, calls, held, pol: s == "P" and c["full"] == full and held["deep"] == want and pol["deep_auto"] == want and held["ahead"] == 1)
    # ... and for the count query's copy: declined by the sample (nothing built), built and dropped (the sample above, every row below), kept
    assert some(lambda c, s, calls, held, pol: s == CV0 + "C" and c["sample"] == "0.6699" and "ahead_auto" not in names(calls) and pol["count_declined_ahead"] == 1)
    assert some(lambda c, s, calls, held, pol: s == CV0 + "C" and (c["sample"], c["full"]) == ("0.67", "0.6699") and names(calls)[-2:] == ["ahead_auto", "drop_ahead"] and
                pol["count_declined_ahead"] == 1 and held["ahead"] == 0)
    assert some(lambda c, s, calls, held, pol: s == CV0 + "C P" and (c["sample"], c["full"]) == ("0.67", "0.6699") and names(calls).count("ahead_auto") == 2 and held["ahead"] == 1 and
                held["rows2_count"] == 0)
    assert some(lambda c, s, calls, held, pol: s == CV0 + "C" and (c["sample"], c["full"]) == ("0.6699", "0.67") and pol["count_declined_ahead"] == 1)
    assert some(lambda c, s, calls, held, pol: s == CV0 + "C" and (c["sample"], c["full"]) == ("0.67", "0.67") and held["ahead"] == 1 and held["rows2_count"] == 1 and
                pol["count_declined_ahead"] == 0)
    # room for the look-ahead rows, either side of both bounds, on both paths; room for the deep rows; the memory query failing
    for script in ("P", CV0 + "C"):
        for want in (0, 1):
            assert some(lambda c, s, calls, held, pol: s == script and c["total"] != DEFAULTS["total"] and c["r"] != DEFAULTS["r"] and held["ahead"] == want and
                        pol["ahead_retry_in"] == (0 if want else 63)), (script, want)
            assert some(lambda c, s, calls, held, pol: s == script and c["free"] != DEFAULTS["free"] and c["r"] != DEFAULTS["r"] and held["ahead"] == want and
                        pol["ahead_retry_in"] == (0 if want else 63)), (script, want)
    for want in (0, 1):
        assert some(lambda c, s, calls, held, pol: s == "P" and c["free"] != DEFAULTS["free"] and held["ahead"] == 1 and held["deep"] == want and pol["deep_auto"] == want), want
    assert some(lambda c, s, calls, held, pol: s == "P x3" and c["mem_fails"] == "1" and names(calls) == ["kmer_12", "mem", "sample", "mem"] and held["ahead"] == held["deep"] == 0 and
                (pol["ahead_auto"], pol["deep_auto"], pol["ahead_retry_in"]) == (1, 0, 61))
    # declined for lack of memory: asked at calls 1 and 65 and at no other, on either path and on both in turn; a prepare asks at once
    # (the count path's calls are steps 2 .. 67 behind the option; on real text the first PML query asks a second time, for the deep rows;
    # P, 32 x C, P: one question and 33 calls counted down from 63)
    for script, sample, asked, left in (("P x66", "0.51", [1, 65], 62), (CV0 + "C x66", "0.83", [2, 66], 62), (CV0 + "P C x32 P", "0.83", [2, 2], 30)):
        assert some(lambda c, s, calls, held, pol: s == script and c["free"] == str(GIB) and c["sample"] == sample and
                    [st for st, call in calls if call == "mem"] == asked and pol["ahead_retry_in"] == left), script
    assert some(lambda c, s, calls, held, pol: s == "P x10 Rp P x10" and c["free"] == str(GIB) and c["sample"] == "0.51" and [st for st, call in calls if call == "mem"] == [1, 11])
    # (... and any prepare ends the queries' asking: a count-only one resets the counter, and the PML queries behind it leave it at 0)
    assert some(lambda c, s, calls, held, pol: s == "P x10 Rc P x60" and c["free"] == str(GIB) and c["sample"] == "0.51" and [st for st, call in calls if call == "mem"] == [1] and
                (pol["ahead_retry_in"], pol["prepared"]) == (0, 1))
    # each build failing: one attempt, its auto-build off for good (the checkpoints have none: every call fails)
    for mask, script, call, auto in (("1", "P x3", "kmer_12", "kmer_auto"), ("2", "C x3", "ftab_12", "ftab_auto"), ("4", "P x3", "ahead_auto", "ahead_auto"),
                                     ("8", "P x3", "deep_4", "deep_auto")):
        assert some(lambda c, s, calls, held, pol: s == script and c["fail_mask"] == mask and names(calls).count(call) == 1 and pol[auto] == 0), mask
        assert some(lambda c, s, calls, held, pol: s == script and c["fail_mask"] == "0" and names(calls).count(call) == 1 and pol[auto] != 0), mask
    assert some(lambda c, s, calls, held, pol: s == "C x3" and c["fail_mask"] == "16" and names(calls) == ["ckpt", "failed"] * 3 and held["ftab"] == 0)
    assert some(lambda c, s, calls, held, pol: s == "Rpc Rpc" and c["fail_mask"] == "16" and pol["prepared"] == 0)
    # the sample failing: the next count query samples again
    assert some(lambda c, s, calls, held, pol: s == CV0 + "C x3" and c["sample"] == "x" and [st for st, call in calls if call == "sample"] == [2, 3, 4] and pol["ahead_tallied"] == 0)
    # prepared: a query builds the two lookup tables still, never a row copy; a second prepare builds nothing more
    assert some(lambda c, s, calls, held, pol: s == "Rc P" and c == DEFAULTS and (held["kmer"], held["ftab"], held["ckpt"], held["ahead"], held["deep"]) == (1, 1, 1, 0, 0))
    assert some(lambda c, s, calls, held, pol: s == "Rp C" and c == DEFAULTS and (held["kmer"], held["ftab"], held["ckpt"], held["ahead"], held["deep"]) == (1, 1, 1, 1, 1))
    assert some(lambda c, s, calls, held, pol: s == "Rpc Rpc" and c == DEFAULTS and {st for st, _ in calls} == {1})
    assert some(lambda c, s, calls, held, pol: s == "Rp F %d P Rp" % (200 * GIB) and c["sample"] == "0.51" and [st for st, call in calls if call == "ahead_auto"] == [4])
    # "ahead_rows" either way takes the deep rows along; "deep_rows" 1 brings them back; the hint width is the next build's
    for v in (0, 1):
        assert some(lambda c, s, calls, held, pol: s == "P S ahead_rows %d P" % v and c == DEFAULTS and "drop_deep" in names(calls) and
                    (held["ahead"], held["deep"], pol["ahead_auto"], pol["deep_auto"]) == (v, 0, 0, 0))
    assert some(lambda c, s, calls, held, pol: s == "S ahead_rows 0 P S deep_rows 1 P" and c == DEFAULTS and (held["ahead"], held["deep"]) == (0, 1))
    for r, bits, want in ((118209, 2, 2), (118209, 4, 4), (118209, -1, 4), ((1 << 26) - 1, 4, 4), (1 << 26, 4, 2), (1 << 26, -1, 2), ((1 << 28) - 2, 2, 2)):
        assert some(lambda c, s, calls, held, pol: s == "S deep_hint_bits %d S deep_rows 1" % bits and int(c["r"]) == r and held["deep_width"] == want and pol["deep_hint_bits"] == bits), (r, bits)
    assert some(lambda c, s, calls, held, pol: s == "P S deep_hint_bits 2 P S deep_rows 1" and c == DEFAULTS and [call for _, call in calls if call.startswith("deep_")] == ["deep_4", "deep_2"])


def test_decisions_by_hand(driver):
    # The golden index: 118209 rows of DNA in the thresholds layout, 288 GiB of device memory of which 200 GiB are free, a sample and a
    # builder's tally of 0.83.  Its look-ahead rows take ((118209 + 7) / 8 + 1) * 128 = 14778 * 128 = 1891584 bytes, its deep rows
    # (118209 + 2) / 3 * 64 = 39403 * 64 = 2521792.
    # First PML query: the top-of-walk table at K = 12; the device is asked once for the look-ahead rows (1891584 <= 72 GiB and
    # 200 GiB > 1891584 + 2 GiB), whose builder tallies 0.83 -- so no sample --; 0.83 >= 0.67 and 200 GiB >= 2521792 + 2 GiB: deep rows
    # with 4-bit hints (118209 <= 2^26 - 1).  The copy was built by itself and 0.83 >= 0.67: the count query may use it.
    calls, held, pol = run(driver, "P")
    assert calls == [(1, "kmer_12"), (1, "mem"), (1, "ahead_auto"), (1, "mem"), (1, "deep_4")]
    assert held == dict(kmer=1, ftab=0, ahead=1, deep=1, ckpt=0, rows2_count=1, deep_width=4)
    assert (pol["ahead_tallied"], pol["ahead_no_ff"], pol["prepared"], pol["ahead_retry_in"]) == (1, 0.83, 0, 0)
    # The same with free memory of exactly 1891584 + 2 GiB: not MORE than the copy and 2 GiB, so the look-ahead rows are declined and asked
    # for again in 63 calls' time; the deep rows sample (nothing has tallied), and 1891584 + 2 GiB < 2521792 + 2 GiB: no room, off for good.
    # The second query only counts down.
    calls, held, pol = run(driver, "P x2", free=1891584 + 2 * GIB)
    assert calls == [(1, "kmer_12"), (1, "mem"), (1, "sample"), (1, "mem")] and (held["ahead"], held["deep"]) == (0, 0)
    assert (pol["ahead_auto"], pol["deep_auto"], pol["ahead_retry_in"]) == (1, 0, 62)
    # One byte more and both fit?  The look-ahead rows do (free > 1891584 + 2 GiB); the deep rows need 2521792 + 2 GiB: still not.
    calls, held, pol = run(driver, "P", free=1891584 + 2 * GIB + 1)
    assert names(calls) == ["kmer_12", "mem", "ahead_auto", "mem"] and (held["ahead"], held["deep"], pol["deep_auto"]) == (1, 0, 0)
    # A count query under "count_variant" 0 on a random table whose sample happens to say 0.67: checkpoints, interval table, the sample, the
    # device, the copy -- whose own tally of every row says 0.51 < 0.67: dropped, and not built by a count query again.  The PML query
    # builds it again (for itself: rows2_count 0) and, 0.51 < 0.67, no deep rows.
    calls, held, pol = run(driver, CV0 + "C C P", sample="0.67", full="0.51")
    assert calls == [(2, "ckpt"), (2, "ftab_12"), (2, "sample"), (2, "mem"), (2, "ahead_auto"), (2, "drop_ahead"), (4, "kmer_12"), (4, "mem"), (4, "ahead_auto")]
    assert (held["ahead"], held["rows2_count"], held["deep"], pol["count_declined_ahead"], pol["deep_auto"], pol["ahead_no_ff"]) == (1, 0, 0, 1, 0, 0.51)
    # Prepared for count only, then a PML query: the 256 MB top-of-walk table is built inside the query, neither row copy is.
    calls, held, pol = run(driver, "Rc P")
    assert calls == [(1, "ckpt"), (1, "ftab_12"), (2, "kmer_12")] and (held["ahead"], held["deep"], pol["prepared"]) == (0, 0, 1)
    # "ahead_rows" 1 on a `regular` index (kmode 3): both copies dropped, both auto-builds off, refused; "ftab_k" 8 builds there.
    calls, held, pol = run(driver, "S ahead_rows 1 S ftab_k 8", kmode=3)
    assert calls == [(1, "drop_ahead"), (1, "drop_deep"), (1, "refused"), (2, "drop_ftab"), (2, "ftab_8")]
    assert (pol["ahead_auto"], pol["deep_auto"], pol["ftab_auto"], held["ftab"]) == (0, 0, 0, 1)
    # 2^26 rows: "deep_hint_bits" 4 is narrowed to 2 (wide ids); one row fewer takes 4
    assert run(driver, "S deep_hint_bits 4 S deep_rows 1", r=1 << 26)[1]["deep_width"] == 2
    assert run(driver, "S deep_hint_bits 4 S deep_rows 1", r=(1 << 26) - 1)[1]["deep_width"] == 4
