"""CPU suite: the plan of a *_host call (movi_amd/csrc/movi_host_plan.hpp: plan_host_call, HostCall::settle, plan_chunks, the one
cutter) through tests/host/host_plan_driver.cpp.  tests/golden/host_plan_table.txt varies one input at a time around 1 M reads of 150
bases and crosses what interacts; beside every case it holds what movi_abi.hip decided BEFORE the plan moved into the header -- in five
places, three cutting loops among them (tools/host_plan_cases.py writes the table and says how it was recorded) -- so a call whose
route, overlap, page-locking, upload or any chunk boundary changes for these inputs shows here, without a GPU."""
import os
import random
import subprocess

import pytest

from conftest import GOLDEN, ROOT

TABLE = open(os.path.join(GOLDEN, "host_plan_table.txt")).read().splitlines()
FIELDS = TABLE[0].split()[1:]                                     # the driver's 22 inputs ...
DEFAULTS = dict(zip(FIELDS, map(int, TABLE[1].split()[1:])))      # ... and the values a case leaves unsaid
ML, LOGS, SA, PER_READ, MULTI, COMPACT = range(6)
CONST, ALT, ZERO_RUN, ONE_LONG, LCG = range(5)


def feed(**kw):
    assert set(kw) <= set(FIELDS), kw
    return " ".join(str(dict(DEFAULTS, **kw)[f]) for f in FIELDS) + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostplan") / "host_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "host_plan_driver.cpp")])
    return exe


CALL = "route overlapped pin_reads pin_vector demoted ahead quartered vector_down words_in_block small target min_reads".split()


def parse(line):
    """A driver line: (the call's decisions by name, the number of chunks, the chunks it prints as tuples, the hash)."""
    parts = line.split(" | ")
    w = parts[0].split()
    assert len(w) == len(CALL), line
    call = dict(zip(CALL, [w[0]] + [int(x) for x in w[1:]]))
    return call, int(parts[1]), [tuple(int(x) for x in p.split()) for p in parts[2:-1]], parts[-1]


def plan(driver, **kw):
    return parse(subprocess.run([driver], input=feed(**kw).encode(), capture_output=True, check=True).stdout.decode().strip())


def all_chunks(driver, cases):
    """Every chunk (first, nr, b0, nb, masks, phase) of every case."""
    out = subprocess.run([driver, "chunks"], input="".join(feed(**c) for c in cases).encode(), capture_output=True, check=True).stdout.decode()
    return [[tuple(int(x) for x in ln.split()) for ln in block.splitlines()] for block in out.split("\n\n")[:len(cases)]]


def test_plans_equal_the_recorded_calls(driver):
    assert len(FIELDS) == 22 and len(DEFAULTS) == 22
    rows = [ln.split(" => ") for ln in TABLE[2:]]
    cases = [{k: int(v) for k, v in (kv.split("=") for kv in left.split())} for left, _ in rows]
    got = subprocess.run([driver], input="".join(feed(**c) for c in cases).encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(rows) >= 400 and len(got) == len(rows)
    # the table names both values of every decision, every route, and the three floors of a chunk's reads
    calls = [parse(want)[0] for _, want in rows]
    for key in ("overlapped", "pin_reads", "pin_vector", "demoted", "ahead", "quartered", "vector_down", "words_in_block"):
        assert {c[key] for c in calls} == {0, 1}, key
    assert {c["route"] for c in calls} == {"vector", "masks", "mixed"}
    assert {c["min_reads"] for c in calls if c["overlapped"]} == {1 << 12, 1 << 15, 1}
    assert {c["min_reads"] for c in calls if not c["overlapped"]} == {1 << 18}
    assert {dict(DEFAULTS, **c)["query"] for c in cases} == {ML, LOGS, SA, PER_READ, MULTI, COMPACT}
    bad = [(left, g, want) for (left, want), g in zip(rows, got) if g != want]
    assert not bad, (len(bad), bad[:3])


def test_chunks_by_hand(driver):
    # Synchronous path (pageable reads, no page-locking): target 2^28 = 268435456 bases.  2.5 M reads of 100 and 200 bases in turn, so
    # a pair is 300 bases: 894784 pairs are 268435200 bases, one more read of 100 makes 268435300 <= 2^28, the next one (200) does
    # not fit: chunk 0 = 1789569 reads, 268435300 bases; chunk 1 = the other 710431 reads, 375000000 - 268435300 = 106564700 bases.
    # (An MI355X run of the commit before the plan printed exactly these two lines under MOVI_TRACE_HOST_CALLS: profiles/host_plan.txt.)
    sync = dict(reads_pinned=0, vector_pinned=0, host_autopin=0, host_masks=0, n_reads=2_500_000, off0=5, pattern=ALT, a=100, b=200)
    call, n, chunks, _ = plan(driver, **sync)
    assert (call["overlapped"], call["route"], call["target"], call["min_reads"]) == (0, "vector", 1 << 28, 1 << 18) and n == 2
    # (index, first, nr, b0, nb, masks, phase): chunk 1 starts at base 5 + 268435300, and 268435300 % 32 = 4
    assert chunks[0] == (0, 0, 1789569, 5, 268435300, 0, 0) and chunks[1] == (1, 1789569, 710431, 268435305, 106564700, 0, 4)
    # Overlapped, the vector comes down: 1 M x 150 = 150 000 000 bases / 8 = 18 750 000 per chunk (between 2^22 and 2^28), the first two
    # a quarter (4 687 500 -> 31 250 reads, under the floor of 2^15 = 32 768 reads: 4 915 200 bases) and a half (9 375 000 -> 62 500 reads),
    # then 125 000 reads each: 1 000 000 - 32 768 - 62 500 = 904 732 = 7 x 125 000 + 29 732.  2 B per base come down: nothing goes up ahead.
    call, n, chunks, _ = plan(driver, host_masks=0)
    assert (call["overlapped"], call["route"], call["quartered"], call["ahead"], call["vector_down"]) == (1, "vector", 1, 0, 1)
    assert (call["target"], call["min_reads"], n) == (18_750_000, 1 << 15, 10)
    assert [c[2] for c in chunks] == [32_768, 62_500, 125_000, 29_732]
    # Masks (the default for >= 2^22 bases): sixteen equal chunks of 9 375 000 bases = 62 500 reads, none quartered, all reads up ahead
    call, n, chunks, _ = plan(driver)
    assert (call["route"], call["quartered"], call["ahead"], call["words_in_block"], call["target"], n) == ("masks", 0, 1, 1, 9_375_000, 16)
    assert all(c[2] == 62_500 and c[5] == 1 for c in chunks)
    # phase: chunk k starts at base 5 + k * 9 375 000; 9 375 000 % 32 = 24, so the phases run 0, 24, 16, ... and chunk 15's is 15 * 24 % 32 = 8;
    # packed, chunk 1 starts in byte (5 + 9375000) >> 2 = 2343751 (at its second base) and spans (9375005 + 9375000 + 3 >> 2) - 2343751 bytes
    _, _, chunks, _ = plan(driver, off0=5, packed=1)
    assert [c[6] for c in chunks] == [0, 24, 16, 8]
    assert chunks[1][7:] == (2_343_751, ((9_375_005 + 9_375_000 + 3) >> 2) - 2_343_751) == (2_343_751, 2_343_751)
    # "pipe_chunk_bases" 9 on reads of 150: one read per chunk (never none); 5000: 33 reads = 4950 bases
    assert plan(driver, pipe_chunk_bases=9, n_reads=1000)[1] == 1000
    assert [c[2] for c in plan(driver, pipe_chunk_bases=5000, n_reads=1000)[2]] == [33, 33, 33, 1000 - 30 * 33]
    # a mixed call at 50 %: chunk 0 comes down as it is (nb * 100 <= 50 * nb is false), chunk 1 as masks ((0 + nb) * 100 <= 50 * 2 nb), and so on in turn
    call, n, chunks, _ = plan(driver, host_masks=2, host_mask_share=50)
    assert call["route"] == "mixed" and n == 16 and [c[5] for c in chunks] == [0, 1, 0, 1]
    # ... and with pageable buffers that could not be page-locked it is a masks call on the synchronous path
    call, n, chunks, _ = plan(driver, host_masks=2, reads_pinned=0, vector_pinned=0, pin_ok=0)
    assert (call["route"], call["demoted"], call["overlapped"], call["pin_reads"], call["pin_vector"], n) == ("masks", 1, 0, 1, 1, 1) and chunks[0][5] == 1


def test_chunk_properties_on_random_offsets(driver):
    rng = random.Random(20)
    cases = []
    for _ in range(150):
        pattern = rng.choice((CONST, ALT, ZERO_RUN, LCG, LCG, LCG))
        a = rng.choice((0, 1, 31, 150, 3000))
        c = dict(n_reads=rng.choice((1, 2, 63, 1000, 40_000, 300_000)), off0=rng.choice((0, 5, 33)), pattern=pattern, a=a,
                 b=a + rng.choice((0, 1, 100, 20_000)), seed=rng.randrange(1 << 30), query=rng.choice((ML, ML, ML, PER_READ, COMPACT)),
                 reads_pinned=rng.choice((0, 1)), host_masks=rng.choice((-1, 0, 1, 2, 2)), host_mask_share=rng.choice((0, 1, 30, 50, 70, 99, 100)),
                 pipe_chunk_bases=rng.choice((0, 0, 1, 9, 5000, 1 << 32)), seg_seen=rng.choice((0, 1)), host_overlap=rng.choice((0, 1, 1)))
        cases.append(c)
    cases.append(dict(pattern=ONE_LONG, a=150, b=(1 << 31) + 1000, reads_pinned=0, host_autopin=0))       # one read over the cap
    cases.append(dict(pattern=ONE_LONG, a=150, b=(1 << 31) + 1000, pipe_chunk_bases=1 << 32))
    for c, chunks in zip(cases, all_chunks(driver, cases)):
        full = dict(DEFAULTS, **c)
        cap = (1 << 27) if full["query"] == COMPACT else (1 << 31)
        assert chunks, c
        nxt, base = 0, full["off0"]
        for first, nr, b0, nb, masks, phase in chunks:               # they tile [0, n_reads) in order, and the bases with them
            assert first == nxt and nr >= 1 and b0 == base and phase == (b0 - full["off0"]) % 32, (c, first)
            # over the cap only as a single read -- or where "pipe_chunk_bases" itself is above the cap
            assert nb <= max(cap, full["pipe_chunk_bases"]) or nr == 1, (c, first, nr, nb)
            nxt, base = first + nr, b0 + nb
        assert nxt == full["n_reads"], c
        as_masks, total = sum(ch[3] for ch in chunks if ch[4]), sum(ch[3] for ch in chunks)
        call = plan(driver, **c)[0]
        if call["route"] == "mixed":
            assert as_masks * 100 <= full["host_mask_share"] * total, (c, as_masks, total)
        else:
            assert as_masks == (total if call["route"] == "masks" else 0) or full["query"] != ML, c
