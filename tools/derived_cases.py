"""Writes tests/golden/derived_table.txt, the table of tests/test_derived_cpu.py:  derived_cases.py PROGRAM OUT.
A case is written as what it changes of the defaults (the table's second header line: the golden index's shape on an idle MI355X), a
colon and a script of steps on one handle; tests/host/derived_driver.cpp says what the fields and the steps are.  One input varies at
a time, then what interacts is crossed.  PROGRAM reads the cases as that driver does and prints its line per case; the table keeps it
beside the case.  The committed table was NOT made with the header under test: PROGRAM was a recorder that includes nothing of the
project and restates, expression by expression, what movi_abi.hip did at the commit before movi_derived.hpp existed (b9af9e7) -- the
eligibility predicates, drop_* and build_* functions, sample_no_ff, ahead_wanted and ensure_pml_tables (lines 857-1047), the build-now
options of movi_set_option and "deep_hint_bits" (1249-1301), ensure_ckpt and ensure_count_tables (2465-2506) and movi_index_prepare's
retry reset, calls and `prepared` (2541-2570) -- against the same scripted device.  Its source is not kept in the tree: it went with
the description of the pull request that introduced the table."""
import subprocess
import sys

FIELDS = "kmode r dna total free mem_fails sample full fail_mask".split()
GIB = 1 << 30
BASE = dict(kmode=6, r=118209, dna=1, total=288 * GIB, free=200 * GIB, mem_fails=0, sample="0.83", full="0.83", fail_mask=0)
KMER, FTAB, AHEAD, DEEP, CKPT = 1, 2, 4, 8, 16                                  # fail_mask
DEEP_AUTO_ROWS = 48 << 20
RANDOM = dict(sample="0.51", full="0.51")                                       # a uniformly random run sequence
CV0 = "S count_variant 0"
cases = []


def ahead_bytes(r):
    return ((r + 7) // 8 + 1) * 128


def deep_bytes(r):
    return (r + 2) // 3 * 64


def add(script, *parts, **kw):
    c = {}
    for p in parts:
        c.update(p)
    c.update(kw)
    left = " ".join("%s=%s" % (f, c[f]) for f in FIELDS if f in c and str(c[f]) != str(BASE[f]))
    line = (left + " : " if left else ": ") + script
    if line not in cases:
        cases.append(line)


def derived_cases():
    QUERIES = ("P", "C", CV0 + " C", "Rpc", "P C")
    BUILD_NOW = ("S kmer_k 8", "S ftab_k 8", "S ahead_rows 1", "S deep_rows 1")
    # eligibility, both sides: the row layout, the alphabet, the row count at 7 / 8, at kDeepAutoRows, at 2^28 - 2 and at 2^36
    for facts in (dict(), dict(kmode=3), dict(kmode=7), dict(dna=0), dict(kmode=3, dna=0), dict(r=7), dict(r=8), dict(r=DEEP_AUTO_ROWS),
                  dict(r=DEEP_AUTO_ROWS + 1), dict(r=(1 << 28) - 2), dict(r=(1 << 28) - 1), dict(r=(1 << 36) - 1), dict(r=1 << 36)):
        for q in QUERIES + BUILD_NOW:
            add(q, facts)
        add("P S kmer_k 0 S ftab_k 0 S ahead_rows 0 S deep_rows 0", facts)
    # the share at 0.67: the sample and the builder's tally of every row on either side of it, for the deep rows and the count query's copy
    for sample in ("0.6699", "0.67", "x"):
        for full in ("0.6699", "0.67"):
            for q in ("P", CV0 + " C", CV0 + " C P", CV0 + " C C P", "S ahead_rows 0 P", "S ahead_rows 1 P", "Rpc", CV0 + " Rpc C P"):
                add(q, sample=sample, full=full)
    # the sample failing: tried again by the next call
    # (the PML path samples for the deep rows only, and settles them in the same call: built without the statistic where there is room)
    for q in ("P x3", CV0 + " C x3", CV0 + " C P C", "S ahead_rows 0 S deep_rows 0 P"):
        add(q, sample="x")
        add(q, sample="x", free=GIB)
        add(q, sample="x", total=4 * ahead_bytes(118209) - 1)
    # room for the look-ahead rows, one byte either side: bytes <= total / 4 and free > bytes + max(2 GiB, bytes / 2)
    for r in (118209, 113_000_000, 1_000_000_000):
        b = ahead_bytes(r)
        for total in (4 * b - 1, 4 * b, 4 * b + 3, 4 * b + 4):
            for q in ("P", CV0 + " C"):
                add(q, r=r, total=total)
        edge = b + max(2 * GIB, b // 2)
        for free in (edge - 1, edge, edge + 1):
            for q in ("P", CV0 + " C", "Rp", "P x2"):
                add(q, r=r, free=free)
    # room for the deep rows: free >= bytes + 2 GiB (no quarter rule, no retry)
    for r in (118209, DEEP_AUTO_ROWS):
        edge = deep_bytes(r) + 2 * GIB
        for free in (edge - 1, edge, edge + 1):
            for q in ("P", "P x3", "S ahead_rows 1 S deep_rows 0 P", "Rp Rp"):
                add(q, r=r, free=free)
            add("S ahead_rows 0 P S deep_rows 1", r=r, free=free)
    # the memory query failing
    for q in ("P", "P x3", CV0 + " C x2", "Rp Rp", "S ahead_rows 1 P", "S deep_rows 1 P"):
        add(q, mem_fails=1)
    # declined for lack of memory: the device is asked at calls 1 and 65 and at no other; the two paths share the counter; a prepare resets it
    NO_ROOM = dict(free=GIB)
    for q in ("P x66", CV0 + " C x66", CV0 + " P C x32 P", CV0 + " P x10 C x60", "P x10 Rp P x10", "P x10 Rc P x60", "Rp P x70", "Rp Rp P",
              "P x30 F %d P x40" % (200 * GIB), "P F %d Rp" % (200 * GIB), "Rp F %d P Rp" % (200 * GIB), CV0 + " Rc F %d C Rc" % (200 * GIB),
              "P x64", "P x65", CV0 + " C x65 P"):
        add(q, NO_ROOM)
        add(q, NO_ROOM, RANDOM)
    # each of the five builds failing: its auto-build goes off and is not tried again (the checkpoints fail the call, every time)
    for mask in (0, KMER, FTAB, AHEAD, DEEP, CKPT, KMER | DEEP, AHEAD | DEEP, 31):
        for q in ("P x3", "C x3", CV0 + " C x3", "Rpc Rpc", "Rpc P C", CV0 + " C P", "Rc P") + BUILD_NOW:
            add(q, fail_mask=mask)
        add("S kmer_k 8 S ftab_k 8 S ahead_rows 1 S deep_rows 1 P C", fail_mask=mask)
    # prepared: queries build the two lookup tables still, the row copies never; a second prepare builds what is missing
    for q in ("Rc P", "Rp C", CV0 + " Rp C", CV0 + " Rc P", "Rpc Rpc", "Rpc P C", "Rc Rp", "Rc P Rp", "Rp S ahead_rows 0 P", "Rp S deep_rows 0 P Rp",
              "Rc S kmer_k 0 P", "Rp S ftab_k 0 C", "R P C", "R Rpc"):
        add(q)
        add(q, RANDOM)
        add(q, NO_ROOM)
    # every build-now option at 0 and at a building value, before and after the auto-build
    for key, v in (("kmer_k", 8), ("kmer_k", 12), ("kmer_k", 1), ("ftab_k", 8), ("ahead_rows", 1), ("deep_rows", 1)):
        for facts in (dict(), RANDOM, NO_ROOM):
            for q in ("S %s 0 P C", "P C S %s 0 P C", "S %s {v} P C", "P C S %s {v} P C", "S %s {v} S %s 0 P C", "S %s 0 Rpc", "S %s 0 S %s {v} S %s {v}"):
                add(q.replace("%s", key).replace("{v}", str(v)), facts)
    # "ahead_rows" 0 / 1 drop the deep rows and switch their auto-build off; "deep_rows" 1 brings them back
    for q in ("P S ahead_rows 0 P", "P S ahead_rows 1 P", "S ahead_rows 0 P S deep_rows 1 P", "P S ahead_rows 1 S deep_rows 1 P", "S deep_rows 1 S ahead_rows 0",
              "S deep_rows 0 P S ahead_rows 0 P", "S deep_rows 1 P"):
        add(q)
        add(q, RANDOM)
    # "deep_hint_bits": at the next build of the deep rows only; 4 bits need narrow ids (fewer than 2^26 rows)
    for r in (118209, (1 << 26) - 1, 1 << 26, (1 << 28) - 2):
        for bits in (2, 4, -1):
            add("S deep_hint_bits %d P" % bits, r=r)
            add("S deep_hint_bits %d S deep_rows 1" % bits, r=r)
            add("P S deep_hint_bits %d P S deep_rows 1" % bits, r=r)
            add("S deep_rows 1 S deep_hint_bits %d S deep_rows 1 S deep_hint_bits -1 S deep_rows 1" % bits, r=r)
    # the count query's copy: built and kept, built and dropped (then a PML query builds it again), declined by the sample, and the options beside it
    for facts in (dict(), RANDOM, dict(sample="0.83", full="0.51"), dict(sample="0.51", full="0.83")):
        for q in (CV0 + " C", CV0 + " C C", CV0 + " C P", CV0 + " C P C", "C", "S count_variant 1 C", CV0 + " P C", CV0 + " S ahead_rows 1 C",
                  CV0 + " S ahead_rows 0 C", CV0 + " C S count_variant -1 C", CV0 + " Rc", CV0 + " Rc Rc P"):
            add(q, facts)


if __name__ == "__main__":
    derived_cases()
    feed = ""
    for c in cases:
        left, script = c.split(":")
        full = dict(BASE, **dict(kv.split("=") for kv in left.split()))
        feed += " ".join(str(full[f]) for f in FIELDS) + " : " + script.strip() + "\n"
    out = subprocess.run([sys.argv[1]], input=feed.encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases), (len(out), len(cases))
    with open(sys.argv[2], "w") as f:
        f.write("# " + " ".join(FIELDS) + "\n# " + " ".join(str(BASE[k]) for k in FIELDS) + "\n")
        for c, line in zip(cases, out):
            f.write("%s => %s\n" % (c.strip(), line))
    print(len(cases), "cases")
