"""CPU suite: the plan of a `movi query` command line (movi_amd/host/query_kind.hpp: the query kind and everything the command derives
from its flags) through tests/host/query_kind_driver.cpp.  tests/golden/query_kind_table.txt crosses the seven query flags with
--classify / --filter, --stdout, --logs, --no-output and --report-all; beside every command line it holds what run_query computed from
the flags BEFORE the plan existed -- the prepare flag, the reservations, the buffers, the files, the engine call of a shard -- or the
message parse_args refuses it with (tools/query_kind_cases.py writes the table and says how it was recorded)."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

KINDS = {"pml_verdict_bins", "pml_logs", "multi_classify", "sa_entries", "pml", "zml", "mem", "kmer", "count"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("querykind") / "query_kind_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "query_kind_driver.cpp")])
    return exe


def test_plans_equal_the_recorded_command(driver):
    table = [ln for ln in open(os.path.join(GOLDEN, "query_kind_table.txt")).read().splitlines() if not ln.startswith("#")]
    rows = [ln.split(" => ", 1) for ln in table]
    got = subprocess.run([driver], input="".join(c + "\n" for c, _ in rows).encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(rows) == 640 and len(got) == len(rows)
    planned = [want for _, want in rows if not want.startswith("rejected: ")]
    assert {w.split()[0][len("kind="):] for w in planned} == KINDS              # every arm is reached ...
    assert len(planned) == 130                                                # ... and the 510 refusals are listed, with their message
    assert {w.split()[1] for w in planned} == {"prepare=%s" % p for p in ("none", 1, 2, 4, 8, 16)}
    bad = [(c, g, want) for (c, want), g in zip(rows, got) if g != want]
    assert not bad, (len(bad), bad[:5])


def test_table_is_the_tools_cross_product():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import query_kind_cases
    finally:
        sys.path.pop(0)
    table = [ln.split(" => ", 1)[0] for ln in open(os.path.join(GOLDEN, "query_kind_table.txt")).read().splitlines() if not ln.startswith("#")]
    assert table == query_kind_cases.cases
