"""Writes tests/golden/query_kind_table.txt, the table of tests/test_query_kind_cpu.py:  query_kind_cases.py PROGRAM OUT.
A case is a `movi query` command line: the seven query flags (and no flag: PML by default; --mem with and without its --ftab-k,
--multi-classify with and without its -o) crossed with --classify / --filter, --stdout, --logs, --no-output and --report-all.  PROGRAM reads
the lines as tests/host/query_kind_driver.cpp does and prints one line per case; the table keeps it beside the case ("CASE => LINE").
The committed table was NOT made with movi_amd/host/query_kind.hpp: PROGRAM was a recorder over the options.cpp of the commit before
that header existed, which restates the expressions that commit's run_query (movi_main.cpp) spread over its flag ladders -- the prepare
flag, the reservations, the files it opened, the buffers it sized, the engine call of a shard; its source is not kept in the tree -- it
went with the description of the pull request that introduced the table."""
import itertools
import subprocess
import sys

QUERIES = ("", "--pml", "--zml", "--count", "--mem", "--mem --ftab-k 8", "--kmer -k 12", "--sa-entries", "--multi-classify",
           "--multi-classify -o rep")
CLASSIFY = ("", "--classify", "--filter", "--classify --filter")
SWITCHES = ("--stdout", "--logs", "--no-output", "--report-all")

cases = []
for q, c in itertools.product(QUERIES, CLASSIFY):
    for on in itertools.product((False, True), repeat=len(SWITCHES)):
        words = ["query -i idx -r reads.fq", q, c] + [s for s, x in zip(SWITCHES, on) if x]
        cases.append(" ".join(w for w in words if w))

if __name__ == "__main__":
    program, out = sys.argv[1], sys.argv[2]
    got = subprocess.run([program], input="".join(c + "\n" for c in cases).encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(got) == len(cases), (len(got), len(cases))
    with open(out, "w") as f:
        f.write("# %d command lines of `movi query` => their plan, recorded before query_kind.hpp existed (tools/query_kind_cases.py)\n" % len(cases))
        for c, g in zip(cases, got):
            f.write("%s => %s\n" % (c, g))
