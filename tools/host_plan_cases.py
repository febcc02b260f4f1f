"""Writes tests/golden/host_plan_table.txt, the table of tests/test_host_plan_cpu.py:  host_plan_cases.py PROGRAM OUT.
A case is written as what it changes of the defaults (the table's second header line): one input at a time around 1 M reads of 150
bases, then what interacts, crossed.  PROGRAM reads the cases as tests/host/host_plan_driver.cpp does and prints its line per case; the
table keeps it beside the case.  The committed table was NOT made with the header under test: PROGRAM was a recorder that includes
nothing of the project and restates, expression by expression, what movi_abi.hip did at the commit before movi_host_plan.hpp existed
(4bb1fc5) -- the scans of run_chunked (lines 1706-1715) and run_compact (1809-1817), run_pipelined's target, first chunks and
upper_bound cut (1875-1909) and its upload ahead of the loop (2048), run_host (2107-2113), worth_overlapping_small_results (2101-2104),
autopin_worthwhile (2195-2198), ml_host's route (2242-2248), its deal in launch order (2257-2266) and its overlap, page-locking,
demotion and arguments (2332-2345), and the count, classify, logs, sa-entries and multi-classify entry points' own lines (2682-2686,
2533-2537, 2439, 3033, 3316-3318).  Its source is not kept in the tree: it went with the description of the pull request that
introduced the table."""
import itertools
import subprocess
import sys

FIELDS = ("query zml want_vector want_words reads_pinned vector_pinned small_bytes host_overlap host_autopin host_masks host_mask_share "
          "pipe_chunk_bases seg_seen seg_len pin_ok packed n_reads off0 pattern a b seed").split()
BASE = dict(query=0, zml=0, want_vector=1, want_words=0, reads_pinned=1, vector_pinned=1, small_bytes=0, host_overlap=1, host_autopin=1,
            host_masks=-1, host_mask_share=70, pipe_chunk_bases=0, seg_seen=0, seg_len=2048, pin_ok=1, packed=0, n_reads=1_000_000, off0=0,
            pattern=0, a=150, b=0, seed=1)
ML, LOGS, SA, PER_READ, MULTI, COMPACT = range(6)                              # query
CONST, ALT, ZERO_RUN, ONE_LONG, LCG = range(5)                                 # pattern
PINNED, READS_ONLY, PAGEABLE = (dict(), dict(vector_pinned=0), dict(reads_pinned=0, vector_pinned=0))
KPIPE_MIN = 1 << 22
cases = []


def add(*parts, **kw):
    c = {}
    for p in parts:
        c.update(p)
    c.update(kw)
    line = " ".join("%s=%d" % (f, c[f]) for f in FIELDS if f in c and c[f] != BASE[f])
    if line not in cases:
        cases.append(line)


def crossed(contexts, **dims):
    for vals in itertools.product(*dims.values()):
        for ctx in contexts:
            add(ctx, **dict(zip(dims, vals)))


def plan_cases():
    PER_READ_CALL, COMPACT_CALL = dict(query=PER_READ, small_bytes=16, want_vector=0), dict(PAGEABLE, query=COMPACT, want_vector=0)
    # totals on both sides of 2^22 (masks by policy, the smallest target), 8 x and 16 x kPipeMinBases (the target leaves its floor),
    # 2^27 (autopin), 2^28 (a synchronous chunk), 2^31 (upload ahead, the cap): T - 1 and T, at 2^31 also T + 1
    for T, a in ((1 << 22, 64), (8 * KPIPE_MIN, 64), (16 * KPIPE_MIN, 64), (1 << 27, 256), (1 << 28, 256), (1 << 31, 1024)):
        for d in (-1, 0, 1) if T == 1 << 31 else (-1, 0):
            size = dict(n_reads=T // a + d, a=a)
            crossed([size], host_masks=(-1, 0))
            if T == 1 << 31:
                add(size, want_vector=0)
            add(size, PAGEABLE)
            add(size, PER_READ_CALL)
            add(size, COMPACT_CALL)
    # n_reads on both sides of 2^12, 2^15, 3 * 2^15 (autopin) and 2^18, short and long reads, segment-parallel seen or not
    for n in (1 << 12, 1 << 15, 3 << 15, 1 << 18):
        for d in (-1, 0):
            for a in (150, 10_000):
                size = dict(n_reads=n + d, a=a)
                crossed([size], seg_seen=(0, 1))
                add(size, PAGEABLE)
            add(PAGEABLE, PER_READ_CALL, n_reads=n + d)
            add(COMPACT_CALL, n_reads=n + d)
    # the mean read length on both sides of 1024, 2048 (per-read results overlap up to there) and 2 x seg_len
    for m in (1023, 1024, 2048, 2049, 4095, 4096):
        size = dict(n_reads=200_000, a=m)
        crossed([size], seg_seen=(0, 1))
        add(size, PER_READ_CALL)
        crossed([dict(size, **PER_READ_CALL)], reads_pinned=(0,), pin_ok=(0, 1))
        add(size, query=MULTI, small_bytes=24, want_vector=0)
    crossed([dict(n_reads=200_000, a=4096, seg_seen=1)], seg_len=(0, 512))
    # the way down: "host_masks" x what is page-locked x "host_overlap" x "host_autopin"; "host_mask_share" matters to a mixed call alone,
    # so it is crossed with what is page-locked and "host_overlap" there, and with the other "host_masks" as they stand
    crossed([PINNED, READS_ONLY, PAGEABLE], host_masks=(-1, 0, 1, 2), host_overlap=(0, 1), host_autopin=(0, 1))
    crossed([PINNED, READS_ONLY, PAGEABLE], host_masks=(2,), host_mask_share=(0, 1, 50, 70, 99, 100), host_overlap=(0, 1))
    crossed([PINNED], host_masks=(-1, 0, 1), host_mask_share=(0, 100))
    crossed([PAGEABLE, READS_ONLY], host_masks=(-1, 0, 1, 2), pin_ok=(0,))
    crossed([dict(pattern=LCG, a=30, b=400, seed=7), dict(pattern=ALT, a=100, b=200, n_reads=2_500_000, off0=5)],
            host_masks=(2,), host_mask_share=(1, 50, 99), pipe_chunk_bases=(0, 5000))
    add(PAGEABLE, host_autopin=0, host_masks=0, pattern=ALT, a=100, b=200, n_reads=2_500_000, off0=5)   # (the traced call: profiles/host_plan.txt)
    # "pipe_chunk_bases" above and below everything else, on every pattern of lengths
    SHAPES = [dict(), dict(pattern=ALT, a=40, b=260), dict(pattern=ZERO_RUN, a=150, b=70_000), dict(pattern=ZERO_RUN, a=150, b=400_000),
              dict(pattern=ONE_LONG, a=150, b=(1 << 31) + 1000), dict(pattern=ONE_LONG, a=150, b=(1 << 32) - 1),
              dict(pattern=LCG, a=0, b=300, seed=3), dict(pattern=LCG, a=1, b=20_000, seed=5, n_reads=100_000), dict(n_reads=1, a=150),
              dict(n_reads=1, a=0), dict(n_reads=5, a=0), dict(n_reads=4_000_000, pattern=LCG, a=50, b=250, seed=11)]
    crossed(SHAPES, pipe_chunk_bases=(0, 1, 9, 5000, 1 << 32))
    crossed(SHAPES, host_masks=(0,))
    crossed(SHAPES, reads_pinned=(0,), host_autopin=(0,))
    crossed([dict(s, **COMPACT_CALL) for s in SHAPES])
    crossed([dict(s, **PER_READ_CALL) for s in SHAPES], pipe_chunk_bases=(9,))
    # packed against ASCII, offsets[0] no multiple of 4 or of 32
    crossed([dict(pattern=LCG, a=0, b=300, seed=3)], packed=(1,), off0=(0, 5, 33, 4099), pipe_chunk_bases=(0, 9), host_masks=(-1, 2))
    crossed([dict(pattern=LCG, a=0, b=300, seed=3)], packed=(0,), off0=(0, 5, 33, 4099), host_masks=(-1, 2))
    crossed([PAGEABLE], packed=(0, 1), off0=(5,), want_words=(0, 1), host_autopin=(0, 1))
    # every kind of query: PML, ZML, masks only, no output, logs, count / classify, sa-entries, multi-classify without and with the vector, MEM / k-mer
    KINDS = [dict(), dict(zml=1), dict(want_vector=0, want_words=1), dict(want_vector=1, want_words=1), dict(want_vector=0), dict(query=LOGS),
             PER_READ_CALL, dict(query=SA), dict(query=SA, want_vector=0),
             dict(query=MULTI, small_bytes=24, want_vector=0), dict(query=MULTI, small_bytes=1048, want_vector=0),
             dict(query=MULTI, small_bytes=24, want_vector=1), dict(query=COMPACT, want_vector=0)]
    for kind in KINDS:
        crossed([dict(kind, **buf) for buf in (PINNED, READS_ONLY, PAGEABLE)], host_overlap=(0, 1))
        crossed([dict(kind, **PAGEABLE)], host_autopin=(0,))
        crossed([dict(kind, **PAGEABLE)], pin_ok=(0,))
        if kind.get("query", ML) == ML:                           # (the other kinds read neither option)
            crossed([kind], host_masks=(0, 1, 2))
            add(kind, n_reads=100_000, a=10_000, seg_seen=1)
        add(kind, pipe_chunk_bases=5000)
        add(kind, n_reads=100_000, a=10_000)
        add(kind, n_reads=3, a=5)


if __name__ == "__main__":
    plan_cases()
    feed = "".join(" ".join(str(dict(BASE, **{k: int(v) for k, v in (kv.split("=") for kv in c.split())})[f]) for f in FIELDS) + "\n" for c in cases)
    out = subprocess.run([sys.argv[1]], input=feed.encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases), (len(out), len(cases))
    with open(sys.argv[2], "w") as f:
        f.write("# " + " ".join(FIELDS) + "\n# " + " ".join(str(BASE[k]) for k in FIELDS) + "\n")
        for c, line in zip(cases, out):
            f.write("%s => %s\n" % (c, line))
    print(len(cases), "cases")
