"""Writes tests/golden/launch_policy_table.txt, the table of tests/test_launch_policy_cpu.py:  launch_policy_cases.py PROGRAM OUT.
A case is written as what it changes of the defaults (the table's second header line): one input at a time, then the options that
interact, crossed.  PROGRAM reads the cases as tests/host/launch_policy_driver.cpp does and prints its four lines per case; the table
keeps them beside the case.  The committed table was NOT made with the header under test: PROGRAM was one that includes the
movi_kernels.hip of the commit before movi_launch_policy.hpp existed as text, calls its plan_pml / call_seg_len and restates the
expressions of its launch_pml_segmented, launch_zml, launch_count and launch_count_flat."""
import itertools
import subprocess
import sys

FIELDS = ("r idx32 sep rows2 rows3 hints rows2_count block_threads pml_variant zml_variant count_variant num_cus waves_per_cu seg_len "
          "stage_reads out_ring pair_loads zml_ahead deep n_reads n_bases cm logging have_seg_ws ordered want_mask mode big_batch_cap").split()
BASE = dict(r=14_000_000, idx32=1, sep=0, rows2=1, rows3=1, hints=1, rows2_count=1, block_threads=0, pml_variant=-1, zml_variant=-1,
            count_variant=-1, num_cus=256, waves_per_cu=0, seg_len=2048, stage_reads=1, out_ring=-1, pair_loads=-1, zml_ahead=0, deep=-1,
            n_reads=1_000_000, n_bases=150_000_000, cm=0, logging=0, have_seg_ws=1, ordered=0, want_mask=0, mode=6, big_batch_cap=1)
PLAIN = dict(rows2=0, rows3=0, hints=0, rows2_count=0)                             # plain rows only
BIG2 = dict(r=1 << 28, rows3=0, rows2_count=0)                                     # 2 GB of plain rows, look-ahead rows, no deep rows
BIG8 = dict(r=1 << 30, **PLAIN)                                                    # 8 GB of plain rows
SHORT, FEW, LONG, BIGLONG, TINY = (1_000_000, 150), (100_000, 150), (25_000, 10_000), (500_000, 5000), (3, 5)
cases = []


def add(n_reads, mean, *tables, **kw):
    c = dict(n_reads=n_reads, n_bases=n_reads * mean)
    for t in tables:
        c.update(t)
    c.update(kw)
    line = " ".join("%s=%d" % (f, c[f]) for f in FIELDS if f in c and c[f] != BASE[f])
    if line not in cases:
        cases.append(line)


def crossed(contexts, **dims):
    for vals in itertools.product(*dims.values()):
        for ctx in contexts:
            add(ctx[0], ctx[1], *ctx[2:], **dict(zip(dims, vals)))


# n_reads x mean read length; the batch sizes again on plain rows
W = 256 * 64
NR = [1, 64, 65] + [x for k in (4, 8, 18, 24) for x in (W * k, W * k + 1)]
for n in NR:
    for m in (15, 16, 150, 1023, 1024, 4095, 4096, 10_000):
        add(n, m)
    for m in (150, 10_000):
        add(n, m, PLAIN)
# r: the windows' minimum, the deep rows' and the pair loads' 2 GB boundary, the ZML state machine's 3 GB, look-ahead rows against
# kPairLoadBytes (r * 16), the count cap's 256 MiB (r * 8, r * 16)
for r in (7, 8, (1 << 28) - 1, 1 << 28, (3 << 30) // 8, (3 << 30) // 8 + 1, 1 << 30, (1 << 27) - 1, 1 << 27,
          1 << 25, (1 << 25) + 1, 1 << 24, (1 << 24) + 1):
    for t in (dict(rows3=1 if r < (1 << 28) - 1 else 0), PLAIN):
        for cv in (-1, 0):
            add(*SHORT, t, r=r, count_variant=cv)
        add(*LONG, t, r=r)
    add(*SHORT, r=r, rows3=0, idx32=0)
    add(*SHORT, r=r, rows3=0, rows2_count=0, count_variant=0)
for rows2, rows3, idx32 in itertools.product((0, 1), (0, 1), (0, 1)):
    for ctx in (SHORT, LONG):
        add(*ctx, rows2=rows2, hints=rows2, rows2_count=rows2, rows3=rows3, idx32=idx32)
# the options that interact
MAIN = [SHORT, FEW, LONG, SHORT + (PLAIN,)]
crossed(MAIN + [TINY], waves_per_cu=(0, 5, 40), block_threads=(0, 64, 256))
crossed([SHORT], waves_per_cu=(0, 5, 40), block_threads=(0, 64, 256), mode=(3,))
crossed([SHORT, LONG], waves_per_cu=(-1, 31, 32))
crossed(MAIN + [BIGLONG], stage_reads=(0, 1), out_ring=(-1, 0, 1))
crossed(MAIN + [SHORT + (BIG2,), LONG + (BIG2,)], deep=(-1, 0, 1), pair_loads=(-1, 0, 1))
crossed([SHORT, LONG, SHORT + (BIG8,), TINY], zml_variant=(-1, 0, 1), zml_ahead=(0, 1))
crossed([SHORT, SHORT + (PLAIN,), SHORT + (BIG8,), TINY], count_variant=(-1, 0, 1), zml_ahead=(0, 1))
crossed(MAIN, want_mask=(0, 1), out_ring=(-1, 1))
crossed(MAIN, ordered=(0, 1))
crossed(MAIN, logging=(0, 1))
crossed([SHORT, LONG], cm=(0, 1, 2), pml_variant=(-1, 0))
crossed([SHORT, LONG], mode=(6, 3, 5), count_variant=(-1, 1))
crossed([SHORT, LONG, BIGLONG], big_batch_cap=(0, 1), pml_variant=(-1, 14))
crossed([LONG, BIGLONG], have_seg_ws=(0, 1))
crossed([LONG, FEW], seg_len=(0, 31, 32, 256))
crossed([SHORT, LONG, TINY], pml_variant=(0, 1, 14))
crossed([SHORT, LONG], sep=(0, 1))
crossed([SHORT, FEW, LONG], num_cus=(64,))

feed = "".join(" ".join(str(dict(BASE, **{k: int(v) for k, v in (kv.split("=") for kv in c.split())})[f]) for f in FIELDS) + "\n" for c in cases)
out = subprocess.run([sys.argv[1]], input=feed.encode(), capture_output=True, check=True).stdout.decode().splitlines()
assert len(out) == 4 * len(cases), (len(out), len(cases))
with open(sys.argv[2], "w") as f:
    f.write("# " + " ".join(FIELDS) + "\n# " + " ".join(str(BASE[k]) for k in FIELDS) + "\n")
    for i, c in enumerate(cases):
        f.write("%s => %s\n" % (c, " | ".join(out[4 * i:4 * i + 4])))
print(len(cases), "cases")
