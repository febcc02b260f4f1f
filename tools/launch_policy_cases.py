"""Writes tests/golden/launch_policy_table.txt, the table of tests/test_launch_policy_cpu.py:  launch_policy_cases.py PROGRAM OUT.
A case is written as what it changes of the defaults (the table's second header line): one input at a time, then the options that
interact, crossed.  PROGRAM reads the cases as tests/host/launch_policy_driver.cpp does and prints its four lines per case; the table
keeps them beside the case.  The committed table was NOT made with the header under test: PROGRAM was one that includes the
movi_kernels.hip of the commit before movi_launch_policy.hpp existed as text, calls its plan_pml / call_seg_len and restates the
expressions of its launch_pml_segmented, launch_zml, launch_count and launch_count_flat.

launch_policy_cases.py route PROGRAM OUT  writes tests/golden/launch_route_table.txt, the routes of PML calls (plan_pml), the same way: a
case is the 28 inputs above and the 8 of the driver's "route" mode.  PROGRAM reads them and prints one "route ..." line per case.  The
committed table was NOT made with the header under test either: PROGRAM was a recorder compiled against the movi_launch_policy.hpp of
the commit before the route moved into plan_pml, which restates what that commit's launch_pml (movi_kernels.hip) and ml_device,
movi_pml_device, movi_pml_mask_device and ml_host (movi_abi.hip) derived around its plan_pml: the fall-back of a lent-masks call, the
fused expansion, the park queue's fit, hint_w, ff_skip and the template selectors; its source is not kept in the tree -- it went with the
description of the pull request that introduced the table.  Two columns are then set by this tool from the recorder's OTHER columns, because the one planner changes them on purpose;
a comment line above a case says where that changed the recorded value:
  (a) needs_tmp of a masks call = the segment plan goes first or the walk cannot write masks (the recorder planned it with ordered = 0
      whatever the call passed: an ordered call on long reads grew a scratch vector it never read);
  (b) words = the route is vector_fused or vector_expand (the recorder: wherever the caller lent them -- "pml_via_mask" 1 grew mask
      words that a call falling back to the plain vector never used)."""
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


def plan_cases():
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


ROUTE_BASE = dict(want=0, aligned=1, fused_expand=1, hints_opt=1, ff_skip=-1, park_lanes=-1, park_cap=-1, pml_via_mask=-1)
VECTOR, MASKS, LENDS = 0, 1, 2                                                     # want


def park_records(n_reads, lanes, bt=64):
    """Records a queue needs: every lane of the second launch's grid (whole blocks)."""
    waves = (n_reads + bt - 1) // bt * (bt // 64)
    return (waves * lanes + bt - 1) // bt * bt


def route_cases():
    WANTS = (VECTOR, MASKS, LENDS)
    ROWS = (PLAIN, dict(rows3=0), {})                                              # plain / look-ahead / deep rows
    crossed([SHORT, LONG], want=WANTS, cm=(0, 1, 2), logging=(0, 1))
    # the mean read length around kOutRingReadLen and 2 x seg_len, with and without a read order, by the policy and forced
    crossed([(25_000, m) for m in (150, 1023, 1024, 4096, 10_000)], want=WANTS, ordered=(0, 1), pml_via_mask=(-1, 1))
    crossed([SHORT], want=WANTS, aligned=(0, 1), fused_expand=(0, 1), block_threads=(0, 64, 256))
    # the park queue: none, one record short, exactly enough
    for lanes in (-1, 0, 2, 63):
        need = park_records(SHORT[0], max(lanes, 2))
        crossed([SHORT], want=WANTS, park_lanes=(lanes,), park_cap=(-1, need - 1, need))
    crossed([SHORT], want=(MASKS, LENDS), park_lanes=(2,), park_cap=(1 << 40,), block_threads=(64, 256), ordered=(0, 1), aligned=(0, 1))
    crossed([LONG, TINY], want=(MASKS, LENDS), park_lanes=(2,), park_cap=(1 << 40,), pml_via_mask=(-1, 1))
    for rows in ROWS:
        crossed([SHORT + (rows,), LONG + (rows,)], want=WANTS, ff_skip=(-1, 0, 1))
    for rows in ROWS + (dict(rows3=0, hints=0),):
        crossed([SHORT + (rows,), LONG + (rows,)], hints_opt=(0, 1))
    crossed([SHORT, LONG, TINY], want=(LENDS,), pml_via_mask=(-1, 0, 1), ordered=(0, 1))
    crossed([LONG], want=(LENDS,), pml_via_mask=(-1, 0, 1), seg_len=(0,))        # long reads the segment plan has no say on
    crossed([SHORT], want=WANTS, r=(7, 8))
    crossed([(1, 15), (1, 16)], want=WANTS)
    crossed([(1 << 32, 150)], want=WANTS, park_lanes=(-1, 2), park_cap=(1 << 40,))
    crossed([SHORT, LONG], want=WANTS, stage_reads=(0, 1), out_ring=(-1, 1))
    crossed([SHORT, LONG], want=WANTS, pml_variant=(0, 1, 14))
    crossed([LONG], want=(VECTOR, MASKS), have_seg_ws=(0, 1), ordered=(0, 1))
    crossed([LONG], want=WANTS, seg_len=(0, 32, 256))
    crossed([SHORT, LONG], want=WANTS, num_cus=(64,))
    crossed([SHORT], want=WANTS, waves_per_cu=(5, 40))
    crossed([SHORT + (BIG2,), SHORT + (BIG8,)], want=WANTS)


def run(program, args, per_case):
    feed = "".join(" ".join(str(dict(BASE, **{k: int(v) for k, v in (kv.split("=") for kv in c.split())})[f]) for f in FIELDS) + "\n" for c in cases)
    out = subprocess.run([program] + args, input=feed.encode(), capture_output=True, check=True).stdout.decode().splitlines()
    assert len(out) == per_case * len(cases), (len(out), len(cases))
    return out


def permitted(case, line):
    """(line with needs_tmp and words as the one planner sets them, the comment for a value that changed)."""
    w = line.split()
    if w[1] == "invalid":
        return line, None
    c = dict(BASE, **{k: int(v) for k, v in (kv.split("=") for kv in case.split())})
    tmp = int(c["want"] == MASKS and (w[2] == "1" or w[1] == "mask_from_tmp"))
    words = int(w[1] in ("vector_fused", "vector_expand"))
    note = None
    if str(tmp) != w[3]:
        note = "# (a) needs_tmp was %s: planned with the call's own `ordered`, the walk writes these masks itself" % w[3]
    if str(words) != w[4]:
        note = "# (b) words was %s: the call falls back to the plain vector and uses no mask words" % w[4]
    w[3], w[4] = str(tmp), str(words)
    return " ".join(w), note


if __name__ == "__main__":
    route = sys.argv[1] == "route"
    if route:
        FIELDS += list(ROUTE_BASE)
        BASE.update(ROUTE_BASE)
        route_cases()
        out = run(sys.argv[2], [], 1)
    else:
        plan_cases()
        out = run(sys.argv[1], [], 4)
    with open(sys.argv[-1], "w") as f:
        f.write("# " + " ".join(FIELDS) + "\n# " + " ".join(str(BASE[k]) for k in FIELDS) + "\n")
        for i, c in enumerate(cases):
            if route:
                line, note = permitted(c, out[i])
                if note:
                    f.write(note + "\n")
                f.write("%s => %s\n" % (c, line))
            else:
                f.write("%s => %s\n" % (c, " | ".join(out[4 * i:4 * i + 4])))
    print(len(cases), "cases")
