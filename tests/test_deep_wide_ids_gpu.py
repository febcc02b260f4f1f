"""GPU suite (-m gpu): the deep rows' two field maps (movi_deep_fields.hpp) AT THE SIZES WHERE THEY PART -- synthetic tables of 2^26 - 1,
2^26 and 2^28 - 2 rows, the smallest that have an id with bit 26 set:

  N   2^26 - 1 rows (r mod 3 = 0): the largest table with narrow ids.  r equals the 26-bit "not a row" value; the largest id is 0x03FFFFFE.
  W0  2^26 rows     (r mod 3 = 1): the first table that keeps wide ids and 2-bit hints whatever "deep_hint_bits" asks; id 0x03FFFFFF is a row.
  W   2^28 - 2 rows (r mod 3 = 2): the largest eligible table: ids with bits 27:26 = 0, 1, 2, 3, hints directly on top of id bit 27, j3 with
      its top bits at the top of dword 4; r itself is a value the 28-bit field holds and that is no row.

Per table: the walk of a short-read batch in which repositions dominate, against the oracle under the three settings of
test_deep_hints_gpu.py (vector, mask words, error bytes, counters; lane steps ordered as the hint rule says); on W the segment walk on the
deep rows; on N and W ids that are no row but become one when cut to 26 or 28 bits, against the walk on the plain rows.

One table is held at a time (W: 2.1 GB image, ~8 GB of host memory while the generator lives, ~12 GB of HBM with the look-ahead copy the
first query builds).  Skipped when the machine has less than 24 GB of host memory or the GPU less than 20 GB free."""
import os

import numpy as np
import pytest

from test_deep_hints_gpu import _set, _three_ways
from test_gpu_parity import check_segmented

pytestmark = pytest.mark.gpu

ROWS = {"N": (1 << 26) - 1, "W0": 1 << 26, "W": (1 << 28) - 2}
NARROW_MAX = (1 << 26) - 1                                 # tables of more rows keep wide ids and 2-bit hints
SEEDS = {"N": 20261020, "W0": 20261021, "W": 20261022}
N_READS, READ_LEN = 20_000, 150
STRIDE = 9973                                              # corrupt ids: one row in ~3300

_held = {}                                                 # the one table in memory: name, image, batches, the oracle's answers


def _mem_ok():
    try:
        kb = int([l for l in open("/proc/meminfo") if l.startswith("MemAvailable")][0].split()[1])
        lim = open("/sys/fs/cgroup/memory.max").read().strip() if os.path.exists("/sys/fs/cgroup/memory.max") else "max"
        avail = kb * 1024 if lim == "max" else min(kb * 1024, int(lim))
        return avail >= 24 << 30
    except Exception:
        return True


def _table(name):
    """Image, batches and the oracle's answers of table `name` -- made once, left unchanged, dropped when another table is asked for."""
    import torch
    from oracle.oracle import Oracle
    from tools import synth
    if _held.get("name") == name:
        return _held
    _held.clear()
    if not _mem_ok():
        pytest.skip("needs 24 GB of host memory")
    if torch.cuda.mem_get_info()[0] < 20 << 30:
        pytest.skip("needs 20 GB of free HBM")
    r = ROWS[name]
    six = synth.synth_index(r, mode=6, seed=SEEDS[name])
    img = six.image()
    # 20 k reads of 150 bases, a few of 1, 2 and 3 bases, and one that is all N (written over the last read)
    lens = np.array([READ_LEN] * N_READS + [1, 2, 3, 1, 2, 3, 40], np.uint64)
    bases, offs = synth.synth_reads(six, lens.size, 0, seed=SEEDS[name] + 100, sub_rate=0.02, n_rate=0.001, lens=lens)
    bases[int(offs[-2]):] = ord("N")
    seg = None
    if name == "W":                                        # long reads for the segment walk, short ones beside them
        slens = np.array([3000] * 40 + [150] * 2000, np.uint64)
        seg = synth.synth_reads(six, slens.size, 0, seed=SEEDS[name] + 200, sub_rate=0.02, n_rate=0.001, lens=slens)
    del six                                                # the generator's arrays, before the oracle copies the rows
    cpu = Oracle(img)
    exp, ff, sc = cpu.pml_batch(bases, offs, threads=8)
    t = dict(name=name, r=r, img=img, bases=bases, offs=offs, exp=exp, ff=ff, sc=sc)
    if seg is not None:
        sexp, sff, ssc = cpu.pml_batch(seg[0], seg[1], threads=8)
        t.update(seg_bases=seg[0], seg_offs=seg[1], seg_exp=sexp, seg_ff=sff, seg_sc=ssc)
    cpu.close()
    print("%s: %d fast-forwards, %d scans in %d bases" % (name, ff, sc, bases.size))
    assert ff > bases.size // 2 and sc > bases.size // 4    # repositions dominate the walk
    _held.update(t)
    return _held


@pytest.fixture(scope="module", autouse=True)
def _drop_table():
    yield
    _held.clear()


def _id_column(img):
    """(desc, the ids of a regular-thresholds image as a view into it: the first four bytes of every 8-byte row)."""
    import movi_amd
    d, _, off, _ = movi_amd.parse_index_image(img)
    assert d.mode == 6 and d.row_bytes == 8
    return d, img[off: off + d.r * 8].view(np.uint32)[0::2]


def _check_image(t):
    """What the table is there for, from the image itself: its size and the id bits it reaches."""
    d, ids = _id_column(t["img"])
    assert d.r == ROWS[t["name"]] == t["r"]
    sample = ids[::997]
    assert int(sample.max()) < d.r
    if t["name"] == "W":
        assert sorted(np.unique(sample >> 26).tolist()) == [0, 1, 2, 3]
    else:
        assert ((sample >> 25) & 1).any()
    return d, ids


@pytest.fixture(scope="module")
def default_bits(built_lib, golden_image):
    """The library's default width of a hint ("deep_hint_bits" -1), asked of a small table, where every width can be built."""
    import movi_amd
    gpu = movi_amd.MoveIndex.from_image(golden_image(6))
    try:
        gpu.set_option("deep_hint_bits", -1)
        gpu.set_option("deep_rows", 1)
        bits = int(gpu.info("deep_hint_bits"))
    finally:
        gpu.close()
    assert bits in (2, 4)
    return bits


# ------------------------------------------------------------------------------------------------------ 1. parity under the settings
def _parity(t, default_bits):
    import movi_amd
    name, r, wide = t["name"], t["r"], t["r"] > NARROW_MAX
    _check_image(t)
    gpu = movi_amd.MoveIndex.from_image(t["img"])
    try:
        assert gpu.desc.r == r
        gpu.set_option("deep_hint_bits", -1)                 # the default: 2 bits where nothing else fits
        gpu.set_option("deep_rows", 1)
        assert int(gpu.info("deep_hint_bits")) == (2 if wide else default_bits)
        assert gpu.info("deep_rows_bytes") == ((r + 2) // 3) * 64
        steps = _three_ways(gpu, t["bases"], t["offs"], t["exp"], t["ff"], t["sc"], name, wide_only=wide)
        assert steps[(2, 1)] < steps[(4, 0)], (name, steps)   # the hints are live at this size
        if wide:
            assert steps[(4, 1)] == steps[(2, 1)], (name, steps)   # the same map both times
        else:
            assert steps[(4, 1)] < steps[(2, 1)], (name, steps)
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------- 2. the segment walk, 2-bit rows where 4 are asked
def _segments(t, default_bits):
    import movi_amd
    assert t["name"] == "W"
    _check_image(t)
    bases, offs = t["seg_bases"], t["seg_offs"]
    assert bases.size >= 64 * (offs.size - 1)                # (check_segmented then insists on segments)
    gpu = movi_amd.MoveIndex.from_image(t["img"])
    try:
        gpu.set_option("deep", 1)                            # (segments are long reads: they walk on the deep rows on request only)
        _set(gpu, 4, 1, built=2)
        check_segmented(gpu, bases, offs, t["seg_exp"], t["seg_ff"], t["seg_sc"], "W segments")
        assert gpu.last_launch()["ahead"] == 2, gpu.last_launch()
    finally:
        gpu.set_option("deep", -1)
        gpu.close()


# ---------------------------------------------------------------------------------- 3. ids that are a row only when cut to the field
def _corrupt(t, default_bits):
    """N: r (the 26-bit "not a row" value itself), r + 1 = 2^26 (cut to 26 bits: row 0), 2^26 + 5.  W: r = 2^28 - 2 (fits the 28-bit field
    and is no row: only the comparisons with r catch it), r + 1 = 2^28 - 1, 2^28 + 5.  Everything as on the plain rows of the same handle."""
    import movi_amd
    name, r = t["name"], t["r"]
    top = 1 << (26 if name == "N" else 28)
    d, ids = _check_image(t)
    bad_ids = ((11, r), (3001, r + 1), (7013, top + 5))
    saved = [(start, ids[start::STRIDE].copy()) for start, _ in bad_ids]
    bad = None
    try:
        for start, bad_id in bad_ids:
            ids[start::STRIDE] = bad_id
        bad = movi_amd.MoveIndex.from_image(t["img"])
        bad.set_option("ahead_rows", 0)
        bad.set_option("pml_via_mask", 0)
        bad.set_option("host_masks", 0)
        exp, est, eerr, erc = bad.query_pml_packed(t["bases"], t["offs"], want_err=True)
        assert bad.last_launch()["ahead"] == 0 and est.errors > 0 and erc != 0
        want = (exp, eerr, erc, (est.fast_forwards, est.scans, est.repositions, est.errors))
        _three_ways(bad, t["bases"], t["offs"], None, None, None, name + " corrupt", want=want, wide_only=r > NARROW_MAX)
    finally:
        if bad is not None:
            bad.close()
        for start, old in saved:                             # the image as it was, for whoever reads it next
            ids[start::STRIDE] = old


# One table at a time, each made once: the cases in the order of their tables.
CASES = [("N", _parity), ("N", _corrupt), ("W0", _parity), ("W", _parity), ("W", _segments), ("W", _corrupt)]


@pytest.mark.parametrize("name,check", CASES, ids=["%s-%s" % (n, c.__name__[1:]) for n, c in CASES])
def test_boundary_table(built_lib, default_bits, name, check):
    check(_table(name), default_bits)
