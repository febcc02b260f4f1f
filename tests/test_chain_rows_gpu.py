"""GPU suite (-m gpu): CHAIN ROWS ("chain_rows" option; movi_chain_fields.hpp) -- the PML walk's 32-byte rows that carry what the walk reads
at the next three LF targets, in windows of two rows: up to four bases per gather (pml_kernel_chain).  Same automaton as on every other
layout: the u16 vector, the reset-mask words, the error bytes and the fast-forward / scan / reposition / error counters must be the
oracle's (on corrupt tables: the plain walk's) -- on every index type, through the register packer and as reset masks, on tables whose
last window is padded, on reads that end at every depth of a chain, with illegal and lower-case bases at every place of a step, on reads
that roll through the staged stretch, with and without reposition hints and the fast-forward skip.  Only lane steps may differ."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_fastx
from test_deep_hints_gpu import _hint_table, _random_reads
from test_gpu_parity import mutated_reads, pack

pytestmark = pytest.mark.gpu

VEC, MASK = "pml_kernel_chain<%d, 0>", "pml_kernel_chain<%d, 2>"
DEEP_MASK = "pml_kernel_flatp<6, unsigned int, 0, 0, 0, 1, 2, 0, 2>"
K = 12                                                          # the top-of-walk table's K-mer length


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _chain(gpu, on=1):
    gpu.set_option("chain_rows", on)
    assert gpu.info("chain_rows_bytes") == (((gpu.desc.r + 1) // 2) * 64 if on else 0)


def _both_routes(gpu, bases, offs, exp, ff, sc, tag, sep=0, want=None):
    """The batch on the chain rows through the register packer and as reset masks, against the oracle's (exp, ff, sc) or -- a table on
    which reads fail -- against `want` = (vector, error bytes, rc, counters) of the plain walk.  Returns the vector route's stats."""
    from movi_amd import engine as E
    gpu.set_option("pml_via_mask", 0)                           # the vector from the walk itself
    gpu.set_option("host_masks", 0)
    out, st, err, rc = gpu.query_pml_packed(bases, offs, want_err=True)
    li = gpu.last_launch()
    assert li["ahead"] == 3 and li["kernel"] == VEC % sep and li["staged"] > 0, (tag, li)
    words, mst, merr, mrc = gpu.query_pml_mask_packed(bases, offs, want_err=True)
    li = gpu.last_launch()
    assert li["ahead"] == 3 and li["kernel"] == MASK % sep, (tag, li)
    c = (st.fast_forwards, st.scans, st.repositions, st.errors)
    assert c == (mst.fast_forwards, mst.scans, mst.repositions, mst.errors) and (err == merr).all() and rc == mrc, (tag, c)
    assert st.lane_steps == mst.lane_steps, tag
    print("%s: lane steps %d, counters %s" % (tag, st.lane_steps, c))
    if want is None:
        assert (out == exp).all(), (tag, np.flatnonzero(out != exp)[:8])
        assert rc == 0 and (err == 0).all() and c[:2] == (ff, sc) and c[3] == 0, (tag, c, ff, sc)
        mexp, valid = E.masks_of_pml(exp, offs)
        assert (words[valid] == mexp[valid]).all(), (tag, "mask words")
    else:
        assert (out == want[0]).all() and (err == want[1]).all() and rc == want[2] and c == want[3], (tag, c, want[3])
    return st


# ---------------------------------------------------------------------------------------------------------------- 1. golden index
@pytest.fixture(scope="module")
def golden(built_lib, golden_image):
    """Per index type: image, batch (the golden reads, reads that end at every depth of a chain, illegal and lower-case bases at every
    place of a step, mutated reads) and the oracle's answers -- computed once, shared, left unchanged."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref = _ref()
    rng = np.random.default_rng(52000)
    reads = [s for _, s in read_fastx(os.path.join(GOLDEN, "sample.fastq"))]
    reads += [ref[100 + 31 * L: 100 + 32 * L] for L in range(1, 7)] + [ref[5000 + 40 * d: 5000 + 40 * d + K + d] for d in range(1, 6)]
    for p in range(12):                                         # an N / a lower-case base 0 .. 11 bases from the read's end, with and without the K-mer lookup in front
        for tail in (30, 3):
            s = bytearray(ref[9000 + 50 * p: 9000 + 50 * p + p + 1 + tail])
            n, lc = bytearray(s), bytearray(s)
            n[len(s) - 1 - p] = ord("N")
            lc[len(s) - 1 - p] = s[len(s) - 1 - p] | 0x20
            reads += [bytes(n), bytes(lc)]
    reads += [b"A", b"N", b"NN", b"", ref[700:800].lower()] + mutated_reads(rng, ref, 300, 20, 330)
    bases, offs = pack(reads)
    out = {}
    for mode in (6, 8, 7):
        img = golden_image(mode) if mode != 7 else B.build_index_from_seqs([ref], 7)
        cpu = Oracle(img)
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
        cpu.close()
        out[mode] = dict(img=img, bases=bases, offs=offs, exp=exp, ff=ff, sc=sc)
    return out


@pytest.mark.parametrize("mode", [6, 8, 7])
def test_golden_index(golden, mode):
    """Modes 6, 8 and 7, both routes, with and without the top-of-walk table and the hints; the fast-forward skip changes lane steps only;
    and the chain rows take no more lane steps than the deep rows."""
    import movi_amd
    b = golden[mode]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.set_option("pml_via_mask", 0)
        gpu.set_option("host_masks", 0)
        gpu.set_option("deep_rows", 1)
        out, dst = gpu.query_pml_packed(b["bases"], b["offs"])   # on the deep rows: the counters and lane steps to compare with
        assert gpu.last_launch()["ahead"] == 2 and (out == b["exp"]).all()
        _chain(gpu)
        assert gpu.info("derived_bytes") >= gpu.info("chain_rows_bytes") + gpu.info("deep_rows_bytes")
        steps = {}
        for kmer in (K, 0):
            gpu.set_option("kmer_k", kmer)
            for hints in (1, 0):
                gpu.set_option("repo_hints", hints)
                for skip in (1, 0):
                    gpu.set_option("ff_skip", skip)
                    st = _both_routes(gpu, b["bases"], b["offs"], b["exp"], b["ff"], b["sc"], (mode, kmer, hints, skip))
                    assert st.repositions == dst.repositions
                    steps[(kmer, hints, skip)] = st.lane_steps
                assert steps[(kmer, hints, 1)] <= steps[(kmer, hints, 0)], steps
            assert steps[(kmer, 1, 1)] <= steps[(kmer, 0, 1)], steps
        gpu.set_option("ff_skip", -1)
        gpu.set_option("repo_hints", 1)
        gpu.set_option("kmer_k", K)
        assert steps[(K, 1, 1)] <= dst.lane_steps, (steps, dst.lane_steps)
        # "chain_rows" 0 frees them: the deep rows again
        _chain(gpu, 0)
        out, st = gpu.query_pml_packed(b["bases"], b["offs"])
        assert gpu.last_launch()["ahead"] == 2 and (out == b["exp"]).all()
    finally:
        gpu.close()


def test_default_policy_keeps_the_deep_rows(golden):
    """The golden index sits in the caches: by itself the handle builds the deep rows and no chain rows, and walks on the deep rows."""
    import movi_amd
    b = golden[6]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare(gpu.PREPARE_PML)
        assert gpu.info("chain_rows_bytes") == 0 and gpu.info("deep_rows_bytes") > 0
        gpu.query_pml_mask_packed(b["bases"], b["offs"])
        li = gpu.last_launch()
        assert li["kernel"] == DEEP_MASK and li["ahead"] == 2, li
        gpu.set_option("chain_rows", -1)                        # the policy's own rule, said aloud: the same
        gpu.query_pml_mask_packed(b["bases"], b["offs"])
        assert gpu.last_launch()["kernel"] == DEEP_MASK and gpu.info("chain_rows_bytes") == 0
        for bad in (-2, 2):
            with pytest.raises(movi_amd.MoviError):
                gpu.set_option("chain_rows", bad)
    finally:
        gpu.close()


def test_long_reads_stay_off_the_chain_rows(golden):
    """Batches whose mean length is 1024 bases and more keep the look-ahead rows (and the LDS ring), chain rows or not."""
    import movi_amd
    ref = _ref()
    gpu = movi_amd.MoveIndex.from_image(golden[6]["img"])
    try:
        _chain(gpu)
        lb, lo = pack([ref[3000 * i: 3000 * i + 2000] for i in range(30)])
        gpu.query_pml_packed(lb, lo)
        assert gpu.last_launch()["ahead"] in (1, 2) and gpu.last_launch()["kernel"].startswith("pml_kernel_flatp<")
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------- 2. rolling reads, tiny tables
def test_reads_that_roll_through_the_staged_stretch(golden):
    """Reads of 130 .. 400 bases with 112 bases staged per lane ("waves_per_cu" 20): every read rolls, the roll looks three bases ahead."""
    import movi_amd
    from oracle.oracle import Oracle
    ref = _ref()
    bases, offs = pack(mutated_reads(np.random.default_rng(52001), ref, 400, 130, 401) + [ref[200:200 + L] for L in range(109, 120)])
    gpu, cpu = movi_amd.MoveIndex.from_image(golden[6]["img"]), Oracle(golden[6]["img"])
    try:
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
        _chain(gpu)
        gpu.set_option("waves_per_cu", 20)
        _both_routes(gpu, bases, offs, exp, ff, sc, "roll")
        assert gpu.last_launch()["staged"] == 112
    finally:
        gpu.close()
        cpu.close()


@pytest.mark.parametrize("r,unit", [(8, b"ACG"), (8, b"CTTG"), (9, b"TTC"), (9, b"CGTA"), (10, b"GTGG"), (10, b"ACGTA"), (11, b"GAATC"), (11, b"CGGTT")])
def test_tables_of_8_to_11_rows(built_lib, tmp_path, r, unit):
    """The smallest tables: with odd r the last window is padded, and every walk starts in it, at row r - 1; a 15-row hint would reach
    beyond either end."""
    import movi_amd
    from oracle.oracle import Oracle
    tool = os.path.join(ROOT, "tools", "build_index")
    if not os.path.exists(tool):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", tool, tool + ".cpp"])
    text = unit * 9
    fa = tmp_path / "t.fa"
    fa.write_bytes(b">s\n" + text + b"\n")
    subprocess.check_call([tool, "fasta", str(fa), "6", str(tmp_path / "i")], stderr=subprocess.DEVNULL)
    img = open(str(tmp_path / "i" / "index.movi"), "rb").read()
    rng = np.random.default_rng(r * 131 + len(unit))
    reads = [text[:L] for L in range(1, 20)]
    for _ in range(150):
        L = int(rng.integers(1, 60))
        p = int(rng.integers(0, max(1, len(text) - L)))
        s = bytearray(text[p:p + L])
        for k in range(len(s)):
            if rng.random() < 0.08:
                s[k] = b"ACGTN"[rng.integers(0, 5)]
        reads.append(bytes(s))
    bases, offs = pack(reads)
    gpu, cpu = movi_amd.MoveIndex.from_image(img), Oracle(img)
    try:
        assert gpu.desc.r == r
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=2)
        _chain(gpu)
        for kmer in (0, K):
            gpu.set_option("kmer_k", kmer)
            _both_routes(gpu, bases, offs, exp, ff, sc, (r, unit, kmer))
    finally:
        gpu.close()
        cpu.close()


# --------------------------------------------------------------------------------------------- 3. hinted scans, separators
@pytest.mark.parametrize("case", ["reach", "beyond"])
def test_hinted_scan_texts(built_lib, case):
    """The run sequences of tests/deep_hint_texts.py (scans that end 1 .. 16 and more rows beyond a window's edge, in both directions, at
    both ends of the table) under "repo_hints" 1 and 0: same answers, fewer lane steps with the hints."""
    import movi_amd
    from oracle.oracle import Oracle
    period, rule = (19, "any") if case == "reach" else (38, "avoid_4_15")
    img, c, up, end = _hint_table(period, 12 if case == "reach" else 8, rule)
    bases, offs = pack(_random_reads(np.random.default_rng(period), 600, 1, 120))
    gpu, cpu = movi_amd.MoveIndex.from_image(img), Oracle(img)
    try:
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=2)
        _chain(gpu)
        steps = {}
        for hints in (1, 0):
            gpu.set_option("repo_hints", hints)
            steps[hints] = _both_routes(gpu, bases, offs, exp, ff, sc, (case, hints)).lane_steps
        assert steps[1] < steps[0], steps
    finally:
        gpu.close()
        cpu.close()


def test_separators_index(built_lib):
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref = _ref()
    img = B.build_index_from_seqs([ref[:60000], ref[60000:]], 6, separators=True)
    reads = mutated_reads(np.random.default_rng(52002), ref, 400, 1, 400) + [ref[59990:60010], b"%", b"A%C", ref[59900:60100]]
    bases, offs = pack(reads)
    gpu, cpu = movi_amd.MoveIndex.from_image(img), Oracle(img)
    try:
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
        _chain(gpu)
        _both_routes(gpu, bases, offs, exp, ff, sc, "separators", sep=1)
    finally:
        gpu.close()
        cpu.close()


# ------------------------------------------------------------------------------------------------------------------ 4. corrupt ids
def test_corrupt_ids_at_each_depth(built_lib, golden_image):
    """Ids that are no row -- r, r + 5, the 28-bit "not a row" value itself, 2^32 - 1, and 2^28 + 5 and 2^31 + 7, which cut to 28 bits are
    rows 5 and 7: only the builder's comparison with r makes them "not a row" -- every 97th row from several starts, so that rows have
    their first invalid entry at depth 0, 1, 2, 3 and at j4: the reads that fail, their error codes and everything else as on the plain rows
    (a lane that meets such an id stops where it stands: the builder never lets a gather follow it)."""
    import movi_amd
    ref = _ref()
    img = bytearray(golden_image(6))
    d, _, off, _ = movi_amd.parse_index_image(bytes(img))
    rows = np.frombuffer(img, np.uint8, count=d.r * 8, offset=off).reshape(-1, 8).copy()
    ids = rows[:, 0:4].copy().view(np.uint32)[:, 0]
    for start, bad_id in ((0, d.r), (31, d.r + 5), (57, 0x0FFFFFFF), (71, 0xFFFFFFFF), (43, (1 << 28) + 5), (91, 0x80000007)):
        ids[start::97] = bad_id
    rows[:, 0:4] = ids.view(np.uint8).reshape(-1, 4)
    img[off: off + rows.size] = rows.tobytes()
    bad = movi_amd.MoveIndex.from_image(bytes(img))
    try:
        bases, offs = pack(mutated_reads(np.random.default_rng(52003), ref, 600, 20, 300))
        bad.set_option("ahead_rows", 0)
        bad.set_option("pml_via_mask", 0)
        bad.set_option("host_masks", 0)
        exp, est, eerr, erc = bad.query_pml_packed(bases, offs, want_err=True)
        assert bad.last_launch()["ahead"] == 0 and est.errors > 0 and erc != 0
        want = (exp, eerr, erc, (est.fast_forwards, est.scans, est.repositions, est.errors))
        _chain(bad)
        for skip in (1, 0):
            bad.set_option("ff_skip", skip)
            _both_routes(bad, bases, offs, None, None, None, ("corrupt", skip), want=want)
    finally:
        bad.close()
