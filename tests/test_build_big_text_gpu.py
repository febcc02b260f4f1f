"""GPU suite (-m gpu): the run-length BWT builder (movi_build_from_rlbwt, `movi build --preprocessed`) on texts of 2^31, 2^32 and 2^33
characters -- the texts it exists for.  A table that describes such a text is small (6001 runs, one of them giant; MAX_RUN_LENGTH
makes 0.5 M to 8.4 M rows of it), and every comparison is byte equality of the whole image with B.serialize(build_rows_rl(...)) of
tests/rlbwt_ref.py, the run-length restatement of oracle/build_index.py build_rows that tests/test_rlbwt_ref_cpu.py holds to
build_rows on every small text -- and which pins there what these tables contain: LF targets, row starts made by thresholds and
thresholds themselves past 2^32 (2^31), so that a position, a sort key or a sum kept in 32 bits anywhere in the builder shows here."""
import os
import subprocess

import numpy as np
import pytest

from oracle import build_index as B
import rlbwt_ref as R
from test_build_rlbwt_cpu import MOVI, write_rlbwt
from test_build_rlbwt_gpu import same

pytestmark = pytest.mark.gpu

CASES = ([("2^31", False, m) for m in (6, 3, 8, 2, 7, 5)] + [("2^32", False, m) for m in (6, 3, 8, 2, 7, 5)] +
         [("2^32", True, m) for m in (6, 8, 7)] + [("2^33", False, m) for m in (3, 6)])


@pytest.mark.parametrize("name,separators,mode", CASES)
def test_image_equals_the_run_length_reference(built_lib, name, separators, mode):
    import movi_amd
    n = R.BIG_N[name]
    heads, lens, thr, _ = R.big_table(n, separators)
    f, want = R.big_fields(n, separators, mode)
    got = movi_amd.build_image(heads, lens.astype(np.uint64), thr.astype(np.uint64) if mode in B.THRESHOLD_MODES else None, mode)
    assert same(got, want)
    # the header's n, also as the engine's parser hands it on
    assert int(np.frombuffer(got, "<u8", 1, 16)[0]) == n == int(lens.sum())
    desc = movi_amd.parse_index_image(got)[0]
    assert (desc.length, desc.r, desc.end_bwt_idx, desc.mode) == (n, f["r"], f["end_bwt_idx"], mode)


def spelled_reads(f, edge, count, rng):
    """Reads that occur in the text the table describes, out of the reference's fields alone: from a random row that starts past
    `edge`, emit the row's character and take the LF step, up to 300 times or until the terminator's row; the read is the
    emitted bytes reversed."""
    all_p, code, pp_id, offset, alphabet = f["all_p"], f["code"], f["pp_id"], f["offset"], f["alphabet"]
    rows = rng.choice(np.flatnonzero((all_p >= edge) & (np.arange(f["r"]) != f["end_bwt_idx"])), count, replace=False)
    want = rng.integers(1, 301, count)
    reads = []
    for row, k in zip(rows.tolist(), want.tolist()):
        pos, out = int(all_p[row]), bytearray()
        while len(out) < k and row != f["end_bwt_idx"]:
            out.append(alphabet[int(code[row])])
            pos = int(all_p[pp_id[row]]) + int(offset[row]) + (pos - int(all_p[row]))
            row = int(np.searchsorted(all_p, pos, side="right")) - 1
        reads.append(bytes(out[::-1]))
    return reads


def test_cli_build_and_queries_at_2_32(built_lib, tmp_path):
    """`movi build --preprocessed` from files whose 5-byte values have bit 32 set; the index it writes is the reference's image, and
    the engine answers PML, ZML and count batches on it like the oracle."""
    import movi_amd
    from oracle.oracle import Oracle
    n = R.BIG_N["2^32"]
    heads, lens, thr, edge = R.big_table(n, False)
    f, want = R.big_fields(n, False, 6)
    prefix, out = str(tmp_path / "ref"), str(tmp_path / "idx")
    write_rlbwt(prefix, heads, lens.astype(np.uint64), thr.astype(np.uint64))
    assert os.path.getsize(prefix + ".bwt.len") == 5 * heads.size and max(open(prefix + ".thr_pos", "rb").read()[4::5]) >= 1
    r = subprocess.run([MOVI, "build", "-i", out, "-f", prefix, "--preprocessed", "--type", "regular-thresholds"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert same(open(os.path.join(out, "index.movi"), "rb").read(), want)

    rng = np.random.default_rng(232)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = [bytes(acgt[rng.integers(0, 4, int(k))]) for k in rng.integers(1, 301, 200)]
    spelled = spelled_reads(f, edge, 200, rng)
    cpu = Oracle(want)
    assert (cpu.length, cpu.r) == (n, f["r"])
    # the condition, from the oracle alone: the spelled reads are matched, at least half of them 20 bases deep
    assert sum(1 for s in spelled if len(s) >= 20 and int(cpu.pml(s).max()) >= 20) >= len(spelled) // 2
    reads += spelled + [b"A", b"AA", b"A" * 300]                        # (the giant run: counts past 2^32)
    bases = np.frombuffer(b"".join(reads), np.uint8)
    offs = np.concatenate(([0], np.cumsum([len(s) for s in reads]))).astype(np.uint64)
    gpu = movi_amd.MoveIndex.load(out)
    try:
        assert (gpu.desc.length, gpu.desc.r) == (n, f["r"])
        # The two lookup tables at K = 6, not the K = 12 the first queries would build by themselves: their builders walk every K-mer
        # from the whole text, and a random 12-mer meets the giant run -- 2.1 M rows to scan for the next C, G or T -- often enough to
        # make 11 s and 8 s of 16 M of them on this table (K = 6: milliseconds, and the queries go through the tables all the same).
        gpu.set_option("kmer_k", 6)
        gpu.set_option("ftab_k", 6)
        pml, _ = gpu.query_pml_packed(bases, offs)
        assert (pml == cpu.pml_batch(bases, offs, threads=4)[0]).all()
        zml, _ = gpu.query_zml_packed(bases, offs)
        assert (zml == cpu.zml_batch(bases, offs, threads=4)).all()
        matched, count = gpu.query_count_packed(bases, offs)[:2]
        m, c = cpu.count_batch(bases, offs, threads=4)
        assert (np.asarray(matched) == m).all() and (np.asarray(count) == c).all()
        assert int(c.max()) >= edge                                  # counts that need their upper bits, too
    finally:
        gpu.close()
        cpu.close()
