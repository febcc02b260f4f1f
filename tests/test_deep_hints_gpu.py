"""GPU suite (-m gpu): the deep rows' two FIELD MAPS and their reposition hints ("deep_hint_bits" option; movi_deep_fields.hpp).  Tables of
at most 2^26 - 1 rows hold 26-bit ids and three 4-bit hints a row (reach 15) in the bytes that held 28-bit ids and 2-bit hints (reach 3).
A hint only says where a reposition scan that leaves the window ends (reposition_up / _down, src/move_structure_query.cpp:188-232), so
the u16 vector, the mask words, the per-read error bytes and the fast-forward / scan / reposition / error counters must be the oracle's
with "deep_hint_bits" 4, with 2 and with "repo_hints" 0 -- only lane steps may differ.  Every case runs all three.  The tables of 2^26
rows and more, which have the wide map only, and the ids whose bits 27:26 are set: test_deep_wide_ids_gpu.py, with _set and _three_ways."""
import os
import subprocess

import numpy as np
import pytest

import deep_hint_texts as D
from conftest import GOLDEN
from test_gpu_parity import check_segmented, mutated_reads, pack

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
MASK_KERNEL = "pml_kernel_flatp<6, unsigned int, 0, 0, 0, 1, 2, 0, 2>"
VECTOR_KERNEL = "pml_kernel_flatp<6, unsigned int, 0, 0, 0, 1, 2, 0, 0>"
SETTINGS = ((4, 1), (2, 1), (4, 0))          # ("deep_hint_bits", "repo_hints"): 4 bits, 2 bits, hints not looked at


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _set(gpu, bits, hints, built=None):
    """Build the deep rows with hints of `bits` bits (the option takes effect when they are next built) and switch the hints on or off.
    `built`: the width the rows must then have -- `bits`, or 2 whatever is asked on a table of 2^26 rows and more, which keeps wide ids."""
    gpu.set_option("deep_hint_bits", bits)
    gpu.set_option("deep_rows", 1)
    gpu.set_option("repo_hints", hints)
    assert int(gpu.info("deep_hint_bits")) == (bits if built is None else built)
    assert gpu.info("deep_rows_bytes") == ((gpu.desc.r + 2) // 3) * 64


def _three_ways(gpu, bases, offs, exp, ff, sc, tag, want=None, sep=0, wide_only=False):
    """Vector, mask words, error bytes and counters under the three SETTINGS, against the oracle's (exp, ff, sc) or -- a table on which
    reads fail -- against `want` = (vector, error bytes, rc, counters) of the walk on the plain rows.  `wide_only`: a table of 2^26 rows
    and more, whose rows are built with 2-bit hints under every setting.  Returns the lane steps by setting."""
    from movi_amd import engine as E
    steps, repos, first_words = {}, set(), None
    for bits, hints in SETTINGS:
        _set(gpu, bits, hints, 2 if wide_only else None)
        gpu.set_option("pml_via_mask", 0)                   # the vector from the walk itself
        gpu.set_option("host_masks", 0)
        out, st, err, rc = gpu.query_pml_packed(bases, offs, want_err=True)
        li = gpu.last_launch()
        assert li["ahead"] == 2 and li["kernel"] == VECTOR_KERNEL.replace("0, 0, 0, 1, 2", "0, %d, 0, 1, 2" % sep), (tag, li)
        words, mst, merr, mrc = gpu.query_pml_mask_packed(bases, offs, want_err=True)
        assert gpu.last_launch()["kernel"] == MASK_KERNEL.replace("0, 0, 0, 1, 2", "0, %d, 0, 1, 2" % sep), (tag, gpu.last_launch())
        c = (st.fast_forwards, st.scans, st.repositions, st.errors)
        assert c == (mst.fast_forwards, mst.scans, mst.repositions, mst.errors) and (err == merr).all() and rc == mrc, (tag, bits, hints)
        print("%s bits %d hints %d: lane steps %d, counters %s" % (tag, bits, hints, st.lane_steps, c))
        if want is None:
            assert (out == exp).all(), (tag, bits, hints, np.flatnonzero(out != exp)[:8])
            assert rc == 0 and (err == 0).all() and c[:2] == (ff, sc) and c[3] == 0, (tag, bits, hints, c, ff, sc)
            vec = exp
        else:
            assert (out == want[0]).all() and (err == want[1]).all() and rc == want[2] and c == want[3], (tag, bits, hints, c, want[3])
            vec = want[0]
        if want is None:
            mexp, valid = E.masks_of_pml(vec, offs)
            assert (words[valid] == mexp[valid]).all(), (tag, bits, hints, "mask words")
        first_words = words.copy() if first_words is None else first_words
        assert (words == first_words).all(), (tag, bits, hints, "mask words differ between the settings")
        repos.add(c[2])
        steps[(bits, hints)] = st.lane_steps
    assert len(repos) == 1, (tag, repos)
    assert steps[(4, 1)] <= steps[(2, 1)] <= steps[(4, 0)], (tag, steps)
    return steps


# ---------------------------------------------------------------------------------------------------------------- 1. golden index
@pytest.fixture(scope="module")
def golden_cases(built_lib, golden_image):
    """Per (index type, separators): image, batch and the oracle's answers -- computed once, shared, left unchanged."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref = _ref()
    rng = np.random.default_rng(41000)
    special = [b"A", ref[10:12], ref[300:313], b"N", b"N" * 20, ref[500:560] + b"N" + ref[561:640], ref[700:800].lower(),
               ref[900:950] + b"\x80\xff" + ref[952:1000], ref[59990:60010]]
    bases, offs = pack(special + mutated_reads(rng, ref, 400, 20, 330) + mutated_reads(rng, ref, 6, 700, 1100))
    out = {}
    for mode in (6, 7, 8):
        for sep in (0, 1):
            if sep:
                img = B.build_index_from_seqs([ref[:60000], ref[60000:]], mode, separators=True)
            else:
                img = golden_image(mode) if mode != 7 else B.build_index_from_seqs([ref], 7)
            cpu = Oracle(img)
            exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
            cpu.close()
            out[(mode, sep)] = dict(img=img, bases=bases, offs=offs, exp=exp, ff=ff, sc=sc)
    return out


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("mode", [6, 7, 8])
def test_golden_index(golden_cases, mode, sep):
    import movi_amd
    b = golden_cases[(mode, sep)]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        steps = _three_ways(gpu, b["bases"], b["offs"], b["exp"], b["ff"], b["sc"], (mode, sep), sep=sep)
        if not sep:                                         # (an index with separators carries no hints)
            assert steps[(2, 1)] < steps[(4, 0)]
    finally:
        gpu.close()


@pytest.mark.parametrize("mode", [6, 8])
def test_golden_index_segments(golden_cases, mode):
    """The segment walk sets the width of a hint on a line of its own: the batch's long reads cut into 32-base segments, on the deep rows
    ("deep" 1) under the three SETTINGS."""
    import movi_amd
    b = golden_cases[(mode, 0)]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.set_option("deep", 1)
        for bits, hints in SETTINGS:
            _set(gpu, bits, hints)
            check_segmented(gpu, b["bases"], b["offs"], b["exp"], b["ff"], b["sc"], (mode, bits, hints))
            assert gpu.last_launch()["ahead"] == 2, (mode, bits, hints, gpu.last_launch())
    finally:
        gpu.set_option("deep", -1)
        gpu.close()


# ------------------------------------------------------------------------------------------------------------- 2. small indexes
# tandem repeats whose indexes (with their reverse complements) have 8 .. 14 rows, by the letters of the fuzzed texts they go with
SMALL_UNITS = {b"ACGT": (b"ATC", b"AACGC", b"ACCGA", b"ATTAAC"), b"ACG": (b"ACG", b"AACGC", b"ACCGA"), b"AT": (b"ATTTT", b"ATAA", b"ATATAA", b"ATTAT")}


@pytest.mark.parametrize("alphabet", [b"ACGT", b"ACG", b"AT"])
def test_fuzz_small_indexes(built_lib, tmp_path, alphabet):
    """Tiny indexes (reduced alphabets, long runs split at MAX_RUN_LENGTH, the terminator row in odd places, every residue of r modulo 3)
    and the smallest tables there are -- tandem repeats with 8 .. 20 rows, where a 15-row hint would reach beyond either end."""
    import movi_amd
    from oracle.oracle import Oracle
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "build_index")
    if not os.path.exists(tool):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", tool, tool + ".cpp"])
    rng = np.random.default_rng(len(alphabet) * 91 + alphabet[1])
    texts = []
    for trial in range(4):
        recs = []
        for _ in range(int(rng.integers(1, 4))):
            unit = bytes(rng.choice(list(alphabet), size=int(rng.integers(5, 400))).astype(np.uint8))
            recs.append(unit * int(rng.integers(1, 6)) + bytes([alphabet[0]]) * int(rng.integers(0, 3000)))
        texts.append(recs)
    for u in SMALL_UNITS[alphabet]:
        texts.append([u * 9])
    seen_r, small = set(), 0
    for trial, recs in enumerate(texts):
        fa = tmp_path / ("f%d.fa" % trial)
        fa.write_bytes(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(recs)))
        text = b"".join(recs)
        reads = []
        for _ in range(120):
            L = int(rng.integers(1, 200))
            p = int(rng.integers(0, max(1, len(text) - L)))
            r = bytearray(text[p:p + L])
            for k in range(len(r)):
                if rng.random() < 0.08:
                    r[k] = b"ACGTN"[rng.integers(0, 5)]
            reads.append(bytes(r))
        bases, offs = pack(reads)
        out_dir = str(tmp_path / ("i%d" % trial))
        subprocess.check_call([tool, "fasta", str(fa), "6", out_dir], stderr=subprocess.DEVNULL)
        img = open(os.path.join(out_dir, "index.movi"), "rb").read()
        gpu, cpu = movi_amd.MoveIndex.from_image(img), Oracle(img)
        try:
            if gpu.desc.r < 8:
                continue
            seen_r.add(gpu.desc.r % 3)
            small += 8 <= gpu.desc.r <= 20
            exp, ff, sc = cpu.pml_batch(bases, offs, threads=2)
            _three_ways(gpu, bases, offs, exp, ff, sc, (alphabet, trial, gpu.desc.r))
        finally:
            gpu.close()
            cpu.close()
    assert len(seen_r) >= 2 and small >= 3, (seen_r, small)


# ------------------------------------------------------------------------------------- 3. targets 3, 4, 15 and 16 rows beyond the edge
def _hint_table(period, periods, rule):
    """An index built from deep_hint_texts' run sequence, with the rows' threshold bits set so that every scan has a run to end at
    (choose_directions) -> (image, letter codes of the rows, up bits, the terminator's row)."""
    import movi_amd
    from movi_amd import engine as E
    codes = D.run_heads(period, periods)
    rng = np.random.default_rng(period)
    heads = np.array([D.LETTER[int(c)] for c in codes], np.uint8)
    lens = np.where(codes == D.END, 1, rng.integers(1, 4, codes.size)).astype(np.uint64)
    img = bytearray(E.build_image(heads, lens, np.zeros(codes.size, np.uint64), 6))
    d, _, off, _ = movi_amd.parse_index_image(bytes(img))
    assert d.r == codes.size                                 # one row per run
    raw = np.frombuffer(img, np.uint8, count=d.r * 8, offset=off).reshape(-1, 8).copy()
    w4, w6 = raw[:, 4:6].copy().view(np.uint16)[:, 0], raw[:, 6:8].copy().view(np.uint16)[:, 0]
    c = (w4 >> 13).astype(np.int64)                          # the table's own letter codes (the builder's hints go by them)
    end = int(d.end_bwt_idx)
    keep = np.arange(d.r) != end
    assert (c[keep] == codes[keep]).all()
    up = D.choose_directions(c, rule, seed=period, end=end)
    w6 = (w6 & ~np.uint16(1 << 11)) | (up[:, 0].astype(np.uint16) << 11)            # thr0
    w4 = (w4 & ~np.uint16(3 << 11)) | (up[:, 1].astype(np.uint16) << 11) | (up[:, 2].astype(np.uint16) << 12)   # thr1, thr2
    w4[end], w6[end] = raw[end, 4:6].copy().view(np.uint16)[0], raw[end, 6:8].copy().view(np.uint16)[0]
    raw[:, 4:6] = w4.view(np.uint8).reshape(-1, 2)
    raw[:, 6:8] = w6.view(np.uint8).reshape(-1, 2)
    img[off: off + raw.size] = raw.tobytes()
    return bytes(img), c, up, end


def _random_reads(rng, n, lo, hi):
    return [bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(lo, hi))).astype(np.uint8)) for _ in range(n)]


@pytest.mark.parametrize("case", ["reach", "beyond"])
def test_targets_at_the_reach(built_lib, case):
    """"reach": Gs and Ts 19 rows apart -- scans that end exactly 3, 4, 15 and 16 rows beyond the window's edge, upwards and downwards, with
    targets in the first and in the last window: 4-bit hints jump where 2-bit hints walk, so the lane steps fall.  "beyond": 38 rows
    apart and directions chosen so that no scan ends 4 .. 15 rows out, though some end exactly 3 and exactly 16 rows out: a 16-row scan
    is beyond 4 bits too, and the lane steps are the same."""
    import movi_amd
    from oracle.oracle import Oracle
    period, rule = (19, "any") if case == "reach" else (38, "avoid_4_15")
    img, c, up, end = _hint_table(period, 12 if case == "reach" else 8, rule)
    dist = D.distances(c, up, end=end)
    last_win = (len(c) - 1) // 3 * 3
    for way in ("up", "down"):
        for e in (3, 4, 15, 16) if case == "reach" else (3, 16):
            assert dist.get((way, e)), (case, way, e)
    if case == "reach":
        far = [x for (way, e), v in dist.items() if 4 <= e <= 15 for x in v]
        assert any(t < 3 for _, _, t in far) and any(t >= last_win for _, _, t in far)
    else:
        assert not any(4 <= e <= 15 for _, e in dist)
    bases, offs = pack(_random_reads(np.random.default_rng(period), 600, 1, 120))
    gpu, cpu = movi_amd.MoveIndex.from_image(img), Oracle(img)
    try:
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=2)
        steps = _three_ways(gpu, bases, offs, exp, ff, sc, case)
        if case == "reach":
            assert steps[(4, 1)] < steps[(2, 1)] < steps[(4, 0)], steps
        else:
            assert steps[(4, 1)] == steps[(2, 1)] < steps[(4, 0)], steps
    finally:
        gpu.close()
        cpu.close()


# ------------------------------------------------------------------------------------------------------------------ 4. corrupt ids
def test_corrupt_ids(built_lib, golden_image):
    """Ids that are no row -- the 26-bit "not a row" value itself, r, r + 5, 2^28 - 1, 2^32 - 1, and 2^26 + 5, 2^28 + 5, 2^31 + 7, which
    cut to 26 or 28 bits are rows 5 and 7: only the builder's comparison with r makes them "not a row", a mask would not -- at rows whose
    entries of depth one and two become invalid at different places: the reads that fail, their error codes and everything else as on
    the plain rows."""
    import movi_amd
    ref = _ref()
    img = bytearray(golden_image(6))
    d, _, off, _ = movi_amd.parse_index_image(bytes(img))
    rows = np.frombuffer(img, np.uint8, count=d.r * 8, offset=off).reshape(-1, 8).copy()
    ids = rows[:, 0:4].copy().view(np.uint32)[:, 0]
    for start, bad_id in ((0, 0x03FFFFFF), (31, d.r), (57, d.r + 5), (71, 0x0FFFFFFF), (83, 0xFFFFFFFF),
                          (13, (1 << 26) + 5), (43, (1 << 28) + 5), (91, 0x80000007)):
        ids[start::97] = bad_id
    rows[:, 0:4] = ids.view(np.uint8).reshape(-1, 4)
    img[off: off + rows.size] = rows.tobytes()
    bad = movi_amd.MoveIndex.from_image(bytes(img))
    try:
        bases, offs = pack(mutated_reads(np.random.default_rng(41001), ref, 600, 20, 300))
        bad.set_option("ahead_rows", 0)
        bad.set_option("pml_via_mask", 0)
        bad.set_option("host_masks", 0)
        exp, est, eerr, erc = bad.query_pml_packed(bases, offs, want_err=True)
        assert bad.last_launch()["ahead"] == 0 and est.errors > 0 and erc != 0
        want = (exp, eerr, erc, (est.fast_forwards, est.scans, est.repositions, est.errors))
        _three_ways(bad, bases, offs, None, None, None, "corrupt", want=want)
    finally:
        bad.close()


# ---------------------------------------------------------------------------------------------------------------- 5. parked lanes
def test_parked_lanes_on_the_narrow_map(golden_cases):
    """"park_lanes" 8 on both maps: the first launch parks a wavefront's last lanes, the second resumes them -- same kernel, same answers."""
    import movi_amd
    import torch
    b = golden_cases[(6, 0)]
    n, nb = b["offs"].size - 1, int(b["bases"].size)
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare(gpu.PREPARE_PML)
        gpu.set_option("pml_via_mask", 1)
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        for bits in (4, 2):
            _set(gpu, bits, 1)
            got = {}
            for T in (0, 8):
                gpu.set_option("park_lanes", T)
                out = torch.full((nb + 8,), SENT, dtype=torch.int16, device="cuda")
                err = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
                gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), err.data_ptr())
                st = gpu.last_stats()
                v = out.cpu().numpy().view(np.uint16)
                assert (v[nb:] == SENT).all() and (v[:nb] == b["exp"]).all() and (err.cpu().numpy() == 0).all(), (bits, T)
                assert gpu.last_launch()["kernel"] == MASK_KERNEL and gpu.last_launch()["ahead"] == 2
                assert int(gpu.info("park_lanes")) == T and (int(gpu.info("parked_reads")) > 0) == (T > 0), (bits, T)
                got[T] = (st.fast_forwards, st.scans, st.repositions, st.errors)
            assert got[0] == got[8] and got[0][:2] == (b["ff"], b["sc"]) and got[0][3] == 0, (bits, got)
    finally:
        gpu.close()


# -------------------------------------------------------------------------------------------------------- 6. what must not change
def test_names_and_sizes(golden_cases):
    import movi_amd
    b = golden_cases[(6, 0)]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        assert int(gpu.info("deep_hint_bits")) == 0            # no deep rows yet
        gpu.prepare(gpu.PREPARE_PML)
        auto = int(gpu.info("deep_hint_bits"))
        assert auto in (2, 4)                                  # "deep_hint_bits" -1: the library's default
        for bits in (4, 2):
            gpu.set_option("deep_hint_bits", bits)
            assert int(gpu.info("deep_hint_bits")) == auto     # takes effect when the deep rows are next built ...
            gpu.set_option("deep_rows", 1)                     # ... as here
            assert int(gpu.info("deep_hint_bits")) == bits
            assert gpu.info("deep_rows_bytes") == ((gpu.desc.r + 2) // 3) * 64
            gpu.query_pml_mask_packed(b["bases"], b["offs"])
            li = gpu.last_launch()
            assert li["kernel"] == MASK_KERNEL and li["ahead"] == 2, li
        gpu.set_option("deep_hint_bits", -1)
        gpu.set_option("deep_rows", 1)
        assert int(gpu.info("deep_hint_bits")) == auto
        for bad in (0, 1, 3, 6, 8):
            with pytest.raises(movi_amd.MoviError):
                gpu.set_option("deep_hint_bits", bad)
    finally:
        gpu.close()
