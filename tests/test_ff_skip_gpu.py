"""GPU suite (-m gpu): the FAST-FORWARD SKIP of the PML walk ("ff_skip" option; DevIndex::ff_skip).  A row of the look-ahead / deep rows
carries n(j) of its LF target j (and, deep rows, n(j2) of j's target).  Where the offset arrives at or beyond it the reference's next
action is decided whatever the next base is -- LF_move lands on j and fast_forward passes it (src/move_structure.cpp:524-545) -- so the
walk gathers the window of j + 1 with that fast-forward taken instead of j's.  Vectors, mask words, error bytes and the fast-forward /
scan / reposition counters must be what they are with "ff_skip" 0 and what the oracle says; only lane steps fall.  Every case asserts
that they do fall, so none is vacuous.  The smallest tables are checked against a host-side walk of the table that says which
situations the batch holds (the offset exactly n(j) and one below it, j first / middle / last of its window, j = r - 2 and r - 1, a skip
at level 2, a skip followed by further fast-forwards inside and beyond the window).  On a consistent table a walk that lands on row
r - 1 has an offset below n(r - 1), so the `j < r - 1` guard is reached for real only on the corrupt table."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, classify_py
from test_gpu_parity import mutated_reads, pack

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
LAYOUTS = {"deep": ("deep_rows", 2, 2, 3), "ahead": ("ahead_rows", 1, 1, 4)}   # option, last_launch()["ahead"], entry depth S, rows per window W


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def _layout(gpu, rows):
    gpu.set_option(LAYOUTS[rows][0], 1)
    return LAYOUTS[rows][1]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _query(gpu, bases, offs, skip, masks):
    """One host call at "ff_skip" `skip` -> (vector or mask words, error bytes, rc, counters, lane steps, last_launch)."""
    gpu.set_option("ff_skip", skip)
    if masks:
        res, st, err, rc = gpu.query_pml_mask_packed(bases, offs, want_err=True)
    else:
        res, st, err, rc = gpu.query_pml_packed(bases, offs, want_err=True)
    assert int(gpu.info("ff_skip")) == skip
    return res.copy(), err.copy(), rc, (st.fast_forwards, st.scans, st.repositions, st.errors), st.lane_steps, gpu.last_launch()


def _ab(gpu, bases, offs, want_ahead, exp, ff, sc, masks, tag, fewer=True):
    """"ff_skip" 0 against 1 against the oracle's vector (None: 0 against 1 only); returns (lane steps without, with)."""
    from movi_amd import engine as E
    r0, e0, rc0, c0, l0, li0 = _query(gpu, bases, offs, 0, masks)
    r1, e1, rc1, c1, l1, li1 = _query(gpu, bases, offs, 1, masks)
    print("%s masks %d: lane steps %d -> %d, counters %s" % (tag, masks, l0, l1, c1))
    assert li0["ahead"] == li1["ahead"] == want_ahead and li0["kernel"] == li1["kernel"], (tag, li0, li1)
    assert (r0 == r1).all() and (e0 == e1).all() and rc0 == rc1 and c0 == c1, (tag, masks, c0, c1)
    if exp is not None:
        if masks:
            mexp, valid = E.masks_of_pml(exp, offs)
            assert (r1[valid] == mexp[valid]).all(), (tag, "mask words")
        else:
            assert (r1 == exp).all(), (tag, np.flatnonzero(r1 != exp)[:8])
        assert (e1 == 0).all() and rc1 == 0 and c1[:2] == (ff, sc) and c1[3] == 0, (tag, c1, ff, sc)
    assert l1 < l0 if fewer else l1 <= l0, (tag, masks, l0, l1)
    return l0, l1


def _vector_from_the_walk(gpu):
    gpu.set_option("pml_via_mask", 0)                       # the vector itself (register packer), not masks expanded on the host
    gpu.set_option("host_masks", 0)


# ---------------------------------------------------------------------------------------------------------------- golden index
def _golden_reads(ref):
    rng = np.random.default_rng(31000)
    special = [b"A", ref[10:12], ref[100:107], ref[200:212], ref[300:313], ref[1100:1113].lower(), b"N", b"N" * 20,
               ref[500:560] + b"N" + ref[561:640], ref[700:800].lower(), ref[900:950] + b"\x80\xff" + ref[952:1000], b"acgtn" * 9]
    return special + mutated_reads(rng, ref, 300, 20, 330)


@pytest.fixture(scope="module")
def golden_batches(built_lib, golden_image):
    """Per index type: image, batch and the oracle's answers -- computed once, shared, left unchanged."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref = _ref()
    bases, offs = pack(_golden_reads(ref))
    out = {}
    for mode in (6, 8, 7):
        img = golden_image(mode) if mode != 7 else B.build_index_from_seqs([ref], 7)
        cpu = Oracle(img)
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
        cpu.close()
        out[mode] = dict(img=img, bases=bases, offs=offs, exp=exp, ff=ff, sc=sc)
    return out


@pytest.mark.parametrize("rows", ["deep", "ahead"])
@pytest.mark.parametrize("mode", [6, 8, 7])
def test_golden_index(golden_batches, mode, rows):
    import movi_amd
    b = golden_batches[mode]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        want = _layout(gpu, rows)
        _vector_from_the_walk(gpu)
        for masks in (0, 1):
            _ab(gpu, b["bases"], b["offs"], want, b["exp"], b["ff"], b["sc"], masks, (mode, rows))
        gpu.set_option("ff_skip", -1)                       # the policy: the layout's default
        gpu.query_pml_packed(b["bases"], b["offs"])
        assert int(gpu.info("ff_skip")) in (0, 1)
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------------------- smallest tables
# Tandem repeats (the last four over two letters): r = 8 .. 14 rows with their reverse complements, every residue of r modulo 3 and 4
SMALL_UNITS = (b"ATC", b"ATTTT", b"ATTAT", b"ATCTAT", b"ATAA", b"ATTAAC", b"ATTTC", b"ATCAC", b"ATCCCA", b"ATATAA")


def _table(img):
    """Host-side view of an index of regular-thresholds rows (8 bytes: id[31:0]; n | thr1 << 11 | thr2 << 12 | c << 13; off | thr0 << 11 | id[35:32] << 12)."""
    import movi_amd
    d, _, off, _ = movi_amd.parse_index_image(img)
    raw = np.frombuffer(img, np.uint8, count=d.r * 8, offset=off).reshape(-1, 8)
    lo = raw[:, 0:4].copy().view(np.uint32)[:, 0].astype(np.int64)
    w4 = raw[:, 4:6].copy().view(np.uint16)[:, 0].astype(np.int64)
    w6 = raw[:, 6:8].copy().view(np.uint16)[:, 0].astype(np.int64)
    return dict(code_of=d.code_of, r=d.r, end=d.end_bwt_idx, end_thr=list(d.end_bwt_idx_thresholds), n=w4 & 0x7FF, c=w4 >> 13, off=w6 & 0x7FF,
                id=lo | ((w6 >> 12) << 32), thr=np.stack([(w6 >> 11) & 1, (w4 >> 11) & 1, (w4 >> 12) & 1], 1))


def _situations(T, reads, S, W):
    """The reference's walk of `reads` over table T (LF_move, fast_forward, match / reposition scan) with the kernel's entry chain beside
    it (an entry S levels deep, windows of W rows, no top-of-walk table): how often each situation of the skip rule occurs, and the PMLs
    and fast-forward total of the walk, which the caller holds to the oracle's."""
    r, n, c, roff, rid, thr = T["r"], T["n"], T["c"], T["off"], T["id"], T["thr"]
    code = {b: T["code_of"][b] for b in range(256) if T["code_of"][b] < 4}
    seen, pmls, fft = {}, [], 0

    def note(k):
        seen[k] = seen.get(k, 0) + 1
    for rd in reads:
        L = len(rd)
        idx, off, chain, ml, row = r - 1, int(n[r - 1]) - 1, 0, 0, []
        for k in range(L):
            a = code.get(rd[L - 1 - k], -1)
            rode = False
            if k:
                j = int(rid[idx])
                off_e = off + int(roff[idx])
                nj = int(n[j])
                off, jj, ff = off_e, j, 0
                while jj < r - 1 and off >= n[jj]:
                    off -= int(n[jj])
                    jj += 1
                    ff += 1
                fft += ff
                if chain > 0:                               # the LF was taken from an entry that holds n(j)
                    level = S - chain + 1
                    if j == r - 1:
                        note("lf_to_last_row")
                    if off_e >= nj and j < r - 1:
                        note("skip")
                        note("skip_level%d" % level)
                        note("skip_pos%d" % (0 if j % W == 0 else (2 if j % W == W - 1 else 1)))
                        if off_e == nj:
                            note("skip_exact")
                        if j == r - 2:
                            note("skip_to_last_row")
                        if (j + 1) // W > j // W:
                            note("saves")                   # j is its window's last row: the skipped gather learnt only "next window"
                        if (W == 3 and (j + 1) // 3 == (r - 1) // 3) or (W == 4 and j + 1 >= r - 4):
                            note("skip_into_last_window")   # padded (deep rows) / pulled back (look-ahead rows)
                        if ff > 1 and jj // W == (j + 1) // W:
                            note("skip_then_inwin")
                        if ff > 1 and jj // W > (j + 1) // W:
                            note("skip_then_outwin")
                    elif off_e == nj - 1:
                        note("noskip_below")
                if chain > 0 and ff == 0 and a >= 0 and c[j] == a:
                    rode = True
                    chain -= 1
                else:
                    chain = 0
                idx = jj
            if rode:
                ml += 1
                row.append(ml)
                continue
            chain = S
            if a < 0:
                ml = 0
                row.append(0)
                continue
            if c[idx] == a:
                ml += 1
                row.append(ml)
                continue
            ml = 0
            row.append(0)
            if idx == T["end"]:
                down = off >= T["end_thr"][a]
            else:
                cc = int(c[idx])
                down = off >= (int(n[idx]) if thr[idx][min((a - (1 if a > cc else 0)) & 3, 2)] else 0)
            if down:
                idx += 1
                while idx < r - 1 and c[idx] != a:
                    idx += 1
                off = 0
            else:
                idx -= 1
                while idx > 0 and c[idx] != a:
                    idx -= 1
                off = int(n[idx]) - 1
            assert 0 <= idx < r and c[idx] == a, "the batch holds no read whose walk throws"
        pmls.extend(row)
    return seen, np.array(pmls, np.uint16), fft


@pytest.fixture(scope="module")
def small_tables(built_lib):
    from oracle import build_index as B
    from oracle.oracle import Oracle
    out = []
    for unit in SMALL_UNITS:
        text = unit * 20
        img = B.build_index_from_seqs([text], 6)
        full = text + bytes(B.clean_text([text])[len(text):-1])     # ... and its reverse complement
        reads = [full[p:p + l] for l in (2, 3, 5, 8, 13, 21, 40) for p in range(0, len(full) - l, len(full) // 12)]
        reads += [reads[7][:3] + b"N" + reads[7][4:], reads[40][:9] + b"n" + reads[40][10:], b"N", b""]
        bases, offs = pack(reads)
        cpu = Oracle(img)
        exp, ff, sc = cpu.pml_batch(bases, offs, threads=2)
        cpu.close()
        out.append(dict(unit=unit, img=img, reads=reads, bases=bases, offs=offs, exp=exp, ff=ff, sc=sc, T=_table(img)))
    return out


@pytest.mark.parametrize("rows", ["deep", "ahead"])
def test_smallest_tables(small_tables, rows):
    import movi_amd
    _, want, S, W = LAYOUTS[rows]
    union, mods, saving = set(), set(), 0
    for t in small_tables:
        r = t["T"]["r"]
        assert 8 <= r <= 14, (t["unit"], r)
        mods.add((r % 3, r % 4))
        seen, pml, fft = _situations(t["T"], t["reads"], S, W)
        assert (pml == t["exp"]).all() and fft == t["ff"], t["unit"]      # the host-side walk is the oracle's walk
        assert seen.get("skip", 0) > 0, t["unit"]
        union |= set(seen)
        saving += seen.get("saves", 0) > 0
        gpu = movi_amd.MoveIndex.from_image(t["img"])
        try:
            assert _layout(gpu, rows) == want
            _vector_from_the_walk(gpu)
            for K in (0, 12) if b"C" in t["unit"] else (0,):     # (the top-of-walk table serves ACGT indexes only)
                gpu.set_option("kmer_k", K)
                for masks in (0, 1):
                    _ab(gpu, t["bases"], t["offs"], want, t["exp"], t["ff"], t["sc"], masks, (t["unit"], r, rows, K),
                        fewer=K == 0 and seen.get("saves", 0) > 0)
        finally:
            gpu.close()
    assert {m[0] for m in mods} == {0, 1, 2} and {m[1] for m in mods} == {0, 1, 2, 3}, mods
    need = {"skip_exact", "noskip_below", "skip_pos0", "skip_pos1", "skip_pos2", "skip_to_last_row", "lf_to_last_row", "skip_into_last_window",
            "skip_then_inwin", "skip_then_outwin", "saves"} | ({"skip_level2"} if S == 2 else set())
    assert need <= union, need - union
    assert saving >= len(small_tables) - 2, saving          # (an 8-row table has no four-row window whose last row is skipped to)


# -------------------------------------------------------------------------------------------- corrupt table, separators index
@pytest.mark.parametrize("rows", ["deep", "ahead"])
def test_corrupt_table(built_lib, golden_image, rows):
    """Every 97th id is no row: entries of depth one and two are invalid at different rows, and `jj < r - 1` fails for an id that is none.
    Same error codes, zeroed reads and counters with 0 and 1 -- and as on the plain rows."""
    import movi_amd
    ref = _ref()
    img = bytearray(golden_image(6))
    _, _, off, _ = movi_amd.parse_index_image(bytes(img))
    tab = np.frombuffer(img, np.uint8, count=118209 * 8, offset=off).reshape(-1, 8).copy()
    tab[::97, 0:4] = 0xFF
    img[off: off + tab.size] = tab.tobytes()
    bases, offs = pack(mutated_reads(np.random.default_rng(9801), ref, 400, 20, 300))
    bad = movi_amd.MoveIndex.from_image(bytes(img))
    try:
        bad.set_option("ahead_rows", 0)
        exp, est, eerr, erc = bad.query_pml_packed(bases, offs, want_err=True)
        assert est.errors > 0 and erc != 0
        want = _layout(bad, rows)
        _vector_from_the_walk(bad)
        for masks in (0, 1):
            _ab(bad, bases, offs, want, None, 0, 0, masks, ("corrupt", rows))
        out, err, rc, c, _, _ = _query(bad, bases, offs, 1, 0)
        assert (out == exp).all() and (err == eerr).all() and rc == erc
        assert c == (est.fast_forwards, est.scans, est.repositions, est.errors)
        for i in np.flatnonzero(err != 0):
            assert (out[int(offs[i]):int(offs[i + 1])] == 0).all()
    finally:
        bad.close()


@pytest.mark.parametrize("rows", ["deep", "ahead"])
def test_separators_index(built_lib, rows):
    import movi_amd
    from oracle import build_index as B
    from oracle.oracle import Oracle
    ref = _ref()
    img = B.build_index_from_seqs([ref[:60000], ref[60000:]], 6, separators=True)
    reads = mutated_reads(np.random.default_rng(9800), ref, 300, 20, 330) + [ref[59990:60010], b"%", b"A%C"]
    bases, offs = pack(reads)
    cpu = Oracle(img)
    exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
    cpu.close()
    gpu = movi_amd.MoveIndex.from_image(img)
    try:
        want = _layout(gpu, rows)
        _vector_from_the_walk(gpu)
        for masks in (0, 1):
            _ab(gpu, bases, offs, want, exp, ff, sc, masks, ("separators", rows))
    finally:
        gpu.close()


# ----------------------------------------------------------------------------------------------- the paths that share the code
def _pml_device(gpu, d_bases, d_offs, n, nb, stream=0):
    import torch
    out = torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
    err = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), err.data_ptr(), stream)
    st = gpu.last_stats(stream)
    return out.cpu().numpy().view(np.uint16).copy(), err.cpu().numpy().copy(), (st.fast_forwards, st.scans, st.repositions, st.errors), st.lane_steps


def test_parked_lanes_after_a_skip(golden_batches):
    """Deep rows, "park_lanes" 8: a lane parked right after a skip resumes at j + 1 with ff_run = 1 and the offset already reduced."""
    import movi_amd
    b = golden_batches[6]
    n, nb = b["offs"].size - 1, int(b["bases"].size)
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare(gpu.PREPARE_PML)
        gpu.set_option("deep_rows", 1)
        gpu.set_option("pml_via_mask", 1)
        gpu.set_option("park_lanes", 8)
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        got = {}
        for skip in (0, 1):
            gpu.set_option("ff_skip", skip)
            got[skip] = _pml_device(gpu, d_bases, d_offs, n, nb)
            assert int(gpu.info("parked_reads")) > 0 and int(gpu.info("park_lanes")) == 8 and int(gpu.info("ff_skip")) == skip
            assert gpu.last_launch()["ahead"] == 2
            v, e, c, _ = got[skip]
            assert (v == b["exp"]).all() and (e == 0).all() and c[:2] == (b["ff"], b["sc"]) and c[3] == 0, skip
        assert got[0][2] == got[1][2] and got[1][3] < got[0][3], (got[0][2:], got[1][2:])
    finally:
        gpu.close()


def test_pair_shared_gathers(golden_batches):
    """Look-ahead rows with "pair_loads" 1 (PSH = 1): the pair's exchanged windows and entries feed the same rule."""
    import movi_amd
    b = golden_batches[6]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        want = _layout(gpu, "ahead")
        _vector_from_the_walk(gpu)
        gpu.set_option("pair_loads", 1)
        for masks in (0, 1):
            _ab(gpu, b["bases"], b["offs"], want, b["exp"], b["ff"], b["sc"], masks, "pairs")
        assert ", 1, 1, 1, " in gpu.last_launch()["kernel"], gpu.last_launch()      # STG, AHD, PSH
    finally:
        gpu.close()


def test_segment_plan_on_look_ahead_rows(built_lib, golden_image):
    """Reads of 2 - 3 kbp cut into 256-base segments: K1's checkpoints are taken before the LF, so the stitched vector and the
    counters are the oracle's with the rule on."""
    import movi_amd
    from oracle.oracle import Oracle
    ref = _ref()
    img = golden_image(6)
    bases, offs = pack(mutated_reads(np.random.default_rng(31001), ref, 96, 2000, 3000))
    cpu = Oracle(img)
    exp, ff, sc = cpu.pml_batch(bases, offs, threads=4)
    cpu.close()
    gpu = movi_amd.MoveIndex.from_image(img)
    try:
        want = _layout(gpu, "ahead")
        gpu.set_option("seg_len", 256)
        gpu.set_option("seg_probe", 0)
        got = {}
        for skip in (0, 1):
            gpu.set_option("ff_skip", skip)
            out, st = gpu.query_pml_packed(bases, offs)
            li = gpu.last_launch()
            assert li["segmented"] == 1 and li["ahead"] == want and st.segments > offs.size - 1 and int(gpu.info("ff_skip")) == skip
            assert (out == exp).all() and (st.fast_forwards, st.scans, st.errors) == (ff, sc, 0), skip
            got[skip] = (st.repositions, st.lane_steps)
        assert got[0][0] == got[1][0] and got[1][1] < got[0][1], got
    finally:
        gpu.close()


@pytest.mark.parametrize("rows", ["deep", "ahead"])
def test_fused_classify(golden_batches, rows):
    """Bins fused into the walk, with the vector (CLS 1) and without (CLS 2)."""
    import movi_amd
    import torch
    b = golden_batches[6]
    offs, exp = b["offs"], b["exp"]
    n, nb = offs.size - 1, int(b["bases"].size)
    want_bins = [classify_py(exp[int(offs[i]):int(offs[i + 1])], 4, 40) for i in range(n)]
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        want = _layout(gpu, rows)
        gpu.set_option("classify_fused", 1)
        d_bases, d_offs = _dev(b["bases"]), _dev(offs.view(np.int64))
        for with_vector in (True, False):
            lanes = {}
            for skip in (0, 1):
                gpu.set_option("ff_skip", skip)
                d_out = torch.zeros(nb, dtype=torch.int16, device="cuda")
                d_a = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                d_b = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                d_s = torch.full((n,), -1, dtype=torch.int64, device="cuda")
                gpu.pml_classify_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, 40, 4, d_out.data_ptr() if with_vector else 0,
                                        d_a.data_ptr(), d_b.data_ptr(), d_s.data_ptr())
                torch.cuda.synchronize()
                st, li = gpu.last_stats(), gpu.last_launch()
                assert li["ahead"] == want and li["kernel"].startswith("pml_kernel_flatp<6, unsigned int, %d," % (1 if with_vector else 2)), li
                a, bb, sm = d_a.cpu().numpy(), d_b.cpu().numpy(), d_s.cpu().numpy()
                for i, (_, avg, ea, eb) in enumerate(want_bins):
                    assert (a[i], bb[i]) == (ea, eb) and sm[i] == round(avg * (ea + eb)), (rows, with_vector, skip, i)
                if with_vector:
                    assert (d_out.cpu().numpy().view(np.uint16) == exp).all()
                assert (st.fast_forwards, st.scans, st.errors) == (b["ff"], b["sc"], 0)
                lanes[skip] = st.lane_steps
            assert lanes[1] < lanes[0], (rows, with_vector, lanes)
    finally:
        gpu.close()


def test_captured_and_replayed_call(golden_batches):
    """One movi_pml_device call with the rule on, captured and replayed twice: the oracle's vector and counters each time."""
    import movi_amd
    import torch
    b = golden_batches[6]
    n, nb = b["offs"].size - 1, int(b["bases"].size)
    gpu = movi_amd.MoveIndex.from_image(b["img"])
    try:
        gpu.prepare()
        gpu.set_option("ff_skip", 1)
        d_bases, d_offs = _dev(b["bases"]), _dev(b["offs"].view(np.int64))
        out = torch.full((nb,), SENT, dtype=torch.int16, device="cuda")
        err = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                gpu.pml_device(d_bases.data_ptr(), d_offs.data_ptr(), n, nb, out.data_ptr(), err.data_ptr(), s.cuda_stream)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert gpu.last_launch()["ahead"] == 2 and int(gpu.info("ff_skip")) == 1
        for _ in range(2):
            out.fill_(SENT)
            err.fill_(0x77)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert (out.cpu().numpy().view(np.uint16) == b["exp"]).all() and (err.cpu().numpy() == 0).all()
            st = gpu.last_stats()
            assert (st.fast_forwards, st.scans, st.errors) == (b["ff"], b["sc"], 0)
        gpu.set_option("ff_skip", 0)
        _, _, c0, l0 = _pml_device(gpu, d_bases, d_offs, n, nb)
        assert c0[:2] == (b["ff"], b["sc"]) and st.lane_steps < l0, (st.lane_steps, l0)
    finally:
        gpu.close()
