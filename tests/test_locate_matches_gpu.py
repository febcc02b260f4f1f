"""GPU suite (-m gpu): text positions of count and MEM hits (movi_locate_matches_device / movi_locate_matches_host,
`movi query --count --locate`, `movi query --mem --locate`) against the contract of include/movi_hip.h, stated on the text itself
in tests/locate_ref.py (a brute force over the cleaned text and its suffix array; the reference has no such mode)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_fastx
from test_gpu_parity import mutated_reads, pack
from test_kernel_coverage_gpu import read_log, take_log
from test_kmer_gpu import SHAPES
import locate_ref
import odd_texts

pytestmark = pytest.mark.gpu

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
FILL = np.uint64(0x5A5A5A5A5A5A5A5A)
POS_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


def items_array(items):
    import movi_amd
    a = np.zeros(len(items), movi_amd.MoveIndex.MATCH_DTYPE)
    for k, (r, s, e) in enumerate(items):
        a[k] = (r, s, e)
    return a


def device_locate(gpu, reads, items, max_occ, cap=None, want_err=True):
    """movi_locate_matches_device on torch buffers pre-filled with 0x5A -> (occ, first, the whole position buffer, item err)."""
    import torch
    bases, offs = pack(reads)
    ni = len(items)
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(bases) if len(bases) else np.zeros(1, np.uint8)).to(dev)
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    it = items_array(items)
    di = torch.from_numpy(np.frombuffer(it.tobytes() + b"\0" * 12, np.uint8).copy()).to(dev)
    if cap is None:
        cap = ni * min(max_occ, int(gpu.desc.length)) + 7
    docc = torch.full((max(ni, 1) * 8,), 0x5A, dtype=torch.uint8, device=dev)
    dfirst = torch.full(((ni + 1) * 8,), 0x5A, dtype=torch.uint8, device=dev)
    dpos = torch.full((max(cap, 1) * 8,), 0x5A, dtype=torch.uint8, device=dev)
    derr = torch.full((max(ni, 1),), 0x5A, dtype=torch.uint8, device=dev)
    wb = gpu.locate_matches_work_bytes(ni)
    dwork = torch.full((wb,), 0x5A, dtype=torch.uint8, device=dev)
    gpu.locate_matches_device(db.data_ptr(), do.data_ptr(), len(reads), di.data_ptr(), ni, max_occ, docc.data_ptr(), dfirst.data_ptr(),
                              dpos.data_ptr(), cap, dwork.data_ptr(), wb, d_item_err=derr.data_ptr() if want_err else 0)
    torch.cuda.synchronize()
    return (docc.cpu().numpy().view(np.uint64)[:ni], dfirst.cpu().numpy().view(np.uint64), dpos.cpu().numpy().view(np.uint64)[:cap],
            derr.cpu().numpy()[:ni])


def check_both_forms(gpu, tx, reads, items, max_occ, tag):
    """Device and host forms against the brute force: every slot of occ, first and the positions; slots past the total stay 0x5A."""
    exp = tx.expect(reads, items, max_occ)
    occ, first, pos = locate_ref.flat(exp)
    total = int(first[-1])
    gocc, gfirst, gpos, gerr = device_locate(gpu, reads, items, max_occ)
    assert (gocc == occ).all() and (gfirst == first).all(), ("device", tag, max_occ)
    assert (gpos[:total] == pos).all() and (gpos[total:] == FILL).all() and gpos.size > total, ("device", tag, max_occ)
    assert (gerr == 0).all() and gpu.last_stats().errors == 0
    bases, offs = pack(reads)
    hocc, hfirst, hpos, st, herr, htotal, rc = gpu.locate_matches_packed(bases, offs, items_array(items), max_occ, positions_cap=total + 3, want_err=True)
    assert rc == 0 and htotal == total and (hocc == occ).all() and (hfirst == first).all(), ("host", tag, max_occ)
    assert (hpos[:total] == pos).all() and (hpos[total:] == 0).all() and (herr == 0).all() and st.errors == 0, ("host", tag, max_occ)
    return exp


def item_mix(gpu, tx, reads, singles=False):
    """The items of the tests over `reads` (which this extends by a few fixed reads), ordered by read: count items, every MEM at L = 1
    and L = 25, an item equal to the first bytes of T, items with N and, if asked for, single bases."""
    reads = list(reads) + [tx.T[:40], tx.T[:40][:7] + b"N" + tx.T[8:40], b"NNNN"]
    i_first, i_n, i_nn = len(reads) - 3, len(reads) - 2, len(reads) - 1
    items = []
    for i, (m, _) in enumerate(gpu.query_count(reads)):
        if m > 0:
            items.append((i, len(reads[i]) - m, len(reads[i])))
    for L in (1, 25):
        for i, mems in enumerate(gpu.query_mems(reads, L)):
            items += [(i, s, e) for s, e, _ in mems]
    items += [(i_first, 0, 40), (i_first, 0, 1), (i_n, 0, 40), (i_n, 5, 10), (i_n, 8, 40), (i_n, 7, 8), (i_nn, 0, 4), (i_nn, 1, 2)]
    if singles:
        reads += [b"ACGT", b"TTAA"]
        items += [(len(reads) - 2, k, k + 1) for k in range(4)] + [(len(reads) - 1, 0, 2), (len(reads) - 1, 1, 3), (len(reads) - 1, 2, 4)]
    items.sort(key=lambda x: x[0])
    return reads, items


def rows_spanned(tx, f, o, p):
    """Rows of the table that the interval of an item with occ o and first hit p[0] touches, less one."""
    all_p = np.asarray(f["all_p"])
    s = tx.ISA[int(p[0])]
    return int(np.searchsorted(all_p, s + o - 1, "right") - np.searchsorted(all_p, s, "right"))


def one_row_intervals(tx, f, exp):
    """Items with occ > 1 whose interval of BWT positions lies inside one row of the table."""
    all_p = np.asarray(f["all_p"])
    n = 0
    for o, l, p in exp:
        if o > 1 and l:
            s = tx.ISA[int(p[0])]
            n += int(np.searchsorted(all_p, s, "right") == np.searchsorted(all_p, s + o - 1, "right"))
    return n


@pytest.fixture(scope="module")
def ref_text(built_lib):
    """{separators: (Text, {mode: (fields, image)})} over ref.fasta; computed once, left unchanged."""
    from oracle import build_index as B
    ref = _ref()
    out = {}
    for sep, modes in ((False, (6, 8, 7, 3, 2, 5)), (True, (6, 8))):
        t = B.clean_text([ref], separators=sep)
        bwt, thr = B.bwt_and_thresholds(t)
        tx = locate_ref.Text([ref], separators=sep)
        per = {}
        for mode in modes:
            f = B.build_rows(bwt, thr, mode)
            per[mode] = (f, B.serialize(f))
        out[sep] = (tx, per)
    return out


def _ref_reads():
    ref = _ref()
    return [r for r in mutated_reads(np.random.default_rng(717), ref, 120, 1, 300)] + [b"", ref[:1], ref[4000:4300]]


@pytest.mark.parametrize("sep,mode", SHAPES)
def test_six_index_types(ref_text, sep, mode):
    import movi_amd
    tx, per = ref_text[sep]
    f, img = per[mode]
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_ssa(7)
    reads, items = item_mix(gpu, tx, _ref_reads())
    top = max(o for o, _, _ in tx.expect(reads, items, 1))
    assert top >= 3 and len(items) > 300
    wrapped = False
    for rate in (1, 7, 100, tx.n + 13):
        gpu.build_ssa(rate)
        for max_occ in (1, 2, top):
            exp = check_both_forms(gpu, tx, reads, items, max_occ, (sep, mode, rate))
        wrapped = wrapped or rate > tx.n
        assert gpu.last_launch()["kernel"].startswith("hits_walk_kernel<%d, " % (3 if mode in (3, 2) else 6))
    # not vacuous: some item lists fewer than it has, some item has t = 0 among its hits, some interval lies inside one row
    exp2 = tx.expect(reads, items, 2)
    assert any(o > 2 for o, _, _ in exp2) and any(0 in p.tolist() for _, _, p in exp) and any(o > 1000 for o, _, _ in exp)
    assert one_row_intervals(tx, f, exp) > 0 and wrapped
    # the Python per-item form
    per_item = gpu.locate_matches(reads, items_array(items), max_occ=2)
    assert [(o, p.tolist()) for o, p in per_item] == [(o, p.tolist()) for o, _, p in exp2]
    gpu.close()


@pytest.mark.parametrize("kind", ["tandem", "two_letters", "pangenome"])
@pytest.mark.parametrize("mode", [6, 3])
def test_odd_texts(built_lib, kind, mode):
    """Long rows, a reduced alphabet, near-identical genomes.  Single bases on the two-letter and tandem texts: intervals of tens of
    thousands of positions that cross many rows and many 32-row checkpoints."""
    import movi_amd
    _, _, SA = odd_texts.table(kind, False)
    tx = locate_ref.Text(odd_texts.odd_text(kind), False, SA=SA)
    f, img = odd_texts.fields(kind, False, mode)
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_ssa(7)
    reads, items = item_mix(gpu, tx, [r for r in odd_texts.reads_of(kind)[:80] if len(r) < 400], singles=kind != "pangenome")
    top = max(o for o, _, _ in tx.expect(reads, items, 1))
    for rate in (7, tx.n + 13):
        gpu.build_ssa(rate)
        for max_occ in (1, 2, top):
            exp = check_both_forms(gpu, tx, reads, items, max_occ, (kind, mode, rate))
    if kind != "pangenome":
        assert top > 1000 and int(locate_ref.flat(exp)[1][-1]) > 10000
    if kind == "two_letters":                                 # a single base: an interval over hundreds of 32-row checkpoint blocks
        assert max(rows_spanned(tx, f, o, p) for o, _, p in exp if o) > 64 * 32
    if kind == "pangenome":
        assert top >= 12                                      # (a 25-mer of the ancestor survives 1 % substitutions in 0.78 of 24 genomes)
    assert one_row_intervals(tx, f, exp) > 0
    gpu.close()


def test_record_junctions(built_lib):
    """Two records without separators: X spanning record 0 / its reverse complement, and that / record 1, occurs and is located;
    with separators the same X does not occur."""
    import movi_amd
    from oracle import build_index as B
    ref = _ref()
    seqs = [ref[:3000], ref[5000:8000]]
    for mode in (6, 3):
        tx = locate_ref.Text(seqs, False)
        gpu = movi_amd.MoveIndex.from_image(B.build_index_from_seqs(seqs, mode))
        gpu.build_ssa(7)
        reads = [tx.T[3000 - 15:3000 + 15], tx.T[6000 - 12:6000 + 18], tx.T[9000 - 20:9000 + 5]]
        items = [(0, 0, 30), (0, 5, 25), (1, 0, 30), (2, 0, 25)]
        exp = check_both_forms(gpu, tx, reads, items, 5, ("junction", mode))
        assert all(t in p.tolist() for t, (_, _, p) in zip((2985, 2990, 5988, 8980), exp))
        gpu.close()
    txs = locate_ref.Text(seqs, True)
    gpu = movi_amd.MoveIndex.from_image(B.build_index_from_seqs(seqs, 6, separators=True))
    gpu.build_ssa(7)
    exp = check_both_forms(gpu, txs, reads, items, 5, ("junction", "sep"))
    assert [o for o, _, _ in exp] == [0, 0, 0, 0]
    gpu.close()


def test_positions_cap_below_the_total(ref_text):
    import movi_amd
    tx, per = ref_text[False]
    gpu = movi_amd.MoveIndex.from_image(per[6][1])
    gpu.build_ssa(100)
    reads, items = item_mix(gpu, tx, _ref_reads())
    occ, first, pos = locate_ref.flat(tx.expect(reads, items, 3))
    total = int(first[-1])
    for cap in (total - 1, total // 2, 1, 0):
        gocc, gfirst, gpos, gerr = device_locate(gpu, reads, items, 3, cap=cap)
        assert (gocc == occ).all() and (gfirst == first).all() and (gerr == 0).all(), cap      # d_first is complete
        assert (gpos[:cap] == pos[:cap]).all(), cap
    # nothing at or past the cap is written: a buffer with room behind the cap
    gocc, gfirst, gpos, _ = device_locate(gpu, reads, items, 3, cap=total + 100)
    assert (gpos[:total] == pos).all() and (gpos[total:] == FILL).all()
    bases, offs = pack(reads)
    # host: MOVI_ERR_ARG with h_occ, h_first and the total filled
    hocc, hfirst, hpos, st, herr, htotal, rc = gpu.locate_matches_packed(bases, offs, items_array(items), 3, positions_cap=total - 1, want_err=True)
    assert rc == -1 and htotal == total and (hocc == occ).all() and (hfirst == first).all()
    from movi_amd._lib import lib
    assert b"positions_cap" in lib().movi_last_error()
    gpu.close()


@pytest.mark.parametrize("mode", [6, 3])
def test_walk_is_locate_mod_n(built_lib, mode):
    """hits_walk_kernel and locate_kernel are one loop (locate_walk, movi_sa.hpp): the slots of the whole call are movi_locate_device's
    entries of the packed positions the expansion left (stages = 2), reduced modulo n, slot for slot, and no slot at or past the total
    is touched.  The first 3000 bases of ref.fasta, 300 items, max_occ = 4; rates 7 and n + 13, so that walks pass text position 0."""
    import torch
    import movi_amd
    from oracle import build_index as B
    ref = _ref()
    gpu = movi_amd.MoveIndex.from_image(B.build_index_from_seqs([ref[:3000]], mode))
    n = int(gpu.desc.length)
    rng = np.random.default_rng(4242)
    reads = [ref[a:a + 50] for a in rng.integers(0, 2950, 60).tolist()]
    items = [(i, s, s + L) for i in range(len(reads)) for s, L in ((0, 2), (3, 4), (10, 6), (20, 12), (5, 45))]
    assert len(items) == 300
    wrapped = 0
    for rate in (7, n + 13):
        gpu.build_ssa(rate)
        gpu.set_option("locate_matches_stages", 2)
        _, first2, packed, _ = device_locate(gpu, reads, items, 4)
        gpu.set_option("locate_matches_stages", 3)
        occ, first, pos, err = device_locate(gpu, reads, items, 4)
        assert gpu.last_launch()["kernel"].startswith("hits_walk_kernel<%d, " % mode) and gpu.last_stats().errors == 0
        total = int(first[-1])
        assert (first2 == first).all() and (err == 0).all() and (occ > 4).any() and (occ < 4).any()
        assert 300 < total < pos.size and (packed[total:] == FILL).all() and (pos[total:] == FILL).all()
        d = torch.from_numpy(packed[:total].view(np.int64).copy()).to(torch.device("cuda", 0))
        gpu.locate_device(d.data_ptr(), total)
        torch.cuda.synchronize()
        assert gpu.last_launch()["kernel"].startswith("locate_kernel<%d, " % mode) and gpu.last_stats().errors == 0
        entries = d.cpu().numpy().view(np.uint64)
        assert (entries % np.uint64(n) == pos[:total]).all(), (mode, rate)
        wrapped += int((entries >= np.uint64(n)).sum())
    assert wrapped > 0                                        # some walk passed text position 0: its entry is SA + n
    gpu.close()


def built_hits_kernels(tmp_dir):
    """Demangled names of the hits_*_kernel instantiations in the library's gfx950 code object."""
    import movi_amd
    data = open(movi_amd.lib_path(), "rb").read()
    names, pos = set(), 0
    tmp = os.path.join(str(tmp_dir), "hits_co.o")
    while True:
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", pos)
        if i < 0:
            break
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, ts = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + ts].decode()
            p += ts
            if "gfx950" in triple and size:
                open(tmp, "wb").write(data[i + off:i + off + size])
                syms = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-sW", tmp], capture_output=True, check=True).stdout.decode()
                mangled = [ln.split()[-1] for ln in syms.splitlines() if " FUNC " in ln and "hits_" in ln and "_kernel" in ln]
                dem = subprocess.run(["c++filt"], input="\n".join(mangled).encode(), capture_output=True, check=True).stdout.decode()
                for ln in dem.splitlines():
                    k = ln.strip()
                    if k.startswith("void movi::"):
                        k = k[len("void movi::"):]
                    names.add(k.split(">(")[0] + ">")
        pos = i + 24
    if os.path.exists(tmp):
        os.remove(tmp)
    return names


def test_more_items_than_lanes_and_every_kernel_runs(ref_text, tmp_path):
    """About 70 000 short items: more than one launch has lanes (256 CUs x 16 wavefronts x 64 = 262 144 at most, 16 384 blocks of
    one wavefront -- fewer CUs, fewer lanes), so the strided lists are walked; n_items = 0; both index widths; every built kernel."""
    import movi_amd
    built = built_hits_kernels(tmp_path)
    assert len(built) == 10 and not any(bad in k for k in built for bad in ("mem_kernel", "locate_kernel", "sa_pos_kernel", "kmer_occ_kernel",
                                                                            "kmer_kernel", "zml_kernel_flat", "pml_kernel_flatp")), sorted(built)
    tx, per = ref_text[False]
    ref = _ref()
    rng = np.random.default_rng(99)
    reads = [ref[a:a + 64] for a in rng.integers(0, len(ref) - 64, 200).tolist()] * 11      # (200 windows: the brute force caches by X)
    items = [(i, s, s + 9 + (i + s) % 6) for i in range(len(reads)) for s in range(0, 32)]          # 70 400 items of 9 .. 14 bases
    assert len(items) > 70000
    exp = tx.expect(reads, items, 4)
    occ, first, pos = locate_ref.flat(exp)
    total = int(first[-1])
    assert total > len(items) and (occ > 4).any()
    take_log()
    for mode in (6, 3):
        for idx64 in (0, 1):
            gpu = movi_amd.MoveIndex.from_image(per[mode][1])
            gpu.set_option("idx64", idx64)
            gpu.build_ssa(100)
            for K in (0, 8):
                gpu.set_option("ftab_k", K)
                gocc, gfirst, gpos, gerr = device_locate(gpu, reads, items, 4)
                assert (gocc == occ).all() and (gfirst == first).all() and (gpos[:total] == pos).all() and (gpos[total:] == FILL).all(), (mode, idx64, K)
                assert (gerr == 0).all()
                st = gpu.last_stats()
                assert st.errors == 0 and 0 < st.lane_steps <= 64 * st.wave_steps
            li = gpu.last_launch()
            assert li["idx64"] == idx64 and li["kernel"] == "hits_walk_kernel<%d, %s>" % (mode, "unsigned long" if idx64 else "unsigned int")
            # n_items = 0: d_first[0] = 0, nothing else is written
            gocc, gfirst, gpos, gerr = device_locate(gpu, reads, [], 4, cap=5)
            assert gfirst.tolist() == [0] and (gpos == FILL).all()
            bases, offs = pack(reads)
            hocc, hfirst, hpos, st, herr, htotal, rc = gpu.locate_matches_packed(bases, offs, items_array([]), 4, positions_cap=0, want_err=True)
            assert rc == 0 and htotal == 0 and hfirst.tolist() == [0]
            gpu.close()
    seen = read_log()
    assert {k for k in seen if k.startswith("hits_")} == built


def test_host_in_several_chunks(ref_text):
    """"pipe_chunk_bases" 3000: a dozen chunks of reads with their items through the handle's staging; stretches of reads without items."""
    import movi_amd
    tx, per = ref_text[True]
    gpu = movi_amd.MoveIndex.from_image(per[6][1])
    gpu.build_ssa(7)
    reads, items = item_mix(gpu, tx, _ref_reads())
    items = [it for it in items if not 20 <= it[0] < 60]       # forty reads in a row without an item
    occ, first, pos = locate_ref.flat(tx.expect(reads, items, 3))
    bases, offs = pack(reads)
    gpu.set_option("pipe_chunk_bases", 3000)
    hocc, hfirst, hpos, st, herr, htotal, rc = gpu.locate_matches_packed(bases, offs, items_array(items), 3, want_err=True)
    gpu.set_option("pipe_chunk_bases", 0)
    assert rc == 0 and htotal == int(first[-1]) and (hocc == occ).all() and (hfirst == first).all() and (hpos[:htotal] == pos).all()
    assert (herr == 0).all() and 0 < st.bases <= len(bases)
    gpu.close()


def test_bad_items_and_argument_errors(ref_text):
    import torch
    import movi_amd
    from movi_amd._lib import lib
    L = lib()
    tx, per = ref_text[False]
    gpu = movi_amd.MoveIndex.from_image(per[6][1])
    ref = _ref()
    reads = [ref[100:160], ref[300:330], b"", ref[900:1000]]
    good = [(0, 0, 60), (0, 10, 40), (1, 0, 30), (3, 50, 100)]
    bases, offs = pack(reads)
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    its = items_array(good)
    # no suffix array attached: MOVI_ERR_ARG, the message names build-SA (both forms)
    assert L.movi_locate_matches_host(gpu._h, bases.ctypes.data, offs.ctypes.data, 4, its.ctypes.data, 4, 5, p, p, p, 20, None, None, None) == -1
    assert b"build-SA" in L.movi_last_error()
    with pytest.raises(movi_amd.MoviError) as e:
        device_locate(gpu, reads, good, 5)
    assert e.value.code == -1 and "build-SA" in str(e.value)
    gpu.build_ssa(100)
    # max_occ == 0, too small a d_work, NULL required buffers, unordered host items
    with pytest.raises(movi_amd.MoviError) as e:
        device_locate(gpu, reads, good, 0)
    assert e.value.code == -1 and "max_occ" in str(e.value)
    assert L.movi_locate_matches_host(gpu._h, bases.ctypes.data, offs.ctypes.data, 4, its.ctypes.data, 4, 0, p, p, p, 20, None, None, None) == -1
    dev = torch.device("cuda", 0)
    d = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    dp = d.data_ptr()
    wb = gpu.locate_matches_work_bytes(4)
    assert L.movi_locate_matches_device(gpu._h, dp, dp, 4, dp, 4, 5, dp, dp, dp, 20, None, dp, wb - 1, None) == -1
    assert b"d_work" in L.movi_last_error() and b"movi_locate_matches_work_bytes" in L.movi_last_error()
    assert L.movi_locate_matches_device(gpu._h, dp, dp, 4, dp, 4, 5, dp, None, dp, 20, None, dp, wb, None) == -1        # no d_first
    assert L.movi_locate_matches_device(gpu._h, dp, dp, 4, dp, 4, 5, None, dp, dp, 20, None, dp, wb, None) == -1        # no d_occ
    assert L.movi_locate_matches_device(gpu._h, dp, dp, 4, None, 4, 5, dp, dp, dp, 20, None, dp, wb, None) == -1        # no d_items
    assert L.movi_locate_matches_device(gpu._h, dp, dp, 4, dp, 4, 5, dp, dp, None, 20, None, dp, wb, None) == -1        # no d_positions with a cap
    assert L.movi_locate_matches_device(gpu._h, dp, dp, 4, dp, 4, 5, dp, dp, dp, 20, None, None, wb, None) == -1        # no d_work
    torch.cuda.synchronize()
    unordered = items_array([(1, 0, 30), (0, 0, 60)])
    assert L.movi_locate_matches_host(gpu._h, bases.ctypes.data, offs.ctypes.data, 4, unordered.ctypes.data, 2, 5, p, p, p, 20, None, None, None) == -1
    assert b"ordered by read" in L.movi_last_error()
    # bad items: occ = listed = 0 and 0xFF; the good ones beside them are answered
    items = [(0, 0, 60), (0, 30, 30), (0, 40, 20), (0, 0, 61), (1, 0, 30), (2, 0, 1), (3, 50, 100), (3, 99, 101), (4, 0, 1), (2 ** 32 - 1, 0, 5)]
    is_bad = np.array([0, 1, 1, 1, 0, 1, 0, 1, 1, 1], bool)
    exp = tx.expect(reads, [it if not b else (0, 0, 0) for it, b in zip(items, is_bad)], 5)
    occ, first, pos = locate_ref.flat(exp)
    assert (occ[~is_bad] >= 1).all() and (occ[is_bad] == 0).all()
    gocc, gfirst, gpos, gerr = device_locate(gpu, reads, items, 5)
    total = int(first[-1])
    assert (gocc == occ).all() and (gfirst == first).all() and (gpos[:total] == pos).all() and (gpos[total:] == FILL).all()
    assert (gerr[is_bad] == 0xFF).all() and (gerr[~is_bad] == 0).all() and gpu.last_stats().errors == 0
    # the measurement hook: stopped after the scan nothing is listed, after the expansion the slots hold packed positions of the table
    with pytest.raises(movi_amd.MoviError):
        gpu.set_option("locate_matches_stages", 0)
    gpu.set_option("locate_matches_stages", 1)
    socc, sfirst, spos, _ = device_locate(gpu, reads, items, 5)
    assert (socc == occ).all() and (sfirst == first).all() and (spos == FILL).all()
    gpu.set_option("locate_matches_stages", 2)
    socc, sfirst, spos, _ = device_locate(gpu, reads, items, 5)
    assert (sfirst == first).all() and ((spos[:total] >> np.uint64(gpu.POS_OFFSET_BITS)) < np.uint64(gpu.desc.r)).all() and (spos[total:] == FILL).all()
    gpu.set_option("locate_matches_stages", 3)
    hocc, hfirst, hpos, st, herr, htotal, rc = gpu.locate_matches_packed(bases, offs, items_array(items), 5, want_err=True)
    assert rc == -1 and b"0xFF" in L.movi_last_error()          # answered, and said
    assert htotal == total and (hocc == occ).all() and (hfirst == first).all() and (hpos[:total] == pos).all() and (herr == gerr).all()
    gpu.close()


def test_options_and_rates_change_nothing(ref_text):
    """The answers as sets and as lists: equal with and without the interval table, and across two sample rates."""
    import movi_amd
    tx, per = ref_text[False]
    gpu = movi_amd.MoveIndex.from_image(per[8][1])
    gpu.build_ssa(3)
    reads, items = item_mix(gpu, tx, _ref_reads())
    got = {}
    for rate in (3, 64):
        gpu.build_ssa(rate)
        for K in (0, 6, 12):
            gpu.set_option("ftab_k", K)
            gocc, gfirst, gpos, _ = device_locate(gpu, reads, items, 50)
            got[(rate, K)] = (gocc.tolist(), gfirst.tolist(), gpos[:int(gfirst[-1])].tolist())
    base = got[(3, 0)]
    assert all(v == base for v in got.values()) and len(base[2]) > len(items)
    occ, first, pos = locate_ref.flat(tx.expect(reads, items, 50))
    assert base == (occ.tolist(), first.tolist(), pos.tolist())
    gpu.close()


def test_corrupt_table(ref_text, tmp_path):
    """A quarter of the rows' destination ids set to 2^32 - 1 (the corruption of test_sa_gpu.py and test_color_types_gpu.py): the call
    returns; the failing items report codes or MOVI_POS_NONE, errors > 0; everything else is a position of the text.  Run once."""
    import movi_amd
    tx, per = ref_text[False]
    f, img = per[6]
    good = movi_amd.MoveIndex.from_image(img)
    good.build_ssa(100)
    ssa_path = str(tmp_path / "ssa.movi")
    good.save_ssa(ssa_path)
    reads, items = item_mix(good, tx, _ref_reads())
    good.close()
    bad_img = bytearray(img)
    desc, _, off, _ = movi_amd.parse_index_image(bytes(bad_img))
    rows = np.frombuffer(bad_img, np.uint8, count=desc.r * 8, offset=off).reshape(-1, 8).copy()
    rng = np.random.default_rng(8600)
    rows[rng.choice(desc.r, desc.r // 4, replace=False), 0:4] = 0xFF
    bad_img[off: off + rows.size] = rows.tobytes()
    bad = movi_amd.MoveIndex.from_image(bytes(bad_img))
    bad.load_ssa(ssa_path)
    gocc, gfirst, gpos, gerr = device_locate(bad, reads, items, 3)            # the call returns
    st = bad.last_stats()
    total = int(gfirst[-1])
    none = gpos[:total] == POS_NONE
    assert st.errors > 0 and st.errors == int((gerr != 0).sum()) + int(none.sum())
    assert set(np.unique(gerr[gerr != 0])) <= {1, 2} and (gocc[gerr != 0] == 0).all()
    assert (np.diff(gfirst.astype(np.int64)) == np.minimum(gocc, 3).astype(np.int64)).all()
    assert (gpos[:total][~none] < np.uint64(tx.n)).all() and (gpos[total:] == FILL).all()
    bases, offs = pack(reads)
    hocc, hfirst, hpos, hst, herr, htotal, rc = bad.locate_matches_packed(bases, offs, items_array(items), 3, want_err=True)
    assert rc == -6 and hst.errors == st.errors and (hocc == gocc).all() and (herr == gerr).all() and (hpos[:total] == gpos[:total]).all()
    bad.close()


def test_capture_without_warmup(ref_text):
    import torch
    import movi_amd
    tx, per = ref_text[True]
    gpu = movi_amd.MoveIndex.from_image(per[6][1])
    gpu.build_ssa(100)
    reads0 = _ref_reads()
    other = movi_amd.MoveIndex.from_image(per[6][1])                          # (the items come from another handle: this one runs nothing first)
    reads, items = item_mix(other, tx, reads0)
    other.close()
    gpu.prepare(gpu.PREPARE_COUNT | gpu.PREPARE_SA)
    scratch0, derived0 = gpu.info("device_scratch_bytes"), gpu.info("derived_bytes")
    occ, first, pos = locate_ref.flat(tx.expect(reads, items, 4))
    total, ni = int(first[-1]), len(items)
    bases, offs = pack(reads)
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(bases)).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    di = torch.from_numpy(np.frombuffer(items_array(items).tobytes(), np.uint8).copy()).to(dev)
    cap = total + 9
    docc = torch.full((ni,), -1, dtype=torch.int64, device=dev)
    dfirst = torch.full((ni + 1,), -1, dtype=torch.int64, device=dev)
    dpos = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    derr = torch.full((ni,), 0x77, dtype=torch.uint8, device=dev)
    wb = gpu.locate_matches_work_bytes(ni)
    dwork = torch.zeros(wb, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()                                                    # one stream, no parallel branches
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            gpu.locate_matches_device(db.data_ptr(), do.data_ptr(), len(reads), di.data_ptr(), ni, 4, docc.data_ptr(), dfirst.data_ptr(),
                                      dpos.data_ptr(), cap, dwork.data_ptr(), wb, d_item_err=derr.data_ptr(), stream=s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert (docc.cpu().numpy() == -1).all() and (dpos.cpu().numpy() == -1).all()          # nothing ran at capture
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    for _ in range(2):
        docc.fill_(-1)
        dfirst.fill_(-1)
        dpos.fill_(-1)
        derr.fill_(0x77)
        g.replay()
        torch.cuda.synchronize()
        assert (docc.cpu().numpy().view(np.uint64) == occ).all() and (dfirst.cpu().numpy().view(np.uint64) == first).all()
        gp = dpos.cpu().numpy()
        assert (gp[:total].view(np.uint64) == pos).all() and (gp[total:] == -1).all() and (derr.cpu().numpy() == 0).all()
    del g
    gocc, gfirst, gpos, gerr = device_locate(gpu, reads, items, 4)            # the eager result
    assert (gocc == occ).all() and (gfirst == first).all() and (gpos[:total] == pos).all()
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived0
    gpu.close()


def _write_fastq(path, ids, reads):
    with open(path, "wb") as f:
        for i, r in zip(ids, reads):
            f.write(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


def _count_locs(tx, by_id, matches, max_occ):
    """The .matches.locs bytes for the lines of a .matches file (`id <TAB> matched/len <TAB> count`), in their order."""
    out = []
    for ln in matches.split(b"\n")[:-1]:
        rid, frac, _ = ln.split(b"\t")
        m, length = (int(x) for x in frac.split(b"/"))
        r = by_id[rid]
        assert len(r) == length
        h = tx.hits(r[length - m:]) if m else np.zeros(0, np.uint64)
        assert (len(h) > 0) == (m > 0)
        out.append(locate_ref.count_line(rid, m, length, len(h), h[:max_occ]))
    return b"".join(out)


def _mem_locs(tx, by_id, mems, max_occ):
    out = []
    for ln in mems.split(b"\n")[:-1]:
        rid, s, e, _ = ln.split(b"\t")
        h = tx.hits(by_id[rid][int(s):int(e)])
        assert len(h) > 0
        out.append(locate_ref.mem_line(rid, int(s), int(e), len(h), h[:max_occ]))
    return b"".join(out)


def test_cli(ref_text, tmp_path):
    tx, per = ref_text[False]
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(per[6][1])
    recs = read_fastx(os.path.join(GOLDEN, "sample.fastq"))
    ids = [i.encode() if isinstance(i, str) else i for i, _ in recs][:60]
    reads = [s for _, s in recs][:60]
    more = [x for x in mutated_reads(np.random.default_rng(98), _ref(), 80, 1, 300) if x] + [b"NNNNNN", b"ACGTNACGT"]
    ids += [b"m%d" % i for i in range(len(more))]
    reads += more
    fq = str(tmp_path / "reads.fq")
    _write_fastq(fq, ids, reads)
    q = [MOVI, "query", "-i", str(idx), "-r", fq]
    # before build-SA: the missing ssa.movi is named
    r = subprocess.run(q + ["--count", "--locate", "-o", str(tmp_path / "x")], capture_output=True)
    assert r.returncode == 1 and b"build-SA" in r.stderr
    r = subprocess.run([MOVI, "build-SA", "-i", str(idx), "--sample-rate", "7"], capture_output=True)
    assert r.returncode == 0, r.stderr
    for rev in (False, True):
        rd = [x[::-1] for x in reads] if rev else reads
        by_id = dict(zip(ids, rd))
        flags = ["--reverse"] if rev else []
        # (a reversed read is no substring of the text: its MEMs are chance matches, so -l 9 there, the default 25 otherwise)
        for kind, args, suffix, locs in (("count", ["--count"], ".count.matches", _count_locs),
                                         ("mem", ["--mem", "--ftab-k", "8"] + (["-l", "9"] if rev else []), ".mems", _mem_locs)):
            plain, out = str(tmp_path / ("plain_%s_%d" % (kind, rev))), str(tmp_path / ("o_%s_%d" % (kind, rev)))
            r = subprocess.run(q + args + flags + ["-o", plain], capture_output=True)
            assert r.returncode == 0, r.stderr
            ordinary = open(plain + suffix, "rb").read()
            assert ordinary, (kind, rev, sorted(os.listdir(str(tmp_path))), r.stderr[-400:])
            for extra, max_occ in (([], 100), (["--max-occ", "3"], 3)):
                want = locs(tx, by_id, ordinary, max_occ)
                assert want.count(b"\n") == ordinary.count(b"\n") > 50, (kind, rev, ordinary[:200])
                r = subprocess.run(q + args + flags + ["--locate", "-o", out] + extra, capture_output=True)
                assert r.returncode == 0, r.stderr
                assert open(out + suffix, "rb").read() == ordinary                       # the ordinary file: as without --locate
                assert open(out + suffix + ".locs", "rb").read() == want
                os.remove(out + suffix + ".locs")
                r = subprocess.run(q + args + flags + ["--locate", "--stdout"] + extra, capture_output=True)
                assert r.returncode == 0 and r.stdout == want, r.stderr
            if kind == "count":
                assert b"\t0\t0\t\n" in want and any(int(ln.split(b"\t")[2]) > 3 for ln in want.split(b"\n")[:-1])   # matched = 0; occ > max_occ
            none = str(tmp_path / ("none_%s_%d" % (kind, rev)))
            r = subprocess.run(q + args + flags + ["--locate", "--no-output", "-o", none], capture_output=True)
            assert r.returncode == 0 and r.stdout == b"" and not os.path.exists(none + suffix) and not os.path.exists(none + suffix + ".locs"), r.stderr
    # --gpus N shards each chunk over N handles (MOVI_SHARE_GPU=1: every logical GPU is device 0): the same bytes
    by_id = dict(zip(ids, reads))
    for kind, args, suffix, locs in (("count", ["--count"], ".count.matches", _count_locs), ("mem", ["--mem", "--ftab-k", "8"], ".mems", _mem_locs)):
        ordinary = open(str(tmp_path / ("plain_%s_0" % kind)) + suffix, "rb").read()
        r = subprocess.run(q + args + ["--locate", "--stdout", "--gpus", "3"], capture_output=True,
                           env=dict(os.environ, MOVI_SHARE_GPU="1"))
        assert r.returncode == 0 and r.stdout == locs(tx, by_id, ordinary, 100), r.stderr
    # a FASTA input with N and lower case, read as given and with --ignore-illegal-chars 1
    fa = tmp_path / "n.fa"
    ref = _ref()
    seqs = [ref[100:300], ref[500:560] + b"NNN" + ref[600:700], b"ACGTN" * 10, ref[900:1000].lower() + ref[1000:1100]]
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    qa = [MOVI, "query", "-i", str(idx), "-r", str(fa), "--count"]
    for flags, rd in (([], seqs), (["--ignore-illegal-chars", "1"], [bytes(c if c in b"ACGT" else ord("A") for c in s) for s in seqs])):
        r = subprocess.run(qa + flags + ["-o", str(tmp_path / "fa")], capture_output=True)
        assert r.returncode == 0, r.stderr
        ordinary = (tmp_path / "fa.count.matches").read_bytes()
        r = subprocess.run(qa + flags + ["--locate", "--stdout"], capture_output=True)
        assert r.returncode == 0 and r.stdout == _count_locs(tx, dict((b"r%d" % i, s) for i, s in enumerate(rd)), ordinary, 100), r.stderr
