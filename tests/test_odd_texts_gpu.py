"""GPU suite (-m gpu): locate, MEM finding and k-mer presence on the texts of tests/odd_texts.py -- rows at MAX_RUN_LENGTH, packed
offsets up to 2046 / 4094, fast-forward chains through rows of one character, tandem repeats, a two-letter alphabet, and a pangenome
with more BWT positions than a locate launch has lanes -- against tests/sa_ref.py, mem_ref.py and kmer_ref.py.
tests/test_odd_texts_cpu.py pins what the texts hold and holds those references to the literal algorithms on them."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_parity import pack
from test_kmer_gpu import _kmer_lines, device_kmers
from test_mem_gpu import _mem_lines, device_mems
from test_sa_gpu import check_locate_everything, device_entries
import kmer_ref
import mem_ref
import odd_texts
import sa_ref
from conftest import ROOT
from oracle import build_index as B

pytestmark = pytest.mark.gpu

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
LOCATE_WAVES = 16                                            # wavefronts per CU of a locate launch (kLocateWaves, movi_kernels.hpp)
MEM_LS = (1, 12, 25)
KMER_KS = (1, 12, 31)
QUERY_CASES = [(kind, False, mode) for kind in ("poly", "tandem", "two_letters") for mode in (6, 3, 7)] + [("poly", True, 6)]


def kmode(mode):
    return 3 if mode in (3, 2) else 6


@pytest.fixture(scope="module")
def images(built_lib):
    """(kind, separators, mode) -> (build_rows fields, index image, suffix array), built on first use and shared."""
    def get(kind, sep, mode):
        f, img = odd_texts.fields(kind, sep, mode)
        return f, img, odd_texts.table(kind, sep)[2]
    return get


def walk_dists(SA, rate):
    """The LF steps locate takes from every BWT position: from text position t down to the nearest sampled one at or below it (the
    sampled ones are the text positions whose BWT position is a multiple of rate), t + 1 steps to BWT position 0 where there is none."""
    SA = np.asarray(SA, np.int64)
    n = len(SA)
    bwt_pos = np.empty(n, np.int64)
    bwt_pos[SA] = np.arange(n)
    t = np.arange(n)
    below = np.maximum.accumulate(np.where(bwt_pos % rate == 0, t, -1))
    return (t - below)[SA]


def walk_steps(SA, rate):
    return int(walk_dists(SA, rate).sum())


# ------------------------------------------------------------------------------------------------ a. exhaustive locate
@pytest.mark.parametrize("kind,sep,mode", [(kind, False, mode) for kind in ("poly", "tandem", "two_letters") for mode in (6, 3, 7, 2)] +
                         [("poly", True, 6), ("poly", True, 3)])
def test_exhaustive_locate_on_long_rows(images, tmp_path, kind, sep, mode):
    import movi_amd
    f, img, SA = images(kind, sep, mode)
    n, longest = f["n"], int(np.asarray(f["lens"]).max())
    gpu = movi_amd.MoveIndex.from_image(img)
    wraps = []
    for rate in (1, 7, 100, 3000, longest + 1):              # longest + 1: no row holds two samples, many hold one
        assert rate < n
        wraps.append(check_locate_everything(gpu, f, SA, rate, tmp_path))     # (asserts locate_kernel<3 or 6, ...> itself)
        st = gpu.last_stats()
        assert st.errors == 0, rate
        assert st.lane_steps == walk_steps(SA, rate), rate
        assert gpu.last_launch()["kernel"].startswith("locate_kernel<%d, " % kmode(mode))
    assert not wraps[0] and any(wraps[1:])
    gpu.close()


# ------------------------------------------------------------------------------------------------ b. per-base entries
@pytest.fixture(scope="module")
def entry_cases(images):
    """(kind, sep, mode) -> (reads, {rate: expected entries per read}, oracle PMLs per read, highest offset among the positions)."""
    from oracle.oracle import Oracle
    done = {}

    def get(kind, sep, mode):
        if (kind, sep, mode) not in done:
            f, img, SA = images(kind, sep, mode)
            reads = list(odd_texts.reads_of(kind))
            o = Oracle(img)
            pos = sa_ref.positions(f, o, reads)                              # (holds the restatement's PMLs to the oracle's)
            pmls = [np.asarray(o.pml(r)) for r in reads]
            o.close()
            all_p = np.asarray(f["all_p"])
            want = {}
            for rate in (100, 7):
                ent = sa_ref.entries(SA, rate)
                want[rate] = [ent[all_p[rows] + offs] if len(rows) else np.zeros(0, np.uint64) for rows, offs in pos]
            done[(kind, sep, mode)] = (reads, want, pmls, max(int(offs.max()) for _, offs in pos if len(offs)))
        return done[(kind, sep, mode)]
    return get


@pytest.mark.parametrize("kind,sep,mode", [(kind, sep, mode) for kind in ("poly", "tandem") for sep in (False, True) for mode in (6, 8, 7)])
def test_per_base_entries_on_long_rows(images, entry_cases, kind, sep, mode):
    import movi_amd
    f, img, SA = images(kind, sep, mode)
    reads, want, pmls, top = entry_cases(kind, sep, mode)
    # the packed positions sa_pos_kernel hands to locate_kernel: offsets beyond 1024 where the layout has them (11 bits in mode 6; rows
    # of modes 8 and 7 end at 1023 and 511 characters, there more than half of that)
    assert top >= (1024 if mode == 6 else B.MAX_RUN[mode] // 2 + 1), top
    gpu = movi_amd.MoveIndex.from_image(img)
    bases, offs = pack(reads)
    wpml = np.concatenate(pmls).astype(np.uint16)
    perm = np.random.default_rng(3).permutation(len(reads))
    for rate in (100, 7):
        gpu.build_ssa(rate)
        wsa = np.concatenate(want[rate])
        got = gpu.query_sa_entries(reads)
        assert all((g == w).all() for g, w in zip(got, want[rate])), rate
        sa, pml, st = gpu.query_sa_entries_packed(bases, offs)
        assert (sa == wsa).all() and (pml == wpml).all() and st.errors == 0 and st.bases == len(bases), rate
        dsa, dpml, derr, _ = device_entries(gpu, reads, order=perm)
        assert (dsa == wsa).all() and (dpml == wpml).all() and (derr == 0).all(), rate
        assert gpu.last_stats().errors == 0
        dsa, _, derr, _ = device_entries(gpu, reads, want_pml=False)
        assert (dsa == wsa).all() and (derr == 0).all(), rate
        assert gpu.last_stats().errors == 0
        assert gpu.last_launch()["kernel"].startswith("locate_kernel<6, ")
    gpu.close()


# ------------------------------------------------------------------------------------------------ c. the strided lists
@pytest.mark.parametrize("mode,idx64", [(6, 0), (6, 1), (3, 0), (3, 1)])
def test_strided_item_lists(images, mode, idx64):
    """More items than a launch has lanes: every lane of locate_kernel walks a list of items, in place on the caller's buffer."""
    import torch
    import movi_amd
    f, img, SA = images("pangenome", False, mode)
    n, r = f["n"], f["r"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = cus * LOCATE_WAVES * 64
    copies = -(-3 * lanes // n) + 1
    rows, offs = sa_ref.all_positions(f)
    tile = (rows.astype(np.uint64) << np.uint64(12)) | offs.astype(np.uint64)
    assert int(offs.max()) < 4096
    items = np.concatenate([np.tile(tile, copies), tile[:37]])
    n_items = len(items)
    assert n_items > 3 * lanes and n_items % 64 != 0
    NONE = np.uint64(movi_amd.MoveIndex.POS_NONE)
    i = np.arange(n_items)
    is_none = i % 97 == 0
    is_out = (i % 101 == 0) & ~is_none
    dirty = items.copy()
    dirty[is_none] = NONE
    dirty[is_out] = ((np.uint64(r) + (i[is_out] % 5).astype(np.uint64)) << np.uint64(12))
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.set_option("idx64", idx64)
    T = "unsigned long" if idx64 else "unsigned int"
    dev = torch.device("cuda", 0)
    for rate in (7, 100):
        gpu.build_ssa(rate)
        ent = sa_ref.entries(SA, rate)
        want = np.concatenate([np.tile(ent, copies), ent[:37]])
        d = torch.from_numpy(items.view(np.int64).copy()).to(dev)
        gpu.locate_device(d.data_ptr(), n_items)
        torch.cuda.synchronize()
        st = gpu.last_stats()
        assert (d.cpu().numpy().view(np.uint64) == want).all(), rate
        dists = walk_dists(SA, rate)
        assert st.errors == 0 and st.lane_steps == copies * int(dists.sum()) + int(dists[:37].sum()), rate
        li = gpu.last_launch()
        assert li["idx64"] == idx64 and li["kernel"] == "locate_kernel<%d, %s>" % (mode, T)
        d = torch.from_numpy(dirty.view(np.int64).copy()).to(dev)
        gpu.locate_device(d.data_ptr(), n_items)
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(np.uint64)
        assert (got[is_none] == NONE).all() and (got[is_out] == NONE).all(), rate
        assert gpu.last_stats().errors == int(is_out.sum()) > 0, rate
        keep = ~(is_none | is_out)
        assert (got[keep] == want[keep]).all(), rate
    # the builder's list in successor mode, one item per sample: m = n samples at rate 1
    gpu.build_ssa(1)
    got_rate, got = gpu.ssa()
    assert got_rate == 1 and len(got) == n + 1 and (got == sa_ref.samples(SA, 1)).all()
    gpu.close()


# ------------------------------------------------------------------------------------------------ d. MEMs, e. k-mers
@pytest.fixture(scope="module")
def query_refs(images):
    """(kind, sep) -> (reads, code_of, {L: MEMs per read}, {k: (found, runs) per read}) from the oracle on the mode-6 image."""
    from oracle.oracle import Oracle
    done = {}

    def get(kind, sep):
        if (kind, sep) not in done:
            f, img, _ = images(kind, sep, 6)
            reads = list(odd_texts.reads_of(kind))
            code_of = sa_ref.code_table(f)
            o = Oracle(img)
            mems, _ = mem_ref.restate(o, reads, code_of, MEM_LS)
            kmers, _ = kmer_ref.restate(o, reads, KMER_KS)
            o.close()
            done[(kind, sep)] = (reads, code_of, mems, kmers)
        return done[(kind, sep)]
    return get


def table_sizes(gpu, kind):
    """The ftab_k values to run with: 0 and 12 on a DNA index; on the two-letter one 12 is refused and the default route answers."""
    import movi_amd
    if kind != "two_letters":
        return (0, 12)
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.set_option("ftab_k", 12)
    assert e.value.code == -1
    return (None,)


@pytest.mark.parametrize("kind,sep,mode", QUERY_CASES)
def test_mems_on_long_rows(images, query_refs, kind, sep, mode):
    import movi_amd
    reads, _, exp, _ = query_refs(kind, sep)
    gpu = movi_amd.MoveIndex.from_image(images(kind, sep, mode)[1])
    for K in table_sizes(gpu, kind):
        if K is not None:
            gpu.set_option("ftab_k", K)
        for L in MEM_LS:
            assert gpu.query_mems(reads, L) == exp[L], (K, L)
            got, err = device_mems(gpu, reads, L, with_err=True)
            assert got == exp[L] and (err == 0).all(), (K, L)
            assert gpu.last_launch()["kernel"].startswith("mem_kernel<%d, " % kmode(mode))
    if kind == "poly":
        assert max(c for ms in exp[1] for _, _, c in ms) > 4095              # intervals of thousands of occurrences
    gpu.close()


@pytest.mark.parametrize("kind,sep,mode", QUERY_CASES)
def test_kmers_on_long_rows(images, query_refs, kind, sep, mode):
    import movi_amd
    reads, _, _, exp = query_refs(kind, sep)
    gpu = movi_amd.MoveIndex.from_image(images(kind, sep, mode)[1])
    for K in table_sizes(gpu, kind):
        if K is not None:
            gpu.set_option("ftab_k", K)
        for la in (-1, 0, 3):
            gpu.set_option("kmer_lookahead", la)
            for k in KMER_KS:
                assert gpu.query_kmers(reads, k) == exp[k], (K, la, k)
                got, err = device_kmers(gpu, reads, k, with_err=True)
                assert got == exp[k] and (err == 0).all(), (K, la, k)
                assert gpu.last_launch()["kernel"].startswith("kmer_kernel<%d, " % kmode(mode))
    assert sum(f for f, _ in exp[31]) > 10000                                # matches that run the length of the reads
    gpu.close()


# ------------------------------------------------------------------------------------------------ f. the command line
def test_cli_on_poly(images, query_refs, tmp_path):
    from oracle.oracle import Oracle
    f, img, SA = images("poly", False, 6)
    reads, code_of, _, _ = query_refs("poly", False)
    ref_fa, reads_fa, idx = tmp_path / "poly.fa", tmp_path / "reads.fa", tmp_path / "idx"
    ref_fa.write_bytes(b">poly\n" + odd_texts.odd_text("poly")[0] + b"\n")
    ids = [b"q%d" % i for i in range(len(reads))]
    reads_fa.write_bytes(b"".join(b">%s\n%s\n" % (i, s) for i, s in zip(ids, reads)))
    r = subprocess.run([MOVI, "build", "-i", str(idx), "-f", str(ref_fa)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (idx / "index.movi").read_bytes() == img
    r = subprocess.run([MOVI, "build-SA", "-i", str(idx), "--sample-rate", "100"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (idx / "ssa.movi").read_bytes() == sa_ref.ssa_bytes(f, SA, 100)
    o = Oracle(img)
    out = tmp_path / "o"
    r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", str(reads_fa), "-o", str(out), "-n", "--sa-entries"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.pml.sa_entries.bpf").read_bytes() == sa_ref.sa_entries_file(ids, sa_ref.read_entries(f, o, SA, 100, reads))
    r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", str(reads_fa), "--mem", "-l", "25", "--ftab-k", "12", "--stdout"], capture_output=True)
    assert r.returncode == 0 and r.stdout == _mem_lines(ids, reads, o, code_of, 25), r.stderr
    r = subprocess.run([MOVI, "query", "-i", str(idx), "-r", str(reads_fa), "--kmer", "-k", "31", "--stdout"], capture_output=True)
    assert r.returncode == 0 and r.stdout == _kmer_lines(ids, reads, o, 31), r.stderr
    assert r.stdout.count(b"\n") == len(reads)
    o.close()
