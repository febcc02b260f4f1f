"""GPU suite (-m gpu): Movi Color in its default colour mode -- the colour tables built on the device (movi_color_build), doc_sets_flat.bin,
movi_multi_classify_device / _host and `movi color` / `movi build --color` / `movi query --multi-classify` -- against tests/color_ref.py:
the documents of the BWT positions from the suffix array of the text, and process_char's scoring over the restatement of query_pml's
walk, which is itself held to the oracle's PMLs."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_parity import mutated_reads, pack
import color_ref
import odd_texts
import sa_ref

pytestmark = pytest.mark.gpu

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
TEXTS = ("ref3", "pangenome", "poly", "short70", "one", "taxa")
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


@functools.lru_cache(maxsize=None)
def text(name):
    """(records, build_rows fields, index image, SA, doc_offsets, doc_ids or None) of one of the texts; mode 6, no separators."""
    from oracle import build_index as B
    rng = np.random.default_rng(4100 + TEXTS.index(name))
    doc_ids = None
    if name in ("ref3", "taxa"):                              # ref.fasta cut into 3 documents
        ref = _ref()
        third = len(ref) // 3
        seqs = [ref[:third], ref[third:2 * third + 17], ref[2 * third + 17:]]
        if name == "taxa":                                    # six documents, several per taxon, gaps in the ids
            seqs = [s[:len(s) // 2] for s in seqs] + [s[len(s) // 2:] for s in seqs]
            doc_ids = [9606, 12, 9606, 70000, 12, 3]
    elif name == "pangenome":                                 # one document per genome
        seqs = odd_texts.odd_text("pangenome")
        f, img = odd_texts.fields("pangenome", False, 6)
        return seqs, f, img, odd_texts.table("pangenome")[2], color_ref.doc_offsets_of(seqs), None
    elif name == "poly":                                      # runs split at MAX_RUN_LENGTH; documents cut inside the runs of A
        seqs = odd_texts.odd_text("poly")
        f, img = odd_texts.fields("poly", False, 6)
        n = f["n"]
        return seqs, f, img, odd_texts.table("poly")[2], list(range(700, n - 1, 700)) + [n - 1], None
    elif name == "short70":                                   # 70 near-identical short documents: sets of more than 64 members
        anc = _ACGT[rng.integers(0, 4, 48)]
        seqs = []
        for _ in range(70):
            g = anc.copy()
            g[rng.integers(0, 48, 2)] = _ACGT[rng.integers(0, 4, 2)]
            seqs.append(bytes(g))
    elif name == "one":                                       # one document: every set is {0}
        seqs = [_ref()[:3000]]
    f, SA = sa_ref.text_fields(seqs, 6)
    return seqs, f, B.serialize(f), SA, color_ref.doc_offsets_of(seqs), doc_ids


@functools.lru_cache(maxsize=None)
def expected_tables(name):
    _, f, _, SA, offsets, doc_ids = text(name)
    return color_ref.tables(f, SA, offsets, doc_ids)


def test_restatement_covers_every_run():
    """The coverage cap, checked before anything runs on the device: no text makes the reference throw (every run has a document,
    offsets strictly increasing, the flat offsets fit 40 bits), and the texts have the shapes they are there for."""
    for name in TEXTS:
        _, f, _, _, offsets, _ = text(name)
        flat, inds, ns, taxa = expected_tables(name)
        assert len(inds) == f["r"] and all(b > a for a, b in zip([0] + offsets, offsets)) and offsets[-1] == f["n"] - 1
        assert len(flat) < 1 << 40 and ns == len(taxa)
    sizes = lambda name: [int(expected_tables(name)[0][int(a)]) for a in expected_tables(name)[1]]
    assert max(sizes("short70")) > 64 and max(sizes("pangenome")) == 24 and set(sizes("one")) == {1}
    assert max(sizes("poly")) >= 3 and max(text("poly")[1]["lens"]) == 2047          # one full-length run holds several documents
    assert expected_tables("taxa")[2:] == (4, [3, 12, 9606, 70000])


def check_tables(gpu, name, tmp_path, tag):
    flat, inds, ns, taxa = expected_tables(name)
    gflat, ginds, gns, gtaxa = gpu.colors()
    assert gns == ns and list(gtaxa) == taxa
    assert (gflat == flat).all() and (ginds == inds).all(), (name, tag)
    path = str(tmp_path / ("doc_sets_%s_%s.bin" % (name, tag)))
    gpu.save_colors(path)
    assert open(path, "rb").read() == color_ref.flat_file(flat, inds) and not os.path.exists(path + ".tmp")
    assert gpu.info("color_bytes") == 2 * len(flat) + 8 * len(inds)


@pytest.mark.parametrize("name", TEXTS)
def test_builder(name, tmp_path):
    import movi_amd
    _, f, img, _, offsets, doc_ids = text(name)
    # none attached: one is built at the default rate and stays
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    assert gpu.ssa()[0] == 100 and gpu.info("color_chunks") == 1
    assert gpu.last_launch()["kernel"] == "color_walk_kernel<6, unsigned int>"
    check_tables(gpu, name, tmp_path, "none")
    gpu.close()
    # rate 7 attached; the chunk budget forced small: several chunks, the same tables
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_ssa(7)
    gpu.set_option("color_chunk_keys", max(64, f["n"] // 3))
    gpu.build_colors(offsets, doc_ids)
    assert gpu.ssa()[0] == 7 and gpu.info("color_chunks") >= 2
    check_tables(gpu, name, tmp_path, "rate7")
    if name == "pangenome":                                    # rate 1: more samples than one launch has lanes; the 64-bit instantiation
        assert f["n"] > 256 * 16 * 64
        gpu.build_ssa(1)
        gpu.set_option("color_chunk_keys", 0)
        gpu.set_option("idx64", 1)
        gpu.build_colors(offsets, doc_ids)
        assert gpu.last_launch()["kernel"] == "color_walk_kernel<6, unsigned long>"
        check_tables(gpu, name, tmp_path, "rate1")
    gpu.close()


def test_builder_refusals(tmp_path):
    import movi_amd
    _, f, img, SA, offsets, _ = text("ref3")
    gpu = movi_amd.MoveIndex.from_image(img)
    for call in (lambda: gpu.colors(), lambda: gpu.save_colors(str(tmp_path / "x")), lambda: gpu.prepare(gpu.PREPARE_COLOR),
                 lambda: gpu.multi_classify([b"ACGT"])):
        with pytest.raises(movi_amd.MoviError) as e:
            call()
        assert e.value.code == -1 and "movi color" in str(e.value)
    for bad in ([], [0, 5], [10, 10, 20], [30, 20]):
        with pytest.raises(movi_amd.MoviError) as e:
            gpu.build_colors(bad)
        assert e.value.code == -1
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.load_colors(str(tmp_path / "missing.bin"), 3)
    assert e.value.code == -3 and "Failed to open document sets flat file at" in str(e.value)
    # round trip through the expected bytes; a file of another index, a truncated one, a set beyond num_species
    flat, inds, ns, _ = expected_tables("ref3")
    good = tmp_path / "doc_sets_flat.bin"
    good.write_bytes(color_ref.flat_file(flat, inds))
    gpu.load_colors(str(good), ns)
    assert (gpu.colors()[0] == flat).all() and (gpu.colors()[1] == inds).all() and len(gpu.colors()[3]) == 0
    (tmp_path / "short.bin").write_bytes(good.read_bytes()[:-3])
    (tmp_path / "other.bin").write_bytes(color_ref.flat_file(flat, inds[:-1]))
    for nm, species in (("short.bin", ns), ("other.bin", ns), ("doc_sets_flat.bin", ns - 1)):
        with pytest.raises(movi_amd.MoviError) as e:
            gpu.load_colors(str(tmp_path / nm), species)
        assert e.value.code == -2, nm
    # a sampled suffix array of another text: MOVI_ERR_INVARIANT, never a wrong table
    wrong = tmp_path / "ssa.movi"
    wrong.write_bytes(sa_ref.ssa_bytes(f, np.roll(np.asarray(SA), 1), 100))
    gpu.load_ssa(str(wrong))
    with pytest.raises(movi_amd.MoviError) as e:
        gpu.build_colors(offsets)
    assert e.value.code == -6
    gpu.close()


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """~200 reads: mutated substrings (N and lower case among them) of the forward text, drawn inside documents, and stretches of the
    indexed text across the documents' ends, then the fixed lengths and the edge cases -- more than 64 of them, very different lengths side by side."""
    seqs = text(name)[0]
    fwd = b"".join(seqs)
    rng = np.random.default_rng(5200 + TEXTS.index(name))
    reads = mutated_reads(rng, fwd, 150, 1, min(300, len(fwd)))
    from oracle import build_index as B
    t = bytes(B.clean_text(seqs)[:-1])                         # the indexed text: every record followed by its reverse complement
    for end in text(name)[4][:-1][:20]:                        # across a document boundary: the text on both sides of a document's end
        reads.append(t[max(0, end - 40): end + 40])
    one = max(seqs, key=len)
    for ln in (1, 2, 63, 64, 65, 300):
        reads.append((one * (300 // len(one) + 1))[:ln] if len(one) < ln else one[5:5 + ln] if len(one) >= ln + 5 else one[:ln])
    reads += [b"", b"N" * 40, fwd[:33] + b"NN" + fwd[35:80], bytes(_ACGT[rng.integers(0, 4, 200)])]    # the last one: absent from the text
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def expected_scores(name, min_len):
    from oracle.oracle import Oracle
    _, f, img, _, _, _ = text(name)
    flat, inds, ns, _ = expected_tables(name)
    o = Oracle(img)
    codes = sa_ref.code_table(f)
    out = [color_ref.score(f, o, rd, flat, inds, ns, min_len, codes) for rd in reads_of(name)]
    o.close()
    return out


def expected_lines(name, min_len, reads=None, scores=None, **kw):
    """The report of the CLI tests: their FASTA holds every read but the empty one (a record without a sequence line is no record)."""
    reads = reads if reads is not None else reads_of(name)
    scores = scores if scores is not None else expected_scores(name, min_len)
    taxa = expected_tables(name)[3]
    return [color_ref.mls_line(b"r%d" % i, len(rd), s, taxa, **kw) for i, (rd, s) in enumerate(zip(reads, scores)) if len(rd)]


def check_records(out, counts, want):
    assert [(int(o["best"]), int(o["second"]), int(o["colors_count"]), int(o["sum_ml"])) for o in out] == [w[:4] for w in want]
    if counts is not None:
        assert [list(map(int, c)) for c in counts] == [w[4] for w in want]
    for o, w in zip(out, want):
        assert int(o["best_count"]) == (w[4][w[0]] if w[0] != color_ref.NONE else 0)
        assert int(o["second_count"]) == (w[4][w[1]] if w[1] != color_ref.NONE else 0)


def device_call(gpu, reads, min_len, want_counts, ns, order=None):
    import torch
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(bases)).to(dev)
    do = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dout = torch.full((n * 24,), 0x5A, dtype=torch.uint8, device=dev)
    dcnt = torch.full((n, ns), 77, dtype=torch.int32, device=dev) if want_counts else None
    dp = torch.full((max(nb, 1),), 0x5A5A, dtype=torch.int16, device=dev)
    de = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)
    dord = torch.from_numpy(np.asarray(order, np.int32)).to(dev) if order is not None else None
    gpu.multi_classify_device(db.data_ptr(), do.data_ptr(), n, nb, min_len, dout.data_ptr(), d_counts=dcnt.data_ptr() if want_counts else 0,
                              d_pml=dp.data_ptr(), d_err=de.data_ptr(), d_order=dord.data_ptr() if dord is not None else 0)
    torch.cuda.synchronize()
    out = dout.cpu().numpy().view(gpu.MC_DTYPE)
    return out, (dcnt.cpu().numpy().view(np.uint32) if want_counts else None), dp.cpu().numpy().view(np.uint16)[:nb], de.cpu().numpy()


@pytest.mark.parametrize("name", TEXTS)
def test_scoring(name):
    import movi_amd
    from oracle.oracle import Oracle
    _, f, img, _, offsets, doc_ids = text(name)
    reads = reads_of(name)
    assert len(reads) > 128 and {1, 2, 63, 64, 65, 300} <= {len(r) for r in reads}
    ns = expected_tables(name)[2]
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    o = Oracle(img)
    pml = np.concatenate([np.asarray(o.pml(r)) for r in reads]).astype(np.uint16)
    o.close()
    bases, offs = pack(reads)
    for min_len in ((1, 5, 255) if name in ("ref3", "short70") else (1,)):
        want = expected_scores(name, min_len)
        out, counts, gp, st = gpu.multi_classify_packed(bases, offs, min_len, want_pml=True)
        check_records(out, counts, want)
        assert (gp == pml).all() and st.errors == 0 and st.bases == len(bases)
        out, counts, gp, err = device_call(gpu, reads, min_len, True, ns)
        check_records(out, counts, want)
        assert (gp == pml).all() and (err == 0).all()
    assert gpu.last_launch()["kernel"] == "color_kernel<6, unsigned int>"
    want = expected_scores(name, 1)
    assert any(w[0] == color_ref.NONE for w in want) and any(w[1] != color_ref.NONE for w in want) or name == "one"
    # the counters in the handle's scratch, forced small: the reads go through it in many chunks; a permuted read order; 64-bit rows
    gpu.set_option("color_scratch_bytes", 4 * ns * 50)
    gpu.set_option("release_scratch", 1)
    perm = np.random.default_rng(3).permutation(len(reads))
    out, _, _, err = device_call(gpu, reads, 1, False, ns, order=perm)
    check_records(out, None, want)
    assert gpu.info("device_scratch_bytes") <= 4 * ns * 50 * 9 // 8 + 64
    gpu.set_option("idx64", 1)
    out, counts, _, _ = gpu.multi_classify_packed(bases, offs, 1)
    check_records(out, counts, want)
    assert gpu.last_launch()["kernel"] == "color_kernel<6, unsigned long>"
    gpu.close()


def test_prepared_handle_allocates_nothing_and_can_be_captured():
    """After movi_index_prepare(MOVI_PREPARE_COLOR) the first movi_multi_classify_device call on the handle leaves the device's memory
    where it was and can be captured into a graph with no warm-up call (a hipMalloc or a synchronise inside would fail the capture)."""
    import torch
    import movi_amd
    _, f, img, _, offsets, doc_ids = text("ref3")
    reads = reads_of("ref3")
    want = expected_scores("ref3", 1)
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    gpu.set_option("color_scratch_bytes", 4 * 3 * 100)          # two chunks of reads inside the captured call
    derived = gpu.prepare(gpu.PREPARE_COLOR)
    assert derived == gpu.info("derived_bytes") and derived >= gpu.info("color_bytes") + gpu.info("locate_bytes")
    bases, offs = pack(reads)
    n, nb = len(reads), int(offs[-1])
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(bases)).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    dout = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    # (torch's own first reduction and read-back load their kernels and workspace -- 6 MiB of the device's memory that is not the
    # engine's: taken before the baseline, so that the bound below is about the captured call and the graph alone)
    assert int(dout.sum().item()) == 0 and dout.cpu().numpy().size == n * 24
    torch.cuda.synchronize()
    free0, scratch0 = torch.cuda.mem_get_info()[0], gpu.info("device_scratch_bytes")
    assert scratch0 >= 4 * 3 * 100
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            gpu.multi_classify_device(db.data_ptr(), do.data_ptr(), n, nb, 1, dout.data_ptr(), stream=s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert int(dout.sum().item()) == 0                          # captured, not run
    for _ in range(2):
        dout.zero_()
        g.replay()
        torch.cuda.synchronize()
        check_records(dout.cpu().numpy().view(gpu.MC_DTYPE), None, want)
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)    # (the graph's own bookkeeping aside)
    assert gpu.info("device_scratch_bytes") == scratch0 and gpu.info("derived_bytes") == derived
    del g
    gpu.close()


def write_index(name, d, with_ids=True):
    _, _, img, _, offsets, doc_ids = text(name)
    d.mkdir()
    (d / "index.movi").write_bytes(img)
    (d / "ref.fa.doc_offsets").write_text("".join("%d\n" % x for x in offsets))
    if doc_ids is not None and with_ids:
        (d / "ref.fa.doc_ids").write_text(" ".join(str(x) for x in doc_ids) + "\n")


@pytest.mark.parametrize("name", TEXTS)
def test_cli_color(name, tmp_path):
    flat, inds, _, _ = expected_tables(name)
    d = tmp_path / "idx"
    write_index(name, d)
    env = dict(os.environ, MOVI_COLOR_CHUNK_KEYS=str(max(64, text(name)[1]["n"] // 2))) if name == "short70" else None
    r = subprocess.run([MOVI, "color", "-i", str(d)], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    assert (d / "doc_sets_flat.bin").read_bytes() == color_ref.flat_file(flat, inds)
    assert sorted(os.listdir(d)) == sorted(["index.movi", "ref.fa.doc_offsets", "doc_sets_flat.bin"] + (["ref.fa.doc_ids"] if name == "taxa" else []))


def test_cli_build_color(tmp_path):
    """`movi build --color`: index, document offsets and colour tables from the FASTA alone; the plain build's index.movi."""
    seqs = text("ref3")[0]
    flat, inds, _, _ = expected_tables("ref3")
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    d = tmp_path / "idx"
    r = subprocess.run([MOVI, "build", "-i", str(d), "-f", str(fa), "--color"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (d / "index.movi").read_bytes() == text("ref3")[2]
    assert (d / "ref.fa.doc_offsets").read_text().split() == [str(x) for x in text("ref3")[4]]
    assert (d / "doc_sets_flat.bin").read_bytes() == color_ref.flat_file(flat, inds)


def test_overlapped_host_chunks_keep_their_own_counters():
    """movi_multi_classify_host on page-locked reads with the chunk size forced small: several chunks of the overlapped path are in
    flight together, each with counters of its own -- with and without counter rows coming back, equal to the restatement."""
    import movi_amd
    name = "pangenome"
    _, f, img, _, offsets, doc_ids = text(name)
    reads = [r for r in reads_of(name)] * 3
    want = expected_scores(name, 1) * 3
    bases, offs = pack(reads)
    pb = movi_amd.pinned_empty(bases.size, np.uint8)
    pb[:] = bases
    gpu = movi_amd.MoveIndex.from_image(img)
    gpu.build_colors(offsets, doc_ids)
    gpu.set_option("pipe_chunk_bases", 3000)                   # ~25 chunks of ~20 reads
    gpu.set_option("color_scratch_bytes", 4 * 24 * 8)          # and every chunk's reads through its scratch eight at a time
    for rep in range(2):
        for want_counts in (False, True):
            out, counts, _, st = gpu.multi_classify_packed(pb, offs, 1, want_counts=want_counts)
            check_records(out, counts, want)
            assert st.errors == 0 and st.bases == len(bases)
    gpu.close()


@pytest.mark.parametrize("name", TEXTS)
def test_cli_multi_classify(name, tmp_path):
    reads = reads_of(name)
    d = tmp_path / "idx"
    write_index(name, d)
    assert subprocess.run([MOVI, "color", "-i", str(d)], capture_output=True).returncode == 0
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads) if len(s)))
    base = [MOVI, "query", "-i", str(d), "-r", str(fa), "--multi-classify", "-n"]

    def lines(extra, env=None):
        r = subprocess.run(base + extra, capture_output=True, env=env)
        assert r.returncode == 0, r.stderr
        return r.stdout.split(b"\n")[:-1]

    assert lines(["--stdout"]) == expected_lines(name, 1)
    if name != "ref3":
        return
    small = dict(os.environ, MOVI_COLOR_SCRATCH_BYTES="600")
    assert lines(["--stdout", "--min-len", "5"], env=small) == expected_lines(name, 5)
    assert lines(["--stdout", "--min-len", "255"]) == expected_lines(name, 255)
    assert lines(["--stdout", "--report-all"]) == expected_lines(name, 1, report_all=True)
    assert lines(["--stdout", "--report-all", "--min-diff-frac", "0.3"]) == expected_lines(name, 1, report_all=True, min_diff_frac=0.3)
    assert lines(["--stdout", "--report-all", "--min-score-frac", "0.5"]) == expected_lines(name, 1, report_all=True, min_score_frac=0.5)
    # --reverse: the reads reversed (not complemented) before the walk
    from oracle.oracle import Oracle
    _, f, img, _, _, _ = text(name)
    flat, inds, ns, _ = expected_tables(name)
    o = Oracle(img)
    rev = [r[::-1] for r in reads]
    rs = [color_ref.score(f, o, rd, flat, inds, ns, 1) for rd in rev]
    o.close()
    assert lines(["--stdout", "--reverse"]) == expected_lines(name, 1, reads=rev, scores=rs)
    # the report file; --no-output; two logical GPUs; the strand scheduler's record order is the PML file's
    assert lines(["-o", str(tmp_path / "rep.txt")]) == [] and (tmp_path / "rep.txt").read_bytes().split(b"\n")[:-1] == expected_lines(name, 1)
    assert lines(["-o", str(tmp_path / "none.txt"), "--no-output"]) == [] and not (tmp_path / "none.txt").exists()
    assert lines(["--stdout", "--gpus", "2"], env=dict(os.environ, MOVI_SHARE_GPU="1")) == expected_lines(name, 1)
    r = subprocess.run([MOVI, "query", "-i", str(d), "-r", str(fa), "--multi-classify", "--stdout"], capture_output=True)
    assert r.returncode == 0 and sorted(r.stdout.split(b"\n")[:-1]) == sorted(expected_lines(name, 1))
    r2 = subprocess.run([MOVI, "query", "-i", str(d), "-r", str(fa), "-o", str(tmp_path / "p")], capture_output=True)
    assert r2.returncode == 0
    from test_sa_gpu import pml_file_ids
    assert [ln.split(b",")[0] for ln in r.stdout.split(b"\n")[:-1]] == pml_file_ids((tmp_path / "p.pml.bpf").read_bytes())
