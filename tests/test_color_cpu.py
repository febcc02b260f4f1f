"""CPU suite: Movi Color -- tests/color_ref.py's restatement against a brute-force set computation, the flat file image, write_mls on
hand-made counter rows (the restatement and the CLI's writer), the command lines of `movi color` / `movi query --multi-classify`, and
the new ABI symbols."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import color_ref
import sa_ref

MOVI = os.path.join(ROOT, "movi_amd", "bin", "movi")
NONE = color_ref.NONE


def run(args):
    return subprocess.run([MOVI] + args, capture_output=True)


@pytest.fixture(scope="module")
def small():
    """A text of a few hundred bases in 3 documents (rc and separators included): (fields, SA, text, offsets)."""
    from oracle import build_index as B
    rng = np.random.default_rng(77)
    anc = rng.choice(list(b"ACGT"), 60).astype(np.uint8)
    seqs = []
    for _ in range(3):                                            # near-identical documents: runs shared by several of them
        g = anc.copy()
        g[rng.integers(0, 60, 4)] = rng.choice(list(b"ACGT"), 4)
        seqs.append(bytes(g))
    t = B.clean_text(seqs, separators=True)
    f, SA = sa_ref.text_fields(seqs, 6, separators=True)
    return f, SA, t, color_ref.doc_offsets_of(seqs, separators=True), seqs


def test_restatement_against_brute_force(small):
    f, SA, t, offsets, seqs = small
    n = f["n"]
    assert 300 <= n <= 400 and offsets == [122, 244, 366] and offsets[-1] == n - 1
    for doc_ids in (None, [7, 3, 7], [500, 20, 1]):
        ids, to_taxon = color_ref.species(doc_ids, 3)
        assert to_taxon == sorted(set(doc_ids or [1, 2, 3])) and [to_taxon[i] for i in ids] == list(doc_ids or [1, 2, 3])
        # brute force: the document of a text position is the first one that ends beyond it (the terminator: the last one); the
        # set of a run is what its BWT positions -- found through the sorted suffixes themselves -- fall into
        order = sorted(range(n), key=lambda i: bytes(t[i:]))
        assert order == [int(x) for x in SA]
        doc_of_text = [ids[min(int(np.searchsorted(offsets, p, "right")), 2)] for p in range(n)]
        sets, pos = [], 0
        for ln in f["lens"]:
            sets.append(sorted({doc_of_text[order[p]] for p in range(pos, pos + int(ln))}))
            pos += int(ln)
        assert pos == n
        docs = color_ref.doc_of_bwt(SA, offsets, ids)
        assert [int(d) for d in docs] == [doc_of_text[p] for p in order]
        assert color_ref.run_sets(f, docs) == sets
        flat, inds, ns, taxa = color_ref.tables(f, SA, offsets, doc_ids)
        assert ns == len(to_taxon) and taxa == to_taxon
        # first-appearance numbering: offsets appear in increasing order of first use, and every run reads its own set back
        firsts = []
        for i, at in enumerate(inds):
            at = int(at)
            assert list(flat[at + 1: at + 1 + flat[at]]) == sets[i]
            if at not in firsts:
                assert not firsts or at > firsts[-1]
                firsts.append(at)
        assert sum(1 + len(s) for s in {tuple(s) for s in sets}) == len(flat)
        if doc_ids is None:
            assert len({tuple(s) for s in sets}) > 2                   # some runs are shared between documents


def test_flat_file_round_trip(small):
    f, SA, _, offsets, _ = small
    flat, inds, _, _ = color_ref.tables(f, SA, offsets)
    raw = color_ref.flat_file(flat, inds)
    assert len(raw) == 8 + 2 * len(flat) + 5 * f["r"] and raw[:8] == len(flat).to_bytes(8, "little")
    flat2, inds2 = color_ref.read_flat_file(raw, f["r"])
    assert (flat2 == flat).all() and (inds2 == inds).all()
    big = color_ref.flat_file(flat, [(1 << 39) + 5])                   # the 5-byte offsets: u32 low, u8 high
    assert big[-5:] == bytes([5, 0, 0, 0, 0x80]) and int(color_ref.read_flat_file(big[:8 + 2 * len(flat)] + big[-5:], 1)[1][0]) == (1 << 39) + 5


def test_scoring_reads_the_row_before_the_reposition(small, built_lib):
    """process_char scores after the LF step and before the comparison (src/read_processor.cpp:100-186): on reads whose bases
    reposition, the scored rows are the LF targets, they differ from the rows the walk stands on after those bases, and a literal
    replay of the counters over them gives score()'s answer."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    f, SA, t, offsets, seqs = small
    flat, inds, ns, _ = color_ref.tables(f, SA, offsets)
    o = Oracle(B.serialize(f))
    rng = np.random.default_rng(12)
    differ = 0
    for _ in range(40):
        rd = bytearray(seqs[int(rng.integers(0, 3))][int(rng.integers(0, 20)):][:int(rng.integers(5, 40))])
        rd[int(rng.integers(0, len(rd)))] = b"ACGT"[int(rng.integers(0, 4))]
        rd = bytes(rd)
        w = sa_ref.walk(f, rd)
        idx, off, ml = f["r"] - 1, int(f["lens"][f["r"] - 1]) - 1, 0
        cnt, cc = [0] * ns, 0
        for k, (row_after, off_after, pml) in enumerate(w):
            if k:
                idx, off = sa_ref._lf(f, idx, off)
            if ml >= 1:
                cc += 1
                at = int(inds[idx])
                for d in flat[at + 1: at + 1 + int(flat[at])]:
                    cnt[int(d)] += 1
            differ += idx != row_after
            idx, off, ml = row_after, off_after, pml
        res = color_ref.score(f, o, rd, flat, inds, ns, 1)
        assert res[2] == cc and res[4] == cnt and res[3] == sum(x[2] for x in w)
        assert res[0] == color_ref.NONE or cnt[res[0]] == max(cnt)
    o.close()
    assert differ > 10


# (id, length, best, second, colors_count, sum_ml, counters), taxa, kwargs -> line
TAXA = [11, 22, 33, 44]
MLS_CASES = [
    ((b"tie", 100, 1, 2, 90, 4000, [3, 50, 50, 0]), {}, b"tie,22,33"),                      # a tie between best and second: diff 0 < 5 %
    ((b"close", 100, 1, 2, 90, 4000, [3, 100, 96, 0]), {}, b"close,22,33"),                 # 4 < 0.05 * 100
    ((b"edge", 100, 1, 2, 90, 4000, [3, 100, 95, 0]), {}, b"edge,22,0"),                    # 5 < 5.0 is false
    ((b"alone", 100, 3, NONE, 90, 4000, [0, 0, 0, 9]), {}, b"alone,44,0"),                  # second == none
    ((b"low", 100, 1, 2, 90, 39, [3, 50, 50, 0]), {}, b"low,0,0"),                          # PML mean 0.39 < 0.4
    ((b"at", 100, 1, 2, 90, 40, [3, 50, 50, 0]), {}, b"at,22,33"),                          # float(0.4f) = 0.4000000059... is not < 0.4
    ((b"nodoc", 100, NONE, NONE, 0, 5000, [0, 0, 0, 0]), {}, b"nodoc,0,0"),
    ((b"low", 100, 1, 2, 90, 39, [3, 50, 50, 0]), {"report_all": True}, b"low,0"),
    ((b"all", 100, 1, 2, 90, 4000, [3, 100, 96, 95]), {"report_all": True}, b"all,22,33"),   # default min-diff-frac 0.05, in document order
    ((b"wide", 100, 2, 1, 90, 4000, [80, 96, 100, 3]), {"report_all": True, "min_diff_frac": 0.25}, b"wide,33,11,22"),
    ((b"frac", 100, 1, 2, 90, 4000, [3, 100, 96, 95]), {"report_all": True, "min_diff_frac": 0.05000001}, b"frac,22,33,44"),   # float(0.05000001) * 100 = 5.000001 > 5, where 0.05f * 100 is 5
    ((b"score", 100, 1, 2, 200, 4000, [99, 100, 150, 0]), {"report_all": True, "min_score_frac": 0.5}, b"score,,22,33"),   # no best up front
    ((b"none", 100, 1, 2, 200, 4000, [3, 99, 96, 95]), {"report_all": True, "min_score_frac": 0.5}, b"none,0"),           # no document qualifies
]


def test_write_mls_restatement():
    for (rid, ln, best, second, cc, total, cnt), kw, want in MLS_CASES:
        assert color_ref.mls_line(rid, ln, (best, second, cc, total, cnt), TAXA, **kw) == want, rid


def test_write_mls_writer(tmp_path):
    """The CLI's writer gives the restatement's lines, on the hand-made rows and on random ones near the thresholds."""
    exe = str(tmp_path / "mls_line_driver")
    host = os.path.join(ROOT, "movi_amd", "host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "mls_line_driver.cpp"),
                           os.path.join(host, "output.cpp"), os.path.join(host, "options.cpp"), os.path.join(host, "reads.cpp"), "-lpthread"])
    cases = [(c, kw) for c, kw, _ in MLS_CASES]
    rng = np.random.default_rng(9)
    for k in range(300):
        cnt = [int(x) for x in rng.integers(0, 120, 4)]
        order = sorted(range(4), key=lambda i: -cnt[i])
        kw = [{}, {"report_all": True}, {"report_all": True, "min_diff_frac": float(rng.random() * 0.3)},
              {"report_all": True, "min_score_frac": float(rng.random())}][k % 4]
        cases.append(((b"r%d" % k, int(rng.integers(1, 300)), order[0], order[1] if k % 7 else NONE, int(rng.integers(0, 300)),
                       int(rng.integers(0, 200)), cnt), kw))
    text, want = [], []
    for (rid, ln, best, second, cc, total, cnt), kw in cases:
        text.append(" ".join([rid.decode(), str(ln), str(best), str(second), str(cc), str(total), str(int(kw.get("report_all", False))),
                              repr(kw.get("min_diff_frac", 0.05)), repr(kw.get("min_score_frac", 0.0)), "4"] + [str(t) for t in TAXA] + [str(c) for c in cnt]))
        want.append(color_ref.mls_line(rid, ln, (best, second, cc, total, cnt), TAXA, **kw))
    got = subprocess.run([exe], input="\n".join(text).encode(), capture_output=True, check=True).stdout
    assert got.split(b"\n")[:-1] == want


def test_command_lines(built_lib, tmp_path):
    # movi color: the reference's error without -i (src/movi_parser.cpp:319-330); a command now
    r = run(["color"])
    assert r.returncode == 1 and b"Please specify the index directory file." in r.stderr
    r = run(["color", "-i", str(tmp_path / "nothing")])
    assert r.returncode == 1 and b"not part of the MI355X engine" not in r.stderr and b"Error parsing command line" not in r.stderr
    assert b"doc_offsets file not found at \"" + str(tmp_path / "nothing").encode() + b"/ref.fa.doc_offsets\"" in r.stderr
    # --multi-classify is a query flag now: a missing index is reported as that
    r = run(["query", "-i", str(tmp_path / "nothing"), "-r", "y", "--multi-classify", "--stdout"])
    assert r.returncode == 1 and b"not supported" not in r.stderr and b"Error parsing command line" not in r.stderr
    assert b"index does not exist at " + str(tmp_path / "nothing").encode() in r.stderr
    idx = tmp_path / "idx"
    idx.mkdir()
    (idx / "index.movi").write_bytes(b"x")
    r = run(["query", "-i", str(idx), "-r", "y", "--multi-classify", "--stdout"])
    assert r.returncode == 1 and b"Failed to open document sets flat file at " + str(idx).encode() + b"/doc_sets_flat.bin" in r.stderr
    (idx / "doc_sets_flat.bin").write_bytes(b"x")
    r = run(["query", "-i", str(idx), "-r", "y", "--multi-classify", "--stdout"])
    assert r.returncode == 1 and b"doc_offsets file not found at \"" + str(idx).encode() + b"/ref.fa.doc_offsets\"" in r.stderr
    (idx / "ref.fa.doc_offsets").write_text("10\n20\n30\n")            # doc_ids must name every document
    (idx / "ref.fa.doc_ids").write_text("5 6\n")
    for args in (["query", "-i", str(idx), "-r", "y", "--multi-classify", "--stdout"], ["color", "-i", str(idx)]):
        r = run(args)
        assert r.returncode == 1 and b"ref.fa.doc_ids holds 2 ids for the 3 documents" in r.stderr, args
    # the colour modes outside the default one: each refusal names its flag
    for flag in ("full", "compress", "freq-compress", "tree-compress", "color-vectors", "pvalue-scoring", "early-stop", "report-colors",
                 "report-color-ids", "color-move-rows"):
        r = run(["query", "-i", "x", "-r", "y", "--multi-classify", "--stdout", "--" + flag])
        assert r.returncode == 1 and b"Error parsing command line" in r.stderr and b"--" + flag.encode() + b" is not supported" in r.stderr, flag
    for flag in ("full", "compress", "color-vectors"):
        r = run(["color", "-i", "x", "--" + flag])
        assert r.returncode == 1 and b"--" + flag.encode() + b" is not supported" in r.stderr, flag
    r = run(["build", "-i", "x", "-f", "y", "--color", "--color-vectors"])
    assert r.returncode == 1 and b"--color-vectors is not supported" in r.stderr
    # the forbidden combinations
    for other in (["--zml"], ["--count"], ["--kmer"], ["--mem", "--ftab-k", "8"], ["--sa-entries"]):
        r = run(["query", "-i", "x", "-r", "y", "--multi-classify", "--stdout"] + other)
        assert r.returncode == 1 and b"--multi-classify" in r.stderr and b"cannot be combined" in r.stderr, other
    for extra in ("--classify", "--filter", "--logs"):
        r = run(["query", "-i", "x", "-r", "y", "--multi-classify", "--stdout", extra])
        assert r.returncode == 1 and b"--multi-classify cannot be combined" in r.stderr, extra
    r = run(["query", "-i", "x", "-r", "y", "--multi-classify"])               # the report needs a place
    assert r.returncode == 1 and b"-o / --out-file" in r.stderr
    r = run(["query", "-i", "x", "-r", "y", "--report-all"])
    assert r.returncode == 1 and b"belong to --multi-classify" in r.stderr
    for bad in ("abc", "256", "-1"):
        r = run(["query", "-i", "x", "-r", "y", "--multi-classify", "--stdout", "--min-len", bad])
        assert r.returncode == 1 and b"failed to parse for option 'min-len'" in r.stderr, bad
    r = run(["query", "-i", "x", "-r", "y", "--multi-classify", "--stdout", "--min-diff-frac", "x"])
    assert r.returncode == 1 and b"failed to parse for option 'min-diff-frac'" in r.stderr
    for bad in ("--kmer-count", "--rpml"):                                      # still refused
        r = run(["query", "-i", "x", "-r", "y", bad])
        assert r.returncode == 1 and b"not supported" in r.stderr, bad
    r = run(["--help"])
    assert b"movi color -i DIR" in r.stdout + r.stderr and b"--multi-classify" in r.stdout + r.stderr and b"[--color]" in r.stdout + r.stderr


def test_abi_symbols(built_lib):
    """Every new entry point is bound, is in the header and refuses a NULL handle with MOVI_ERR_ARG."""
    from movi_amd._lib import SYMBOLS, lib
    L = lib()
    new = ("movi_color_build", "movi_color_save", "movi_color_load", "movi_color_get", "movi_multi_classify_device", "movi_multi_classify_host")
    assert all(n in SYMBOLS and hasattr(L, n) for n in new)
    header = open(os.path.join(ROOT, "include", "movi_hip.h")).read()
    assert all(("int %s(" % n) in header for n in new) and "#define MOVI_PREPARE_COLOR 16u" in header and "movi_mc_read_t" in header
    assert L.movi_color_build(None, None, None, 0, None) == -1 and L.movi_last_error()
    assert L.movi_color_save(None, b"x") == -1 and L.movi_color_load(None, b"x", 1) == -1
    assert L.movi_color_get(None, None, None, 0, None, 0, None, None, 0) == -1
    assert L.movi_multi_classify_device(None, None, None, 0, 0, 1, None, None, None, None, None, None) == -1
    assert L.movi_multi_classify_host(None, None, None, 0, 1, None, None, None, None, None) == -1
    assert L.movi_index_prepare(None, 16, None, None) == -1
    import movi_amd
    assert movi_amd.MoveIndex.MC_DTYPE.itemsize == 24 and movi_amd.MoveIndex.PREPARE_COLOR == 16


def test_build_color_writes_the_document_offsets(built_lib, tmp_path):
    """`movi build --color` writes ref.fa.doc_offsets by prepare_ref's rule before the colour step (which needs the GPU and fails here
    or succeeds there); a plain build writes no such file."""
    seqs = [b"ACGTACGTTGCA" * 5, b"acgtnnACGT" * 3, b"TTTTGGGCCCAT" * 4]
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    for sep in (False, True):
        d = tmp_path / ("c%d" % sep)
        run(["build", "-i", str(d), "-f", str(fa), "--color"] + (["--separators"] if sep else []))
        want = color_ref.doc_offsets_of(seqs, separators=sep)
        assert (d / "ref.fa.doc_offsets").read_text().split() == [str(x) for x in want]
        p = tmp_path / ("p%d" % sep)
        r = run(["build", "-i", str(p), "-f", str(fa)] + (["--separators"] if sep else []))
        assert r.returncode == 0 and sorted(os.listdir(p)) == ["index.movi"]
        assert (p / "index.movi").read_bytes() == (d / "index.movi").read_bytes()
