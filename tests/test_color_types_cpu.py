"""CPU suite: the references of tests/test_color_types_gpu.py, checked before anything on the device relies on them -- the texts
(small4, poly, long1), tests/color_ref.py's tables on every index type (each type's own run boundaries: 12-bit lengths, blocks, samples)
with and without separators and with document offsets that do not end at n - 1, against a brute force over the text and the suffix
array; color_ref.score past PML 65535 against the closed form of a read that matches from its first base to its last."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_parity import mutated_reads
import color_ref
import odd_texts
import sa_ref

MODES = (6, 8, 7, 3, 2, 5)
THRESHOLD_MODES = (6, 8, 7)
SMALL4_IDS = [9606, 12, 9606, 70000]                         # two documents of one taxon, gaps in the ids
LONG1_LEN = 100_000
LONG1_SUM = 705_082_704                                      # 100000 * 100001 / 2 mod 2^32
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _ref():
    from oracle import build_index as B
    return B.read_fasta(os.path.join(GOLDEN, "ref.fasta"))[0][1]


@functools.lru_cache(maxsize=None)
def small4_seqs():
    """Four documents of 3 - 6 kb cut from ref.fasta; the second overlaps the first and the fourth by 1 kb each, so that runs hold
    several documents and reads drawn there have a runner-up."""
    ref = _ref()
    return (ref[1000:4000], ref[3000:9000], ref[30100:35100], ref[8000:13800])


@functools.lru_cache(maxsize=None)
def _small4_table(sep):
    from oracle import build_index as B
    t = B.clean_text(small4_seqs(), separators=sep)
    bwt, thr = B.bwt_and_thresholds(t)
    return t, bwt, thr, B.suffix_array(t)


@functools.lru_cache(maxsize=None)
def small4(mode, sep):
    """(seqs, build_rows fields, index image, SA, doc_offsets, doc_ids) of small4 as `movi build --type <mode> [--separators]` indexes it."""
    from oracle import build_index as B
    _, bwt, thr, SA = _small4_table(sep)
    f = B.build_rows(bwt, thr, mode)
    return small4_seqs(), f, B.serialize(f), SA, color_ref.doc_offsets_of(small4_seqs(), separators=sep), SMALL4_IDS


@functools.lru_cache(maxsize=None)
def poly(mode, sep):
    """odd_texts' poly (runs split at MAX_RUN_LENGTH), the documents cut inside the runs of A, as tests/test_color_gpu.py cuts them."""
    f, img = odd_texts.fields("poly", sep, mode)
    n = f["n"]
    return tuple(odd_texts.odd_text("poly")), f, img, odd_texts.table("poly", sep)[2], list(range(700, n - 1, 700)) + [n - 1], None


@functools.lru_cache(maxsize=None)
def long1():
    """One document of 100 000 uniformly random bases -- its last 20 set to A -- and two short ones; mode 6.  Every PML walk starts on the
    last BWT row, the largest suffix of the text.  The document's reverse complement follows it and opens with 20 T, the longest run of T
    there is, so the largest suffix starts right behind the document: read as a whole, the document matches from its first base
    (counted from its end) to its last, base k with match length k + 1.  (A walk that had to reposition at its first base would
    give k.)"""
    from oracle import build_index as B
    rng = np.random.default_rng(6400)
    doc = _ACGT[rng.integers(0, 4, LONG1_LEN)].copy()
    doc[-20:] = ord("A")
    seqs = (bytes(doc), bytes(_ACGT[rng.integers(0, 4, 300)]), bytes(_ACGT[rng.integers(0, 4, 500)]))
    f, SA = sa_ref.text_fields(seqs, 6)
    return seqs, f, B.serialize(f), SA, color_ref.doc_offsets_of(seqs), None


def text_of(name, mode, sep):
    return {"small4": small4, "poly": poly}[name](mode, sep)


@functools.lru_cache(maxsize=None)
def expected_tables(name, mode, sep, last=None):
    """color_ref.tables of a text; `last`: the last document's end in place of n - 1."""
    _, f, _, SA, offsets, doc_ids = long1() if name == "long1" else text_of(name, mode, sep)
    return color_ref.tables(f, SA, odd_offsets(offsets, last), doc_ids)


def odd_offsets(offsets, last):
    return list(offsets) if last is None else list(offsets[:-1]) + [last]


def odd_lasts(n):
    """The last document ends early; it ends beyond the text."""
    return (n - 1 - 37, n + 1000)


def boundary_reads(seqs, offsets, sep):
    """Stretches of the indexed text across every document's end but the last and, with separators, across every '%' of the text (small4:
    the documents' ends fall on them): the text itself and the two sides joined without the '%' -- a read that spans a '%' of the
    indexed text."""
    from oracle import build_index as B
    t = bytes(B.clean_text(seqs, separators=sep)[:-1])
    out = [t[max(0, end - 40): end + 40] for end in offsets[:-1][:20]]
    for p in [i for i in range(len(t)) if t[i] == B.SEPARATOR][:20]:
        out += [t[max(0, p - 40): p + 41], t[max(0, p - 40): p] + t[p + 1: p + 41]]
    return out


@functools.lru_cache(maxsize=None)
def reads_of(name, sep):
    """tests/test_color_gpu.py::reads_of's recipe: mutated substrings (N and lower case among them), stretches across the documents'
    ends, the fixed lengths, empty, all-N, N inside, a read absent from the text; with separators the reads across a '%' and one that
    holds a '%' itself."""
    seqs, _, _, _, offsets, _ = text_of(name, 6, sep)
    fwd = b"".join(seqs)
    rng = np.random.default_rng(6500 + (name == "poly") * 2 + sep)
    reads = mutated_reads(rng, fwd, 130, 1, 300)
    reads += boundary_reads(seqs, offsets, sep)
    one = max(seqs, key=len)
    for ln in (1, 2, 63, 64, 65, 300):
        reads.append(one[5:5 + ln])
    reads += [b"", b"N" * 40, fwd[:33] + b"NN" + fwd[35:80], bytes(_ACGT[rng.integers(0, 4, 200)])]
    if sep:
        reads.append(fwd[100:140] + b"%" + fwd[140:180])
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def expected_scores(name, mode, sep, min_len):
    """Per read (score, number of times the lead changed hands) by color_ref.score."""
    from oracle.oracle import Oracle
    _, f, img, _, _, _ = text_of(name, mode, sep)
    flat, inds, ns, _ = expected_tables(name, mode, sep)
    o = Oracle(img)
    codes = sa_ref.code_table(f)
    out = []
    for rd in reads_of(name, sep):
        changes = []
        out.append((color_ref.score(f, o, rd, flat, inds, ns, min_len, codes, changes), len(changes)))
    o.close()
    return out


def long1_reads():
    """The whole document beside ~70 short reads: its wavefront's other lanes finish early."""
    seqs = long1()[0]
    rng = np.random.default_rng(6600)
    fwd = b"".join(seqs)
    short = mutated_reads(rng, fwd, 66, 1, 200) + [b"", b"N" * 10, seqs[1][:64], seqs[2][:65]]
    return short[:30] + [seqs[0]] + short[30:], 30


@functools.lru_cache(maxsize=None)
def long1_scores(min_len=1):
    from oracle.oracle import Oracle
    _, f, img, _, _, _ = long1()
    flat, inds, ns, _ = expected_tables("long1", 6, False)
    o = Oracle(img)
    codes = sa_ref.code_table(f)
    out = [color_ref.score(f, o, rd, flat, inds, ns, min_len, codes) for rd in long1_reads()[0]]
    o.close()
    return out


def corrupt_image(img, stride=97):
    """The image with the destination id of every `stride`-th row set to 0xFFFFFFFF (mode 6: the id's low 32 bits lead the row)."""
    import movi_amd
    desc, _, off, nbytes = movi_amd.parse_index_image(img)
    assert desc.mode == 6 and nbytes == desc.r * 8
    out = bytearray(img)
    rows = np.frombuffer(img, np.uint8, count=nbytes, offset=off).reshape(-1, 8).copy()
    rows[::stride, 0:4] = 0xFF
    out[off: off + nbytes] = rows.tobytes()
    return bytes(out)


def corrupt_reads():
    """Lengths of 20 - 300 over a table with every 97th id off: a walk of L bases leaves ~L distinct rows by an LF step, so about
    (96 / 97)^L of them meet no corrupted row -- both populations are well above a tenth of the batch."""
    fwd = b"".join(small4_seqs())
    return mutated_reads(np.random.default_rng(6700), fwd, 200, 20, 300)


# ------------------------------------------------------------------------------------------------------------------ the tests

@functools.lru_cache(maxsize=None)
def _small4_sa_checked(sep):
    """The suffix array is THE sorted order of the suffixes (checked once per text)."""
    t, _, _, SA = _small4_table(sep)
    tb, sa = bytes(t), [int(x) for x in SA]
    assert sorted(sa) == list(range(len(tb))) and all(tb[sa[i]:] < tb[sa[i + 1]:] for i in range(len(tb) - 1))
    return np.asarray(SA)


def brute_force_sets(sep, lens, offsets, ids):
    """The document of a text position is the first one that ends beyond it, the last one for what lies past every end; the set of
    a run is what its BWT positions -- found through the sorted suffixes -- fall into."""
    SA = _small4_sa_checked(sep)
    n = len(SA)
    doc_of_text = np.array(ids)[np.minimum(np.searchsorted(offsets, np.arange(n), "right"), len(offsets) - 1)]
    docs = doc_of_text[SA]
    sets, pos = [], 0
    for ln in lens:
        sets.append(sorted(set(int(x) for x in docs[pos: pos + int(ln)])))
        pos += int(ln)
    assert pos == n
    return docs, sets


def check_against_brute_force(sep, f, SA, offsets, doc_ids):
    ids, to_taxon = color_ref.species(doc_ids, len(offsets))
    docs, sets = brute_force_sets(sep, f["lens"], offsets, ids)
    assert (color_ref.doc_of_bwt(SA, offsets, ids) == docs).all()
    flat, inds, ns, taxa = color_ref.tables(f, SA, offsets, doc_ids)
    assert ns == len(to_taxon) and taxa == to_taxon and len(inds) == f["r"] == len(sets)
    fresh = 0                                                     # first-appearance numbering: a new set lies right behind the ones before
    for i, at in enumerate(int(a) for a in inds):                 # every run reads its own set back
        assert list(flat[at + 1: at + 1 + flat[at]]) == sets[i]
        assert at <= fresh
        if at == fresh:
            fresh += 1 + len(sets[i])
    assert fresh == len(flat) == sum(1 + len(s) for s in {tuple(s) for s in sets})
    return sets


def test_texts_have_their_shapes():
    seqs = small4_seqs()
    assert [len(s) for s in seqs] == [3000, 6000, 5000, 5800]
    for sep in (False, True):
        n = small4(6, sep)[1]["n"]
        assert n == 2 * 19800 + 1 + 8 * sep
        assert small4(6, sep)[4][-1] == n - 1
        for mode in (7, 5):                                       # (a sampled table of a multiple of 20 rows is no usable index: odd_texts.py)
            assert small4(mode, sep)[1]["r"] % 20 != 0, (mode, sep)
        for mode in MODES:
            assert max(small4(mode, sep)[1]["lens"]) <= {6: 2047, 8: 1023, 7: 511, 3: 4095, 2: 1023, 5: 1023}[mode]
    # the types cut their runs differently: the tables are not one table
    assert len({small4(m, False)[1]["r"] for m in MODES}) >= 2
    for mode, sep in ((6, True), (8, True), (3, True)):
        f = poly(mode, sep)[1]
        assert f["sep"] == 1 and max(f["lens"]) == {6: 2047, 8: 1023, 3: 4095}[mode] and poly(mode, sep)[4][-1] == f["n"] - 1
    assert poly(7, True)[1]["r"] % 20 != 0


@pytest.mark.parametrize("sep", [False, True])
def test_restatement_against_brute_force_on_every_type(sep):
    """tests/test_color_cpu.py::test_restatement_against_brute_force on small4, in every type's own rows."""
    t = _small4_table(sep)[0]
    shared = 0
    for mode in MODES:
        _, f, _, SA, offsets, doc_ids = small4(mode, sep)
        sets = check_against_brute_force(sep, f, SA, offsets, doc_ids)
        assert expected_tables("small4", mode, sep)[2:] == (3, [12, 9606, 70000])
        shared += any(len(s) > 1 for s in sets)
    assert shared == len(MODES)                                   # some runs are shared between documents
    if sep:                                                       # the documents' ends fall on '%' rows
        _, f, _, SA, offsets, _ = small4(6, True)
        assert all(t[e - 1] == 37 for e in offsets) and f["sep"] == 1


@pytest.mark.parametrize("sep", [False, True])
def test_arbitrary_last_offset(sep):
    """doc_of_bwt / tables with a last end that is not n - 1: "the last one takes what lies past every end"."""
    _, f, _, SA, offsets, doc_ids = small4(6, sep)
    base = expected_tables("small4", 6, sep)
    for last in odd_lasts(f["n"]):
        offs = odd_offsets(offsets, last)
        assert offs[-1] != f["n"] - 1 and offs[-1] > offs[-2]
        check_against_brute_force(sep, f, SA, offs, doc_ids)
        got = expected_tables("small4", 6, sep, last)
        # only the last document's end moved, and what lies past it is the last document's either way: the same tables
        assert (got[0] == base[0]).all() and (got[1] == base[1]).all()
    # ... which they are not once an end inside the text moves
    moved = offsets[:-2] + [offsets[-2] - 500, offsets[-1]]
    check_against_brute_force(sep, f, SA, moved, doc_ids)
    other = color_ref.tables(f, SA, moved, doc_ids)
    assert len(other[0]) != len(base[0]) or (other[0] != base[0]).any() or (other[1] != base[1]).any()


def test_long_match_in_closed_form(built_lib):
    """The restatement's validity past PML 65535: long1's document read as a whole."""
    seqs, f, img, SA, offsets, _ = long1()
    n = f["n"]
    assert len(seqs[0]) == LONG1_LEN and n == 2 * (LONG1_LEN + 800) + 1
    assert int(SA[n - 1]) == LONG1_LEN                           # the largest suffix starts right behind the document
    assert LONG1_LEN * (LONG1_LEN + 1) // 2 % (1 << 32) == LONG1_SUM and LONG1_LEN >= 92_682 and 92_682 * 92_683 // 2 >= 1 << 32 > 92_681 * 92_682 // 2
    w = sa_ref.walk(f, seqs[0], clamp=False)
    assert [x[2] for x in w] == list(range(1, LONG1_LEN + 1))
    assert [x[2] for x in sa_ref.walk(f, seqs[0][-70000:])] == [min(k + 1, 65535) for k in range(70000)]      # (the clamped form, as before)
    reads, at = long1_reads()
    assert reads[at] == seqs[0] and len(reads) >= 70 and at % 64 not in (0, 63)
    want = long1_scores()
    best, second, colors_count, sum_ml, cnt = want[at]
    ns = expected_tables("long1", 6, False)[2]
    assert ns == 3 and sum_ml == LONG1_SUM
    # min_len 1: every base but the first is scored; all of them stand in the document, most of them in no other
    assert colors_count == LONG1_LEN - 1 and best == 0 and cnt[0] == LONG1_LEN - 1 and max(cnt[1:]) < 5000
    # 255: the match length is tested unclamped -- past 65535 it still is >= min_len
    assert long1_scores(255)[at][2] == LONG1_LEN - 255 and long1_scores(255)[at][3] == LONG1_SUM


def test_scores_have_their_shapes(built_lib):
    """What the device tests need of their reads, on every thresholds type: a read without a best document, one with a runner-up, one
    whose lead changes hands (the tie rule matters), and the same reads on every type."""
    for name, mode, sep in [("small4", m, s) for m in THRESHOLD_MODES for s in (False, True)] + [("poly", 6, True)]:
        reads = reads_of(name, sep)
        assert len(reads) > 128 and {0, 1, 2, 63, 64, 65, 300} <= {len(r) for r in reads}
        want = expected_scores(name, mode, sep, 1)
        assert any(w[0] == color_ref.NONE for w, _ in want), (name, mode, sep)
        assert any(w[1] != color_ref.NONE for w, _ in want), (name, mode, sep)
        assert any(ch > 0 for _, ch in want), (name, mode, sep)
        if sep:
            assert sum(b"%" in r for r in reads) >= 2
    # min_len 0 scores every base, N included -- the read's first one on the set of the last row, before any LF step
    z, o = expected_scores("small4", 6, False, 0), expected_scores("small4", 6, False, 1)
    assert all(a[0][2] >= b[0][2] for a, b in zip(z, o)) and any(a[0][2] > b[0][2] for a, b in zip(z, o))
    assert [a[0][2] for a, rd in zip(z, reads_of("small4", False))] == [len(rd) for rd in reads_of("small4", False)]
