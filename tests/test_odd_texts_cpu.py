"""CPU suite: the texts of tests/odd_texts.py hold what tests/test_odd_texts_gpu.py relies on (rows at MAX_RUN_LENGTH, packed offsets
above 1024 / 2048, more BWT positions than a locate launch has lanes, a two-letter alphabet), and the references of the locate, MEM
and k-mer queries (tests/sa_ref.py, mem_ref.py, kmer_ref.py) agree with the literal algorithms on them."""
import numpy as np
import pytest

import kmer_ref
import mem_ref
import odd_texts
import sa_ref
from oracle import build_index as B

CASES = [(kind, sep) for kind in odd_texts.KINDS for sep in (False, True)]
RATES = (7, 100, 3000)


def _as_lists(f):
    """The build_rows fields with plain lists for the arrays: the literal walks index them a few million times."""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in f.items()}


def capped_rows(f):
    return np.flatnonzero(np.asarray(f["lens"]) == B.MAX_RUN[f["mode"]])


@pytest.mark.parametrize("kind,sep", CASES)
def test_structure(built_lib, kind, sep):
    from oracle.oracle import Oracle
    bwt, _, SA = odd_texts.table(kind, sep)
    n = len(SA)
    reads = odd_texts.reads_of(kind)
    assert len(reads) == 304 + (kind in ("poly", "tandem")) and reads == tuple(odd_texts.odd_reads(kind, b"".join(odd_texts.odd_text(kind))))
    # (see odd_texts.SEEDS: a sampled-ids table of that many rows is one the reference cannot walk; mode 7 is the one used on these texts)
    assert odd_texts.fields(kind, sep, 7)[0]["r"] % B.TALLY_CHECKPOINTS != 0
    if kind in ("poly", "tandem"):
        for mode in (6, 3, 7):
            f, _ = odd_texts.fields(kind, sep, mode)
            cap, code = capped_rows(f), np.asarray(f["code"])
            assert len(cap) >= 1, mode
            assert (code[cap] == code[np.minimum(cap + 1, f["r"] - 1)]).any(), mode      # consecutive rows of one character
        f, img = odd_texts.fields(kind, sep, 6)
        o = Oracle(img)
        top = max(int(offs.max()) for _, offs in sa_ref.positions(f, o, reads) if len(offs))
        o.close()
        assert top >= 1024, top                              # what sa_pos_kernel packs and locate_kernel unpacks
        if kind == "poly":
            # Mode 3 keeps no thresholds, so there is no PML walk on it (sa_ref.walk and Oracle.pml are not defined there) and no read
            # has positions: what reaches the kernels in mode 3 are the positions of the exhaustive locate, sa_ref.all_positions.
            f3, _ = odd_texts.fields(kind, sep, 3)
            rows, offs = sa_ref.all_positions(f3)
            assert int(offs.max()) >= 2048 and int(offs.max()) == B.MAX_RUN[3] - 1
            assert (np.asarray(f3["all_p"])[rows] + offs == np.arange(f3["n"])).all()
    elif kind == "pangenome":
        assert n > 262144                                    # more items than 256 CUs x 16 wavefronts x 64 lanes
        f, _ = odd_texts.fields(kind, sep, 6)
        assert int(np.asarray(f["lens"]).max()) >= 100
    else:
        f, _ = odd_texts.fields(kind, sep, 6)
        assert len(f["alphabet"]) == (3 if sep else 2)


def _probe_positions(f, SA, rng):
    """500 BWT positions as (row, offset): row r - 1 (both ends), BWT position 0, the last offset of every row at MAX_RUN_LENGTH,
    the BWT position of text position 0 (the one walk that wraps at every rate), the rest drawn."""
    all_p, lens, r, n = np.asarray(f["all_p"]), np.asarray(f["lens"]), f["r"], f["n"]
    fixed = [(r - 1, 0), (r - 1, int(lens[r - 1]) - 1), (0, 0)] + [(int(i), int(lens[i]) - 1) for i in capped_rows(f)]
    p0 = int(np.flatnonzero(np.asarray(SA) == 0)[0])
    row0 = int(np.searchsorted(all_p, p0, "right") - 1)
    fixed.append((row0, p0 - int(all_p[row0])))
    assert len(fixed) <= 500
    ps = rng.integers(0, n, 500 - len(fixed))
    rows = np.searchsorted(all_p, ps, "right") - 1
    return fixed + [(int(i), int(p - all_p[i])) for i, p in zip(rows, ps)]


@pytest.mark.parametrize("kind,sep", CASES)
def test_locate_references_equal_the_literal_walks(kind, sep):
    """sa_ref.samples / entries against find_sampled_SA_entries / get_SA_entries walked literally over the mode-6 rows, and
    get_SA_entries over the mode-3 rows (4095-character rows) too."""
    _, _, SA = odd_texts.table(kind, sep)
    rng = np.random.default_rng(4242 + odd_texts.KINDS.index(kind) * 2 + sep)
    f6 = _as_lists(odd_texts.fields(kind, sep, 6)[0])
    n = f6["n"]
    for rate in RATES:
        smp = sa_ref.samples(SA, rate)
        assert (sa_ref.lf_walk_samples(f6, rate) == smp).all(), rate
        want = sa_ref.entries(SA, rate)
        for mode in (6, 3):
            f = f6 if mode == 6 else _as_lists(odd_texts.fields(kind, sep, 3)[0])
            probes = _probe_positions(odd_texts.fields(kind, sep, mode)[0], SA, rng)
            exp = [int(want[f["all_p"][i] + o]) for i, o in probes]
            assert [sa_ref.lf_walk_entry(f, smp, rate, i, o) for i, o in probes] == exp, (rate, mode)
            assert max(exp) >= n, (rate, mode)               # a walk past text position 0: entry + n


@pytest.mark.parametrize("kind,sep", CASES)
def test_mem_reference(built_lib, kind, sep):
    """The header's loop (mem_ref.restate) on the oracle's searches; on the single-record texts without separators, which are closed
    under reverse complement (tests/test_mem_gpu.py::test_mems_vs_restatement), it equals the set of all MEMs."""
    from oracle.oracle import Oracle
    f, img = odd_texts.fields(kind, sep, 6)
    reads = list(odd_texts.reads_of(kind))
    o = Oracle(img)
    exp, arr = mem_ref.restate(o, reads, sa_ref.code_table(f), (1, 12, 25))
    o.close()
    for L in (1, 12, 25):
        assert sum(len(x) for x in exp[L]) > 100, L
        for r, ms in zip(reads, exp[L]):
            assert all(0 <= s < e <= len(r) and e - s >= L and c >= 1 for s, e, c in ms)
        if not sep and kind != "pangenome":                  # (24 records: the junctions between them are not rc-symmetric)
            assert exp[L] == [mem_ref.mems_set(fw, cnt, len(r), L) for r, (bw, fw, cnt) in zip(reads, arr)], L
    if kind == "poly":
        assert max(c for ms in exp[1] for _, _, c in ms) > 4095
    if kind in ("poly", "tandem"):
        assert any(ms == [(0, 3000, ms[0][2])] for ms in exp[25] if ms)      # the 3000-base read is one match


@pytest.mark.parametrize("kind,sep", CASES)
def test_kmer_reference(built_lib, kind, sep):
    """kmer_ref.restate against the transcription of the reference's control flow over plain substring search in the text."""
    from oracle.oracle import Oracle
    f, img = odd_texts.fields(kind, sep, 6)
    reads = list(odd_texts.reads_of(kind))
    text = bytes(B.clean_text(odd_texts.odd_text(kind), separators=sep)[:-1])
    codes = sa_ref.code_table(f)
    legal = lambda c: codes[c] != 0xFF
    seen = {}

    def occ(x):
        x = bytes(x)
        if x not in seen:
            seen[x] = x in text
        return seen[x]

    o = Oracle(img)
    exp, _ = kmer_ref.restate(o, reads, (1, 12, 31))
    o.close()
    n_def = found = 0
    for k in (1, 12, 31):
        for j, (R, want) in enumerate(zip(reads, exp[k])):
            found += want[0]
            if not R or (j < 300 and j % 3):                 # every third mutated read and all the fixed ones: substring search in
                continue                                     # a repetitive text of 60 - 288 k characters is what this test's time goes to
            for fk in (0, 5):                                # (no table, a table: tests/test_kmer_cpu.py walks the values in between)
                if fk >= k:
                    continue
                got = kmer_ref.literal(occ, legal, R, k, fk)
                if got is None:
                    continue
                n_def += 1
                assert got == want, (R, k, fk)
    assert n_def > 300 and found > 10000
