"""Texts with awkward structure for the locate, MEM and k-mer tests (tests/test_odd_texts_cpu.py pins what they hold,
tests/test_odd_texts_gpu.py runs the kernels on them): the kinds of test_ahead_rows_gpu.py::test_look_ahead_on_odd_texts that
make long rows, plus a pangenome of near-identical genomes.

  poly         12 pieces of A * randint(1, 6000) followed by 1 - 39 random bases: runs split at MAX_RUN_LENGTH in every
               layout (consecutive rows of the same character), offsets up to the 11 / 12 bits a row keeps;
  tandem       ACGTTGCA * 3000, 2000 random bases, GATTACA * 2000: every base of a repeat rides along for thousands of steps;
  pangenome    24 genomes of one 6 kbp random ancestor with 1 % substitutions each: n > 2^18 BWT positions, rows of a hundred
               characters and more, fast-forward chains;
  two_letters  30 000 random bases over AT: a reduced alphabet.

Everything is deterministic: odd_text(kind) and odd_reads(kind, text) give the same bytes on every call."""
import functools

import numpy as np

from oracle import build_index as B
from test_gpu_parity import mutated_reads

KINDS = ("poly", "tandem", "pangenome", "two_letters")
TANDEM_BLOCK = 8 * 3000                                   # where tandem's first repeat ends and its random block starts
# The seeds of the texts.  A sampled-ids table (modes 7 and 5) whose number of rows is a multiple of the checkpoint distance (20) is
# not a usable index: the reference's builder never fills checkpoint r / 20 there (src/move_structure_build.cpp:486-496, :588-593,
# :677-682), get_id reads it for the rows behind the last checkpoint and throws, and the oracle does as the reference does.  tandem's
# first candidate seed gave r = 3420 in mode 7, so it has another; tests/test_odd_texts_cpu.py::test_structure asserts the property.
SEEDS = {"poly": 20000, "tandem": 20101, "pangenome": 20002, "two_letters": 20003}

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def odd_text(kind):
    """The sequences `movi build` would index: one record, 24 for the pangenome."""
    rng = np.random.default_rng(SEEDS[kind])
    if kind == "poly":
        return [b"".join((b"A" * int(rng.integers(1, 6000))) + bytes(_ACGT[rng.integers(0, 4, int(rng.integers(1, 40)))])
                         for _ in range(12))]
    if kind == "tandem":
        return [(b"ACGTTGCA" * 3000) + bytes(_ACGT[rng.integers(0, 4, 2000)]) + (b"GATTACA" * 2000)]
    if kind == "pangenome":
        anc = _ACGT[rng.integers(0, 4, 6000)]
        out = []
        for _ in range(24):
            g = anc.copy()
            at = np.flatnonzero(rng.random(g.size) < 0.01)
            g[at] = _ACGT[rng.integers(0, 4, at.size)]
            out.append(bytes(g))
        return out
    if kind == "two_letters":
        return [bytes(np.frombuffer(b"AT", np.uint8)[rng.integers(0, 2, 30000)])]
    raise ValueError(kind)


def odd_reads(kind, text):
    """Reads over `text` (the records of odd_text(kind) joined): 300 mutated substrings of 1 - 299 bases (substitutions, N, lower
    case), then the fixed edge cases."""
    rng = np.random.default_rng(SEEDS[kind] + 1000)
    text = bytes(text)
    reads = mutated_reads(rng, text, 300, 1, 300) + [b"", text[:1], b"N" * 40, text[:3000]]
    if kind == "poly":
        reads.append(b"A" * 200)
    if kind == "tandem":
        reads.append(text[TANDEM_BLOCK - 60:TANDEM_BLOCK + 60])      # out of the ACGTTGCA repeat into the random block
    return reads


@functools.lru_cache(maxsize=None)
def table(kind, separators=False):
    """(BWT, thresholds, suffix array) of the text `movi build [--separators]` indexes for odd_text(kind); computed once per process."""
    t = B.clean_text(odd_text(kind), separators=separators)
    bwt, thr = B.bwt_and_thresholds(t)
    return bwt, thr, B.suffix_array(t)


@functools.lru_cache(maxsize=None)
def fields(kind, separators, mode):
    """(build_rows fields, index image) of that text in `mode`; shared by the tests, which leave both unchanged."""
    bwt, thr, _ = table(kind, separators)
    f = B.build_rows(bwt, thr, mode)
    return f, B.serialize(f)


@functools.lru_cache(maxsize=None)
def reads_of(kind):
    return tuple(odd_reads(kind, b"".join(odd_text(kind))))
