"""Reference answers for locate (include/movi_hip.h: movi_ssa_build, movi_locate_device, movi_sa_entries_device), from the suffix array
of the text and the fields oracle/build_index.py's build_rows derives.

  * entry(SA, rate, p): what MoveStructure::get_SA_entries returns for BWT position p.  An LF step lowers the text position by one and
    text position 0 is followed by BWT position 0, which is always sampled and holds n - 1; the reference does not reduce modulo n.  So
    with m = min(SA[0::rate]) -- the first sampled text position at or below which every walk from a lower one must wrap -- the answer
    is SA[p] for SA[p] >= m and SA[p] + n below.
  * ssa_bytes(f, SA, rate): the bytes of ssa.movi (serialize_sampled_SA, src/move_structure_io.cpp:710-722).
  * lf_walk_entry / lf_walk_samples: the literal walks of get_SA_entries and find_sampled_SA_entries, for the CPU test of the two above.
  * walk(f, read): query_pml's state per base (src/move_structure_query.cpp:266-361, reposition_thresholds :513-601) over the
    build_rows fields: (row, offset, PML) after process_char and before the LF step, in emission order.  positions() asserts its PMLs
    against Oracle.pml for every read it is used on."""
import struct

import numpy as np

from oracle import build_index as B


def text_fields(seqs, mode, separators=False, rc=True):
    """(build_rows fields, SA) of the text `movi build` indexes."""
    t = B.clean_text(seqs, rc=rc, separators=separators)
    bwt, thr = B.bwt_and_thresholds(t)
    return B.build_rows(bwt, thr, mode), B.suffix_array(t)


def entries(SA, rate):
    """Expected get_SA_entries of every BWT position, as uint64."""
    SA = np.asarray(SA, np.int64)
    n = len(SA)
    m = int(SA[0::rate].min())
    return (SA + np.where(SA < m, n, 0)).astype(np.uint64)


def samples(SA, rate):
    """The n // rate + 1 entries find_sampled_SA_entries fills: SA[0::rate], one unaddressed zero more where rate divides n."""
    n = len(SA)
    out = np.zeros(n // rate + 1, np.uint64)
    s = np.asarray(SA, np.int64)[0::rate]
    out[:len(s)] = s
    return out


def ssa_bytes(f, SA, rate):
    s = samples(SA, rate)
    return (struct.pack("<QQ", rate, len(s)) + s.astype("<u8").tobytes() + struct.pack("<Q", f["r"]) +
            np.asarray(f["all_p"]).astype("<u8").tobytes())


def all_positions(f):
    """(rows, offsets) of the BWT positions 0 .. n - 1."""
    rows = np.repeat(np.arange(f["r"]), f["lens"])
    return rows, np.arange(f["n"]) - np.asarray(f["all_p"])[rows]


def _lf(f, idx, off):
    """LF_move + fast_forward, src/move_structure.cpp:59-87."""
    off += int(f["offset"][idx])
    idx = int(f["pp_id"][idx])
    while idx < f["r"] - 1 and off >= f["lens"][idx]:
        off -= int(f["lens"][idx])
        idx += 1
    return idx, off


def lf_walk_entry(f, sampled, rate, idx, off):
    """get_SA_entries, src/move_structure.cpp:35-48, literally."""
    dist = 0
    while (int(f["all_p"][idx]) + off) % rate:
        idx, off = _lf(f, idx, off)
        dist += 1
    return int(sampled[(int(f["all_p"][idx]) + off) // rate]) + dist


def lf_walk_samples(f, rate):
    """find_sampled_SA_entries, src/move_structure_build.cpp:1191-1210, literally."""
    n = f["n"]
    out = np.zeros(n // rate + 1, np.uint64)
    idx = off = 0
    val = n
    for _ in range(n):
        val -= 1
        p = int(f["all_p"][idx]) + off
        if p % rate == 0:
            out[p // rate] = val
        idx, off = _lf(f, idx, off)
    return out


def code_table(f):
    """ASCII -> alphamap code, 0xFF = illegal in a read (not in the alphabet, or the separator)."""
    t = [0xFF] * 256
    for i, ch in enumerate(f["alphabet"]):
        if ch != B.SEPARATOR:
            t[ch] = i
    return t


def walk(f, read, codes=None, clamp=True):
    """[(row, offset, PML)] per base of `read`, last base first.  clamp=False: the match length itself (process.match_len, a
    uint64_t in the reference) in place of the u16 the PML vector holds -- what color_ref.score adds up and tests against min_len."""
    codes = codes or code_table(f)
    r, sep, end = f["r"], f["sep"], f["end_bwt_idx"]
    code, lens, thr_bits = f["code"], f["lens"], f["thr_bits"]
    idx, off, ml = r - 1, int(lens[r - 1]) - 1, 0          # ReadProcessor::reset_process
    out = []
    for k, ch in enumerate(reversed(read)):
        if k:
            idx, off = _lf(f, idx, off)
        a = codes[ch]
        c = int(code[idx])
        if a == 0xFF:
            ml = 0
        elif c == a:                                       # (the '$' row decodes as code 0)
            ml += 1
        else:
            ml = 0
            if idx == end:
                down = off >= f["end_thr"][a - sep]
            elif sep and c == 0:
                e = f["sep_map"].get(idx)
                down = off >= (f["sep_thr"][e][a - 1] if e is not None else 0)
            else:
                down = off >= (int(lens[idx]) if thr_bits[idx, B.ALPHAMAP_3[c - sep][a - sep]] else 0)
            step = 1 if down else -1
            idx += step
            while int(code[idx]) != a:
                idx += step
                assert 0 <= idx < r, "no run of the base in that direction"
            off = 0 if down else int(lens[idx]) - 1
        out.append((idx, off, min(ml, 65535) if clamp else ml))
    return out


def positions(f, oracle, reads):
    """Per read (rows, offsets) as int64 arrays, emission order; the restatement's PMLs are held to the oracle's."""
    codes = code_table(f)
    out = []
    for rd in reads:
        w = walk(f, rd, codes)
        assert [x[2] for x in w] == [int(v) for v in oracle.pml(rd)], rd
        out.append((np.array([x[0] for x in w], np.int64), np.array([x[1] for x in w], np.int64)))
    return out


def read_entries(f, oracle, SA, rate, reads):
    """Expected `movi query --sa-entries` per read: uint64 arrays, emission order."""
    ent = entries(SA, rate)
    all_p = np.asarray(f["all_p"])
    return [ent[all_p[rows] + offs] if len(rows) else np.zeros(0, np.uint64) for rows, offs in positions(f, oracle, reads)]


def sa_entries_file(ids, per_read):
    """<prefix>.sa_entries.bpf: per read u16 id length, id, u64 count, count x u64 (no header)."""
    return b"".join(struct.pack("<H", len(i)) + i + struct.pack("<Q", len(e)) + np.asarray(e).astype("<u8").tobytes()
                    for i, e in zip(ids, per_read))
