"""Reference answers for Movi Color in its default colour mode (include/movi_hip.h: movi_color_build, movi_multi_classify_device), from the
suffix array of the text, the fields oracle/build_index.py's build_rows derives and tests/sa_ref.py's restatement of query_pml's walk.

  * doc_offsets_of(seqs, ...): the ref.fa.doc_offsets of the reference's reference-preparation step (src/prepare_ref.cpp:33-77,
    :121-127, one FASTA, not a list): one document per record, its reverse complement and its separators included; cumulative ends.
  * species(doc_ids, n_docs): load_document_info (src/move_structure_io.cpp:659-687): the compressed id per document and to_taxon_id.
  * doc_of_bwt(SA, offsets, ids): build_doc_pats (src/move_structure_color.cpp:4-24): the document of every BWT position.
  * run_sets(f, docs): build_doc_sets (:27-55): the sorted set of every run.
  * flat_tables(sets): first-appearance numbering (:57-63) and flat_and_serialize_colors_vectors (src/move_structure_io.cpp:513-548):
    (flat_colors u16, flat offset per run); flat_file(flat, inds) is doc_sets_flat.bin, read_flat_file its reader (:587-607).
  * score(f, oracle, read, flat, inds, num_species, min_len): process_char's scoring (src/read_processor.cpp:122-186, :237) over
    sa_ref.walk's states, whose PMLs are asserted against the oracle's; the set scored at a base is that of the row the LF step
    lands on, before the base is compared and possibly repositions the walk.  Match lengths beyond 65535 are carried as they are.
  * mls_line(...): write_mls (src/read_processor.cpp:489-562) in float32 arithmetic."""
import struct

import numpy as np

import sa_ref

NONE = 0xFFFF
UNCLASSIFIED_THRESHOLD = 0.4          # include/utils.hpp:169


def doc_offsets_of(seqs, rc=True, separators=False):
    ends, at = [], 0
    for s in seqs:
        at += (2 * len(s) if rc else len(s)) + ((2 if rc else 1) if separators else 0)
        ends.append(at)
    return ends


def species(doc_ids, n_docs):
    raw = list(doc_ids) if doc_ids is not None else [i + 1 for i in range(n_docs)]
    assert len(raw) == n_docs
    to_taxon = sorted(set(raw))
    comp = {t: i for i, t in enumerate(to_taxon)}
    return [comp[x] for x in raw], to_taxon


def doc_of_bwt(SA, offsets, ids):
    """The literal rule: from text position n - 1 downwards, the document index drops by one when the position falls below the end of
    the document before."""
    SA = np.asarray(SA, np.int64)
    n = len(SA)
    of_text = np.zeros(n, np.int64)
    d = len(offsets) - 1
    for t in range(n - 1, -1, -1):
        if d > 0 and t < offsets[d - 1]:
            d -= 1
        of_text[t] = ids[d]
    return of_text[SA]


def run_sets(f, docs):
    all_p, lens = np.asarray(f["all_p"]), np.asarray(f["lens"])
    return [sorted(set(int(x) for x in docs[int(all_p[i]): int(all_p[i]) + int(lens[i])])) for i in range(f["r"])]


def flat_tables(sets):
    flat, where, inds = [], {}, []
    for s in sets:
        key = tuple(s)
        if key not in where:
            where[key] = len(flat)
            flat.append(len(s))
            flat.extend(s)
        inds.append(where[key])
    return np.array(flat, np.uint16), np.array(inds, np.uint64)


def flat_file(flat, inds):
    tally = b"".join(struct.pack("<IB", int(v) & 0xFFFFFFFF, int(v) >> 32) for v in inds)
    return struct.pack("<Q", len(flat)) + np.asarray(flat).astype("<u2").tobytes() + tally


def read_flat_file(raw, r):
    fs = struct.unpack_from("<Q", raw, 0)[0]
    flat = np.frombuffer(raw, "<u2", fs, 8)
    assert len(raw) == 8 + 2 * fs + 5 * r
    inds = [lo | (hi << 32) for lo, hi in struct.iter_unpack("<IB", raw[8 + 2 * fs:])]
    return flat, np.array(inds, np.uint64)


def tables(f, SA, offsets, doc_ids=None):
    """(flat, inds, num_species, to_taxon_id) of a text: everything movi_color_build derives."""
    ids, to_taxon = species(doc_ids, len(offsets))
    sets = run_sets(f, doc_of_bwt(SA, offsets, ids))
    assert all(sets)                                            # every run has a document
    flat, inds = flat_tables(sets)
    return flat, inds, len(to_taxon), to_taxon


def score_states(states, flat, inds, num_species, min_len, changes=None):
    """process_char over (the row the walk stands on after the LF step and BEFORE the base is compared -- the one whose set is scored --,
    -, the match length after the base, unclamped) per base: (best, second, colors_count, sum_ml mod 2^32, counters).  `changes`: a
    list that receives (base, member, old best, new best) whenever a document takes the lead from another one."""
    cnt = [0] * num_species
    best = second = NONE
    colors_count = total = 0
    ml = 0
    for k, (row, _, after) in enumerate(states):
        if ml >= min_len:
            colors_count += 1
            at = int(inds[row])
            if at < len(flat):
                for m, doc in enumerate(int(x) for x in flat[at + 1: at + 1 + int(flat[at])]):
                    cnt[doc] += 1
                    if doc != best:
                        if best == NONE or cnt[doc] > cnt[best]:
                            if changes is not None and best != NONE:
                                changes.append((k, m, best, doc))
                            second, best = best, doc
                        elif second == NONE or cnt[doc] > cnt[second]:
                            second = doc
        ml = after
        total += ml
    return best, second, colors_count, total & 0xFFFFFFFF, cnt


def score(f, oracle, read, flat, inds, num_species, min_len, codes=None, changes=None):
    # the match length is carried unclamped (process.match_len is a uint64_t): into the min_len test and into sum_matching_lengths,
    # a uint32_t that wraps (src/read_processor.cpp:123, :237); only the PML vector holds min(ml, 65535), and that is what is held
    # to the oracle's
    w = sa_ref.walk(f, read, codes, clamp=False)
    assert [min(x[2], 65535) for x in w] == [int(v) for v in oracle.pml(read)], read[:80]
    # the scored row is where the LF step from the state after the base before lands (the read's first base: the last row), not where
    # a reposition of this base then takes the walk
    scored = [(f["r"] - 1 if k == 0 else sa_ref._lf(f, w[k - 1][0], w[k - 1][1])[0], None, w[k][2]) for k in range(len(w))]
    return score_states(scored, flat, inds, num_species, min_len, changes)


def mls_line(rid, read_len, res, to_taxon, report_all=False, min_diff_frac=0.05, min_score_frac=0.0):
    """One line of the report, without its newline.  rid: bytes."""
    best, second, colors_count, total, cnt = res
    f32 = np.float32
    out = rid + b","
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = f32(total) / f32(read_len)                       # static_cast<float>(sum) / length: one float division
    # (0 / 0 is NaN and NaN < 0.4 is false: an empty read falls to the second test, which it fails with no best document)
    if float(mean) < UNCLASSIFIED_THRESHOLD or best == NONE:    # the float against the double 0.4
        return out + (b"0" if report_all else b"0,0")
    tx = lambda d: str(to_taxon[d]).encode()
    if report_all:
        msf, mdf = f32(min_score_frac), f32(min_diff_frac)
        if msf == 0:
            out += tx(best)
        n_out = 0
        bc = cnt[best]
        for i in range(len(cnt)):
            if msf == 0:
                if i != best and f32(bc - cnt[i]) < mdf * f32(bc):
                    out += b"," + tx(i)
            elif f32(cnt[i]) >= msf * f32(colors_count):
                out += b"," + tx(i)
                n_out += 1
        if msf != 0 and n_out == 0:
            out += b"0"
        return out
    if second == NONE:
        return out + tx(best) + b",0"
    if float(f32(cnt[best] - cnt[second])) < 0.05 * cnt[best]:  # float against a double product
        return out + tx(best) + b"," + tx(second)
    return out + tx(best) + b",0"
