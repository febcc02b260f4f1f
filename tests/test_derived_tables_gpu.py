"""GPU suite (-m gpu): which derived tables a handle holds after scripts of queries, movi_index_prepare and the build-now options, through
the public API alone -- the check that the HIP side of movi_abi.hip feeds and obeys the rules of movi_amd/csrc/movi_derived.hpp as the
code they came from did.  Every expected value is a literal written from that code's behaviour (the test passes unchanged against the
library of the commit before the header existed).  Nothing here starves the device of memory or makes a build fail: those branches
are tests/test_derived_cpu.py's.  Tables: the golden mode-6 index (real text: 0.83 of its positions reach their LF target without a
fast-forward), a uniformly random run sequence of 300 000 rows (0.51), and a `regular` index without thresholds."""
import numpy as np
import pytest

from test_gpu_parity import pack
from test_top_of_walk_gpu import _ref

pytestmark = pytest.mark.gpu

KEYS = ("kmer_bytes", "ftab_bytes", "ahead_rows_bytes", "deep_rows_bytes", "ckpt_bytes")


def held(gpu):
    """The derived tables the handle reports, by the first word of their info key."""
    return {k.split("_")[0] for k in KEYS if gpu.info(k) > 0}


@pytest.fixture(scope="module")
def tables(built_lib, golden_image):
    """name -> (image, 70 reads of 160 bases and the oracle's PML answer, one 1000-base read and the oracle's count): computed once."""
    from oracle import build_index as B
    from oracle.oracle import Oracle
    from tools import synth
    ref = _ref()
    six = synth.synth_index(300_000, mode=6, seed=4)
    rb, ro = synth.synth_reads(six, 70, 160, seed=5)
    lb, lo = synth.synth_reads(six, 1, 1000, seed=6)
    batches = {"golden": (golden_image(6), pack([ref[1000 * i: 1000 * i + 160] for i in range(70)]), pack([ref[:1000]])),
               "random": (six.image(), (rb, ro), (lb, lo)),
               "regular": (B.build_index_from_seqs([ref], 3), pack([ref[1000 * i: 1000 * i + 160] for i in range(70)]), pack([ref[:1000]]))}
    out = {}
    for name, (img, (bases, offs), (cb, co)) in batches.items():
        cpu = Oracle(img)
        pml = cpu.pml_batch(bases, offs, threads=4) if name != "regular" else None
        out[name] = (img, bases, offs, pml, cb, co, cpu.count_batch(cb, co))
        cpu.close()
    return out


def open_table(tables, name):
    import movi_amd
    return movi_amd.MoveIndex.from_image(tables[name][0])


def pml(gpu, tables, name, ahead):
    """A PML query on the table's batch: the oracle's vector, fast-forwards and scans, on the rows the script expects."""
    _, bases, offs, (exp, ff, sc), _, _, _ = tables[name]
    out, st = gpu.query_pml_packed(bases, offs)
    assert gpu.last_launch()["ahead"] == ahead
    assert (out == exp).all() and (st.fast_forwards, st.scans, st.errors) == (ff, sc, 0)


def count(gpu, tables, name, ahead):
    _, _, _, _, cb, co, (em, ec) = tables[name]
    m, c, _ = gpu.query_count_packed(cb, co)
    assert gpu.last_launch()["ahead"] == ahead
    assert (m == em).all() and (c == ec).all()


def test_first_pml_query(tables):
    gpu = open_table(tables, "golden")                               # real text: the walk of short reads runs on the deep rows
    assert held(gpu) == set() and gpu.info("deep_hint_bits") == 0
    pml(gpu, tables, "golden", 2)
    assert held(gpu) == {"kmer", "ahead", "deep"} and gpu.info("deep_hint_bits") == 4 and gpu.info("kmer_bytes") == 16 << 24
    count(gpu, tables, "golden", 0)
    assert held(gpu) == {"kmer", "ahead", "deep", "ftab", "ckpt"}
    gpu.close()
    gpu = open_table(tables, "random")                               # a random run sequence: the look-ahead rows only
    pml(gpu, tables, "random", 1)
    assert held(gpu) == {"kmer", "ahead"} and gpu.info("deep_hint_bits") == 0 and 0 < gpu.info("ahead_no_ff") < 0.67
    count(gpu, tables, "random", 0)
    gpu.close()


def test_prepared_for_count_then_a_pml_query(tables):
    gpu = open_table(tables, "golden")
    gpu.prepare(gpu.PREPARE_COUNT)
    assert held(gpu) == {"ftab", "ckpt"}
    pml(gpu, tables, "golden", 0)                                    # the top-of-walk table is built by the query, neither row copy is
    assert held(gpu) == {"kmer", "ftab", "ckpt"} and gpu.info("deep_hint_bits") == 0
    count(gpu, tables, "golden", 0)
    gpu.close()


def test_count_variant_0_on_a_random_table_keeps_no_copy(tables):
    gpu = open_table(tables, "random")
    gpu.set_option("count_variant", 0)
    count(gpu, tables, "random", 0)
    assert held(gpu) == {"ftab", "ckpt"} and 0 < gpu.info("ahead_no_ff") < 0.67
    pml(gpu, tables, "random", 1)                                    # ... and the first PML query builds it
    assert held(gpu) == {"kmer", "ftab", "ahead", "ckpt"} and gpu.info("deep_hint_bits") == 0
    count(gpu, tables, "random", 0)                                  # (built by itself on a random table: not the count query's)
    gpu.close()


def test_count_variant_0_on_real_text_keeps_the_copy(tables):
    gpu = open_table(tables, "golden")
    gpu.set_option("count_variant", 0)
    count(gpu, tables, "golden", 1)
    assert held(gpu) == {"ftab", "ahead", "ckpt"} and gpu.info("ahead_no_ff") >= 0.67 and gpu.info("deep_hint_bits") == 0
    pml(gpu, tables, "golden", 2)
    assert held(gpu) == {"kmer", "ftab", "ahead", "deep", "ckpt"}
    gpu.close()


def test_ahead_rows_0_then_deep_rows_1(tables):
    gpu = open_table(tables, "golden")
    gpu.set_option("ahead_rows", 0)
    pml(gpu, tables, "golden", 0)
    assert held(gpu) == {"kmer"} and gpu.info("deep_hint_bits") == 0
    gpu.set_option("deep_rows", 1)
    assert held(gpu) == {"kmer", "deep"} and gpu.info("deep_hint_bits") == 4
    pml(gpu, tables, "golden", 2)
    assert held(gpu) == {"kmer", "deep"} and gpu.info("ahead_rows_bytes") == 0
    count(gpu, tables, "golden", 0)
    gpu.close()


def test_kmer_k_0_then_prepare(tables):
    gpu = open_table(tables, "golden")
    gpu.set_option("kmer_k", 0)
    gpu.prepare(gpu.PREPARE_PML)
    assert held(gpu) == {"ahead", "deep"} and gpu.info("kmer_bytes") == 0 and gpu.info("deep_hint_bits") == 4
    pml(gpu, tables, "golden", 2)
    assert held(gpu) == {"ahead", "deep"}
    count(gpu, tables, "golden", 0)
    assert held(gpu) == {"ahead", "deep", "ftab", "ckpt"}
    gpu.close()


def test_deep_hint_bits_take_effect_at_the_next_build(tables):
    gpu = open_table(tables, "golden")
    gpu.set_option("deep_hint_bits", 2)
    assert held(gpu) == set() and gpu.info("deep_hint_bits") == 0
    gpu.set_option("deep_rows", 1)
    assert held(gpu) == {"deep"} and gpu.info("deep_hint_bits") == 2
    gpu.set_option("deep_hint_bits", -1)
    assert gpu.info("deep_hint_bits") == 2
    gpu.set_option("deep_rows", 1)
    assert held(gpu) == {"deep"} and gpu.info("deep_hint_bits") == 4
    pml(gpu, tables, "golden", 2)
    assert held(gpu) == {"kmer", "ahead", "deep"}                    # ("deep_rows" says nothing about the look-ahead rows: built as ever)
    count(gpu, tables, "golden", 0)
    gpu.close()


def test_a_regular_index_gets_the_interval_table_alone(tables):
    gpu = open_table(tables, "regular")
    _, bases, offs, _, _, _, _ = tables["regular"]
    _, _, _, rc = gpu.query_pml_packed(bases, offs, want_err=True)
    assert rc != 0 and held(gpu) == set()                            # PML needs thresholds: refused, nothing built
    count(gpu, tables, "regular", 0)
    assert held(gpu) == {"ftab", "ckpt"} and gpu.info("deep_hint_bits") == 0
    gpu.close()
