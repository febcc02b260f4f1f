"""CPU suite: rlbwt_check (movi_amd/csrc/movi_build.hpp) at its limits -- texts of 2^40 - 1 and 2^40 characters, lengths whose sum wraps
64 bits, thresholds of n and n + 1 past 2^32, a symbol counted past 2^32 -- through tests/host/rlbwt_check_driver.cpp, compiled with
-fsanitize=address,undefined; and the 2^40 refusal once through the C-ABI, where it comes before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rlbwtcheck") / "rlbwt_check_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "rlbwt_check_driver.cpp")])
    return exe


def ask(driver, heads, lens, thr=None):
    rows = "".join("%d %d %d\n" % (h, l, 0 if thr is None else thr[k]) for k, (h, l) in enumerate(zip(heads, lens)))
    out = subprocess.run([driver], input=("%d %d\n" % (len(heads), thr is not None) + rows).encode(), capture_output=True, check=True).stdout.decode()
    return out.rstrip("\n")


A, CC, G, T = b"ACGT"
HEADS = [A, CC, 0, G, T]


def test_text_of_2_40_minus_1(driver):
    lens = [1 << 39, (1 << 39) - 8, 1, 5, 1]
    assert sum(lens) == (1 << 40) - 1
    assert ask(driver, HEADS, lens) == "ok %d 4 0 2 65 %d 67 %d 71 5 84 1" % ((1 << 40) - 1, 1 << 39, (1 << 39) - 8)
    # with thresholds up to n itself
    n = (1 << 40) - 1
    assert ask(driver, HEADS, lens, [0, n, n - 1, 1 << 32, (1 << 39) + 1]).startswith("ok %d " % n)


def test_text_of_2_40(driver):
    lens = [1 << 39, (1 << 39) - 8, 1, 5, 2]
    assert sum(lens) == 1 << 40
    assert ask(driver, HEADS, lens) == "refused lens the lengths add up to 2^40 characters or more at run 4"
    assert ask(driver, HEADS, [1 << 39, (1 << 39) - 1, 1, 5, 2]) == "refused lens the lengths add up to 2^40 characters or more at run 2"


def test_one_length_of_2_40(driver):
    assert ask(driver, HEADS, [3, 1 << 40, 1, 5, 2]) == "refused lens the lengths add up to 2^40 characters or more at run 1"
    assert ask(driver, [A, 0], [1 << 40, 1]) == "refused lens the lengths add up to 2^40 characters or more at run 0"


def test_lengths_whose_sum_wraps(driver):
    """2^63 + 2^63 = 0 in 64 bits: a check of the sum alone would let the table through with n = 7."""
    assert ask(driver, HEADS, [1 << 63, 1 << 63, 1, 5, 1]) == "refused lens the lengths add up to 2^40 characters or more at run 0"
    assert ask(driver, HEADS, [3, (1 << 64) - 3, 1, 5, 1]) == "refused lens the lengths add up to 2^40 characters or more at run 1"
    assert ask(driver, HEADS, [(1 << 40) - 1, (1 << 64) - (1 << 40) + 1, 1, 5, 1]) == "refused lens the lengths add up to 2^40 characters or more at run 1"


def test_thresholds_of_n_and_n_plus_1(driver):
    lens = [(1 << 32) + 9, 4, 1, 5, 3]
    n = sum(lens)
    assert n == (1 << 32) + 22
    assert ask(driver, HEADS, lens, [0, n, 1 << 32, n - 1, n]) == "ok %d 4 0 2 65 %d 67 4 71 5 84 3" % (n, (1 << 32) + 9)
    assert ask(driver, HEADS, lens, [0, n, 1 << 32, n + 1, n]) == \
        "refused thr threshold 3 is 4294967319, greater than the text's length 4294967318"
    assert ask(driver, HEADS, lens, [0, n, 1 << 32, n, (1 << 64) - 1]) == \
        "refused thr threshold 4 is 18446744073709551615, greater than the text's length 4294967318"
    # a threshold equal to n modulo 2^32, and one equal to n modulo 2^40
    assert ask(driver, HEADS, lens, [22, n, 0, 0, 0]).startswith("ok ")
    assert ask(driver, HEADS, lens, [n + (1 << 40), 0, 0, 0, 0]).startswith("refused thr threshold 0 is %d," % (n + (1 << 40)))


def test_counts_past_2_32(driver):
    """One symbol's count past 2^32 from runs that are each shorter than 2^32, with '%' in front."""
    heads = [37, G, 0, T, G, A, G, CC, G]
    lens = [2, (1 << 31) + 5, 1, 7, (1 << 31) - 1, 3, 1 << 31, 11, 100]
    g = (1 << 31) + 5 + (1 << 31) - 1 + (1 << 31) + 100
    assert g > 1 << 32
    assert ask(driver, heads, lens) == "ok %d 5 1 2 37 2 65 3 67 11 71 %d 84 7" % (sum(lens), g)


def test_2_40_through_the_abi(built_lib):
    """MOVI_ERR_ARG from the host check, whatever the machine holds: no device call has been made when it is refused."""
    from movi_amd._lib import lib
    L = lib()
    heads = np.frombuffer(bytes(HEADS), np.uint8).copy()
    lens = np.array([1 << 39, (1 << 39) - 8, 1, 5, 2], np.uint64)
    thr = np.zeros(5, np.uint64)
    img, nbytes = C.c_void_p(1), C.c_size_t(1)
    rc = L.movi_build_from_rlbwt(0, 6, heads.ctypes.data, lens.ctypes.data, thr.ctypes.data, heads.size, C.byref(img), C.byref(nbytes))
    assert (rc, img.value, nbytes.value) == (-1, None, 0)
    assert L.movi_last_error() == b"h_lens: the lengths add up to 2^40 characters or more at run 4"
