"""The LCP array without a GPU: the new symbols, argument errors before any device is touched, the checker the GPU tests
rest on (hand-worked arrays, a brute-force compare on random short strings, the X.lcp file rule), and the CLI's flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from findex_amd import _lib
import lcp_checker

LCP_SYMBOLS = ["fmx_lcp_from_text_dev", "fmx_lcp_from_text", "fmx_lcp_batch", "fmx_lcp_batch_dev", "fmx_lcp_range",
               "fmx_lcp_range_dev", "fmx_lcp_info", "fmx_write_lcp"]


def test_lcp_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in LCP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"FMX_PREPARE_LCP\s*=\s*64\b", code)
    assert _lib.load().fmx_abi_version() == 5


def test_argument_errors_are_statuses_with_messages():
    L = _lib.load()
    rows = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    out = (ctypes.c_uint32 * 8)()
    text = (ctypes.c_uint8 * 4)(97, 98, 99, 100)
    nbytes, ms, mx, row, total = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    calls = [
        lambda: L.fmx_lcp_batch(None, rows, 4, out),
        lambda: L.fmx_lcp_batch_dev(None, rows, 4, out, None),
        lambda: L.fmx_lcp_range(None, 0, 4, out),
        lambda: L.fmx_lcp_range_dev(None, 0, 4, out, None),
        lambda: L.fmx_lcp_info(None, ctypes.byref(nbytes), ctypes.byref(ms), ctypes.byref(mx), ctypes.byref(row), ctypes.byref(total)),
        lambda: L.fmx_write_lcp(None, b"/nonexistent/dir/x.lcp"),
        lambda: L.fmx_write_lcp(None, None),
        lambda: L.fmx_lcp_from_text(None, 4, out, 0),
        lambda: L.fmx_lcp_from_text(text, 4, None, 0),
        lambda: L.fmx_lcp_from_text_dev(None, 4, rows, out, 0, None),
        lambda: L.fmx_lcp_from_text_dev(text, 4, None, out, 0, None),
        lambda: L.fmx_lcp_from_text_dev(text, 4, rows, None, 0, None),
    ]
    for i, call in enumerate(calls):
        assert call() == 3, i
        assert b"null" in L.fmx_last_error(), i
    assert L.fmx_prepare(None, 64) == 3 and b"null" in L.fmx_last_error()
    assert L.fmx_drop_tables(None, 64) == 3 and b"null" in L.fmx_last_error()
    # values, not pointers
    assert L.fmx_lcp_from_text(text, 0, out, 0) == 3                          # len == 0
    assert L.fmx_lcp_from_text(text, (1 << 32) - 1, out, 0) == 6              # more than 2^32 - 2 bytes
    zero = (ctypes.c_uint8 * 4)(97, 0, 99, 100)
    assert L.fmx_lcp_from_text(zero, 4, out, 0) == 6 and b"byte 0" in L.fmx_last_error()


def test_a_valid_call_without_a_device_is_err_hip():
    L = _lib.load()
    n = ctypes.c_int(-1)
    assert L.fmx_device_count(ctypes.byref(n)) == 0
    if n.value > 0:
        return                                   # (a machine with a device: the GPU tests say what a valid call gives)
    text = (ctypes.c_uint8 * 4)(97, 98, 99, 100)
    out = (ctypes.c_uint32 * 5)()
    sa = (ctypes.c_uint32 * 5)()
    assert L.fmx_lcp_from_text(text, 4, out, 0) == 5
    assert b"no HIP device" in L.fmx_last_error()
    assert L.fmx_lcp_from_text_dev(text, 4, sa, out, 0, None) == 5


# s, SA and LCP written out: row r pairs with row r + 1; the last entry is 0
HAND = {
    # s = "arbadacarba" + sentinel; rows: "", a, acarba, adacarba, arba, arbadacarba, ba, badacarba, carba, dacarba, rba, rbadacarba
    b"abracadabra": ([11, 10, 5, 3, 7, 0, 9, 2, 6, 4, 8, 1], [0, 1, 1, 1, 4, 0, 2, 0, 0, 0, 3, 0]),
    # s = "ippississim" + sentinel; rows: "", im, ippississim, issim, ississim, m, pississim, ppississim, sim, sissim, ssim, ssissim
    b"mississippi": ([11, 9, 0, 6, 3, 10, 2, 1, 8, 5, 7, 4], [0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3, 0]),
    # s = "aaaa" + sentinel; rows: "", a, aa, aaa, aaaa
    b"aaaa": ([4, 3, 2, 1, 0], [0, 1, 2, 3, 0]),
}


@pytest.mark.parametrize("text", sorted(HAND))
def test_checker_on_hand_worked_strings(text):
    sa, lcp = HAND[text]
    s = lcp_checker.s_of_text(text)
    assert lcp_checker.sorted_sa(s).tolist() == sa
    assert lcp_checker.kasai(s, sa).tolist() == lcp
    assert lcp_checker.brute(s, sa).tolist() == lcp
    assert lcp[0] == 0 and lcp[-1] == 0


def test_checker_against_brute_force_on_random_strings():
    rng = np.random.default_rng(31)
    for i in range(400):
        n = int(rng.integers(1, 60))
        sigma = int(rng.integers(1, 5)) if i % 2 else 255
        text = bytes(rng.integers(1, sigma + 1, n, dtype=np.uint8))
        s = lcp_checker.s_of_text(text)
        sa = lcp_checker.sorted_sa(s)
        want = lcp_checker.brute(s, sa)
        assert np.array_equal(lcp_checker.kasai(s, sa), want), text
        assert want[0] == 0 and want[-1] == 0


def test_file_rule():
    sa, lcp = HAND[b"abracadabra"]
    data = lcp_checker.lcp_file_bytes(np.array(lcp, dtype=np.uint32))
    assert len(data) == 4 * (len(lcp) - 1)                       # n - 1 entries: LCPCreator never writes slot n - 1
    assert data[:8] == b"\0\0\0\0\0\0\0\1" and data[16:20] == b"\0\0\0\4"
    assert np.frombuffer(data, dtype=">u4").tolist() == lcp[:-1]


def test_cli_flags():
    from findex_amd import index
    a = index.parser().parse_args(["dir/X.txt"])
    assert not (a.fm or a.sa or a.lcp)
    assert index.planned_outputs(a) == ["dir/X.bwt", "dir/X.aux"]
    a = index.parser().parse_args(["dir/X.txt", "--fm", "--sa", "--lcp"])
    assert a.fm and a.sa and a.lcp
    assert index.planned_outputs(a) == ["dir/X.bwt", "dir/X.aux", "dir/X.fm", "dir/X.sa", "dir/X.lcp"]
    a = index.parser().parse_args(["dir/X.txt", "--lcp", "--little-endian"])
    assert index.planned_outputs(a) == ["dir/X.bwt", "dir/X.aux", "dir/X.lcp"]
    assert index.output_names("dir/X.txt") == ("dir/X.bwt", "dir/X.aux")
