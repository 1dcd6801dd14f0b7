"""Locate without a GPU: the "locate_sample" key, argument errors before any device is touched, the new symbols, and the
text-offset rule (n - 1 - SA - m) on hand-worked examples."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from findex_amd import _lib
from findex_amd.searcher import HipFMSearcher

LOCATE_SYMBOLS = ["fmx_locate_batch", "fmx_locate_batch_dev", "fmx_locate_intervals", "fmx_locate_intervals_dev",
                  "fmx_locate_info", "fmx_write_sa"]


def test_locate_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in LOCATE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"FMX_PREPARE_LOCATE\s*=\s*32\b", code)


def test_locate_sample_takes_its_values_and_refuses_others():
    L = _lib.load()
    try:
        for v in (b"1", b"3", b"32", b"4096"):
            assert L.fmx_config_set(b"locate_sample", v) == 0, v
        for v in (b"0", b"4097", b"-1", b"abc", b"", b"3.5", b"32x", b"auto"):
            assert L.fmx_config_set(b"locate_sample", v) == 3, v
            assert b"locate_sample" in L.fmx_last_error()
        assert L.fmx_index_config_set(None, b"locate_sample", b"32") == 3
    finally:
        assert L.fmx_config_set(b"locate_sample", b"32") == 0


def test_argument_errors_are_statuses_with_messages():
    L = _lib.load()
    rows = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    out = (ctypes.c_uint64 * 4)()
    off = (ctypes.c_uint64 * 5)()
    rate, nbytes, ms = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
    assert L.fmx_locate_batch(None, rows, 4, out) == 3
    assert b"null" in L.fmx_last_error()
    assert L.fmx_locate_batch_dev(None, rows, 4, out, None) == 3
    assert L.fmx_locate_intervals(None, rows, rows, 4, 0, off, out, 4) == 3
    assert L.fmx_locate_intervals_dev(None, rows, rows, 4, 0, off, out, 4, None) == 3
    assert L.fmx_locate_info(None, ctypes.byref(rate), ctypes.byref(nbytes), ctypes.byref(ms)) == 3
    assert L.fmx_write_sa(None, b"/nonexistent/dir/x.sa") == 3
    assert b"null" in L.fmx_last_error()
    assert L.fmx_write_sa(None, None) == 3
    assert L.fmx_prepare(None, 32) == 3
    assert L.fmx_drop_tables(None, 32) == 3
    assert L.fmx_prepare(None, 64) == 3


def _naive_rows_and_sa(text, q):
    """SA of s = reverse(text) + sentinel by sorting, and the rows whose suffix starts with reverse(q)."""
    s = bytes(text[::-1]) + b"\0"
    sa = sorted(range(len(s)), key=lambda i: s[i:])
    rq = q[::-1]
    rows = [r for r, p in enumerate(sa) if s[p:p + len(rq)] == rq]
    return len(s), [sa[r] for r in rows]


def _occurrences(text, q):
    out, i = [], text.find(q)
    while i >= 0:
        out.append(i)
        i = text.find(q, i + 1)
    return out


def test_text_offset_rule_by_hand():
    # text "abab": s = "baba" + sentinel, n = 5.  Suffixes of s that start with reverse("ab") = "ba": positions 0, 2
    # -> text offsets n - 1 - SA - m = 4 - 0 - 2 = 2 and 4 - 2 - 2 = 0: "ab" is at 0 and 2.
    n, sa = _naive_rows_and_sa(b"abab", b"ab")
    assert n == 5 and sorted(sa) == [0, 2]
    assert sorted(HipFMSearcher.text_offsets(np.array(sa, dtype=np.uint64), n, 2).tolist()) == [0, 2]


@pytest.mark.parametrize("text", [b"abracadabra", b"mississippi", b"aaaaaaa", b"the cat sat on the mat"])
def test_text_offset_rule_against_a_scan(text):
    for m in range(1, 5):
        for i in range(len(text) - m + 1):
            q = text[i:i + m]
            n, sa = _naive_rows_and_sa(text, q)
            got = sorted(HipFMSearcher.text_offsets(np.array(sa, dtype=np.uint64), n, m).tolist())
            assert got == _occurrences(text, q), (text, q)
