"""Repeats without a device: the two yardsticks of tests/repeats_ref.py agree with each other and with cases worked out by
hand, the library refuses every bad argument before it touches a device, the structs have the header's sizes, and the
command line takes --dups."""
import ctypes

import numpy as np
import pytest

import repeats_ref
from findex_amd import _lib, index


def both(text, L, later=False, stop=0):
    r1, s1 = repeats_ref.brute(text, L, later, stop)
    r2, s2 = repeats_ref.hashed(text, L, later, stop)
    assert r1.dtype == r2.dtype == np.uint64 and r1.shape == r2.shape and np.array_equal(r1, r2), (text, L, later, stop)
    assert s1 == s2, (text, L, later, stop, s1, s2)
    assert tuple(s1) == repeats_ref.FIELDS
    return [tuple(int(x) for x in r) for r in r1], s1


def summary(ranges, covered, classes, windows, largest, pos):
    return dict(zip(repeats_ref.FIELDS, (ranges, covered, classes, windows, largest, pos)))


def test_hand_written_cases():
    # aaaa at L = 2: one class of three overlapping windows
    assert both(b"aaaa", 2) == ([(0, 4)], summary(1, 4, 1, 3, 3, 0))
    assert both(b"aaaa", 2, later=True) == ([(1, 4)], summary(1, 3, 1, 2, 3, 0))
    # two copies of "abc" exactly L = 3 apart: the two windows abut and are one range
    assert both(b"abcabc", 3) == ([(0, 6)], summary(1, 6, 1, 2, 2, 0))
    assert both(b"abcabc", 3, later=True) == ([(3, 6)], summary(1, 3, 1, 1, 2, 0))
    # L + 1 apart: two ranges
    assert both(b"abcxabc", 3) == ([(0, 3), (4, 7)], summary(2, 6, 1, 2, 2, 0))
    assert both(b"abcxabc", 3, later=True) == ([(4, 7)], summary(1, 3, 1, 1, 2, 0))
    # a stop byte inside the only repeat: nothing is left at L = 3; at L = 1 the letters around it repeat, it never does
    assert both(b"a|bxa|b", 3, stop=ord("|")) == ([], summary(0, 0, 0, 0, 0, 0))
    assert both(b"a|bxa|b", 3) == ([(0, 3), (4, 7)], summary(2, 6, 1, 2, 2, 0))
    assert both(b"a|bxa|b", 1, stop=ord("|")) == ([(0, 1), (2, 3), (4, 5), (6, 7)], summary(4, 4, 2, 4, 2, 0))
    # L > m, L == m
    assert both(b"abc", 4) == ([], summary(0, 0, 0, 0, 0, 0))
    assert both(b"abc", 3) == ([], summary(0, 0, 0, 0, 0, 0))
    # the largest class: among classes of one size the one whose first window comes first
    assert both(b"xyxy-abab", 2)[1] == summary(2, 8, 2, 4, 2, 0)
    assert both(b"ab-xyxyxy", 2)[1] == summary(1, 6, 2, 5, 3, 3)


def test_the_yardsticks_agree_on_random_texts():
    rng = np.random.default_rng(18)
    for _ in range(400):
        sigma = int(rng.integers(1, 4))
        m = int(rng.integers(1, 60))
        text = bytes(rng.integers(1, sigma + 1, m, dtype=np.uint8) + 96)
        for L in (1, 2, 3, 5, 9, 17):
            for later in (False, True):
                both(text, L, later, 0)
                both(text, L, later, 97)


def test_the_yardsticks_agree_beyond_eight_bytes():
    rng = np.random.default_rng(19)
    base = bytes(rng.integers(1, 4, 300, dtype=np.uint8) + 96)
    text = base[:70] + b"q" + base[10:70] + b"r" + base[100:140] + base[100:140]
    for L in (8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 59, 60, 61):
        for later in (False, True):
            both(text, L, later, 0)
            both(text, L, later, ord("q"))


# ---- the library's refusals, before any device is touched
def call(L, idx=1, min_len=(4,), k=None, opts=None, out_off=True, out=None, cap=0, n_out=True, dev=False):
    lv = (ctypes.c_uint32 * max(len(min_len), 1))(*min_len) if min_len is not None else None
    off = (ctypes.c_uint64 * 66)() if out_off else None
    n = ctypes.c_size_t() if n_out else None
    handle = ctypes.c_void_p(idx) if idx else None             # never dereferenced: every case here is refused first
    args = [handle, lv, len(min_len) if k is None else k, ctypes.byref(opts) if opts is not None else None, off, out, cap,
            ctypes.byref(n) if n_out else None, None]
    rc = (L.fmx_repeats_dev(*args, None) if dev else L.fmx_repeats(*args))
    return rc, (L.fmx_last_error() or b"").decode()


@pytest.mark.parametrize("dev", [False, True])
def test_bad_arguments_are_refused_without_a_device(dev):
    L = _lib.load()
    bad = [
        dict(idx=0),
        dict(min_len=None, k=1),
        dict(out_off=False),
        dict(n_out=False),
        dict(min_len=(), k=0),
        dict(min_len=(3,) * 65),
        dict(min_len=(3, 0, 5)),
        dict(opts=_lib.fmx_repeat_opts(2, 0, (0, 0, 0))),
        dict(opts=_lib.fmx_repeat_opts(0, 0, (0, 0, 1))),
        dict(opts=_lib.fmx_repeat_opts(1, 1, (7, 0, 0))),
        dict(cap=1 << 32, out=ctypes.c_void_p(16)),
    ]
    for kw in bad:
        if kw.get("min_len", ()) is None:
            kw = dict(kw)
        rc, msg = call(L, dev=dev, **kw)
        assert rc == 3 and msg, (kw, rc, msg)
    # 64 thresholds are the most a call takes: 65 is refused above, and the message names the limit
    assert "64" in call(L, dev=dev, min_len=(3,) * 65)[1]
    assert L.fmx_repeats_last(None, None, None, None) == 0


def test_struct_sizes_and_constants():
    assert ctypes.sizeof(_lib.fmx_repeat_opts) == 8
    assert ctypes.sizeof(_lib.fmx_repeat_range) == 16
    assert ctypes.sizeof(_lib.fmx_repeat_summary) == 48
    assert [f for f, _ in _lib.fmx_repeat_summary._fields_] == list(repeats_ref.FIELDS)
    assert (_lib.FMX_REPEATS_ALL, _lib.FMX_REPEATS_LATER, _lib.FMX_REPEATS_MAX_LEVELS) == (0, 1, 64)
    import os
    import re
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert int(re.search(r"#define FMX_REPEATS_TILE (\d+)", header).group(1)) == _lib.FMX_REPEATS_TILE
    assert int(re.search(r"#define FMX_REPEATS_MAX_LEVELS (\d+)", header).group(1)) == _lib.FMX_REPEATS_MAX_LEVELS
    assert _lib.load().fmx_abi_version() == 5


def test_cli_arguments():
    ap = index.parser()
    a = ap.parse_args(["x.txt", "--dups", "32"])
    assert a.dups == 32 and index.planned_outputs(a) == ["x.bwt", "x.aux", "x.dups"]
    a = ap.parse_args(["x.txt", "--lcp", "--dups", "1"])
    assert index.planned_outputs(a) == ["x.bwt", "x.aux", "x.lcp", "x.dups"]
    a = ap.parse_args(["--dir", "d", "--out", "o/x", "--dups", "40"])
    assert a.dups == 40 and index.planned_outputs(a) == ["o/x.bwt", "o/x.aux", "o/x.docs", "o/x.dups"]
    a = ap.parse_args(["x.txt"])
    assert a.dups is None and index.planned_outputs(a) == ["x.bwt", "x.aux"]
    for bad in ("0", "-3", "abc", "1.5", str(2 ** 32)):
        with pytest.raises(SystemExit):
            ap.parse_args(["x.txt", "--dups", bad])
    with pytest.raises(SystemExit):
        ap.parse_args(["x.txt", "--dups"])
