"""N-grams without a device: the two yardsticks of tests/ngrams_ref.py agree with each other and with cases worked out by
hand, the identity the call without positions rests on holds, the library refuses every bad argument before it touches a
device, the structs have the header's sizes, and the command line takes --ngrams."""
import ctypes
import os
import re

import numpy as np
import pytest

import ngrams_ref
from findex_amd import _lib, index


def same(a, b, what=""):
    (r1, s1), (r2, s2) = a, b
    assert r1.dtype == r2.dtype == ngrams_ref.RECORD and r1.tobytes() == r2.tobytes(), (what, r1, r2)
    assert set(s1) == set(s2)
    for f in ngrams_ref.FIELDS:
        assert s1[f] == s2[f], (what, f, s1, s2)
    if "spectrum" in s1:
        assert s1["spectrum"].dtype == s2["spectrum"].dtype == np.uint64 and np.array_equal(s1["spectrum"], s2["spectrum"]), what


def both(text, L, **kw):
    a = ngrams_ref.brute(text, L, **kw)
    same(a, ngrams_ref.hashed(text, L, **kw), (text, L, kw))
    rec, s = a
    out = [tuple(int(x) for x in r) for r in rec], [s[f] for f in ngrams_ref.FIELDS]
    return out + (s["spectrum"].tolist(),) if "spectrum" in s else out


def test_hand_written_cases():
    # aaaa at L = 2: one class of three overlapping windows.  s = "aaaa$": rows $, a$, aa$, aaa$, aaaa$ -- "aa" from row 2
    assert both(b"aaaa", 2, bins=4) == ([(2, 3, 0)], [1, 1, 1, 3, 0, 3, 2, 0], [0, 0, 0, 1])
    assert both(b"aaaa", 2, bins=3) == ([(2, 3, 0)], [1, 1, 1, 3, 0, 3, 2, 0], [1, 0, 0])
    # abab at L = 2: s = "baba$": rows $, a$, aba$, ba$, baba$.  "ab" is reverse "ba": rows 3, 4, first at 0; "ba" is
    # reverse "ab": row 2 alone (row 1 has one byte only), at 1
    assert both(b"abab", 2) == ([(3, 2, 0)], [1, 1, 2, 3, 1, 2, 3, 0])
    assert both(b"abab", 2, min_count=1, order="row") == ([(2, 1, 1), (3, 2, 0)], [2, 2, 2, 3, 1, 2, 3, 0])
    assert both(b"abab", 2, min_count=1, order="count") == ([(3, 2, 0), (2, 1, 1)], [2, 2, 2, 3, 1, 2, 3, 0])
    # L = m: the text itself, the last row; L = m + 1: nothing
    assert both(b"abab", 4, min_count=1) == ([(4, 1, 0)], [1, 1, 1, 1, 1, 1, 4, 0])
    assert both(b"abab", 4) == ([], [0, 0, 1, 1, 1, 1, 4, 0])
    assert both(b"abab", 5, min_count=1, bins=2) == ([], [0, 0, 0, 0, 0, 0, 0, 0], [0, 0])
    # a stop byte inside the only repeat: "a|b" twice, and with '|' as the stop byte no window of 3 bytes is left but "bxa"
    # (s = "b|axb|a$": rows $, a$, axb|a$, b|a$, b|axb|a$, xb|a$, |a$, |axb|a$)
    assert both(b"a|bxa|b", 3) == ([(3, 2, 0)], [1, 1, 4, 5, 3, 2, 3, 0])
    assert both(b"a|bxa|b", 3, stop=ord("|"), min_count=1) == ([(2, 1, 2)], [1, 1, 1, 1, 1, 1, 2, 2])
    # a tie in count cut by top: x, y and z twice each; by count the tie is cut by sp, which is the order of the letters
    text = b"zyxzyx"
    assert both(text, 1, top=2) == ([(1, 2, 2), (3, 2, 1)], [2, 3, 3, 6, 0, 2, 1, 2])
    assert both(text, 1, top=2, order="row") == ([(1, 2, 2), (3, 2, 1)], [2, 3, 3, 6, 0, 2, 1, 2])
    assert both(text, 1, top=7) == ([(1, 2, 2), (3, 2, 1), (5, 2, 0)], [3, 3, 3, 6, 0, 2, 1, 2])
    # by count the larger class comes first wherever it stands
    assert both(b"aabbb", 1) == ([(3, 3, 2), (1, 2, 0)], [2, 2, 2, 5, 0, 3, 3, 2])


def test_the_yardsticks_agree_on_random_texts():
    rng = np.random.default_rng(22)
    for i in range(240):
        sigma = int(rng.integers(1, 5))
        m = int(rng.integers(1, 41))
        text = bytes(rng.integers(1, sigma + 1, m, dtype=np.uint8) + 96)
        order = ("row", "count")[i & 1]
        for L in range(1, m + 3):
            both(text, L, min_count=1, order=order, stop=0, bins=4)
            both(text, L, min_count=2, order=order, top=2, stop=97, bins=0)


def test_the_yardsticks_agree_beyond_eight_bytes():
    rng = np.random.default_rng(23)
    base = bytes(rng.integers(1, 4, 300, dtype=np.uint8) + 96)
    text = base[:70] + b"q" + base[10:70] + b"r" + base[100:140] + base[100:140]
    for L in (8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 59, 60, 61):
        both(text, L, min_count=1, order="row", bins=8)
        both(text, L, order="count", stop=ord("q"), top=5)


def test_the_short_rows_are_runs_of_their_own():
    """distinct == heads - min(L, n) without a stop byte: what the call without positions takes off its sums"""
    rng = np.random.default_rng(24)
    for _ in range(300):
        sigma = int(rng.integers(1, 5))
        m = int(rng.integers(1, 41))
        text = bytes(rng.integers(1, sigma + 1, m, dtype=np.uint8) + 96)
        for L in range(1, m + 3):
            s = ngrams_ref.brute(text, L, min_count=1)[1]
            assert s["distinct"] == ngrams_ref.heads(text, L) - min(L, m + 1), (text, L)
            assert s["windows"] == max(m - L + 1, 0)


# ---- the library's refusals, before any device is touched
def opts(order=0, flags=0, min_count=2, top=0, bins=0, stop=0, reserved=(0, 0, 0)):
    return _lib.fmx_ngram_opts(order, flags, min_count, top, bins, stop, reserved)


def call(L, idx=1, lengths=(4,), k=None, o=None, out_off=True, out=None, cap=0, n_out=True, spectrum=None, dev=False):
    lv = (ctypes.c_uint32 * max(len(lengths), 1))(*lengths) if lengths is not None else None
    off = (ctypes.c_uint64 * 66)() if out_off else None
    n = ctypes.c_size_t() if n_out else None
    handle = ctypes.c_void_p(idx) if idx else None             # never dereferenced: every case here is refused first
    args = [handle, lv, len(lengths) if k is None else k, ctypes.byref(o) if o is not None else None, off, out, cap,
            ctypes.byref(n) if n_out else None, None, spectrum]
    rc = (L.fmx_ngrams_dev(*args, None) if dev else L.fmx_ngrams(*args))
    return rc, (L.fmx_last_error() or b"").decode()


@pytest.mark.parametrize("dev", [False, True])
def test_bad_arguments_are_refused_without_a_device(dev):
    L = _lib.load()
    spec = (ctypes.c_uint64 * 8)()
    bad = [
        dict(idx=0),
        dict(lengths=None, k=1),
        dict(out_off=False),
        dict(n_out=False),
        dict(lengths=(), k=0),
        dict(lengths=(3,) * 65),
        dict(lengths=(3, 0, 5)),
        dict(o=opts(order=2)),
        dict(o=opts(flags=2)),
        dict(o=opts(flags=3)),
        dict(o=opts(min_count=0)),
        dict(o=opts(flags=_lib.FMX_NGRAMS_NO_POS, stop=7)),
        dict(o=opts(flags=_lib.FMX_NGRAMS_NO_POS, min_count=1)),
        dict(o=opts(bins=65537), spectrum=spec),
        dict(o=opts(bins=8)),
        dict(o=opts(reserved=(0, 0, 1))),
        dict(o=opts(reserved=(7, 0, 0))),
        dict(cap=1 << 32, out=ctypes.c_void_p(16)),
    ]
    for kw in bad:
        rc, msg = call(L, dev=dev, **kw)
        assert rc == 3 and msg, (kw, rc, msg)
    assert "64" in call(L, dev=dev, lengths=(3,) * 65)[1]
    assert L.fmx_ngrams_last(None, None, None, None) == 0


def test_struct_sizes_and_constants():
    assert ctypes.sizeof(_lib.fmx_ngram_opts) == 32
    assert ctypes.sizeof(_lib.fmx_ngram) == 24
    assert ctypes.sizeof(_lib.fmx_ngram_summary) == 64
    assert [f for f, _ in _lib.fmx_ngram_summary._fields_] == list(ngrams_ref.FIELDS)
    assert [f for f, _ in _lib.fmx_ngram._fields_] == list(ngrams_ref.RECORD.names)
    assert (_lib.FMX_NGRAMS_BY_ROW, _lib.FMX_NGRAMS_BY_COUNT, _lib.FMX_NGRAMS_NO_POS, _lib.FMX_NGRAMS_MAX_LEVELS) == (0, 1, 1, 64)
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert int(re.search(r"#define FMX_NGRAMS_LDS_BINS (\d+)", header).group(1)) == _lib.FMX_NGRAMS_LDS_BINS
    assert int(re.search(r"#define FMX_NGRAMS_MAX_BINS (\d+)", header).group(1)) == _lib.FMX_NGRAMS_MAX_BINS
    assert int(re.search(r"#define FMX_NGRAMS_MAX_LEVELS (\d+)", header).group(1)) == _lib.FMX_NGRAMS_MAX_LEVELS
    assert _lib.load().fmx_abi_version() == 5


def test_cli_arguments():
    ap = index.parser()
    a = ap.parse_args(["x.txt", "--ngrams", "8"])
    assert a.ngrams == [8] and a.min_count == 2 and a.top == 100 and index.planned_outputs(a) == ["x.bwt", "x.aux", "x.ngrams"]
    a = ap.parse_args(["x.txt", "--lcp", "--dups", "4", "--ngrams", "3,5,3", "--min-count", "1", "--top", "0"])
    assert a.ngrams == [3, 5, 3] and a.min_count == 1 and a.top == 0
    assert index.planned_outputs(a) == ["x.bwt", "x.aux", "x.lcp", "x.dups", "x.ngrams"]
    a = ap.parse_args(["--dir", "d", "--out", "o/x", "--ngrams", "40", "--top", "7"])
    assert a.ngrams == [40] and a.top == 7 and index.planned_outputs(a) == ["o/x.bwt", "o/x.aux", "o/x.docs", "o/x.ngrams"]
    a = ap.parse_args(["x.txt"])
    assert a.ngrams is None and index.planned_outputs(a) == ["x.bwt", "x.aux"]
    for bad in ("0", "-3", "abc", "1.5", "3,,4", "3,0", str(2 ** 32), ",".join(["2"] * 65)):
        with pytest.raises(SystemExit):
            ap.parse_args(["x.txt", "--ngrams", bad])
    for flag, bad in (("--min-count", "0"), ("--min-count", "x"), ("--top", "-1")):
        with pytest.raises(SystemExit):
            ap.parse_args(["x.txt", "--ngrams", "3", flag, bad])
    with pytest.raises(SystemExit):
        ap.parse_args(["x.txt", "--ngrams"])
    with pytest.raises(SystemExit):
        index.main(["--append", "base", "x.txt", "--ngrams", "3"])
    assert index.printable(b"a b\\c\x00\xff~!") == b"a\\x20b\\x5Cc\\x00\\xFF~!"
