"""Append (include/fmx.h, "append") without a device: the reference of tests/merge_ref.py against a direct suffix sort,
the piece's context criterion, every refusal that is decided before the device is touched, the structs' sizes and the
command line's new arguments."""
import ctypes
import random

import numpy as np
import pytest

import merge_ref
from findex_amd import _lib, index


def random_case(rng):
    sigma = rng.randint(1, 4)
    alpha = bytes(rng.sample(range(1, 256), sigma))
    A = bytes(rng.choice(alpha) for _ in range(rng.randint(1, 40)))
    B = bytearray(rng.choice(alpha) for _ in range(rng.randint(1, 40)))
    for _ in range(rng.randint(0, 2)):                      # planted copies of stretches of A
        ln = rng.randint(1, len(A))
        at = rng.randint(0, len(A) - ln)
        to = rng.randint(0, len(B))
        B[to:to] = A[at:at + ln]
    return A, bytes(B[:60])


def test_merge_ref_equals_a_direct_suffix_sort():
    rng = random.Random(20261019)
    retries = 0
    for _ in range(400):
        A, B = random_case(rng)
        S, W, ctx = rng.randint(1, 64), rng.randint(0, 5), rng.randint(0, 4)
        got = merge_ref.merge_ref(A, B, segment=S, warmup=W, context=ctx)
        bwt, eof, counts = merge_ref.bwt_direct(A + B, sort=merge_ref.naive_suffix_array)
        assert got["eof"] == eof and np.array_equal(got["bwt"], bwt) and np.array_equal(got["counts"], counts), (A, B, S, W, ctx)
        assert got["fixup_steps"] >= got["longest_run"] >= (1 if got["runs"] else 0)
        retries += got["rounds"] > 1
    assert retries > 20                                     # the retry path was walked, not just present


def test_numpy_suffix_sort_equals_the_naive_one():
    rng = random.Random(7)
    for _ in range(200):
        s = bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 50))) + b"\0"
        assert np.array_equal(merge_ref.suffix_array(s), merge_ref.naive_suffix_array(s))


def test_context_criterion_retry_and_whole_text():
    """The order of two new suffixes is wrong only when one of them, cut at the piece's end, is a prefix of the other: B
    then holds tail(A, M) followed by B's own first byte(s).  The criterion must fail exactly there."""
    A = b"xyzxyzabcabd"
    ra = merge_ref.RankA(*merge_ref.bwt_direct(A))
    B = b"q" + A[-4:] + b"q"                                # tail(A, 4) + B[0] stands in B: 4 fails, 8 passes
    order, M, rounds = merge_ref.new_order(ra, B, context=4)
    assert (M, rounds) == (8, 2)
    order1, M1, rounds1 = merge_ref.new_order(ra, B, context=len(A))
    assert (M1, rounds1) == (len(A), 1) and np.array_equal(order, order1)
    assert merge_ref.new_order(ra, A[-6:] + b"q", context=4)[1:] == (4, 1)       # a copy of the tail alone needs no more
    # M == a: the piece is all of A + B and nothing is checked, whatever B repeats
    P = b"abcab" * 6
    rp = merge_ref.RankA(*merge_ref.bwt_direct(P))
    order2, M2, rounds2 = merge_ref.new_order(rp, P, context=2)
    assert M2 == len(P) and rounds2 == 5                    # 2, 4, 8, 16 fail; 32 -> min(a, 32) = 30 = a
    with pytest.raises(ValueError):
        merge_ref.new_order(rp, P, context=2, max_context=8)
    got = merge_ref.merge_ref(P, P, segment=4, warmup=2, context=2)
    assert np.array_equal(got["bwt"], merge_ref.bwt_direct(P + P, sort=merge_ref.naive_suffix_array)[0])
    # one run: everything but the segments that start exact -- [24, 28) and [28, 30), whose warm-up is clipped at b
    assert got["runs"] == 1 and got["longest_run"] == got["fixup_steps"] == 24


def test_tail_from_the_index_alone():
    A = b"mississippi river"
    ra = merge_ref.RankA(*merge_ref.bwt_direct(A))
    for m in (0, 1, 5, len(A)):
        assert ra.tail_reversed(m) == A[::-1][:m]


def test_struct_sizes_and_constants():
    assert ctypes.sizeof(_lib.fmx_merge_opts) == 40
    assert ctypes.sizeof(_lib.fmx_merge_stats) == 88
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name in ("SEGMENT", "WARMUP", "TILE", "CONTEXT"):
        assert int(re.search(r"#define FMX_MERGE_%s (\d+)" % name, hdr).group(1)) == getattr(_lib, "FMX_MERGE_" + name)


def test_refusals_before_the_device_is_touched():
    L = _lib.load()
    text = np.frombuffer(b"abc", dtype=np.uint8)
    zero = np.frombuffer(b"a\0c", dtype=np.uint8)
    tp, zp = text.ctypes.data_as(ctypes.c_void_p), zero.ctypes.data_as(ctypes.c_void_p)
    out = ctypes.c_void_p()
    eof = ctypes.c_uint64()
    counts = np.zeros(256, dtype=np.int64)
    cp = counts.ctypes.data_as(ctypes.c_void_p)
    err = lambda: L.fmx_last_error().decode()
    # in the header's order; the handle comes last, so a null one shows what was decided before it
    assert L.fmx_append_text(None, None, 3, None, ctypes.byref(out)) == 3 and "text is null" in err()
    assert L.fmx_append_text(None, tp, 3, None, None) == 3 and "output is null" in err()
    assert L.fmx_append_text(None, tp, 0, None, ctypes.byref(out)) == 3 and "len" in err()
    for word in range(4):
        o = _lib.fmx_merge_opts()
        o.reserved[word] = 1
        assert L.fmx_append_text(None, tp, 3, ctypes.byref(o), ctypes.byref(out)) == 3 and "reserved" in err()
    limit = (1 << 32) - 2
    assert L.fmx_append_text(None, tp, limit - 4095, None, ctypes.byref(out)) == 6 and "2^32 - 2" in err()
    o = _lib.fmx_merge_opts()
    o.context = limit
    assert L.fmx_append_text(None, tp, 3, ctypes.byref(o), ctypes.byref(out)) == 6 and "2^32 - 2" in err()
    assert L.fmx_append_text(None, tp, limit + 1, None, ctypes.byref(out)) == 6
    assert L.fmx_append_text(None, zp, 3, None, ctypes.byref(out)) == 6 and "byte 0" in err()
    assert L.fmx_append_text(None, tp, 3, None, ctypes.byref(out)) == 3 and "idx is null" in err()
    # the device form: the same, and its host outputs
    assert L.fmx_append_text_dev(None, tp, 3, None, tp, None, cp, None) == 3
    assert L.fmx_append_text_dev(None, tp, 3, None, tp, ctypes.byref(eof), None, None) == 3
    assert L.fmx_append_text_dev(None, None, 3, None, tp, ctypes.byref(eof), cp, None) == 3 and "text is null" in err()
    assert L.fmx_append_text_dev(None, tp, 3, None, None, ctypes.byref(eof), cp, None) == 3 and "output is null" in err()
    assert L.fmx_append_text_dev(None, tp, 0, None, tp, ctypes.byref(eof), cp, None) == 3
    o = _lib.fmx_merge_opts()
    o.reserved[2] = 7
    assert L.fmx_append_text_dev(None, tp, 3, ctypes.byref(o), tp, ctypes.byref(eof), cp, None) == 3 and "reserved" in err()
    assert L.fmx_append_text_dev(None, tp, limit - 4095, None, tp, ctypes.byref(eof), cp, None) == 6
    assert L.fmx_append_text_dev(None, tp, 3, None, tp, ctypes.byref(eof), cp, None) == 3 and "idx is null" in err()
    assert L.fmx_merge_last(None) == 3


def test_merge_opts_of_the_searcher():
    from findex_amd import HipFMSearcher
    assert HipFMSearcher._merge_opts() is None
    o = HipFMSearcher._merge_opts(context=8192)
    assert (o.context, o.max_context, o.segment, o.warmup) == (8192, 0, 0, 0)
    o = HipFMSearcher._merge_opts(segment=1, warmup=0)
    assert (o.segment, o.warmup) == (1, 0)
    o = HipFMSearcher._merge_opts(warmup=5)
    assert (o.segment, o.warmup) == (_lib.FMX_MERGE_SEGMENT, 5)
    with pytest.raises(ValueError):
        HipFMSearcher._merge_opts(segment=0)


def test_append_and_chunk_arguments(capsys):
    ap = index.parser()
    a = ap.parse_args(["X.txt", "--chunk", "1048576"])
    assert a.chunk == 1048576 and a.append is None and a.text == "X.txt"
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit):
            ap.parse_args(["X.txt", "--chunk", bad])
    a = ap.parse_args(["--append", "out/base", "new.txt", "--sa"])
    assert a.append == "out/base" and a.text == "new.txt" and a.sa and not a.lcp
    assert index.append_outputs(a) == (("out/base.bwt", "out/base.aux", "out/base.docs"),
                                       ("out/base.fm", "out/base.sa", "out/base.lcp", "out/base.dups"))
    assert index.dups_name(a) == "out/base.dups"
    a = ap.parse_args(["--append", "base", "--dir", "more"])
    assert a.dir == "more" and a.text is None
    # combinations main() refuses before anything is opened
    for argv in (["--append", "base"], ["--append", "base", "f.txt", "--dir", "d"], ["--append", "base", "f.txt", "--out", "o"],
                 ["--append", "base", "f.txt", "--chunk", "5"], ["--append", "base", "f.txt", "--data"],
                 ["--dir", "d", "--out", "o", "--chunk", "5"]):
        with pytest.raises(SystemExit):
            index.main(argv)
    capsys.readouterr()
