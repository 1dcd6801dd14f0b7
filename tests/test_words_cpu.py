"""Whole-word matching without a device: the checker (tests/words_ref.py) against a hand-worked text, the mask arithmetic of
findex_amd/csrc/fmx_ctx_math.h under AddressSanitizer + UBSan (tests/native/ctx_math.cpp), the classes, both command lines'
parsing, and every refusal the new entry points decide before they touch a handle or the device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import words_ref
from conftest import ROOT
from findex_amd import _lib

#        0123456789012345
TEXT = b"the then he, the"


# ---- 1. the checker, by hand: "the" is a word at offset 0 and at the very end, "he" stands four times and is a word once
def test_checker_against_a_hand_worked_text():
    r = words_ref.SuffixRef(TEXT)
    B = words_ref.BOUNDARY
    assert r.n == 17 and r.sa[0] == 16 and r.bwt[r.eof] == 0 and r.sa[r.eof] == 0
    sp, ep = r.interval(b"he")
    assert ep - sp == 4 and sorted(r.pos(x, 2) for x in range(sp, ep)) == [1, 5, 9, 14]
    assert [r.pos(x, 2) for x in r.context_rows(b"he", B, B)] == [9]
    rows = r.context_rows(b"the", B, B)
    assert sorted(r.pos(x, 3) for x in rows) == [0, 13]
    assert r.eof in rows                                             # the occurrence that ends where the text ends is row eof
    sp, ep = r.interval(b"the")
    assert ep - sp == 3 and r.lf_chain(3) == sp and r.pos(sp, 3) == 0     # the occurrence at offset 0 is the interval's first row
    assert r.lf_chain(0) == 0 and r.lf_chain(16) == r.eof
    assert r.interval(b"then") == (r.interval(b"then")[0], r.interval(b"then")[0] + 1) and r.lf_chain(4) != r.interval(b"then")[0]
    assert r.context_rows(b"th", B, B) == [] and r.context_rows(b"then", B, B) == list(range(*r.interval(b"then")))
    # the byte in front: the rows of a.X are rows of X, and the same rows give X's start with len(X)
    a_sp, a_ep = r.interval(b" the")
    assert sp <= a_sp < a_ep <= ep and sorted(r.pos(x, 3) for x in range(a_sp, a_ep)) == [4, 13]
    # bit 0 of a class: with the ends of the text shut out, both "the" go
    no_end = bytes(c for c in B if c != 0)
    assert r.context_rows(b"the", no_end, B) == [x for x in rows if r.pos(x, 3) == 13]
    assert r.context_rows(b"the", B, no_end) == [x for x in rows if r.pos(x, 3) == 0]
    # the filter: runs inside a record, the lead, the start mode
    off, runs = r.filter([(7, 3, sp, ep)], B)
    assert off == [0, len(runs)] and sorted(x for _, _, a, b in runs for x in range(a, b)) == sorted(rows)
    assert all(g == 7 and ln == 3 for g, ln, _, _ in runs)
    assert r.filter([(0, 3, sp, ep)], B, [words_ref.CTX_START]) == ([0, 1], [(0, 3, sp, sp + 1)])
    assert r.filter([(0, 3, sp + 1, ep)], B, [words_ref.CTX_START]) == ([0, 0], [])
    last = [x for x in range(a_sp, a_ep) if r.pos(x, 3) == 13]      # " the" + "n" does not pass, " the" + the end does
    assert r.filter([(0, 4, a_sp, a_ep)], B, [1]) == ([0, 1], [(0, 3, last[0], last[0] + 1)])
    assert r.filter([(0, 3, a_sp, a_ep)], B, [3]) == ([0, 0], [])    # len <= lead
    assert r.filter([(0, 1, 0, 99)], bytes(range(256))) == ([0, 1], [(0, 1, 0, 17)])      # ep > n, the full class
    assert r.filter([(0, 1, 0, 17)], b"") == ([0, 0], [])
    assert r.filter([(0, 1, 0, 17)], b"\0") == ([0, 1], [(0, 1, r.eof, r.eof + 1)])


def test_end_to_end_checkers():
    assert words_ref.literal_word_starts(TEXT, b"the") == [0, 13]
    assert words_ref.literal_word_starts(TEXT, b"he") == [9]
    assert words_ref.literal_word_starts(b" he he ", b"he") == [1, 4]
    assert words_ref.word_starts(TEXT, b"th(e|en)") == [(0, 3), (4, 4), (13, 3)]
    assert words_ref.word_starts(TEXT, b".he") == [(0, 3), (13, 3)]               # " he" stands behind the n of "then"
    assert words_ref.word_starts(b"a, he", b".he") == [(2, 3)]
    assert words_ref.disjoint([(0, 3), (0, 5), (4, 2), (5, 1)]) == [(0, 5), (5, 1)]
    caf = "café au".encode()
    assert words_ref.literal_word_starts(caf, b"caf") == [] and words_ref.literal_word_starts(caf, "café".encode()) == [0]


def test_doubling_suffix_array_is_the_naive_one():
    rng = np.random.default_rng(5)
    for n, sigma in ((1, 2), (2, 2), (50, 2), (300, 3), (1000, 4), (700, 1)):
        s = bytes(rng.integers(97, 97 + sigma, n, dtype=np.uint8).tolist())[::-1] + b"\0"
        assert words_ref.doubling_suffix_array(s) == words_ref.naive_suffix_array(s)


def test_classes():
    import findex_amd
    w = findex_amd.WORD_BYTES
    assert w == words_ref.WORD_BYTES and len(w) == 63 + 128
    assert all(bytes([c]) in w for c in b"09AZaz_") and b"\x80" in w and b"\xff" in w
    b = findex_amd.boundary_class()
    assert b == words_ref.BOUNDARY and b[0] == 0 and b[1] == 1 and set(b) | set(w) == set(range(256)) and not set(b) & set(w)
    cw = findex_amd.class_words(b"\x00\x01\x3f\x40\xff")
    assert cw.tolist() == [(1 << 0) | (1 << 1) | (1 << 63), 1, 0, 1 << 63]
    assert findex_amd.class_words(b"").tolist() == [0, 0, 0, 0]


# ---- 2. the mask arithmetic under the sanitizers
@pytest.mark.timeout(300)
def test_ctx_math_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "ctx_math"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "findex_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ctx_math.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "error:" not in build.stderr:
        pytest.skip("sanitizer runtime not available: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=200)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "ctx math ok" in run.stdout


# ---- 3. the command lines
def test_grep_cli_parses_w():
    from findex_amd import grep as cli
    a = cli.parser().parse_args(["base", "re", "-w", "-n"])
    assert a.words and a.line_number and cli.by_lines(a)
    assert cli.parser().parse_args(["base", "re", "--word-regexp"]).words
    d = cli.parser().parse_args(["base", "re"])
    assert d.words is False and not cli.by_lines(d)
    assert "-w" in cli.parser().format_help()


def test_rank_cli_parses_w():
    from findex_amd import rank as cli
    assert cli.parser().parse_args(["base", "q", "-w"]).words and cli.parser().parse_args(["base", "q", "--words"]).words
    assert cli.parser().parse_args(["base", "q"]).words is False
    h = cli.parser().format_help()
    assert "--words" in h and "whole word" in h and "no whole-word matching" not in h


# ---- 4. refusals that need no device: decided before a handle is looked at, so a buffer of zeros stands in for it
def test_abi_and_struct_sizes():
    L = _lib.load()
    assert L.fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_context_opts) == 72 and ctypes.sizeof(_lib.fmx_result) == 24
    assert _lib.FMX_CTX_START == 0x80


def _filter(L, idx, rec, mode=None, right="ok", off="ok", n_out="ok", k=None, dev=False):
    vp = ctypes.c_void_p
    rec = np.asarray(rec, dtype=np.dtype(_lib_result()))
    md = None if mode is None else np.asarray(mode, dtype=np.uint8)
    rw = np.zeros(4, dtype=np.uint64)
    o = np.zeros(rec.size + 1, dtype=np.uint64)
    out = np.zeros(max(rec.size, 1) * 3, dtype=np.uint64)
    n = ctypes.c_size_t()
    args = [idx, rec.ctypes.data_as(vp) if rec.size else None, None if md is None else md.ctypes.data_as(vp),
            rec.size if k is None else k, rw.ctypes.data_as(vp) if right == "ok" else None,
            o.ctypes.data_as(vp) if off == "ok" else None, out.ctypes.data_as(vp), 1, ctypes.byref(n) if n_out == "ok" else None]
    rc = L.fmx_context_filter_dev(*args, None) if dev else L.fmx_context_filter(*args)
    return rc, L.fmx_last_error().decode()


def _lib_result():
    return [("regex", np.uint32), ("len", np.uint32), ("sp", np.uint64), ("ep", np.uint64)]


def test_filter_refusals_need_no_device():
    L = _lib.load()
    fake = ctypes.create_string_buffer(8192)
    i = ctypes.cast(fake, ctypes.c_void_p)
    good = [(0, 3, 1, 5)]
    for dev in (False, True):
        for kw in ({"right": None}, {"off": None}, {"n_out": None}):
            rc, msg = _filter(L, i, good, dev=dev, **kw)
            assert rc == 3 and "null" in msg, kw
        rc, msg = _filter(L, i, good, k=(1 << 26) + 1, dev=dev)
        assert rc == 3 and "2^26" in msg
        rc, msg = _filter(L, None, good, dev=dev)
        assert rc == 3 and "handle" in msg
    for rec, mode, word in (([(0, 65536, 1, 5)], None, "FMX_OCC_MAX_LEN"), ([(0, 3, 6, 5)], None, "sp > ep"),
                            ([(0, 3, 1, 5), (0, 3, 1, 5)], [0, 0x81], "FMX_CTX_START")):
        rc, msg = _filter(L, i, rec, mode)
        assert rc == 3 and word in msg, (word, msg)
    # (a record the host form accepts and a null handle: the records are looked at first)
    assert _filter(L, None, [(0, 65535, 5, 5)], [0x80])[0] == 3


def _search(L, idx, pats, opts="ok", flags=0, reserved=0, off=None, dev=False):
    vp = ctypes.c_void_p
    pat = np.frombuffer(b"".join(pats), dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(p) for p in pats])])
    off = np.asarray(off, dtype=np.uint64)
    o = _lib.fmx_context_opts()
    o.flags, o.reserved = flags, reserved
    out_off = np.zeros(off.size, dtype=np.uint64)
    out = np.zeros(3, dtype=np.uint64)
    n = ctypes.c_size_t()
    args = [idx, pat.ctypes.data_as(vp) if pat.size else None, off.ctypes.data_as(vp), off.size - 1,
            ctypes.byref(o) if opts == "ok" else None, out_off.ctypes.data_as(vp), out.ctypes.data_as(vp), 1, ctypes.byref(n)]
    rc = L.fmx_search_context_batch_dev(*args, None) if dev else L.fmx_search_context_batch(*args)
    return rc, L.fmx_last_error().decode()


def test_search_context_refusals_need_no_device():
    L = _lib.load()
    fake = ctypes.create_string_buffer(8192)
    i = ctypes.cast(fake, ctypes.c_void_p)
    for dev in (False, True):
        rc, msg = _search(L, i, [b"ab"], opts=None, dev=dev)
        assert rc == 3 and "opts" in msg
        for kw in ({"flags": 1}, {"reserved": 7}):
            rc, msg = _search(L, i, [b"ab"], dev=dev, **kw)
            assert rc == 3 and "must be 0" in msg
        rc, msg = _search(L, None, [b"ab"], dev=dev)
        assert rc == 3 and "handle" in msg
    for pats, off, word in (([b"ab", b""], None, "empty"), ([b"a\0b"], None, "byte 0"), ([b"x" * 65535], None, "65534"),
                            ([b"abcd"], [0, 3, 2], "ascend")):
        rc, msg = _search(L, i, pats, off=off)
        assert rc == 3 and word in msg, (word, msg)


def test_rank_sets_refusals_need_no_device():
    L = _lib.load()
    vp = ctypes.c_void_p
    fake_c, fake_i = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    c, i = ctypes.cast(fake_c, vp), ctypes.cast(fake_i, vp)
    prm = _lib.fmx_rank_params(1.2, 0.75, 0, 10, 0)
    sp, ep = np.array([1, 2, 3], dtype=np.uint64), np.array([2, 3, 4], dtype=np.uint64)
    q_off = np.array([0, 2], dtype=np.uint64)
    off, doc, score = np.zeros(2, dtype=np.uint64), np.zeros(16, dtype=np.uint32), np.zeros(16, dtype=np.float64)

    def call(set_off):
        so = None if set_off is None else np.asarray(set_off, dtype=np.uint64)
        rc = L.fmx_corpus_rank_sets(c, i, sp.ctypes.data_as(vp), ep.ctypes.data_as(vp), 3, None if so is None else so.ctypes.data_as(vp),
                                    2, q_off.ctypes.data_as(vp), 1, ctypes.byref(prm), None, off.ctypes.data_as(vp),
                                    doc.ctypes.data_as(vp), score.ctypes.data_as(vp), 16, None, None)
        return rc, L.fmx_last_error().decode()

    rc, msg = call(None)
    assert rc == 3 and "null" in msg
    for bad in ([1, 2, 3], [0, 2, 1], [0, 1, 2], [0, 2, 4]):            # not from 0; decreasing; not up to n_iv (3 intervals)
        rc, msg = call(bad)
        assert rc == 3 and "set_off" in msg, bad
