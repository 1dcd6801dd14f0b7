"""Passages without a device: the checker (tests/passages_ref.py) against a hand-worked example, the key packing and the window
order of findex_amd/csrc/fmx_passage_math.h under AddressSanitizer + UBSan (tests/native/passage_math.cpp), the binding and the
header's structs, the command line's new flags and rendering, and every refusal fmx_corpus_passages decides before it touches
a handle or the device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import corpus_ref
import passages_ref
from conftest import ROOT
from findex_amd import _lib


# ---- 1. the checker, by hand.  Three files; the stream (separator 1 written as |):
#   d0 = "ab..cd.ab"   positions 0 .. 8, separator at 9      ab at 0 and 7, cd at 4
#   d1 = "cd"          positions 10, 11, separator at 12     cd at 10
#   d2 = "xx\0ab"      raw 5 bytes, stream "xx\\0ab" at 13 .. 18, separator at 19; ab at 17 = raw offset 3
# terms ab (weight 1.0) and cd (weight 2.0).
#   window 6, d0: start 0 covers ab [0,1] and cd [4,5]        -> 3.0   start 4 covers cd and ab [7,8] -> 3.0   start 7 -> 1.0
#                 the tie goes to start 0; clipped at min(6, 9) = 6: 6 raw bytes
#   window 5, d0: start 0: cd ends at 5, not below 5          -> 1.0   start 4: [4, 9) holds both     -> 3.0   start 7 -> 1.0
#                 start 4; clipped at min(9, 9): 5 raw bytes
#   window 1, d0: nothing fits                                 -> 0.0 at the smallest start 0, mask 0, 1 raw byte
#   d1: start 10 -> 2.0, mask 2; the window is clipped at the separator: 2 raw bytes
#   d2: start 17 -> 1.0, mask 1, raw offset 3; clipped at the separator: 2 raw bytes
@pytest.fixture(scope="module")
def three():
    return passages_ref.PassagesRef(corpus_ref.RefCorpus([b"ab..cd.ab", b"cd", b"xx\x00ab"]))


def test_checker_against_a_hand_worked_example(three):
    r = three
    assert r.ref.doc_start == [0, 10, 13, 20] and r.ref.stream[13:19] == b"xx\\0ab"
    assert r.occurrences(0, b"ab") == ([0, 7], 2) and r.occurrences(0, b"cd") == ([4], 2) and r.occurrences(2, b"\x00") == ([15], 2)
    q, w = [[b"ab", b"cd"]], [1.0, 2.0]
    recs, tf = r.run(q, [0, 3], [0, 1, 2], 6, weights=w)
    assert recs == [(0, 3, 3.0, 6, 3), (0, 2, 2.0, 2, 1), (3, 1, 1.0, 2, 1)]
    assert tf == [[2, 1], [0, 1], [1, 0]]
    assert r.run(q, [0, 1], [0], 5, weights=w)[0] == [(4, 3, 3.0, 5, 3)]
    assert r.run(q, [0, 1], [0], 1, weights=w)[0] == [(0, 0, 0.0, 1, 3)]
    assert r.run(q, [0, 1], [0], 2, weights=w)[0] == [(4, 2, 2.0, 2, 3)]                  # a window of a term's length
    # the default weights are 1.0 each; a file without occurrences gets zeros; the hits keep the order given
    recs, tf = r.run([[b"cd"], [b"zz", b"ab"]], [0, 2, 4], [1, 0, 2, 1], 100)
    assert recs == [(0, 1, 1.0, 2, 1), (4, 1, 1.0, 5, 1), (3, 2, 1.0, 2, 1), (0, 0, 0.0, 0, 0)]
    assert tf == [[1, 0], [1, 0], [0, 1], [0, 0]]
    # a negative weight lowers a window's value: the window without cd wins
    assert r.run(q, [0, 1], [0], 6, weights=[1.0, -2.0])[0] == [(7, 1, 1.0, 2, 3)]
    # the order of the additions: 0.0 in slot order, 1.0 in any other
    # (terms c, d and . on "ab..cd.ab": every window that holds c holds the dot at 6 too; the starts 5 and 6 are far below)
    assert r.run([[b"c", b"d", b"."]], [0, 1], [0], 9, weights=[1e16, 1.0, -1e16])[0] == [(2, 7, 0.0, 7, 5)]
    assert r.run([[b"c", b".", b"d"]], [0, 1], [0], 9, weights=[1e16, -1e16, 1.0])[0] == [(2, 7, 1.0, 7, 5)]


def test_checker_words_case_and_overlaps():
    r = passages_ref.PassagesRef(corpus_ref.RefCorpus([b"EDGEDGE", b"cat concat Cat cat_ cat", b"\xffcat"]))
    assert r.occurrences(0, b"EDGE") == ([0, 3], 4)
    d1 = r.ref.doc_start[1]
    assert [f - d1 for f in r.occurrences(1, b"cat")[0]] == [0, 7, 15, 20]
    assert [f - d1 for f in r.occurrences(1, b"cat", ignore_case=True)[0]] == [0, 7, 11, 15, 20]
    assert [f - d1 for f in r.occurrences(1, b"cat", words=True)[0]] == [0, 20]
    assert [f - d1 for f in r.occurrences(1, b"CAT", words=True, ignore_case=True)[0]] == [0, 11, 20]
    # raw 255 is the pair backslash f in the stream, and f is a word byte: "cat" behind it is no whole word
    assert r.occurrences(2, b"cat")[0] == [r.ref.doc_start[2] + 2] and r.occurrences(2, b"cat", words=True)[0] == []


# ---- 2. the key packing and the window order, under the sanitizers
@pytest.mark.timeout(300)
def test_passage_math_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "passage_math"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "findex_amd", "csrc"), os.path.join(ROOT, "tests", "native", "passage_math.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "error:" not in build.stderr:
        pytest.skip("sanitizer runtime not available: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=200)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "passage math ok" in run.stdout


# ---- 3. the binding and the header
def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fmx_corpus_passages", "fmx_corpus_passages_dev", "fmx_corpus_passages_last"):
        assert ("int " + name + "(") in header and name in _lib.SYMBOLS and hasattr(L, name)
    assert ctypes.sizeof(_lib.fmx_passage) == 32 and ctypes.sizeof(_lib.fmx_passage_params) == 24
    from findex_amd.corpus import HipCorpusSearcher
    assert HipCorpusSearcher.PASSAGE.itemsize == 32
    assert [(n, HipCorpusSearcher.PASSAGE.fields[n][1]) for n in HipCorpusSearcher.PASSAGE.names] == \
        [(n, getattr(_lib.fmx_passage, n).offset) for n, _ in _lib.fmx_passage._fields_]
    assert _lib.load().fmx_abi_version() == 5


def test_header_structs_in_strict_c99(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use_passages.c"
    src.write_text(
        "#include <fmx.h>\n#include <stddef.h>\n#include <stdio.h>\n"
        "int main(void) {\n"
        "  fmx_passage p; fmx_passage_params q;\n"
        "  p.raw_off = 1; p.mask = 2; p.value = 0.5; p.raw_len = 3; p.n_occ = 4;\n"
        "  q.window = 160; q.max_per = 0; q.flags = 0; q.reserved = 0;\n"
        "  printf(\"%d %d %d %d\\n\", (int)sizeof p, (int)sizeof q, (int)offsetof(fmx_passage, value), (int)offsetof(fmx_passage, n_occ));\n"
        "  return (int)(p.raw_off + q.flags) - 1;\n}\n")
    exe = tmp_path / "use_passages"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ["32", "24", "16", "28"]


# ---- 4. the command line
def test_cli_flags_parse_and_render():
    from findex_amd import rank as cli
    a = cli.parser().parse_args(["base", "two words", "--snippets", "40", "--explain", "-w", "-i", "--all"])
    assert (a.snippets, a.explain, a.words, a.ignore_case, a.all_) == (40, True, True, True, True)
    a = cli.parser().parse_args(["base", "q", "--snippets"])
    assert a.snippets == 160 and not a.explain
    a = cli.parser().parse_args(["base", "q"])
    assert a.snippets is None and a.explain is False and a.top == 10
    with pytest.raises(SystemExit):
        cli.main(["base", "q", "--snippets", "0"])
    names = [b"a.txt", b"dir/b.txt", b"c"]
    off, doc, score = [0, 2, 2, 3], [1, 0, 2], [1.5, 0.1 + 0.2, -2.0]
    queries = [[b"ab", b"cd"], [], [b"x"]]
    raw_off, texts, tf = [7, 0, 12], [b"one\ntwo\tab", b"cd\x00\x1f ", b"x"], [[2, 0], [0, 1], [5, 0]]
    base = [b"1.5\tdir/b.txt", b"0.30000000000000004\ta.txt", b"", b"", b"-2.0\tc"]
    assert cli.render(names, off, doc, score) == base                                    # unchanged
    assert cli.render_passages(names, off, doc, score, queries) == base
    assert cli.render_passages(names, off, doc, score, queries, raw_off, texts, tf) == [
        b"1.5\tdir/b.txt", b"\t7\tone two ab", b"\tab=2 cd=0", b"0.30000000000000004\ta.txt", b"\t0\tcd   ", b"\tab=0 cd=1", b"", b"",
        b"-2.0\tc", b"\t12\tx", b"\tx=5"]
    assert cli.render_passages(names, off, doc, score, queries, raw_off, texts) == [
        b"1.5\tdir/b.txt", b"\t7\tone two ab", b"0.30000000000000004\ta.txt", b"\t0\tcd   ", b"", b"", b"-2.0\tc", b"\t12\tx"]
    assert cli.render_passages(names, off, doc, score, queries, tf=tf) == [
        b"1.5\tdir/b.txt", b"\tab=2 cd=0", b"0.30000000000000004\ta.txt", b"\tab=0 cd=1", b"", b"", b"-2.0\tc", b"\tx=5"]
    assert cli.render_passages(names, [0], [], [], []) == []


# ---- 5. refusals that need no device: decided before a handle is looked at, so two buffers of zeros stand in for them
def call(L, sp=(1, 2), ep=(2, 3), set_off=None, term_len=(2, 2), q_off=(0, 2), hit_off=(0, 1), hit_doc=(0,), weights=None,
         prm=None, cap=4, nulls=()):
    vp = ctypes.c_void_p
    fake_c, fake_i = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    u64 = lambda a: np.asarray(a, dtype=np.uint64)
    sp, ep, q_off, hit_off = u64(sp), u64(ep), u64(q_off), u64(hit_off)
    term_len, hit_doc = np.asarray(term_len, dtype=np.uint32), np.asarray(hit_doc, dtype=np.uint32)
    so = None if set_off is None else u64(set_off)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    out, tf = np.zeros(cap, dtype=np.dtype("V32")), np.zeros(cap * 64, dtype=np.uint32)
    stride = ctypes.c_uint32(99)
    prm = _lib.fmx_passage_params(160, 0, 0, 0) if prm is None else prm
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    args = {"corpus": ctypes.cast(fake_c, vp), "idx": ctypes.cast(fake_i, vp), "sp": p(sp), "ep": p(ep), "term_len": p(term_len),
            "q_off": p(q_off), "hit_off": p(hit_off), "hit_doc": p(hit_doc), "prm": ctypes.byref(prm), "out": p(out), "tf": p(tf),
            "stride": ctypes.byref(stride)}
    for k in nulls:
        args[k] = None
    rc = L.fmx_corpus_passages(args["corpus"], args["idx"], args["sp"], args["ep"], sp.size, p(so), term_len.size, args["term_len"],
                               args["q_off"], q_off.size - 1, args["hit_off"], args["hit_doc"], p(w), args["prm"], args["out"],
                               args["tf"], cap, args["stride"])
    return rc, L.fmx_last_error().decode()


def test_argument_refusals_need_no_device():
    L = _lib.load()
    P = _lib.fmx_passage_params
    for nulls in (("corpus",), ("idx",), ("sp",), ("ep",), ("term_len",), ("q_off",), ("hit_off",), ("hit_doc",), ("prm",), ("out",),
                  ("tf",), ("stride",)):
        rc, msg = call(L, nulls=nulls)
        assert rc == 3 and "null" in msg, nulls
    for prm, word in ((P(0, 0, 0, 0), "window"), (P(1 << 32, 0, 0, 0), "window"), (P(160, 0, 1, 0), "flags"), (P(160, 0, 0, 7), "flags")):
        rc, msg = call(L, prm=prm)
        assert rc == 3 and word in msg, (word, msg)
    for w in ([1.0, float("nan")], [float("inf"), 1.0], [1.0, float("-inf")]):
        rc, msg = call(L, weights=w)
        assert rc == 3 and "weights" in msg
    for tl in ([0, 2], [2, 0]):
        rc, msg = call(L, term_len=tl)
        assert rc == 3 and "term_len" in msg
    for bad in ([0, 2, 1], [1, 2, 3], [0, 1, 0]):                          # decreasing; not from 0
        rc, msg = call(L, sp=[1], ep=[2], term_len=[2], q_off=[0, 1, 1], hit_off=bad, hit_doc=[0, 0, 0])
        assert rc == 3 and "hit_off" in msg, bad
    rc, msg = call(L, sp=[1] * 65, ep=[2] * 65, term_len=[1] * 65, q_off=[0, 65])
    assert rc == 3 and "64" in msg
    for bad in ([0, 2, 1, 3], [1, 3], [0, 2], [0, 4]):                    # decreasing; not from 0; not up to n_terms (3 slots)
        rc, msg = call(L, sp=[1, 2, 3], ep=[2, 3, 4], term_len=[1, 1, 1], q_off=bad, hit_off=[0] * len(bad), hit_doc=[])
        assert rc == 3 and "q_off" in msg, bad
    for bad in ([1, 2, 3], [0, 2, 1], [0, 1, 2], [0, 1, 4]):              # not from 0; decreasing; not up to n_iv (3 intervals, 2 slots)
        rc, msg = call(L, sp=[1, 2, 3], ep=[2, 3, 4], set_off=bad, term_len=[2, 2])
        assert rc == 3 and "set_off" in msg, bad
    rc, msg = call(L, sp=[1, 2, 3], ep=[2, 3, 4], term_len=[2, 2])         # three intervals, two slots, no set_off
    assert rc == 3 and "set_off" in msg
