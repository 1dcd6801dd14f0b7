"""Ranked retrieval without a device: the checker (tests/rank_ref.py) against a hand-worked example, the host arithmetic of
findex_amd/csrc/fmx_rank_math.h under AddressSanitizer + UBSan (tests/native/rank_math.cpp), the command line's parsing and
rendering, and every refusal fmx_corpus_rank decides before it touches a handle or the device."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import corpus_ref
import rank_ref
from conftest import ROOT
from findex_amd import _lib


# ---- 1. the checker, by hand.  Three documents of 6, 2 and 4 raw bytes: N = 3, avglen = 4.  k1 = 1.2, b = 0.75.
#   "ab": tf 2 in d0, 1 in d1; df 2; w = log(1 + 1.5 / 2.5) = log 1.6
#         d0: r = 1.5, nd = 1.2 (0.25 + 1.125) = 1.65, c = w (2 * 2.2 / 3.65)
#         d1: r = 0.5, nd = 1.2 (0.25 + 0.375) = 0.75, c = w (2.2 / 1.75)
#   "cd": tf 2 in d2; df 1; w = log(1 + 2.5 / 1.5); d2: r = 1, nd = 1.2, c = w (4.4 / 3.2)
W_AB, W_CD = 0.47000362924573563, 0.9808292530117263
S_D0, S_D1, S_D2 = 0.5665797174469143, 0.5908617053374963, 1.3486402228911236


@pytest.fixture(scope="module")
def three():
    return rank_ref.RankRef(corpus_ref.RefCorpus([b"ab abx", b"ab", b"cdcd"]))


def test_checker_against_a_hand_worked_example(three):
    r = three
    assert r.avglen == 4.0 and r.raw_len == [6, 2, 4]
    assert r.tf(b"ab") == {0: 2, 1: 1} and r.tf(b"cd") == {2: 2} and r.tf(b"zz") == {}
    assert r.weights(r.postings([[b"ab", b"cd", b"zz"]])) == pytest.approx([W_AB, W_CD, math.log(1.0 + 3.5 / 0.5)], rel=1e-15)
    off, doc, score = r.rank_queries([[b"ab"], [b"ab", b"cd"], [b"cd", b"cd"], [], [b"zz"]])
    assert off == [0, 2, 5, 6, 6, 6]
    assert doc == [1, 0, 2, 1, 0, 2]                                      # the shorter file wins "ab"; a term twice counts twice
    assert score == pytest.approx([S_D1, S_D0, S_D2, S_D1, S_D0, 2 * S_D2], rel=1e-15)
    # top cuts; all-of needs every slot
    assert r.rank_queries([[b"ab", b"cd"]], top=1)[1] == [2]
    assert r.rank_queries([[b"ab", b"cd"]], match="all") == ([0, 0], [], [])
    off, doc, score = r.rank_queries([[b"ab", b"b"]], match="all")
    assert doc == [1, 0] and score == pytest.approx([2 * S_D1, 2 * S_D0], rel=1e-15)
    # caller weights, negative ones included: the order turns round; equal scores go by document
    assert r.rank_queries([[b"ab"]], weights=[-1.0])[1] == [0, 1]
    assert r.rank_queries([[b"ab", b"cd"]], weights=[0.0, 0.0]) == ([0, 3], [0, 1, 2], [0.0, 0.0, 0.0])


def test_checker_counts_overlaps_and_escapes():
    r = rank_ref.RankRef(corpus_ref.RefCorpus([b"aaaa", b"", b"x\x00\x00y\xff", b"aa"]))
    assert r.tf(b"aa") == {0: 3, 3: 1}
    assert r.tf(b"\x00") == {2: 2} and r.tf(b"\xff") == {2: 1} and r.tf(b"\x00\x00") == {2: 1}
    assert r.raw_len == [4, 0, 5, 2] and r.avglen == 11.0 / 4.0


# ---- 2. the key map, its inverse and the weight formula, under the sanitizers
@pytest.mark.timeout(300)
def test_rank_math_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "rank_math"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "findex_amd", "csrc"), os.path.join(ROOT, "tests", "native", "rank_math.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "error:" not in build.stderr:
        pytest.skip("sanitizer runtime not available: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=200)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "rank math ok" in run.stdout


# ---- 3. the command line
def test_cli_parses_and_renders():
    from findex_amd import rank as cli
    a = cli.parser().parse_args(["base", "two words", " another\tquery  here ", "--top", "3", "--all", "--k1", "0.9", "--b", "0"])
    assert (a.base, a.top, a.all_, a.k1, a.b, a.device, a.little_endian) == ("base", 3, True, 0.9, 0.0, 0, False)
    assert cli.split_queries(a.query) == [[b"two", b"words"], [b"another", b"query", b"here"]]
    d = cli.parser().parse_args(["base", "q"])
    assert (d.top, d.all_, d.k1, d.b) == (10, False, 1.2, 0.75)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["base"])                                 # no query
    with pytest.raises(SystemExit):
        cli.main(["base", "q", "--top", "0"])
    assert "substring" in cli.parser().format_help()
    names = [b"a.txt", b"dir/b.txt", b"c"]
    rows = cli.render(names, [0, 2, 2, 3], [1, 0, 2], [1.5, 0.1 + 0.2, -2.0])
    assert rows == [b"1.5\tdir/b.txt", b"0.30000000000000004\ta.txt", b"", b"", b"-2.0\tc"]
    assert cli.render(names, [0], [], []) == []


# ---- 4. refusals that need no device: decided before a handle is looked at, so two buffers of zeros stand in for them
def call(L, corpus, idx, sp, ep, q_off, prm, weights=None, cap=16, nulls=()):
    vp = ctypes.c_void_p
    sp, ep, q_off = (np.asarray(a, dtype=np.uint64) for a in (sp, ep, q_off))
    off = np.zeros(q_off.size, dtype=np.uint64)
    doc, score = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.float64)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    args = {"corpus": corpus, "idx": idx, "sp": sp.ctypes.data_as(vp), "ep": ep.ctypes.data_as(vp), "q_off": q_off.ctypes.data_as(vp),
            "prm": ctypes.byref(prm) if prm is not None else None, "w": None if w is None else w.ctypes.data_as(vp),
            "off": off.ctypes.data_as(vp), "doc": doc.ctypes.data_as(vp), "score": score.ctypes.data_as(vp)}
    for k in nulls:
        args[k] = None
    rc = L.fmx_corpus_rank(args["corpus"], args["idx"], args["sp"], args["ep"], sp.size, args["q_off"], q_off.size - 1, args["prm"],
                           args["w"], args["off"], args["doc"], args["score"], cap, None, None)
    return rc, L.fmx_last_error().decode()


def test_argument_refusals_need_no_device():
    L = _lib.load()
    assert ctypes.sizeof(_lib.fmx_rank_params) == 32
    fake_c, fake_i = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    c, i = ctypes.cast(fake_c, ctypes.c_void_p), ctypes.cast(fake_i, ctypes.c_void_p)
    P = _lib.fmx_rank_params
    good = P(1.2, 0.75, 0, 10, 0)
    sp, ep, q_off = [1, 2], [2, 3], [0, 2]
    for nulls in (("corpus",), ("idx",), ("sp",), ("ep",), ("q_off",), ("prm",), ("off",), ("doc",), ("score",)):
        rc, msg = call(L, c, i, sp, ep, q_off, good, nulls=nulls)
        assert rc == 3 and "null" in msg, nulls
    for prm, word in ((P(1.2, 0.75, 0, 0, 0), "top"), (P(1.2, 0.75, 0, 1025, 0), "top"), (P(1.2, 1.5, 0, 10, 0), "b must"),
                      (P(1.2, -0.1, 0, 10, 0), "b must"), (P(1.2, float("nan"), 0, 10, 0), "b must"), (P(-1.0, 0.75, 0, 10, 0), "k1"),
                      (P(float("inf"), 0.75, 0, 10, 0), "k1"), (P(1.2, 0.75, 0, 10, 2), "flag")):
        rc, msg = call(L, c, i, sp, ep, q_off, prm)
        assert rc == 3 and word in msg, (word, msg)
    for w in ([1.0, float("nan")], [float("inf"), 1.0], [1.0, float("-inf")]):
        rc, msg = call(L, c, i, sp, ep, q_off, good, weights=w)
        assert rc == 3 and "weights" in msg
    rc, msg = call(L, c, i, [1] * 65, [2] * 65, [0, 65], good)
    assert rc == 3 and "64" in msg
    for bad in ([0, 2, 1, 3], [1, 3], [0, 2], [0, 4]):                    # decreasing; not from 0; not up to n_terms (3 slots)
        rc, msg = call(L, c, i, [1, 2, 3], [2, 3, 4], bad, good)
        assert rc == 3 and "q_off" in msg, bad
