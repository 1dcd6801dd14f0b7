"""Lines without a device (fmx_lines_batch, fmx_occurrence_lines): tests/lines_ref.py against plain Python on
hand-worked texts, the layout of fmx_line_hit against a strict-C compile of the header, every refusal the calls decide on the
host, the "lines_shift" key, and the grep tool's new flags and formatting on canned records.  What needs a handle is in
tests/test_gpu_lines.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import corpus_ref
import lines_ref
import occ_ref
from conftest import ROOT
from findex_amd import _lib, grep

ARG = 3
FIELDS = ("group", "doc", "line_no", "start", "len", "n_hits", "raw_off", "raw_len", "first")
OFFSETS = [0, 4, 8, 16, 24, 28, 32, 40, 44]


def occ_of(per_group):
    """[positions] per group -> (off, OCC array)"""
    off = np.zeros(len(per_group) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in per_group])
    occ = np.zeros(int(off[-1]), dtype=occ_ref.OCC)
    occ["pos"] = [p for g in per_group for p in g]
    occ["group"] = [g for g, ps in enumerate(per_group) for _ in ps]
    occ["len"] = 1
    return off, occ


@pytest.mark.parametrize("text", (b"ab\ncd\n\nef", b"ab\ncd\n", b"\n\nx\n", b"x", b"\n"))
def test_reference_against_split(text):
    ref = lines_ref.Lines(text)
    pieces = text.split(b"\n")
    assert ref.n_brk + 1 == len(pieces) == text.count(b"\n") + 1
    at = 0
    for L, piece in enumerate(pieces):
        # the bytes of the line and the break that ends it are on line L
        for p in range(at, min(at + len(piece) + 1, len(text))):
            line, start, end = ref.lookup([p])
            assert (int(line[0]), int(start[0]), int(end[0])) == (L, at, at + len(piece)), (text, p)
        s, e = ref.spans([L])
        assert text[int(s[0]):int(e[0])] == piece
        at += len(piece) + 1
    assert all(int(x[0]) == 2 ** 64 - 1 for x in ref.lookup([len(text)]))
    assert all(int(x[0]) == 2 ** 64 - 1 for x in ref.spans([len(pieces)]))
    for shift in (4, 8):
        d = ref.directory(shift)
        assert d.size == (len(text) >> shift) + 2 and d[0] == 0 and d[-1] == ref.n_brk


def test_break_sets_of_several_bytes():
    text = b"a b\tc\r\nd"
    ref = lines_ref.Lines(text, b"\n\r \t")
    assert ref.brk.tolist() == [1, 3, 5, 6] and ref.line([0, 1, 2, 6, 7]).tolist() == [0, 0, 1, 3, 4]
    s, e = ref.spans(np.arange(6))
    assert [text[int(a):int(b)] for a, b in zip(s[:5], e[:5])] == [b"a", b"b", b"c", b"", b"d"] and int(s[5]) == 2 ** 64 - 1


def test_reduction_hand_worked():
    text = b"ab ab\nab\n\nxab"
    ref = lines_ref.Lines(text)
    ab = [i for i in range(len(text)) if text[i:i + 2] == b"ab"]
    assert ab == [0, 3, 6, 11]
    off, hits = lines_ref.occurrence_lines(ref, *occ_of([ab, [], [6, 11]]))
    assert off.tolist() == [0, 3, 3, 5]
    assert hits["group"].tolist() == [0, 0, 0, 2, 2] and hits["line_no"].tolist() == [1, 2, 4, 2, 4]
    assert hits["n_hits"].tolist() == [2, 1, 1, 1, 1] and hits["first"].tolist() == [0, 2, 3, 0, 1]
    pieces = text.split(b"\n")
    for h in hits[:3]:
        line = text[int(h["start"]):int(h["start"]) + int(h["len"])]
        assert line == pieces[int(h["line_no"]) - 1] and line.count(b"ab") == int(h["n_hits"])
    assert hits["doc"].tolist() == [0xFFFFFFFF] * 5 and np.array_equal(hits["raw_off"], hits["start"])
    assert lines_ref.python_grep([text], b"ab") == [(0, 1, b"ab ab"), (0, 2, b"ab"), (0, 4, b"xab")]


def test_reduction_hand_worked_corpus():
    docs = [b"ab\nxab", b"", b"a\x00b\nab\n", b"\n\n"]
    rc = corpus_ref.RefCorpus(docs)
    S = rc.stream
    assert S == b"ab\nxab\x01\x01a\\0b\nab\n\x01\n\n\x01"
    ref = lines_ref.Lines(S, b"\n\x01")
    ab = [i for i in range(len(S)) if S[i:i + 2] == b"ab"]
    b_ = [i for i in range(len(S)) if S[i:i + 1] == b"b"]
    off, hits = lines_ref.occurrence_lines(ref, *occ_of([ab, b_]), docs=rc)
    got = [(int(h["doc"]), int(h["line_no"]), docs[int(h["doc"])][int(h["raw_off"]):int(h["raw_off"]) + int(h["raw_len"])])
           for h in hits]
    assert got[:int(off[1])] == lines_ref.python_grep(docs, b"ab") == [(0, 1, b"ab"), (0, 2, b"xab"), (2, 2, b"ab")]
    assert got[int(off[1]):] == lines_ref.python_grep(docs, b"b")
    esc = hits[int(off[1]):][2]                              # a\0b: four stream bytes, three raw ones
    assert (int(esc["len"]), int(esc["raw_len"])) == (4, 3)
    assert [lines_ref.wc_l(d) for d in docs] == [2, 0, 2, 2]


def test_struct_layout():
    assert ctypes.sizeof(_lib.fmx_line_hit) == 48
    assert [getattr(_lib.fmx_line_hit, f).offset for f in FIELDS] == OFFSETS
    import findex_amd
    D = findex_amd.HipFMSearcher.LINE_HIT
    assert D.itemsize == 48 and D == lines_ref.LINE_HIT and [D.fields[f][1] for f in FIELDS] == OFFSETS
    assert _lib.FMX_PREPARE_LINES == 256


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_struct_layout_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d\", (int)sizeof(fmx_line_hit));\n"
        + "".join("  printf(\" %%d\", (int)offsetof(fmx_line_hit, %s));\n" % f for f in FIELDS) +
        "  printf(\" %d\\n\", (int)FMX_PREPARE_LINES);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["48"] + [str(o) for o in OFFSETS] + ["256"]


def test_abi_version_stats_size_and_the_flag_stay():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    assert re.search(r"FMX_PREPARE_LINES\s*=\s*256\b", code)


def test_lines_shift_takes_its_values_and_refuses_others():
    L = _lib.load()
    try:
        for v in (b"4", b"16", b"10"):
            assert L.fmx_config_set(b"lines_shift", v) == 0, v
        for v in (b"3", b"17", b"-1", b"x", b""):
            assert L.fmx_config_set(b"lines_shift", v) == ARG, v
            assert b"lines_shift" in L.fmx_last_error()
        assert L.fmx_index_config_set(None, b"lines_shift", b"6") == ARG
    finally:
        assert L.fmx_config_set(b"lines_shift", b"6") == 0           # the default


def test_argument_refusals_before_any_device():
    """What the arguments alone decide comes before the handle is looked at, and the null handle is refused last with a
    message of its own: without a GPU each refusal still shows by its message."""
    L = _lib.load()
    vp = ctypes.c_void_p

    def prepare(b):
        a = np.frombuffer(b, dtype=np.uint8)
        return L.fmx_lines_prepare(None, a.ctypes.data if a.size else None, a.size)

    for b, word in ((b"\n\r \t\x0b", b"at most 4"), (b"\n \n", b"repeated"), (b"\n\x00", b"byte 0"), (b"\n", b"handle"),
                    (b"", b"handle"), (b"\n\x01 \t", b"handle")):
        assert prepare(b) == ARG and word in L.fmx_last_error(), (b, L.fmx_last_error())
    pos = np.zeros(4, dtype=np.uint64)
    for call in (lambda: L.fmx_lines_batch(None, vp(pos.ctypes.data), 4, None, None, None),
                 lambda: L.fmx_lines_batch_dev(None, vp(pos.ctypes.data), 4, None, None, None, None),
                 lambda: L.fmx_line_spans(None, vp(pos.ctypes.data), 4, None, None),
                 lambda: L.fmx_line_spans_dev(None, vp(pos.ctypes.data), 4, None, None, None),
                 lambda: L.fmx_lines_info(None, None, None, None, None, None, None)):
        assert call() == ARG and L.fmx_last_error()
    assert L.fmx_prepare(None, 256) == ARG and L.fmx_drop_tables(None, 256) == ARG

    n_out = ctypes.c_size_t(77)
    off, occ = occ_of([[1, 2], [3]])
    out_off = np.full(3, 99, dtype=np.uint64)
    out = np.zeros(4, dtype=lines_ref.LINE_HIT)

    def ptr(a):
        return vp(a.ctypes.data) if a is not None else None

    def host(io=off, r=occ, g=2, cap=4, n=n_out, oo=out_off, o=out):
        return L.fmx_occurrence_lines(None, None, ptr(io), ptr(r), g, ptr(oo), ptr(o), cap, ctypes.byref(n) if n is not None else None)

    def dev(io=off, r=occ, g=2, cap=4, n=n_out, oo=out_off, o=out, k=3):
        return L.fmx_occurrence_lines_dev(None, None, ptr(io), ptr(r), k, g, ptr(oo), ptr(o), cap,
                                          ctypes.byref(n) if n is not None else None, None)

    cases = [(dict(), b"handle"), (dict(n=None), b"n_out"), (dict(oo=None), b"out_off"), (dict(io=None), b"occ_off"),
             (dict(g=0), b"n_groups"), (dict(g=(1 << 26) + 1), b"n_groups"), (dict(cap=1 << 32), b"2^32"),
             (dict(r=None), b"records are null"), (dict(o=None), b"out is null")]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
        assert form(o=None, cap=0) == ARG and b"handle" in L.fmx_last_error()                 # the counting call's shape is fine
    assert dev(k=(1 << 26) + 1) == ARG and b"2^26 records" in L.fmx_last_error()
    assert host(io=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(io=np.array([1, 2, 3], dtype=np.uint64)) == ARG and b"begin at 0" in L.fmx_last_error()
    assert n_out.value == 77 and out_off.tolist() == [99, 99, 99]      # a refused call writes nothing
    t = [ctypes.c_double(-1) for _ in range(4)]
    assert L.fmx_lines_last(*[ctypes.byref(x) for x in t]) == 0 and all(x.value >= 0 for x in t)
    assert L.fmx_lines_last(None, None, None, None) == 0


# ---------------------------------------------------------------- the grep tool
def test_grep_parser_new_flags():
    P = grep.parser().parse_args
    a = P(["B", "ab"])
    assert not grep.by_lines(a) and (a.context, a.count, a.max_line) == (0, False, 4096)
    a = P(["B", "ab", "-C", "8", "--count"])                 # the old flags keep their meaning
    assert not grep.by_lines(a) and a.context == 8 and a.count
    for argv, ctx in ((["-n"], (0, 0)), (["--line-number"], (0, 0)), (["-A", "2"], (0, 2)), (["-B", "3"], (3, 0)),
                      (["--context-lines", "1"], (1, 1)), (["--context-lines", "2", "-A", "0"], (2, 0)), (["-c"], (0, 0)),
                      (["--count-lines"], (0, 0)), (["-l"], (0, 0)), (["--files-with-matches"], (0, 0))):
        a = P(["B", "ab"] + argv)
        assert grep.by_lines(a) and grep.context_of(a) == ctx, argv
    assert P(["B", "ab", "-n", "--max-line", "80"]).max_line == 80
    assert not grep.by_lines(P(["B", "ab", "--max-line", "80"]))


def canned(rows):
    hits = np.zeros(len(rows), dtype=lines_ref.LINE_HIT)
    for h, (doc, no) in zip(hits, rows):
        h["doc"], h["line_no"] = doc, no
    return hits


NAMES = [b"a.txt", b"dir/b.txt", b"c"]


def test_grep_formatting_of_lines_counts_and_files():
    hits = canned([(0, 1), (0, 7), (2, 3)])
    lines = [b"one", b"seven:x", b""]
    assert grep.format_lines(NAMES, hits, lines) == [b"a.txt:1:one", b"a.txt:7:seven:x", b"c:3:"]
    assert grep.format_lines(NAMES, hits, lines, number=False) == [b"a.txt:one", b"a.txt:seven:x", b"c:"]
    assert grep.format_counts(NAMES, hits) == [b"a.txt:2", b"c:1"]
    assert grep.format_files(NAMES, hits) == [b"a.txt", b"c"]
    assert grep.format_lines(NAMES, hits[:0], []) == [] and grep.format_counts(NAMES, hits[:0]) == []


def test_grep_formatting_of_context_merges_groups():
    # file 0 has 12 lines "L1" .. "L12"; hits on 2, 4, 5 and 10 with one line of context on both sides; a hit in file 2
    text = {n: b"L%d" % n for n in range(1, 13)}
    rows = [(0, 2), (0, 4), (0, 5), (0, 10), (2, 1)]
    hits = canned(rows)
    lines = [text[n] for _, n in rows[:4]] + [b"only"]
    ctx = [([text[n - 1]], [text[n + 1]]) for _, n in rows[:4]] + [([], [b"next"])]
    got = grep.format_context(NAMES, hits, lines, ctx)
    assert got == [b"a.txt-1-L1", b"a.txt:2:L2", b"a.txt-3-L3", b"a.txt:4:L4", b"a.txt:5:L5", b"a.txt-6-L6", b"--",
                   b"a.txt-9-L9", b"a.txt:10:L10", b"a.txt-11-L11", b"--", b"c:1:only", b"c-2-next"]
    # groups that touch (3 | 4) merge without a separator; a gap of one line does not
    got = grep.format_context(NAMES, canned([(0, 2), (0, 5)]), [b"L2", b"L5"], [([b"L1"], [b"L3"]), ([b"L4"], [b"L6"])], number=False)
    assert got == [b"a.txt-L1", b"a.txt:L2", b"a.txt-L3", b"a.txt-L4", b"a.txt:L5", b"a.txt-L6"]
    got = grep.format_context(NAMES, canned([(0, 2), (0, 6)]), [b"L2", b"L6"], [([b"L1"], [b"L3"]), ([b"L5"], [b"L7"])])
    assert got == [b"a.txt-1-L1", b"a.txt:2:L2", b"a.txt-3-L3", b"--", b"a.txt-5-L5", b"a.txt:6:L6", b"a.txt-7-L7"]
    assert grep.format_context(NAMES, hits[:0], [], []) == []
