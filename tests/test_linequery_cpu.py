"""Line queries without a device (fmx_line_query): tests/linequery_ref.py against plain Python run file by file,
hand-worked texts, the layout of fmx_line_term against a strict-C compile of the header, every refusal the calls decide on the
host, and the grep tool's query flags on canned records.  What needs a handle is in tests/test_gpu_linequery.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lines_ref
import linequery_ref as ref
from conftest import ROOT
from findex_amd import _lib, grep

ARG = 3
FIELDS = ("group", "window", "flags", "reserved")


# ---------------------------------------------------------------- the reference against Python, file by file
def corpus_results(docs):
    (off, hits), S, rc = ref.hits_of_needles(docs, ref.WORDS)
    number = {w: i for i, w in enumerate(ref.WORDS)}
    named = ref.five_queries()
    queries = [(None if a is None else number[a], [(number[n], w, neg) for n, w, neg in terms]) for _, a, terms in named]
    qoff, out = ref.line_query(off, hits, queries, lines=S, docs=rc)
    return named, (off, hits), (qoff, out)


def test_reference_against_python_file_by_file():
    docs = ref.seeded_corpus(7)
    assert len(docs) == 37 and docs[3] == b"" and docs[11] == b"\n" and not docs[20].endswith(b"\n")
    assert max(lines_ref.wc_l(d) for d in docs) <= 40
    named, (off, hits), (qoff, out) = corpus_results(docs)
    sizes = []
    for q, (name, a, terms) in enumerate(named):
        got = out[int(qoff[q]):int(qoff[q + 1])]
        want = ref.python_query(docs, a, terms)
        assert [(int(h["doc"]), int(h["line_no"])) for h in got] == [(d, no) for d, no, _ in want], name
        assert [int(h["raw_len"]) for h in got] == [len(t) for _, _, t in want], name
        assert (got["group"] == q).all()
        sizes.append(len(want))
    # with seed 7: 684 real lines; none of the five results is empty
    assert sum(lines_ref.wc_l(d) for d in docs) == 684 and sizes == [36, 109, 539, 90, 48]
    inverted = out[int(qoff[2]):int(qoff[3])]
    assert (inverted["n_hits"] == 0).all() and (inverted["first"] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("seed", (7, 1, 2))
def test_inverted_and_plain_make_up_every_line(seed):
    docs = ref.seeded_corpus(seed)
    (off, hits), S, rc = ref.hits_of_needles(docs, ref.WORDS)
    qoff, out = ref.line_query(off, hits, [(None, [(0, 0, True)]), (0, []), (None, [])], lines=S, docs=rc)
    total = sum(lines_ref.wc_l(d) for d in docs)
    assert int(qoff[1]) + int(qoff[2] - qoff[1]) == total == int(qoff[3] - qoff[2])
    plain = hits[int(off[0]):int(off[1])].copy()
    plain["group"] = 1                                       # a query without terms returns its candidates, under its own index
    assert out[int(qoff[1]):int(qoff[2])].tobytes() == plain.tobytes()
    every = out[int(qoff[2]):]
    assert [(int(h["doc"]), int(h["line_no"])) for h in every] == [(d, i + 1) for d, raw in enumerate(docs) for i in range(lines_ref.wc_l(raw))]


# ---------------------------------------------------------------- hand-worked texts
def plain_hits(text, needles):
    """(off, hits) of literal needles over a plain text (no corpus)."""
    S = lines_ref.Lines(text)
    occ = np.dtype([("group", np.uint32), ("len", np.uint32), ("pos", np.uint64), ("doc", np.uint32), ("raw_len", np.uint32),
                    ("raw_off", np.uint64)])
    off, recs = [0], []
    for needle in needles:
        pos = [i for i in range(len(text)) if text.startswith(needle, i)]
        r = np.zeros(len(pos), dtype=occ)
        r["pos"] = pos
        recs.append(r)
        off.append(off[-1] + len(pos))
    return lines_ref.occurrence_lines(S, np.array(off, dtype=np.uint64), np.concatenate(recs)), S


def test_hand_worked_texts():
    # four lines, the third empty and real, the last unterminated
    (off, hits), S = plain_hits(b"ab\ncd\n\nef", [b"b", b"d", b"f", b"zz"])
    every = ref.real_lines(S)
    assert every["line_no"].tolist() == [1, 2, 3, 4] and every["start"].tolist() == [0, 3, 6, 7] and every["len"].tolist() == [2, 2, 0, 2]
    assert (every["doc"] == 0xFFFFFFFF).all() and every["raw_off"].tolist() == [0, 3, 6, 7]

    def lines(queries):
        qoff, out = ref.line_query(off, hits, queries, lines=S)
        return [out["line_no"][int(qoff[q]):int(qoff[q + 1])].tolist() for q in range(len(queries))]

    assert lines([(None, [(0, 0, True)])]) == [[2, 3, 4]]                              # -v b
    assert lines([(None, [(3, 0, True)]), (None, [])]) == [[1, 2, 3, 4]] * 2            # -v of an empty group; no terms
    assert lines([(0, [(1, 1, False)]), (0, [(1, 0, False)]), (0, [(2, 2, False)]), (0, [(2, "file", False)])]) == [[1], [], [], [1]]
    assert lines([(2, [(0, 3, False), (1, 2, False)]), (2, [(0, 2, False)]), (1, [(0, 1, False), (2, 1, True)])]) == [[4], [], [2]]
    assert lines([(0, [(0, 0, False)]), (0, [(0, 0, True)])]) == [[1], []]              # A and A is A, A not A is empty
    # the piece behind the final newline is no line
    (off, hits), S = plain_hits(b"ab\ncd\n", [b"b"])
    assert ref.real_lines(S)["line_no"].tolist() == [1, 2]
    qoff, out = ref.line_query(off, hits, [(None, [(0, 0, True)])], lines=S)
    assert out["line_no"].tolist() == [2] and out["start"].tolist() == [3] and qoff.tolist() == [0, 1]
    assert ref.real_lines(lines_ref.Lines(b"")).size == 0 and ref.real_lines(lines_ref.Lines(b"\n"))["len"].tolist() == [0]
    # lower saturation: a window larger than the line number begins at line 1; the upper end at 2^32 - 1
    keys = np.array([(0xFFFFFFFF << 32) | 1], dtype=np.uint64)
    assert ref.satisfies((0xFFFFFFFF << 32) | 2, keys, 5) and not ref.satisfies((0xFFFFFFFF << 32) | 3, keys, 1)
    assert ref.satisfies((0xFFFFFFFF << 32) | 3, keys, 0xFFFFFFFF) and not ref.satisfies((7 << 32) | 1, keys, 0xFFFFFFFF)


# ---------------------------------------------------------------- the ABI
def test_term_layout_and_constants():
    assert ctypes.sizeof(_lib.fmx_line_term) == 16
    assert [getattr(_lib.fmx_line_term, f).offset for f in FIELDS] == [0, 4, 8, 12]
    import findex_amd
    D = findex_amd.HipFMSearcher.LINE_TERM
    assert D.itemsize == 16 and [D.fields[f][1] for f in FIELDS] == [0, 4, 8, 12]
    assert _lib.FMX_LQ_ALL_LINES == 0xFFFFFFFF and _lib.FMX_LQ_NOT == 1 and findex_amd.HipFMSearcher.ALL_LINES is None


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_term_layout_against_a_strict_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <fmx.h>\n"
        "int main(void) {\n"
        "  printf(\"%d\", (int)sizeof(fmx_line_term));\n"
        + "".join("  printf(\" %%d\", (int)offsetof(fmx_line_term, %s));\n" % f for f in FIELDS) +
        "  printf(\" %lu %lu\\n\", (unsigned long)FMX_LQ_ALL_LINES, (unsigned long)FMX_LQ_NOT);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == ["16", "0", "4", "8", "12", str(0xFFFFFFFF), "1"]


def test_abi_version_and_stats_size_stay():
    assert _lib.load().fmx_abi_version() == 5
    assert ctypes.sizeof(_lib.fmx_stats_t) == 232


def test_lq_narrow_takes_on_and_off():
    L = _lib.load()
    try:
        assert L.fmx_config_set(b"lq_narrow", b"off") == 0 and L.fmx_config_set(b"lq_narrow", b"on") == 0
        for v in (b"1", b"", b"ON"):
            assert L.fmx_config_set(b"lq_narrow", v) == ARG and b"lq_narrow" in L.fmx_last_error(), v
        assert L.fmx_index_config_set(None, b"lq_narrow", b"on") == ARG
    finally:
        assert L.fmx_config_set(b"lq_narrow", b"off") == 0              # the default


def test_argument_refusals_before_any_device():
    """What the arguments alone decide comes before the handle is looked at, and the null handle is refused last with a
    message of its own: without a GPU each refusal still shows by its message."""
    L = _lib.load()
    vp = ctypes.c_void_p
    hits = np.zeros(3, dtype=lines_ref.LINE_HIT)
    hits["doc"], hits["line_no"] = 0xFFFFFFFF, [1, 2, 2]
    hit_off = np.array([0, 2, 3], dtype=np.uint64)
    q_off = np.array([0, 1, 2], dtype=np.uint64)
    anchor = np.array([0, 0xFFFFFFFF], dtype=np.uint32)
    terms = np.zeros(2, dtype=np.dtype(_lib.fmx_line_term))
    terms["group"], terms["window"], terms["flags"] = [1, 0], [0, 0xFFFFFFFF], [0, 1]
    n_out = ctypes.c_size_t(77)
    out_off = np.full(3, 99, dtype=np.uint64)
    out = np.zeros(4, dtype=lines_ref.LINE_HIT)
    out["line_no"] = 5

    def ptr(a):
        return vp(a.ctypes.data) if a is not None else None

    def host(ho=hit_off, r=hits, g=2, qo=q_off, an=anchor, t=terms, nq=2, oo=out_off, o=out, cap=4, n=n_out, k=None):
        return L.fmx_line_query(None, None, ptr(ho), ptr(r), g, ptr(qo), ptr(an), ptr(t), nq, ptr(oo), ptr(o), cap,
                                ctypes.byref(n) if n is not None else None)

    def dev(ho=hit_off, r=hits, g=2, qo=q_off, an=anchor, t=terms, nq=2, oo=out_off, o=out, cap=4, n=n_out, k=3):
        return L.fmx_line_query_dev(None, None, ptr(ho), ptr(r), k, g, ptr(qo), ptr(an), ptr(t), nq, ptr(oo), ptr(o), cap,
                                    ctypes.byref(n) if n is not None else None, None)

    def term(**kw):
        t = terms.copy()
        for f, v in kw.items():
            t[f][1] = v
        return t

    many = np.zeros(65, dtype=terms.dtype)
    wide_off = np.zeros((1 << 16) + 2, dtype=np.uint64)
    cases = [(dict(), b"handle is null"), (dict(n=None), b"n_out"), (dict(oo=None), b"out_off"), (dict(ho=None), b"hit_off"),
             (dict(qo=None), b"q_off"), (dict(an=None), b"anchor"), (dict(t=None), b"terms is null"),
             (dict(g=0), b"n_groups"), (dict(g=(1 << 26) + 1), b"n_groups"),
             (dict(nq=0), b"n_queries"), (dict(nq=(1 << 16) + 1, qo=wide_off), b"n_queries"),
             (dict(qo=np.array([0, 65], dtype=np.uint64), nq=1, t=many), b"at most 64 terms"),
             (dict(qo=np.array([1, 1, 2], dtype=np.uint64)), b"begin at 0"), (dict(qo=np.array([0, 2, 1], dtype=np.uint64)), b"non-decreasing"),
             (dict(an=np.array([2, 0], dtype=np.uint32)), b"anchor names no group"), (dict(t=term(group=2)), b"term names no group"),
             (dict(t=term(flags=2)), b"unknown bits"), (dict(t=term(flags=3)), b"unknown bits"), (dict(t=term(reserved=1)), b"reserved"),
             (dict(cap=1 << 32), b"2^32"), (dict(r=None), b"records are null"), (dict(o=None), b"out is null")]
    for form in (host, dev):
        for kw, word in cases:
            assert form(**kw) == ARG, (form.__name__, kw)
            assert word in L.fmx_last_error(), (form.__name__, kw, L.fmx_last_error())
        assert form(o=None, cap=0) == ARG and b"handle is null" in L.fmx_last_error()           # the counting call's shape is fine
        assert form(qo=np.array([0, 0, 0], dtype=np.uint64), t=None) == ARG and b"handle is null" in L.fmx_last_error()
    assert dev(k=(1 << 26) + 1) == ARG and b"2^26 hit records" in L.fmx_last_error()
    assert host(ho=np.array([0, 3, 2], dtype=np.uint64)) == ARG and b"non-decreasing" in L.fmx_last_error()
    assert host(ho=np.array([1, 2, 3], dtype=np.uint64)) == ARG and b"begin at 0" in L.fmx_last_error()
    for line_nos in ([2, 1, 2], [2, 2, 2], [0, 1, 2]):
        bad = hits.copy()
        bad["line_no"] = line_nos
        assert host(r=bad) == ARG and b"do not ascend" in L.fmx_last_error(), line_nos
    bad = hits.copy()
    bad["doc"] = [1, 0, 0]
    assert host(r=bad) == ARG and b"do not ascend" in L.fmx_last_error()
    # a refused call writes nothing
    assert n_out.value == 77 and out_off.tolist() == [99, 99, 99] and (out["line_no"] == 5).all()
    t = [ctypes.c_double(-1) for _ in range(3)]
    n = [ctypes.c_uint64(7) for _ in range(2)]
    assert L.fmx_line_query_last(*[ctypes.byref(x) for x in t + n]) == 0 and all(x.value >= 0 for x in t)
    assert L.fmx_line_query_last(None, None, None, None, None) == 0


def test_python_query_lists():
    import findex_amd
    q_off, anchor, terms = findex_amd.HipFMSearcher._line_queries([(None, [(1, 0, True)]), (0, [(1, "file", False), (2, 3, True)]), (2, [])])
    assert q_off.tolist() == [0, 1, 3, 3] and anchor.tolist() == [0xFFFFFFFF, 0, 2]
    assert terms.tolist() == [(1, 0, 1, 0), (1, 0xFFFFFFFF, 0, 0), (2, 3, 1, 0)]
    for bad in ([(-1, [])], [(0, [(0, -1, False)])], [(0, [(0, "line", False)])], [(0, [(2 ** 32, 0, False)])]):
        with pytest.raises(ValueError):
            findex_amd.HipFMSearcher._line_queries(bad)


# ---------------------------------------------------------------- the grep tool
def test_grep_parser_query_flags():
    P = grep.parser().parse_args
    for argv in (["-v"], ["--invert-match"], ["--and", "x"], ["--not", "x"], ["--near", "2"], ["--same-file"]):
        a = P(["B", "ab"] + argv)
        assert grep.by_lines(a) and grep.where(a) and grep.context_of(a) == (0, 0), argv
    with pytest.raises(SystemExit):
        P(["B", "ab", "--near", "1", "--same-file"])
    for bad in ([], ["-1"], ["x"], [str(2 ** 32)]):
        with pytest.raises(SystemExit):
            P(["B", "ab", "--near"] + bad)
    # the old argument lists give what they gave
    a = P(["B", "ab"])
    assert not grep.by_lines(a) and not grep.where(a) and (a.context, a.count, a.max_line) == (0, False, 4096)
    a = P(["B", "ab", "-C", "8", "--count"])
    assert not grep.by_lines(a) and a.context == 8 and a.count
    for argv, ctx in ((["-n"], (0, 0)), (["-A", "2"], (0, 2)), (["-B", "3"], (3, 0)), (["--context-lines", "1"], (1, 1)), (["-c"], (0, 0)),
                      (["-l"], (0, 0))):
        a = P(["B", "ab"] + argv)
        assert grep.by_lines(a) and not grep.where(a) and grep.context_of(a) == ctx, argv
        assert (a.invert_match, a.and_, a.not_, a.near, a.same_file) == (False, [], [], None, False)
    # the queries
    a = P(["B", "ab", "cd", "--and", "x", "--not", "y", "--and", "z", "--near", "2"])
    assert grep.queries_of(a) == [(r, [("x", 2, False), ("z", 2, False), ("y", 2, True)]) for r in ("ab", "cd")]
    a = P(["B", "ab", "--and", "x", "--same-file", "-l"])
    assert grep.queries_of(a) == [("ab", [("x", "file", False)])] and a.files_with_matches
    a = P(["B", "ab", "cd", "-v", "--not", "y"])
    assert grep.queries_of(a) == [(None, [("ab", 0, True), ("y", 0, True)]), (None, [("cd", 0, True), ("y", 0, True)])]
    assert grep.queries_of(P(["B", "ab", "-v"])) == [(None, [("ab", 0, True)])]


class CannedSearcher:
    """What main_lines asks of a HipCorpusSearcher, answered from canned records of an inverted match."""

    class corpus:
        names = [b"a.txt", b"b.txt"]

    text = {(0, 1): b"one", (0, 2): b"two", (0, 3): b"three", (0, 4): b"four", (1, 1): b"only"}
    rows = [(0, 2), (0, 4), (1, 1)]

    def __init__(self):
        self.asked = []

    def grep_lines(self, *a, **kw):
        raise AssertionError("a line query goes through grep_lines_where")

    def grep_lines_where(self, queries, mode="disjoint", max_steps=0, max_per=None, text=False, before=0, after=0, lineOnly=False,
                         max_line=None):
        self.asked.append(queries)
        hits = np.zeros(len(self.rows), dtype=lines_ref.LINE_HIT)
        hits["doc"], hits["line_no"] = [d for d, _ in self.rows], [n for _, n in self.rows]
        hits["first"] = 0xFFFFFFFF
        off = np.array([0, len(self.rows)], dtype=np.uint64)
        if not (text or before or after):
            return off, hits, False
        lines = [self.text[r] for r in self.rows]
        if not (before or after):
            return off, hits, False, lines
        ctx = [([self.text[(d, n - i)] for i in range(min(before, n - 1), 0, -1)],
                [self.text[(d, n + i)] for i in range(1, after + 1) if (d, n + i) in self.text]) for d, n in self.rows]
        return off, hits, False, lines, ctx


@pytest.mark.parametrize("flags, want", (
    (["-v", "-c"], [b"a.txt:2", b"b.txt:1"]),
    (["-v", "-l"], [b"a.txt", b"b.txt"]),
    (["-v", "-n"], [b"a.txt:2:two", b"a.txt:4:four", b"b.txt:1:only"]),
    (["-v"], [b"a.txt:two", b"a.txt:four", b"b.txt:only"]),
    (["-v", "-A", "1"], [b"a.txt:two", b"a.txt-three", b"a.txt:four", b"--", b"b.txt:only"])), ids=("vc", "vl", "vn", "v", "vA"))
def test_grep_inverted_output_through_the_formatters(flags, want):
    import io
    cs, out = CannedSearcher(), io.BytesIO()
    a = grep.parser().parse_args(["B", "x"] + flags)
    assert grep.main_lines(cs, a, out) is False
    assert out.getvalue() == b"".join(r + b"\n" for r in want)
    assert cs.asked == [[(None, [("x", 0, True)])]]
