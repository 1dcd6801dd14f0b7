"""Lines on the device (include/fmx.h) against tests/lines_ref.py: lookups at the directory's edges, full and
empty buckets, the reduction across scan tiles, break sets, the corpus against Python run file by file, the command line,
determinism, capacity and the device form's flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_ref
import findex_amd
import lines_ref
import occ_ref
from conftest import ROOT
from findex_amd import _lib
from helpers import ends_at_a_fault

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, OVERFLOW = 3, 6, 9
H = findex_amd.HipFMSearcher
NONE = 2 ** 64 - 1


def interval(hip, Q):
    r = hip.search(bytes(Q)[::-1])
    assert r is not None, Q
    return int(r[0]), int(r[1])


def hits_of(hip, strings, n_groups=None, corpus=None):
    """(off, occ): all occurrences of [(group, string)]"""
    rec = [(g, len(q)) + interval(hip, q) for g, q in strings]
    return hip.occurrences(np.array(rec, dtype=H.RESULT), n_groups=n_groups, mode="all", corpus=corpus)


def same_lookups(hip, ref, pos):
    got, want = hip.line_of(pos), ref.lookup(pos)
    for g, w, what in zip(got, want, ("line", "start", "end")):
        assert g.dtype == np.uint64 and np.array_equal(g, w), (what, np.flatnonzero(g != w)[:5], g[g != w][:5], w[g != w][:5])


def same_hits(got, want):
    assert np.array_equal(got[0], want[0]), (got[0][:10], want[0][:10])
    assert got[1].dtype == lines_ref.LINE_HIT and got[1].size == want[1].size
    for f in lines_ref.LINE_HIT.names:
        assert np.array_equal(got[1][f], want[1][f]), (f, got[1][f][:8], want[1][f][:8])
    assert got[1].tobytes() == want[1].tobytes()


# ---------------------------------------------------------------- 1. lookups at the directory's edges
def edge_text():
    T = bytearray(b"a" * 5000)
    for p in (0, 255, 256, 257, 511, 512, 4999):
        T[p] = 10
    return bytes(T)


@pytest.fixture(scope="module")
def edges():
    T = edge_text()
    hip = H.from_text(T)
    yield T, hip, lines_ref.Lines(T)
    hip.close()


@pytest.mark.parametrize("shift", (8, 4, 16))
@ends_at_a_fault
def test_lookups_at_directory_edges(edges, shift):
    import torch
    T, hip, ref = edges
    hip.config_set("lines_shift", shift)
    hip.drop_tables(jump=False, frontier=False, lines=True)
    assert hip.lines_info()[3] == 0
    hip.lines_prepare()
    n_brk, bset, s, nbytes, ms = hip.lines_info()
    assert (n_brk, bset, s) == (7, b"\n", shift) and nbytes == 4 * 7 + 4 * ((5000 >> shift) + 2) and ms > 0
    pos = np.arange(5001, dtype=np.uint64)                   # every position, and the first one past the text
    same_lookups(hip, ref, pos)
    assert all(int(a[-1]) == NONE for a in hip.line_of(pos))
    # the device form: the same values, and an output left out is left alone
    d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
    d_out = torch.full((3, pos.size), 7, dtype=torch.int64, device="cuda")
    hip.line_of_dev(d_pos.data_ptr(), pos.size, d_out[0].data_ptr(), 0, d_out[2].data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    want = ref.lookup(pos)
    assert np.array_equal(got[0], want[0]) and (got[1] == 7).all() and np.array_equal(got[2], want[2])
    d_l = torch.from_numpy(np.arange(10, dtype=np.int64)).cuda()
    hip.line_spans_dev(d_l.data_ptr(), 10, d_out[0].data_ptr(), d_out[1].data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    want = ref.spans(np.arange(10))
    assert np.array_equal(got[0][:10], want[0]) and np.array_equal(got[1][:10], want[1])
    assert all(x >= 0 for x in hip.lines_last())


# ---------------------------------------------------------------- 2. full and empty buckets
@pytest.mark.parametrize("text", (b"\n" * 1000, b"a" * 3000, b"a" * 3000 + b"\n", b"\n" + b"a" * 3000), ids=("breaks", "none", "last", "first"))
@ends_at_a_fault
def test_full_and_empty_buckets(text):
    hip = H.from_text(text)
    try:
        hip.config_set("lines_shift", 8)                     # buckets of 256 positions: every one full, or every one empty
        ref = lines_ref.Lines(text)
        same_lookups(hip, ref, np.arange(len(text) + 3, dtype=np.uint64))
        assert hip.lines_info()[2] == 8
        assert hip.lines_info()[0] == ref.n_brk == text.count(b"\n")
        L = np.arange(ref.n_brk + 3, dtype=np.uint64)
        got, want = hip.line_spans(L), ref.spans(L)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert got[0][-2:].tolist() == [NONE, NONE] and got[1][-2:].tolist() == [NONE, NONE] and int(got[1][-3]) == len(text)
        assert hip.line_of([len(text), len(text) + 1, 2 ** 63])[0].tolist() == [NONE] * 3
        assert hip.line_of(np.zeros(0, dtype=np.uint64))[0].size == 0
    finally:
        hip.close()


# ---------------------------------------------------------------- 3. the reduction across scan tiles
@pytest.fixture(scope="module")
def runs():
    one, many = b"a" * 6000, b"a\n" * 6000
    h1, h2 = H.from_text(one), H.from_text(many)
    yield (one, h1), (many, h2)
    h1.close()
    h2.close()


@ends_at_a_fault
def test_reduction_across_scan_tiles(runs):
    (one, h1), (many, h2) = runs
    # one line, 5999 hits over three scan tiles; a group without occurrences in the middle
    off, occ = hits_of(h1, [(0, b"aa"), (2, b"aaa")], n_groups=3)
    assert off.tolist() == [0, 5999, 5999, 5999 + 5998]
    got = h1.occurrence_lines(off, occ)
    same_hits(got, lines_ref.occurrence_lines(lines_ref.Lines(one), off, occ))
    assert got[0].tolist() == [0, 1, 1, 2] and got[1]["n_hits"].tolist() == [5999, 5998] and got[1]["len"].tolist() == [6000, 6000]
    assert got[1]["first"].tolist() == [0, 0] and got[1]["line_no"].tolist() == [1, 1]
    # 6000 lines of one hit each: a head at every element; two groups share the lines
    off, occ = hits_of(h2, [(0, b"a"), (2, b"a\n")], n_groups=3)
    assert off.tolist() == [0, 6000, 6000, 12000]
    got = h2.occurrence_lines(off, occ)
    same_hits(got, lines_ref.occurrence_lines(lines_ref.Lines(many), off, occ))
    assert got[0].tolist() == [0, 6000, 6000, 12000] and (got[1]["n_hits"] == 1).all()
    assert got[1]["line_no"].tolist() == list(range(1, 6001)) * 2 and got[1]["first"].tolist() == list(range(6000)) * 2
    # no occurrences at all
    off0 = np.zeros(4, dtype=np.uint64)
    got = h2.occurrence_lines(off0, occ[:0])
    assert got[0].tolist() == [0, 0, 0, 0] and got[1].size == 0


# ---------------------------------------------------------------- 4. break sets
@ends_at_a_fault
def test_break_sets():
    T = occ_ref.word_text()
    hip = H.from_text(T)
    try:
        pos = np.arange(len(T), dtype=np.uint64)
        hip.prepare(ktab=False, lines=True)                   # fmx_prepare builds the default set
        info = hip.lines_info()
        assert info[:2] == (T.count(b"\n"), b"\n") and info[3] > 0
        same_lookups(hip, lines_ref.Lines(T), pos)
        hip.lines_prepare(b"\n")                             # an equal set: nothing is built
        assert hip.lines_info() == info
        wide = b"\n\r \t"
        hip.lines_prepare(wide)                              # another: rebuilt
        info2 = hip.lines_info()
        assert info2[0] == T.count(b"\n") + T.count(b" ") > info[0] and info2[1] == bytes(sorted(wide))
        ref = lines_ref.Lines(T, wide)
        same_lookups(hip, ref, pos)
        brk = hip.line_spans(np.arange(ref.n_brk, dtype=np.uint64))[1]
        assert np.array_equal(brk.astype(np.int64), ref.brk)
        hip.lines_prepare(b" \t\r\n")                        # the same set in another order: nothing is built
        assert hip.lines_info() == info2
        off, occ = hits_of(hip, [(0, b"ab"), (1, b"b "), (1, b"b\n")])
        same_hits(hip.occurrence_lines(off, occ), lines_ref.occurrence_lines(ref, off, occ))
        hip.drop_tables(jump=False, frontier=False, lines=True)
        assert hip.lines_info()[3] == 0
        hip.line_of_dev(0, 0)                                # nothing to look up: the device forms build nothing for it
        hip.line_spans_dev(0, 0)
        assert hip.lines_info()[3] == 0
        same_lookups(hip, lines_ref.Lines(T), pos)           # a lookup without a table builds the default one
        assert hip.lines_info()[:2] == info[:2]
        same_hits(hip.occurrence_lines(off, occ), lines_ref.occurrence_lines(lines_ref.Lines(T), off, occ))
    finally:
        hip.close()


@ends_at_a_fault
def test_dropping_locate_leaves_lines_and_extract_alone():
    """The line table and the extract samples are built from the locate samples and keep nothing of them."""
    T = occ_ref.word_text()
    hip = H.from_text(T)
    try:
        hip.prepare(ktab=False, locate=True, extract=True, lines=True)
        rows = np.arange(0, hip.n, 7, dtype=np.uint64)
        pos = np.arange(len(T) + 1, dtype=np.uint64)
        loc, lin, ext = hip.locate_info(), hip.lines_info(), hip.extract_info()
        assert loc[1] > 0 and lin[3] > 0 and ext[1] > 0
        sa, lines, text = hip.locate(rows), hip.line_of(pos), hip.extract_text(0, len(T))
        assert text == T
        hip.drop_tables(jump=False, frontier=False, locate=True)
        assert hip.locate_info()[1] == 0
        assert hip.lines_info() == lin and hip.extract_info() == ext
        for g, w in zip(hip.line_of(pos), lines):
            assert np.array_equal(g, w)
        assert hip.extract_text(0, len(T)) == T and hip.extract_text(len(T) // 3, 100) == T[len(T) // 3:len(T) // 3 + 100]
        assert hip.locate_info()[1] == 0                      # neither of them asked for the samples again
        assert np.array_equal(hip.locate(rows), sa)           # the next locate call builds them
        assert hip.locate_info()[:2] == loc[:2]
        assert hip.lines_info() == lin and hip.extract_info() == ext
    finally:
        hip.close()


# ---------------------------------------------------------------- 5. the corpus
LONG = b"ab" + b"c" * 2996 + b"ab"
DOCS = [b"", b"ab\ncab", b"ab\nxab\n", b"\n\n\n", b"x\x00ab\x01y\xffab\nab", b"ab\r\ncd ab\r\nend\r\n", LONG + b"\nab\n", b"", b"b",
        b"zab", b"\nab", b"nothing here\n\nat all\n"]
NAMES = [b"d%02d" % d for d in range(len(DOCS))]
assert len(LONG) == 3000


def pieces_of(raw):
    p = raw.split(b"\n")
    return p[:-1] if raw.endswith(b"\n") or not raw else p


@pytest.fixture(scope="module")
def corpus():
    ref = corpus_ref.RefCorpus(DOCS)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(DOCS, names=NAMES))
    yield ref, cs
    cs.close()


@ends_at_a_fault
def test_corpus_grep_lines_against_python(corpus):
    ref, cs = corpus
    needles = (b"ab", b"b", b"c")
    off, hits, truncated, lines = cs.grep_lines([n.decode() for n in needles], text=True)
    assert not truncated and cs.searcher.lines_info()[1] == b"\x01\n"
    for i, needle in enumerate(needles):
        sel = slice(int(off[i]), int(off[i + 1]))
        got = [(int(h["doc"]), int(h["line_no"]), t) for h, t in zip(hits[sel], lines[sel])]
        assert got == lines_ref.python_grep(DOCS, needle) and len(got) >= 3, needle
        assert hits[sel]["n_hits"].tolist() == [t.count(needle) for t in lines[sel]]
        assert hits[sel]["raw_len"].tolist() == [len(t) for t in lines[sel]]
    # the records, byte for byte, from the reference over the stream and its map
    ooff, occ, _ = cs.grep(["ab", "b", "c"])
    S = lines_ref.Lines(ref.stream, b"\n\x01")
    same_hits((off, hits), lines_ref.occurrence_lines(S, ooff, occ, docs=ref))
    esc = [h for h in hits[:int(off[1])] if int(h["doc"]) == 4 and int(h["line_no"]) == 1][0]
    assert int(esc["raw_len"]) == 9 and int(esc["len"]) == 12 and int(esc["raw_off"]) == 0
    second = [h for h in hits[:int(off[1])] if int(h["doc"]) == 4 and int(h["line_no"]) == 2][0]
    assert int(second["raw_off"]) == 10 and int(second["start"]) - ref.doc_start[4] == 13
    # no line spans two documents: both ends of every line of the stream lie in one
    s, e = cs.searcher.line_spans(np.arange(S.n_brk, dtype=np.uint64))
    assert np.array_equal(cs.corpus.map(s)[0], cs.corpus.map(e)[0]) and int(e[-1]) == len(ref.stream) - 1
    # context lines, clipped to the file
    res = cs.grep_lines(["ab"], text=True, before=1, after=2)
    assert res[1].tobytes() == hits[:int(off[1])].tobytes() and res[3] == lines[:int(off[1])]
    for h, (bf, af) in zip(res[1], res[4]):
        p, i = pieces_of(DOCS[int(h["doc"])]), int(h["line_no"]) - 1
        assert (bf, af) == (p[max(i - 1, 0):i], p[i + 1:i + 3]), (int(h["doc"]), i)
    # a long line is cut around its first match
    cut = cs.grep_lines(["cab"], text=True, max_line=16)
    texts = dict(((int(h["doc"]), int(h["line_no"])), t) for h, t in zip(cut[1], cut[3]))
    assert texts[(1, 2)] == b"cab" and texts[(6, 1)] == LONG[2989:] and len(LONG[2989:]) == 11


@ends_at_a_fault
def test_corpus_line_counts_and_lines(corpus):
    ref, cs = corpus
    assert cs.line_count().tolist() == [lines_ref.wc_l(d) for d in DOCS]
    assert cs.line_count(4) == 2 and cs.line_count(0) == 0
    for d, raw in enumerate(DOCS):
        p = pieces_of(raw)
        for k in sorted({1, len(p)} | {i + 1 for i, x in enumerate(p) if not x}):
            if p:
                assert cs.line(d, k) == p[k - 1], (d, k)
        for k in (0, len(p) + 1):
            with pytest.raises(IndexError):
                cs.line(d, k)


@ends_at_a_fault
def test_fresh_corpus_searcher_counts_and_reads_lines_first():
    """line_count and line before any grep_lines, on a handle that has no table yet: the corpus layer must build {10, 1}
    itself ({10} would count a line for an empty document behind another and let a line run across the separator)."""
    docs = [b"ab", b"", b"ab\n", b"", b"x\ny", b""]
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    try:
        assert cs.searcher.lines_info()[3] == 0
        assert cs.line_count(1) == 0 and cs.searcher.lines_info()[1] == b"\x01\n"
        assert cs.line_count().tolist() == [lines_ref.wc_l(d) for d in docs] == [1, 0, 1, 0, 2, 0]
        assert [cs.line(0, 1), cs.line(2, 1), cs.line(4, 1), cs.line(4, 2)] == [b"ab", b"ab", b"x", b"y"]
        for d in (1, 3, 5):
            with pytest.raises(IndexError):
                cs.line(d, 1)
        with pytest.raises(IndexError):
            cs.line_count(6)
    finally:
        cs.close()
    # line() first of all, and a table of {10} that somebody left on the searcher
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    try:
        assert cs.line(4, 2) == b"y"
        cs.searcher.lines_prepare(b"\n")
        assert cs.line(2, 1) == b"ab" and cs.line_count(3) == 0 and cs.searcher.lines_info()[1] == b"\x01\n"
        cs.searcher.lines_prepare(b"\n")
        off, hits, _, lines = cs.grep_lines(["ab"], text=True)
        assert [(int(h["doc"]), int(h["line_no"]), t) for h, t in zip(hits, lines)] == lines_ref.python_grep(docs, b"ab")
        cs.searcher.lines_prepare(b"\n\x01 ")              # a set that holds the separator is kept as it is
        assert cs.line_count().tolist() == [1, 0, 1, 0, 2, 0] and cs.searcher.lines_info()[1] == b"\x01\n "
    finally:
        cs.close()


@ends_at_a_fault
def test_corpus_needs_the_separator_in_the_set(corpus):
    ref, cs = corpus
    hip = cs.searcher
    off, occ, _ = cs.grep(["ab"])
    hip.lines_prepare(b"\n")
    try:
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.occurrence_lines(off, occ, corpus=cs.corpus)
        assert ei.value.code == ARG and "byte 1" in str(ei.value)
        plain = hip.occurrence_lines(off, occ)              # without the corpus the table serves
        assert (plain[1]["doc"] == 0xFFFFFFFF).all()
    finally:
        hip.lines_prepare(b"\n\x01")
    want = lines_ref.occurrence_lines(lines_ref.Lines(ref.stream, b"\n\x01"), off, occ, docs=ref)
    same_hits(hip.occurrence_lines(off, occ, corpus=cs.corpus), want)
    # a corpus that is not this index's
    other = findex_amd.Corpus.from_documents([b"ab"])
    try:
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.occurrence_lines(off, occ, corpus=other)
        assert ei.value.code == ARG and "not the index of this corpus" in str(ei.value)
    finally:
        other.close()


# ---------------------------------------------------------------- 6. the command line, in a fresh process
@pytest.fixture(scope="module")
def index_on_disk(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lines")
    ref = corpus_ref.RefCorpus(DOCS)
    bwt, eof, counts = findex_amd.bwt_from_text(ref.stream)
    findex_amd.write_bwt(tmp / "x.bwt", tmp / "x.aux", bwt, eof, counts)
    corpus = findex_amd.Corpus.from_documents(DOCS, names=NAMES)
    corpus.save(tmp / "x.docs")
    corpus.close()
    return str(tmp / "x")


def expect_cli(flags):
    found = lines_ref.python_grep(DOCS, b"ab")
    if flags == ["-n"]:
        return [NAMES[d] + b":%d:" % no + t for d, no, t in found]
    if flags == ["-c"]:
        return [NAMES[d] + b":%d" % sum(1 for x in found if x[0] == d) for d in sorted({x[0] for x in found})]
    if flags == ["-l"]:
        return [NAMES[d] for d in sorted({x[0] for x in found})]
    rows, last = [], None                                    # -A 1 -B 1
    for d, raw in enumerate(DOCS):
        p = pieces_of(raw)
        m = {i for i, x in enumerate(p) if b"ab" in x}
        for j in sorted({j for i in m for j in range(max(i - 1, 0), min(i + 2, len(p)))}):
            if last is not None and (last[0] != d or j > last[1] + 1):
                rows.append(b"--")
            rows.append(NAMES[d] + (b":" if j in m else b"-") + p[j])
            last = (d, j)
    return rows


@pytest.mark.parametrize("flags", (["-n"], ["-c"], ["-l"], ["-A", "1", "-B", "1"]), ids=("n", "c", "l", "AB"))
@ends_at_a_fault
def test_command_line(index_on_disk, flags):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.grep", index_on_disk, "ab"] + flags, cwd=ROOT, env=env, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = expect_cli(flags)
    assert len(want) > 3 and r.stdout == b"".join(row + b"\n" for row in want)


# ---------------------------------------------------------------- 7. determinism and capacity, 8. the device form's flag
@ends_at_a_fault
def test_determinism_capacity_and_the_device_flag(runs):
    import torch
    (one, h1), (many, hip) = runs
    off, occ = hits_of(hip, [(0, b"a"), (2, b"a\n")], n_groups=3)
    want = lines_ref.occurrence_lines(lines_ref.Lines(many), off, occ)
    T = want[1].size
    assert T == 12000
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_occ = torch.from_numpy(occ.view(np.int64)).cuda()
    d_loff = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    guard = 256
    d_out = torch.full((T * 48 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    args = (d_off.data_ptr(), d_occ.data_ptr(), occ.size, 3, d_loff.data_ptr())
    assert hip.occurrence_lines_dev(*args, 0, 0) == T        # the counting call
    assert (d_out.cpu().numpy() == 0xCD).all() and np.array_equal(d_loff.cpu().numpy().view(np.uint64), want[0])
    raws = []
    for _ in range(2):                                       # the same call twice: the same bytes
        d_out.fill_(0xCD)
        assert hip.occurrence_lines_dev(*args, d_out.data_ptr(), T) == T
        torch.cuda.synchronize()
        raws.append(d_out.cpu().numpy().copy())
    assert raws[0].tobytes() == raws[1].tobytes()
    assert raws[0][:T * 48].tobytes() == want[1].tobytes() and (raws[0][T * 48:] == 0xCD).all()
    assert np.array_equal(d_loff.cpu().numpy().view(np.uint64), want[0])
    # one short: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrence_lines_dev(*args, d_out.data_ptr(), T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    assert hip.occurrence_lines_dev(*args, d_out.data_ptr(), T - 1, grow=True) == T
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:(T - 1) * 48].tobytes() == want[1][:T - 1].tobytes() and (raw[(T - 1) * 48:] == 0xCD).all()
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrence_lines(off, occ, cap=T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    same_hits(hip.occurrence_lines(off, occ, cap=T), want)
    same_hits(hip.occurrence_lines(off, occ), want)
    # a record at pos = n - 1: the device form finds it on the device, and nothing is reported
    bad = occ.copy()
    bad["pos"][6001] = len(many)
    d_bad = torch.from_numpy(bad.view(np.int64)).cuda()
    d_loff.fill_(7)
    d_out.fill_(0xCD)
    n_out = ctypes.c_size_t(77)
    vp = ctypes.c_void_p
    L = _lib.load()
    assert L.fmx_occurrence_lines_dev(hip.handle, None, vp(d_off.data_ptr()), vp(d_bad.data_ptr()), occ.size, 3, vp(d_loff.data_ptr()),
                                      vp(d_out.data_ptr()), T, ctypes.byref(n_out), None) == ARG
    assert b"pos" in L.fmx_last_error()
    torch.cuda.synchronize()
    assert n_out.value == 77 and d_loff.cpu().tolist() == [7] * 4 and (d_out.cpu().numpy() == 0xCD).all()
    with pytest.raises(findex_amd.FmxError) as ei:           # the host form sees it on the host
        hip.occurrence_lines(off, bad)
    assert ei.value.code == ARG and "n - 1" in str(ei.value)


@ends_at_a_fault
def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = H.from_block(bwt, bs, 3)
    try:
        for call in (lambda: hip.lines_prepare(), lambda: hip.line_of([0]), lambda: hip.line_spans([0]),
                     lambda: hip.prepare(ktab=False, lines=True),
                     lambda: hip.occurrence_lines(np.array([0, 0], dtype=np.uint64), np.zeros(0, dtype=H.OCCURRENCE))):
            with pytest.raises(findex_amd.FmxError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED
    finally:
        hip.close()
