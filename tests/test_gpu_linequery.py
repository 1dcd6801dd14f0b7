"""Line queries on the device (include/fmx.h) against tests/linequery_ref.py and against Python run file by file:
hand-worked texts, candidates across scan tiles, term groups of every small size with candidates at every position around
their keys, documents, the corpus layer end to end, many queries in one call, determinism, capacity, the device form and the
command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_ref
import findex_amd
import lines_ref
import linequery_ref as ref
from conftest import ROOT
from findex_amd import _lib
from helpers import ends_at_a_fault

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, OVERFLOW = 3, 6, 9
H = findex_amd.HipFMSearcher
NO_DOC = 0xFFFFFFFF


def same_hits(got, want):
    assert np.array_equal(got[0], want[0]), (got[0][:10], want[0][:10])
    assert got[1].dtype == lines_ref.LINE_HIT and got[1].size == want[1].size
    for f in lines_ref.LINE_HIT.names:
        assert np.array_equal(got[1][f], want[1][f]), (f, got[1][f][:8], want[1][f][:8])
    assert got[1].tobytes() == want[1].tobytes()


def pipeline(hip, regexes):
    """occurrence -> line: (off, hits) of the regexes over the plain text of `hip`."""
    off, occ, truncated = hip.finditer(regexes, mode="all")
    assert not truncated
    return hip.occurrence_lines(off, occ)


def line_numbers(res, q):
    return res[1]["line_no"][int(res[0][q]):int(res[0][q + 1])].tolist()


def python_lines(text, anchor, terms):
    return [no for _, no, _ in ref.python_query([text], anchor, terms)]


# ---------------------------------------------------------------- 1. hand-worked plain texts
@pytest.mark.parametrize("text", (b"ab\ncd\n\nef", b"ab\ncd\n"), ids=("open", "closed"))
@ends_at_a_fault
def test_hand_worked_texts(text):
    hip = H.from_text(text)
    try:
        needles = (b"b", b"d", b"f", b"a")
        off, hits = pipeline(hip, [n.decode() for n in needles])
        named = [(None, [(0, 0, True)]), (None, []), (0, [(1, 1, False)]), (0, [(1, 0, False)]), (0, [(2, 2, False)]),
                 (0, [(2, "file", False)]), (1, [(0, 1, False), (2, 1, True)]), (0, [(3, 0, False)]), (0, [(3, 0, True)]),
                 (2, [(0, 3, False), (1, 2, False)])]
        got = hip.line_query(off, hits, named)
        same_hits(got, ref.line_query(off, hits, named, lines=lines_ref.Lines(text)))
        for q, (a, terms) in enumerate(named):
            want = python_lines(text, None if a is None else needles[a], [(needles[g], w, neg) for g, w, neg in terms])
            assert line_numbers(got, q) == want, (q, named[q])
        every = got[1][int(got[0][1]):int(got[0][2])]
        if text == b"ab\ncd\n\nef":
            assert every["line_no"].tolist() == [1, 2, 3, 4] and every["len"].tolist() == [2, 2, 0, 2]     # the empty line is real
            assert line_numbers(got, 0) == [2, 3, 4]
        else:
            assert every["line_no"].tolist() == [1, 2] and every["start"].tolist() == [0, 3]           # the piece behind "\n" is not
        assert (every["n_hits"] == 0).all() and (every["first"] == NO_DOC).all() and (every["doc"] == NO_DOC).all()
        assert hip.lines_info()[1] == b"\n"
    finally:
        hip.close()


# ---------------------------------------------------------------- 2. candidates across scan tiles
def tiles_text():
    return b"".join((b"a" if i % 2 == 0 else b"") + (b"b" if i % 3 == 0 else b"") + (b"c" if i % 2 and i % 3 else b"") + b"\n"
                    for i in range(6000))


@pytest.mark.parametrize("text", (b"a\n" * 6000, tiles_text()), ids=("runs", "mixed"))
@ends_at_a_fault
def test_candidates_across_scan_tiles(text):
    hip = H.from_text(text)
    try:
        A, Z, B = 0, 1, 2                                     # "z" matches nowhere: a group without records between the others
        off, hits = pipeline(hip, ["a", "z", "b"])
        assert int(off[Z]) == int(off[Z + 1])
        queries = [(A, [(B, 0, False)]), (A, [(B, 0, True)]), (None, [(A, 0, True)]), (None, [(Z, 0, True)]), (A, []), (None, []),
                   (Z, []), (Z, [(A, 0, True)]), (A, [(Z, "file", True)]), (A, [(Z, "file", False)])]
        got = hip.line_query(off, hits, queries)
        same_hits(got, ref.line_query(off, hits, queries, lines=lines_ref.Lines(text)))
        needles = (b"a", b"z", b"b")
        for q, (a, terms) in enumerate(queries[:4]):
            assert line_numbers(got, q) == python_lines(text, None if a is None else needles[a], [(needles[g], w, neg) for g, w, neg in terms])
        assert line_numbers(got, 3) == list(range(1, 6001)) == line_numbers(got, 5)
        assert len(line_numbers(got, 2)) + len(line_numbers(got, 4)) == 6000
        keys_ms, flags_ms, emit_ms, candidates, probes = hip.line_query_last()
        n_a = int(off[A + 1] - off[A])
        assert candidates == 5 * n_a + 3 * 6001 and probes > 0 and min(keys_ms, flags_ms, emit_ms) >= 0
    finally:
        hip.close()


# ---------------------------------------------------------------- 3. search sizes
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65)
WINDOWS = (0, 1, 2, 0xFFFFFFFF)


def synthetic(lines_per_group, doc=NO_DOC):
    """(off, hits) of groups with the given line numbers; the other fields are told apart by their values."""
    off = np.zeros(len(lines_per_group) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(g) for g in lines_per_group])
    hits = np.zeros(int(off[-1]), dtype=lines_ref.LINE_HIT)
    hits["line_no"] = [x for g in lines_per_group for x in g]
    hits["group"] = [i for i, g in enumerate(lines_per_group) for _ in g]
    hits["doc"] = doc
    hits["start"], hits["len"], hits["n_hits"] = 1000 + np.arange(hits.size), 7, 1 + np.arange(hits.size) % 3
    hits["raw_off"], hits["raw_len"], hits["first"] = hits["start"], 7, np.arange(hits.size) % 5
    return off, hits


@pytest.fixture(scope="module")
def small():
    hip = H.from_text(b"a\n")
    yield hip
    hip.close()


@ends_at_a_fault
def test_search_sizes_and_saturation(small):
    # a term group of s records holds lines 3, 6, .., 3 s; the candidates are every line 1 .. 3 * 65 + 3: before the first key,
    # on each key, between each pair and behind the last, lines 1 and 2 for the lower saturation
    groups = [list(range(1, 3 * 65 + 4))] + [list(range(3, 3 * s + 1, 3)) for s in SIZES]
    off, hits = synthetic(groups)
    queries = [(0, [(1 + i, w, neg)]) for i in range(len(SIZES)) for w in WINDOWS for neg in (False, True)]
    queries += [(0, [(1 + SIZES.index(64), 1, False), (1 + SIZES.index(5), 2, True)]), (1 + SIZES.index(65), [(0, 0, False)])]
    want = ref.line_query(off, hits, queries)
    raws = {}
    try:
        for narrow in ("on", "off"):
            findex_amd.config_set("lq_narrow", narrow)
            got = small.line_query(off, hits, queries)
            same_hits(got, want)
            raws[narrow] = got[0].tobytes() + got[1].tobytes()
    finally:
        findex_amd.config_set("lq_narrow", "off")            # the default
    assert raws["on"] == raws["off"]
    # spot checks by hand: size 1 (line 3), window 2 -> lines 1 .. 5; its negation the rest; window 2^32 - 1 -> every candidate
    q = 8 * SIZES.index(1)
    assert line_numbers(want, q + 4) == [1, 2, 3, 4, 5] and line_numbers(want, q + 5) == list(range(6, 199))
    assert line_numbers(want, q + 6) == list(range(1, 199)) and line_numbers(want, q) == [3]
    assert line_numbers(want, 0) == [] and line_numbers(want, 1) == list(range(1, 199))              # the empty group
    assert small.lines_info()[3] == 0                        # no query asked for all lines: no table was built


# ---------------------------------------------------------------- 4. documents
DOCS = [b"x A y\nq\nB last", b"A first\nw\nB\n", b"", b"B\x00in\x01side\xff A\nA\x01\nplain\n", b"\n", b"A\n\nB", b"A only\n",
        b"tail B\n", b"A head"]
NEEDLES = (b"A", b"B")


@pytest.fixture(scope="module")
def documents():
    rc = corpus_ref.RefCorpus(DOCS)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(DOCS))
    yield rc, cs
    cs.close()


@ends_at_a_fault
def test_documents_bound_the_windows(documents):
    rc, cs = documents
    hip = cs.searcher
    off, occ, _ = cs.grep(["A", "B"], mode="all")
    cs._lines_table()
    loff, hits = hip.occurrence_lines(off, occ, corpus=cs.corpus)
    queries = [(0, [(1, 1, False)]), (0, [(1, "file", False)]), (0, [(1, "file", True)]), (None, [(0, 0, True)]), (None, []),
               (None, [(1, 2, False)]), (1, [(0, 1, False)]), (None, [(0, "file", True), (1, "file", True)])]
    got = hip.line_query(loff, hits, queries, corpus=cs.corpus)
    S = lines_ref.Lines(rc.stream, b"\n\x01")
    same_hits(got, ref.line_query(loff, hits, queries, lines=S, docs=rc))
    for q, (a, terms) in enumerate(queries):
        want = ref.python_query(DOCS, None if a is None else NEEDLES[a], [(NEEDLES[g], w, neg) for g, w, neg in terms])
        sel = got[1][int(got[0][q]):int(got[0][q + 1])]
        assert [(int(h["doc"]), int(h["line_no"])) for h in sel] == [(d, no) for d, no, _ in want], q
        assert sel["raw_len"].tolist() == [len(t) for _, _, t in want], q
        assert cs.read(sel["doc"], sel["raw_off"], sel["raw_len"]) == [t for _, _, t in want] if sel.size else not want
    # file 0 ends in a line with B and file 1 begins with a line with A: one line apart in the stream, not near each other
    near = [(int(h["doc"]), int(h["line_no"])) for h in got[1][int(got[0][0]):int(got[0][1])]]
    assert near == [(3, 1), (3, 2)]                          # not (1, 1), whose neighbour in the stream is file 0's "B last"
    back = [(int(h["doc"]), int(h["line_no"])) for h in got[1][int(got[0][6]):int(got[0][7])]]
    assert back == [(3, 1)]                                  # not (0, 3) nor (7, 1), in front of files that begin with A
    every = got[1][int(got[0][4]):int(got[0][5])]
    assert np.unique(every["doc"]).tolist() == [0, 1, 3, 4, 5, 6, 7, 8]                     # the empty file has no lines
    assert [int(h["raw_len"]) for h in every if int(h["doc"]) == 3] == [12, 2, 5]
    assert [int(h["len"]) for h in every if int(h["doc"]) == 3] == [15, 3, 5]               # three escape pairs, one, none
    # a table without the separator, with a corpus
    hip.lines_prepare(b"\n")
    try:
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.line_query(loff, hits, [(None, [])], corpus=cs.corpus)
        assert ei.value.code == ARG and "byte 1" in str(ei.value)
        same_hits(hip.line_query(loff, hits, queries[:3], corpus=cs.corpus), ref.line_query(loff, hits, queries[:3]))     # needs no table
    finally:
        hip.lines_prepare(b"\n\x01")


# ---------------------------------------------------------------- 5. the corpus layer, end to end
@pytest.fixture(scope="module")
def seeded():
    docs = ref.seeded_corpus(7)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    yield docs, cs
    cs.close()


def pieces_of(raw):
    p = raw.split(b"\n")
    return p[:-1] if raw.endswith(b"\n") or not raw else p


@ends_at_a_fault
def test_grep_lines_where_against_python(seeded):
    docs, cs = seeded
    named = ref.five_queries()
    queries = [(None if a is None else a.decode(), [(n.decode(), w, neg) for n, w, neg in terms]) for _, a, terms in named]
    off, hits, truncated, lines = cs.grep_lines_where(queries, text=True)
    assert not truncated and off.size == 6
    for q, (name, a, terms) in enumerate(named):
        sel = slice(int(off[q]), int(off[q + 1]))
        got = [(int(h["doc"]), int(h["line_no"]), t) for h, t in zip(hits[sel], lines[sel])]
        assert got == ref.python_query(docs, a, terms) and got, name
        assert (hits[sel]["group"] == q).all()
    assert [int(off[q + 1] - off[q]) for q in range(5)] == [36, 109, 539, 90, 48]
    plain = cs.grep_lines(["alpha"])
    inv = cs.grep_lines_inverted(["alpha"], text=True, before=1, after=1)
    same = hits[int(off[2]):int(off[3])].copy()
    same["group"] = 0
    assert inv[1].tobytes() == same.tobytes() and np.array_equal(inv[0], [0, same.size])
    assert int(plain[0][1]) + inv[1].size == sum(lines_ref.wc_l(d) for d in docs) == 684
    assert [(int(h["doc"]), int(h["line_no"])) for h in inv[1]] == [(d, no) for d, no, _ in ref.python_query(docs, None, [(b"alpha", 0, True)])]
    assert inv[3] == [t for _, _, t in ref.python_query(docs, None, [(b"alpha", 0, True)])]
    for h, (bf, af) in zip(inv[1], inv[4]):
        p, i = pieces_of(docs[int(h["doc"])]), int(h["line_no"]) - 1
        assert (bf, af) == (p[max(i - 1, 0):i], p[i + 1:i + 2]), (int(h["doc"]), i)
    # a record without a first match is cut from the line's beginning
    cut = cs.grep_lines_inverted(["alpha"], text=True, max_line=4)
    assert cut[3] == [t[:4] for t in inv[3]] and any(len(t) > 4 for t in inv[3])
    # grep_lines itself gives what it gave
    again = cs.grep_lines(["alpha", "bravo"], text=True, max_line=7)
    assert [(int(h["doc"]), int(h["line_no"])) for h in again[1][:int(again[0][1])]] == [(d, no) for d, no, _ in lines_ref.python_grep(docs, b"alpha")]
    for h, t in zip(again[1], again[3]):
        whole = pieces_of(docs[int(h["doc"])])[int(h["line_no"]) - 1]
        word = (b"alpha", b"bravo")[int(h["group"])]
        assert t in whole and len(t) <= 7 and (len(t) == len(whole) or word[:1] in t)


# ---------------------------------------------------------------- 6. many queries in one call
@ends_at_a_fault
def test_three_hundred_queries(small):
    rng = np.random.RandomState(5)
    groups = [sorted(rng.choice(np.arange(1, 400), size=n, replace=False).tolist()) for n in (150, 90, 1, 0, 260, 33)]
    off, hits = synthetic(groups)
    queries = [(0, [(0, 0, False)]), (0, [(0, 0, True)]), (4, [((0, 1, 4, 5, 3)[g % 5], 3 + g % 4, g % 5 == 4) for g in range(64)])]
    while len(queries) < 300:
        a = int(rng.randint(0, 6))
        terms = [(int(rng.randint(0, 6)), [0, 1, 2, 5, "file"][int(rng.randint(0, 5))], bool(rng.randint(0, 2))) for _ in range(int(rng.randint(0, 4)))]
        queries.append((a, terms))
        if rng.rand() < 0.2:
            queries.append(queries[int(rng.randint(0, len(queries)))])       # a repeat
    queries = queries[:300]
    got = small.line_query(off, hits, queries)
    want = ref.line_query(off, hits, queries)
    same_hits(got, want)
    a_and_a = hits[:150].copy()
    assert got[1][:150].tobytes() == a_and_a.tobytes() and int(got[0][1]) == 150 and int(got[0][2]) == 150       # A and A is A, A not A is empty
    assert len({int(got[0][q + 1] - got[0][q]) for q in range(300)}) > 20 and int(got[0][3]) > 150        # (the 64 terms keep some)


# ---------------------------------------------------------------- 7. determinism, capacity and the device form
@ends_at_a_fault
def test_determinism_capacity_and_the_device_form(small):
    import torch
    hip = small
    groups = [list(range(1, 5001)), list(range(2, 5001, 2)), list(range(3, 5001, 7))]
    off, hits = synthetic(groups)
    queries = [(0, [(1, 0, False)]), (0, [(1, 0, True), (2, 1, False)]), (1, []), (2, [(0, 3, False)])]
    want = ref.line_query(off, hits, queries)
    T = want[1].size
    assert T > 5000
    same_hits(hip.line_query(off, hits, queries), want)
    same_hits(hip.line_query(off, hits, queries, cap=T), want)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.line_query(off, hits, queries, cap=T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_hits = torch.from_numpy(hits.view(np.int64)).cuda()
    d_qoff = torch.full((5,), 7, dtype=torch.int64, device="cuda")
    guard = 48
    d_out = torch.full((T * 48 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    args = (d_off.data_ptr(), d_hits.data_ptr(), hits.size, 3, queries, d_qoff.data_ptr())
    assert hip.line_query_dev(*args, 0, 0) == T                 # the counting call
    assert (d_out.cpu().numpy() == 0xCD).all() and np.array_equal(d_qoff.cpu().numpy().view(np.uint64), want[0])
    raws = []
    for _ in range(2):                                       # the same call twice: the same bytes
        d_out.fill_(0xCD)
        assert hip.line_query_dev(*args, d_out.data_ptr(), T) == T
        torch.cuda.synchronize()
        raws.append(d_out.cpu().numpy().copy())
    assert raws[0].tobytes() == raws[1].tobytes()
    assert raws[0][:T * 48].tobytes() == want[1].tobytes() and (raws[0][T * 48:] == 0xCD).all()
    # one short: the exact total, the canary record behind the capacity untouched
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.line_query_dev(*args, d_out.data_ptr(), T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    assert hip.line_query_dev(*args, d_out.data_ptr(), T - 1, grow=True) == T
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:(T - 1) * 48].tobytes() == want[1][:T - 1].tobytes() and (raw[(T - 1) * 48:] == 0xCD).all()
    # a descending pair of keys inside a group: the device form finds it on the device, and nothing is reported
    bad = hits.copy()
    bad["line_no"][7001] = bad["line_no"][7000]
    d_bad = torch.from_numpy(bad.view(np.int64)).cuda()
    d_qoff.fill_(7)
    d_out.fill_(0xCD)
    n_out = ctypes.c_size_t(77)
    vp = ctypes.c_void_p
    L = _lib.load()
    q_off, anchor, terms = H._line_queries(queries)
    ptr = lambda a: vp(a.ctypes.data)
    assert L.fmx_line_query_dev(hip.handle, None, vp(d_off.data_ptr()), vp(d_bad.data_ptr()), hits.size, 3, ptr(q_off), ptr(anchor),
                                ptr(terms), 4, vp(d_qoff.data_ptr()), vp(d_out.data_ptr()), T, ctypes.byref(n_out), None) == ARG
    assert b"do not ascend" in L.fmx_last_error()
    torch.cuda.synchronize()
    assert n_out.value == 77 and d_qoff.cpu().tolist() == [7] * 5 and (d_out.cpu().numpy() == 0xCD).all()
    with pytest.raises(findex_amd.FmxError) as ei:           # the host form sees it on the host
        hip.line_query(off, bad, queries)
    assert ei.value.code == ARG and "do not ascend" in str(ei.value)
    # offsets on the device that do not cover the records
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.line_query_dev(d_off.data_ptr(), d_hits.data_ptr(), hits.size - 1, 3, queries, d_qoff.data_ptr(), d_out.data_ptr(), T)
    assert ei.value.code == ARG and "end at n_hits" in str(ei.value)


@ends_at_a_fault
def test_block_handles_serve_queries_that_need_no_table():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = H.from_block(bwt, bs, 3)
    try:
        off, hits = synthetic([[1, 2, 5], [2, 6]])
        queries = [(0, [(1, 0, False)]), (0, [(1, 1, True)])]
        same_hits(hip.line_query(off, hits, queries), ref.line_query(off, hits, queries))
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.line_query(off, hits, [(None, [(0, 0, True)])])
        assert ei.value.code == UNSUPPORTED
    finally:
        hip.close()


# ---------------------------------------------------------------- 8. the command line, in a fresh process
@pytest.fixture(scope="module")
def index_on_disk(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("linequery")
    docs = ref.seeded_corpus(7)
    rc = corpus_ref.RefCorpus(docs)
    bwt, eof, counts = findex_amd.bwt_from_text(rc.stream)
    findex_amd.write_bwt(tmp / "x.bwt", tmp / "x.aux", bwt, eof, counts)
    corpus = findex_amd.Corpus.from_documents(docs, names=[b"d%02d" % d for d in range(len(docs))])
    corpus.save(tmp / "x.docs")
    corpus.close()
    return str(tmp / "x"), docs


def expect_cli(docs, flags):
    name = lambda d: b"d%02d" % d
    A, X = b"alpha", b"bravo"
    if flags == ["-v", "-n"]:
        return [name(d) + b":%d:" % no + t for d, no, t in ref.python_query(docs, None, [(A, 0, True)])]
    if flags == ["--and", "bravo", "-n"]:
        return [name(d) + b":%d:" % no + t for d, no, t in ref.python_query(docs, A, [(X, 0, False)])]
    if flags == ["--not", "bravo", "-c"]:
        found = ref.python_query(docs, A, [(X, 0, True)])
        return [name(d) + b":%d" % sum(1 for x in found if x[0] == d) for d in sorted({x[0] for x in found})]
    if flags == ["--and", "bravo", "--near", "1", "-n"]:
        return [name(d) + b":%d:" % no + t for d, no, t in ref.python_query(docs, A, [(X, 1, False)])]
    assert flags == ["--and", "bravo", "--same-file", "-l"]
    return [name(d) for d in sorted({x[0] for x in ref.python_query(docs, A, [(X, "file", False)])})]


@pytest.mark.parametrize("flags", (["-v", "-n"], ["--and", "bravo", "-n"], ["--not", "bravo", "-c"], ["--and", "bravo", "--near", "1", "-n"],
                                   ["--and", "bravo", "--same-file", "-l"]), ids=("vn", "and", "not", "near", "file"))
@ends_at_a_fault
def test_command_line(index_on_disk, flags):
    base, docs = index_on_disk
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.grep", base, "alpha"] + flags, cwd=ROOT, env=env, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = expect_cli(docs, flags)
    assert len(want) > 3 and r.stdout == b"".join(row + b"\n" for row in want)
