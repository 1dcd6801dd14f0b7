"""Whole-word matching on the device (fmx_context_filter, fmx_search_context_batch, fmx_corpus_rank_sets)
against tests/words_ref.py, bit for bit: the filter's shapes (rows that begin and end at every offset around a 16-byte and
a chunk boundary, a run across chunks, waves and workgroups, empty and one-row records, the whole index, ep > n, fifty
thousand one-row records, the alternating worst case), its modes, its plumbing (capacity with guard words, the device form's
flag, a stream capture), the context search, the ranking over interval sets, and finditer / grep / rank with words=True
through Python and the command lines.  Both rank-dictionary layouts, forced as tests/test_gpu_parity.py forces them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_ref
import findex_amd
import rank_ref
import words_ref
from findex_amd import _lib
from helpers import ends_at_a_fault

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = findex_amd.HipFMSearcher
B = words_ref.BOUNDARY
ALL = bytes(range(256))
ARG, HIP, OVERFLOW = 3, 5, 9
CHUNK = 1024                                                     # rows per chunk of the filter (fmx_context.hip)

VOCAB = [b"he", b"the", b"then", b"a", b"an", b"and", b"x_1", "café".encode(), b"hello", b"end"]
SEPS = [b" ", b" ", b" ", b", ", b"-", b".\n", b"\x85", b"\t"]
ABSENT = [b"zebra", b"th", b"x_", b"nd"]                        # the last three occur, but never as words


def words_text():
    """About 40 KB: "the" at offset 0, "then" at the very end, every vocabulary word behind every separator."""
    rng = np.random.default_rng(27)
    parts = [b"the", b" "]
    size = 4
    while size < 40000:
        w, s = VOCAB[int(rng.integers(len(VOCAB)))], SEPS[int(rng.integers(len(SEPS)))]
        parts += [w, s]
        size += len(w) + len(s)
    parts.append(b"then")
    return b"".join(parts)


_refs, _hits = {}, {}


def regex_hits(text, rx):
    """words_ref.word_starts, once per regex for the module."""
    if rx not in _hits:
        _hits[rx] = words_ref.word_starts(text, rx, max_len=6)
    return _hits[rx]


def ref_of(name, make):
    """One checker per text for the whole module, shared by both layouts and left unchanged."""
    if name not in _refs:
        _refs[name] = words_ref.SuffixRef(make())
    return _refs[name]


@pytest.fixture(scope="module", params=["onehot", "bytes"])
def world(request):
    ref = ref_of("words", words_text)
    findex_amd.set_layout(request.param)
    try:
        hip = H.from_text(ref.text)
    finally:
        findex_amd.set_layout("auto")
    assert hip.n == ref.n
    assert hip.search(b"eht") == ref.interval(b"the")              # the same rows: everything below compares row numbers
    yield hip, ref
    hip.close()


@pytest.fixture(scope="module")
def plain():
    ref = ref_of("words", words_text)
    hip = H.from_text(ref.text)
    yield hip, ref
    hip.close()


def tuples(runs):
    return list(zip(runs["regex"].tolist(), runs["len"].tolist(), runs["sp"].tolist(), runs["ep"].tolist()))


def check_filter(hip, ref, records, right, modes=None):
    rec = H.pack_records([r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    off, runs = hip.context_filter(rec, right, modes)
    want_off, want = ref.filter(records, right, modes)
    assert off.tolist() == want_off
    assert tuples(runs) == want
    return off, runs


# ---- 1. filter shapes
@ends_at_a_fault
def test_filter_shapes(world):
    hip, ref = world
    n = ref.n
    recs = []
    for s in range(18):                                          # every start offset, every end offset, each with two partners
        for e in (s, (5 * s + 3) % 18):
            recs.append((0, 2, 4096 - 9 + s, 4096 + 48 - 9 + e))                     # around 16-byte boundaries
            a = 8192 - 9 + s
            recs.append((1, 3, a, (a & ~15) + CHUNK - 9 + e))                        # around the record's chunk boundary
    recs += [(2, 1, 100, 100 + 5 * CHUNK + 7),                                       # a run across chunks, waves and a workgroup
             (3, 1, 50, 50), (3, 1, 51, 52), (3, 1, n - 1, n), (3, 1, 0, 1), (3, 1, ref.eof, ref.eof + 1),
             (4, 1, 0, n), (5, 1, 0, n + 12345), (5, 1, n - 40, n + 1), (6, 1, n, n + 5), (7, 0, 10, 500)]
    for right in (B, b"", b"\0", ALL):
        off, runs = check_filter(hip, ref, recs, right)
    big = recs.index((2, 1, 100, 100 + 5 * CHUNK + 7))
    assert tuples(runs[int(off[big]):int(off[big + 1])]) == [(2, 1, 100, 100 + 5 * CHUNK + 7)]      # ONE run
    whole = recs.index((4, 1, 0, n))
    assert tuples(runs[int(off[whole]):int(off[whole + 1])]) == [(4, 1, 0, n)]                        # rows 0 and eof included
    rows, found = hip.context_last()[3:]
    assert rows == sum(max(0, min(b, n) - a) for _, ln, a, b in recs if ln > 0) and found == runs.size


@ends_at_a_fault
def test_filter_fifty_thousand_one_row_records(plain):
    hip, ref = plain
    rng = np.random.default_rng(3)
    rows = rng.integers(0, ref.n, 50000).tolist()
    check_filter(hip, ref, [(i & 1023, 2, r, r + 1) for i, r in enumerate(rows)], B)


@ends_at_a_fault
def test_filter_alternating_worst_case():
    def make():
        return bytes(np.random.default_rng(11).integers(97, 99, 200000, dtype=np.uint8).tolist())
    ref = ref_of("ab", make)
    assert ref.n == 200001
    hip = H.from_text(ref.text)
    try:
        off, runs = check_filter(hip, ref, [(0, 1, 0, ref.n), (1, 1, 12345, 180001)], b"a")
        assert abs(int(off[1]) - ref.n / 4) < ref.n / 40                           # runs ~ rows / 4
    finally:
        hip.close()


# ---- 2. filter modes
@ends_at_a_fault
def test_filter_modes(world):
    hip, ref = world
    S = words_ref.CTX_START
    the = ref.interval(b"the")
    sp_the = ref.interval(b" the")
    assert ref.lf_chain(3) == the[0] and ref.pos(the[0], 3) == 0
    at0 = ref.lf_chain(300)                                                         # the row of the text's first 300 bytes
    t_iv = ref.interval(b"t")
    assert ref.lf_chain(1) == t_iv[0]
    he = ref.interval(b"he")
    recs = [(0, 3, the[0], the[1]), (0, 4, sp_the[0], sp_the[1]), (0, 4, sp_the[0], sp_the[1]), (0, 3, sp_the[0], sp_the[1]),
            (0, 2, sp_the[0], sp_the[1]), (1, 3, the[0], the[1]), (1, 3, the[0] + 1, the[1]), (1, 1, t_iv[0], t_iv[1]),
            (1, 1, t_iv[0] + 1, t_iv[1]), (2, 300, at0, at0 + 1), (2, 300, at0 + 1, at0 + 2), (2, 300, at0, at0),
            (3, 2, he[0], he[1]), (3, 2, he[0], he[1]), (4, 2, he[0], he[1]), (5, 65535, 0, 3)]
    modes = [0, 1, 3, 3, 3, S, S, S, S, S, S, S, 0, 0, S, S]
    for right in (B, ALL, b"\0"):
        check_filter(hip, ref, recs, right, modes)
    off, runs = check_filter(hip, ref, recs, ALL, modes)
    assert tuples(runs[int(off[5]):int(off[6])]) == [(1, 3, the[0], the[0] + 1)] and off[6] == off[7]
    assert tuples(runs[int(off[9]):int(off[10])]) == [(2, 300, at0, at0 + 1)] and off[10] == off[11] == off[12]
    assert tuples(runs[int(off[12]):int(off[13])]) == tuples(runs[int(off[13]):int(off[14])])       # a duplicated record
    check_filter(hip, ref, recs[:1] + recs[12:14], B, None)                                          # mode = NULL
    assert hip.context_last()[1] == 0.0                                                              # no start record: no chain


# ---- 3. filter plumbing
@ends_at_a_fault
def test_filter_capacity_flag_and_capture(plain):
    import torch
    hip, ref = plain
    he, the = ref.interval(b"he"), ref.interval(b"the")
    records = [(0, 2, he[0], he[1]), (1, 3, the[0], the[1]), (2, 1, 0, ref.n)]
    want_off, want = ref.filter(records, B)
    T = len(want)
    assert T > 100
    rec = H.pack_records([r[0] for r in records], [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    d_rec = torch.from_numpy(rec.view(np.int64)).cuda()
    d_off = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    guard = 256
    d_out = torch.full((T * 24 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    assert hip.context_filter_dev(d_rec.data_ptr(), 0, 3, B, d_off.data_ptr(), 0, 0) == T               # the counting call
    assert (d_out.cpu().numpy() == 0xCD).all()
    with pytest.raises(findex_amd.FmxError) as e:
        hip.context_filter_dev(d_rec.data_ptr(), 0, 3, B, d_off.data_ptr(), d_out.data_ptr(), T - 1)
    assert e.value.code == OVERFLOW and str(T) in str(e.value)
    out = d_out.cpu().numpy()
    assert (out[(T - 1) * 24:] == 0xCD).all()                                                         # nothing past cap - 1
    assert tuples(out[: (T - 1) * 24].view(H.RESULT)) == want[: T - 1]
    d_out.fill_(0xCD)
    assert hip.context_filter_dev(d_rec.data_ptr(), 0, 3, B, d_off.data_ptr(), d_out.data_ptr(), T) == T
    out = d_out.cpu().numpy()
    assert (out[T * 24:] == 0xCD).all() and tuples(out[: T * 24].view(H.RESULT)) == want
    assert d_off.cpu().tolist() == want_off
    # the host form's capacity
    with pytest.raises(findex_amd.FmxError) as e:
        hip.context_filter(rec, B, cap=T - 1)
    assert e.value.code == OVERFLOW
    assert tuples(hip.context_filter(rec, B, cap=T)[1]) == want
    # the device form cannot see its records: a bad one is skipped and flagged
    for field, value, mode in (("len", 65536, None), ("sp", ref.n + 5, None), ("len", 3, [0, 0x81, 0])):
        bad = rec.copy()
        bad[field][1] = value
        if field == "sp":
            bad["ep"][1] = 4
        d_bad = torch.from_numpy(bad.view(np.int64)).cuda()
        d_mode = torch.tensor(mode, dtype=torch.uint8, device="cuda") if mode else None
        d_off.fill_(7)
        d_out.fill_(0xCD)
        n_out = ctypes.c_size_t(77)
        rw = findex_amd.class_words(B)
        vp = ctypes.c_void_p
        rc = _lib.load().fmx_context_filter_dev(hip.handle, vp(d_bad.data_ptr()), vp(d_mode.data_ptr()) if mode else None, 3,
                                                rw.ctypes.data_as(vp), vp(d_off.data_ptr()), vp(d_out.data_ptr()), T, ctypes.byref(n_out),
                                                None)
        assert rc == ARG
        torch.cuda.synchronize()
        assert n_out.value == 77 and d_off.cpu().tolist() == [7] * 4 and (d_out.cpu().numpy() == 0xCD).all()
    # under a stream capture the call is refused before it allocates or launches, and the capture goes on
    st = torch.cuda.Stream()
    launches = hip.stats()["launches"]
    torch.cuda.empty_cache()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g.capture_begin()
        try:
            hip.context_filter_dev(d_rec.data_ptr(), 0, 3, B, d_off.data_ptr(), d_out.data_ptr(), T, stream=st.cuda_stream)
        except findex_amd.FmxError as ex:
            err = ex
        d_off.zero_()
        g.capture_end()
    assert err is not None and err.code == HIP and "stream capture" in str(err)
    d_off.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert not d_off.cpu().numpy().any()
    del g
    assert hip.stats()["launches"] == launches


# ---- 4. the context search
def pack(pats):
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pats], out=off[1:])
    return np.frombuffer(b"".join(p[::-1] for p in pats), dtype=np.uint8), off


@ends_at_a_fault
def test_search_context_batch(world):
    hip, ref = world
    pats = VOCAB + ABSENT
    pat, off = pack(pats)
    no_start = bytes(c for c in B if c != 0)
    nowhere = b"\x02\x03\x7f"                                                      # bytes the text does not hold
    assert not any(c in ref.text for c in nowhere)
    for left, right in ((B, ALL), (ALL, B), (B, B), (no_start, B), (nowhere, B), (nowhere + b"\0", ALL), (b"", ALL), (B, b"")):
        o, runs = hip.search_context_batch(pat, off, left, right)
        for i, x in enumerate(pats):
            mine = runs[int(o[i]):int(o[i + 1])]
            assert (mine["regex"] == i).all() and (mine["len"] == len(x)).all()
            sp, ep = mine["sp"].tolist(), mine["ep"].tolist()
            assert all(a < b for a, b in zip(sp, ep)) and all(b <= a for b, a in zip(ep, sp[1:]))      # ascending, disjoint
            rows = [r for a, b in zip(sp, ep) for r in range(a, b)]
            assert rows == ref.context_rows(x, left, right), (x, left[:4], right[:4])
    o, runs = hip.search_context_batch(pat, off, B, B)
    assert int(o[1] - o[0]) > 0 and int(o[len(VOCAB)]) == int(o[-1])           # "he" is a word; no absent one is
    the0 = ref.interval(b"the")[0]
    i = pats.index(b"the")
    assert the0 in runs["sp"][int(o[i]):int(o[i + 1])].tolist()                     # the word at offset 0 ...
    o2, runs2 = hip.search_context_batch(pat, off, no_start, B)
    assert the0 not in [r for a, b in zip(runs2["sp"][int(o2[i]):int(o2[i + 1])].tolist(), runs2["ep"][int(o2[i]):int(o2[i + 1])].tolist())
                        for r in range(a, b)]                                       # ... goes when bit 0 is cleared
    search_ms, _, _, rows, found = hip.context_last()
    assert found == runs2.size and rows > 0
    assert hip.search_context_batch(pat[:0], off[:1], B, B)[0].tolist() == [0]
    for q in VOCAB + ABSENT:
        assert hip.locate_words(q).tolist() == words_ref.literal_word_starts(ref.text, q), q
    assert hip.locate_words(b"he", max_hits=5).size == 5
    so, sruns = hip.search_words(pats)
    assert so.tolist() == o.tolist() and tuples(sruns) == tuples(runs)


# ---- 5. the ranking over interval sets
class WordRankRef(rank_ref.RankRef):
    """tests/rank_ref.py fed with whole-word occurrences: tf counts a term only where its neighbours in the document's slice of
    the escaped stream are no word bytes (a slice ends at the separator, which is a boundary)."""

    def tf(self, term):
        term = bytes(term)
        if term not in self._tf:
            esc = corpus_ref.escape_bytes(term)
            out = {}
            for d, s in enumerate(self.slices):
                c = len(words_ref.literal_word_starts(s, esc))
                if c:
                    out[d] = c
            self._tf[term] = out
        return self._tf[term]


def word_docs():
    rng = np.random.default_rng(8)
    docs = []
    for d in range(120):
        parts = []
        for _ in range(int(rng.integers(0, 30))):
            parts += [VOCAB[int(rng.integers(len(VOCAB)))], SEPS[int(rng.integers(len(SEPS)))]]
        docs.append(b"".join(parts))
    docs[5] = b"the"                                                               # a whole file; then a word that ends one file
    docs[6] = b"and then the"                                                      # and begins the next
    docs[7] = b"the end \x00 he"
    return docs


@pytest.fixture(scope="module")
def files():
    docs = word_docs()
    ref = corpus_ref.RefCorpus(docs)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    yield cs, ref, docs
    cs.close()


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@ends_at_a_fault
def test_rank_sets(files):
    cs, ref, _ = files
    terms = [b"he", b"the", b"an", b"zebra", b"e", b"x_1"]
    _, sp, ep = cs._intervals(terms)
    q_off = np.array([0, 2, 3, 6], dtype=np.uint64)
    for match in ("any", "all"):
        base = cs.rank_intervals(sp, ep, q_off, top=10, match=match)
        same_bytes(cs.rank_sets_intervals(sp, ep, np.arange(7, dtype=np.uint64), q_off, top=10, match=match), base)
        # a slot in 1, 2 and 7 pieces; "zebra" (slot 3) has no rows and gets no interval at all
        for pieces in (1, 2, 7):
            ssp, sep, set_off = [], [], [0]
            for t in range(6):
                a, b = int(sp[t]), int(ep[t])
                if b > a:
                    cuts = sorted(set([a, b] + [a + (b - a) * j // pieces for j in range(1, pieces)]))
                    ssp += cuts[:-1]
                    sep += cuts[1:]
                set_off.append(len(ssp))
            assert set_off[4] == set_off[3] and len(ssp) > 6 * (pieces > 1)
            same_bytes(cs.rank_sets_intervals(ssp, sep, set_off, q_off, top=10, match=match), base)
    assert base[3][3] == 0                                                         # the empty slot: df 0


@ends_at_a_fault
def test_rank_words(files):
    cs, ref, _ = files
    rr = WordRankRef(ref)
    queries = [[b"he"], [b"the", b"then"], [b"a", b"an", b"and"], [b"x_1", b"zebra"], [b"e"], ["café".encode()], [b"\x00"], []]
    for match in ("any", "all"):
        off, doc, score, df, w = cs.rank(queries, top=10, match=match, words=True)
        post = rr.postings(queries)
        assert df.tolist() == [len(p) for p in post]
        eo, ed, es = rr.rank([len(q) for q in queries], post, w.tolist(), top=10, match=match)
        assert off.tolist() == eo and doc.tolist() == ed
        assert score.view(np.uint64).tolist() == np.array(es, dtype=np.float64).view(np.uint64).tolist()
    assert df[8] == 0                                                              # "e" stands in many words and is none
    assert len(rr.tf(b"e")) == 0 and len(rank_ref.RankRef(ref).tf(b"e")) > 50
    assert {5, 6, 7} <= set(rr.tf(b"the"))                                         # at a file's start, at its end, the whole file
    cs.rank(queries, top=10, words=False)
    rows_sub = cs.rank_last()["rows"]
    cs.rank(queries, top=10, words=True)
    assert 0 < cs.rank_last()["rows"] <= rows_sub
    assert [name for name, _ in cs.rank_files([b"the"], top=3, words=True)] == \
        [cs.corpus.names[d] for d in rr.rank_queries([[b"the"]], top=3)[1]]


# ---- 6. finditer and grep
@ends_at_a_fault
@pytest.mark.parametrize("mode", ["all", "longest", "disjoint"])
def test_finditer_words(plain, mode):
    hip, ref = plain
    regexes = ["he", "the", "x_1", "café".encode().decode("latin-1"), "th(e|en)", "a+n?", ".he", "zebra"]
    off, occ, truncated = hip.finditer(regexes, mode=mode, words=True)
    assert not truncated and off.size == len(regexes) + 1
    for i, rx in enumerate(regexes):
        hits = regex_hits(ref.text, rx)
        want = {"all": sorted(set(hits)), "longest": words_ref.longest(hits), "disjoint": words_ref.disjoint(hits)}[mode]
        mine = occ[int(off[i]):int(off[i + 1])]
        assert list(zip(mine["pos"].tolist(), mine["len"].tolist())) == want, rx
        assert (mine["group"] == i).all()
    assert off[1] > off[0] and off[-1] == off[-2]


@ends_at_a_fault
def test_finditer_does_not_consume_the_boundary():
    hip = H.from_text(b" he he ")
    try:
        off, occ, _ = hip.finditer(["he"], mode="disjoint", words=True)
        assert list(zip(occ["pos"].tolist(), occ["len"].tolist())) == [(1, 2), (4, 2)]
        assert hip.locate_words(b"he").tolist() == [1, 4]
    finally:
        hip.close()
    hip = H.from_text(b"he")                                                       # the whole text: both ends
    try:
        off, occ, _ = hip.finditer(["he", "h"], mode="all", words=True)
        assert off.tolist() == [0, 1, 1] and occ["pos"].tolist() == [0]
    finally:
        hip.close()


@ends_at_a_fault
def test_grep_words_across_files(files):
    cs, ref, docs = files
    off, occ, _ = cs.grep(["the", "then"], mode="all", words=True)
    want = [[(d, p) for d, doc in enumerate(docs) for p in words_ref.literal_word_starts(doc, q)] for q in (b"the", b"then")]
    for i in range(2):
        mine = occ[int(off[i]):int(off[i + 1])]
        assert list(zip(mine["doc"].tolist(), mine["raw_off"].tolist())) == want[i]
    assert (6, 9) in want[0] and (7, 0) in want[0] and (5, 0) in want[0]
    doc, raw = cs.locate_docs(b"the", words=True)
    assert list(zip(doc.tolist(), raw.tolist())) == want[0]
    loff, hits, _ = cs.grep_lines(["the"], words=True)
    assert sorted(set(hits["doc"].tolist())) == sorted({d for d, _ in want[0]})


def test_command_lines(tmp_path):
    root = tmp_path / "d"
    root.mkdir()
    (root / "a.txt").write_bytes(b"the cat\nconcatenate\nthen\n")
    (root / "b.txt").write_bytes(b"cat the\nthe\n")
    (root / "c.txt").write_bytes(b"catcat theme\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = tmp_path / "x"

    def run(*args):
        r = subprocess.run([sys.executable, "-m"] + list(args), cwd=ROOT, env=env, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout.split(b"\n")[:-1]

    run("findex_amd.index", "--dir", str(root), "--out", str(base))
    assert run("findex_amd.grep", str(base), "the", "cat", "-w", "-n") == \
        [b"a.txt:1:the cat", b"b.txt:1:cat the", b"b.txt:2:the", b"a.txt:1:the cat", b"b.txt:1:cat the"]
    got = [ln.split(b"\t")[1] for ln in run("findex_amd.rank", str(base), "cat", "-w")]
    assert sorted(got) == [b"a.txt", b"b.txt"]                                    # not c.txt: catcat is no word
