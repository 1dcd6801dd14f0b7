"""Passages on the device (fmx_corpus_passages) through the C ABI against tests/passages_ref.py: records and
counts bit for bit (values as uint64 views) at the occurrence counts around a wave, a workgroup and the wave's loop, for
every query shape, window length, tie, escape and set the contract names; the counts reproduce the ranking's score; the
device form, capacity, refusals, captures; rank_files and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_ref
import findex_amd
import passages_ref
import rank_ref
from findex_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")

N_DOCS = 3000
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]                  # PLNT per file: the wave's edge, the workgroup's edge
CNT_DOC = {k: 100 + i for i, k in enumerate(COUNTS)}
BIG, BIG_DOC = 5000, 120                                    # the loop of one wave
# planted files: upper case and digits, which the filler never holds
SPECIAL = {
    200: b"xxALPHAyyyyBETAzz",                              # ALPHA at 2, BETA at 11: the span of both is 13 bytes
    201: b"EDGE" + b"qrs" * 5 + b"EDGE",                    # a file's first and last bytes
    202: b"EDGEDGE",                                        # overlapping occurrences
    203: b"zzzzLEFT", 204: b"RIGHTzzz",                     # neighbours: 5 stream bytes apart, across a separator
    205: b"TIEAqqqqqqqqqqqqTIEA",                           # two windows of one value
    206: b"AA1BB2" + b"w" * 20 + b"CC3",                    # weights 1, 2, 3: {0, 1} ties {2}
    207: b"CC3" + b"w" * 20 + b"AA1BB2",                    # the same with {2} first
    208: b"CEEDEEDOT",                                      # weights 1e16, 1, -1e16: all three in every window that holds CEE
    209: b"POSxNEGyyyyyyyyPOS",                             # a negative weight
    210: b"a\x00b\xff0\x00\x00c0\xff",                      # escapes; 0 also matches the second byte of a pair
    211: b"Error error ERROR errors _error error.",         # case and words
    212: b"",                                               # an empty file as a hit
}


def filler(rng, n, escapes=0.1):
    b = rng.integers(97, 123, n, dtype=np.uint8)
    b[rng.random(n) < 0.02] = 92
    m = rng.random(n) < escapes
    b[m] = rng.choice(np.array([0, 1, 255], dtype=np.uint8), int(m.sum()))
    return b.tobytes()


def planted(rng, k, marks):
    """k times PLNT with 0 .. 3 letters between two of them, and QX behind the occurrences listed in `marks`."""
    out = bytearray(b"qq")
    for i in range(k):
        out += b"PLNT" + rng.integers(97, 123, int(rng.integers(0, 4)), dtype=np.uint8).tobytes()
        if i in marks:
            out += b"QX"
    return bytes(out) if k else b"qqqqQXqq"


def make_docs():
    rng = np.random.default_rng(2029)
    docs = [filler(rng, int(n)) for n in rng.integers(0, 41, N_DOCS)]
    for k, d in CNT_DOC.items():
        docs[d] = planted(rng, k, {k // 2})
    docs[BIG_DOC] = planted(rng, BIG, {7, 2500, 4999})
    for d, text in SPECIAL.items():
        docs[d] = text
    return docs


@pytest.fixture(scope="module")
def world():
    docs = make_docs()
    ref = corpus_ref.RefCorpus(docs)
    assert len(ref.stream) < (1 << 20)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    yield cs, passages_ref.PassagesRef(ref), rank_ref.RankRef(ref), docs
    cs.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def same(psg, tf, recs, rows):
    assert psg.size == len(recs) and tf.shape[0] == len(rows)
    assert psg["raw_off"].tolist() == [r[0] for r in recs]
    assert psg["mask"].tolist() == [r[1] for r in recs]
    assert bits(psg["value"]) == bits([r[2] for r in recs])
    assert psg["raw_len"].tolist() == [r[3] for r in recs]
    assert psg["n_occ"].tolist() == [r[4] for r in recs]
    assert tf.tolist() == rows


def check(world, queries, hit_off, hit_doc, window, weights=None, **kw):
    cs, pr = world[0], world[1]
    psg, tf = cs.passages(queries, hit_off, hit_doc, window=window, weights=weights, **kw)
    recs, rows = pr.run(queries, hit_off, hit_doc, window, weights=weights, **kw)
    same(psg, tf, recs, rows)
    return psg, tf


# ---- 1. occurrence counts per hit: 0, 1, the wave's edge, the workgroup's edge, one wave's loop
@pytest.mark.parametrize("window", [4, 9, 40, 100000])
def test_occurrence_counts_per_hit(world, window):
    files = [BIG_DOC] + [CNT_DOC[k] for k in reversed(COUNTS)]        # not in file order; every file a hit of both queries
    psg, tf = check(world, [[b"PLNT"], [b"QX", b"PLNT"]], [0, len(files), 2 * len(files)], files + files[::-1], window,
                    weights=[1.0, 5.0, 1.0])
    assert tf[:len(files), 0].tolist() == [BIG] + COUNTS[::-1]
    assert psg["n_occ"][:len(files)].tolist() == [BIG] + COUNTS[::-1]
    assert psg["n_occ"][len(files)] == 1 and psg["mask"][len(files)] == 1 and tf[len(files)].tolist() == [1, 0]      # the file without PLNT
    assert psg[len(files) - 1].tobytes() == bytes(32)                  # no occurrence: all zeros
    if window >= 9:
        assert (psg["mask"][len(files) + 1:] == 3).all()               # QX and a PLNT behind it fit 9 bytes


# ---- 2. query shapes
SIXTY_FOUR = [bytes([97 + i % 26, 97 + (7 * i + i // 26) % 26]) for i in range(64)]


def test_query_shapes(world):
    cs = world[0]
    d = CNT_DOC[65]
    off, doc, _, _, _ = cs.rank([SIXTY_FOUR], top=10)
    assert doc.size == 10
    psg, tf = check(world, [SIXTY_FOUR], off, doc, 12, weights=[float(1 + t % 7) for t in range(64)])
    assert tf.shape == (10, 64) and (psg["n_occ"] == tf.sum(axis=1)).all()
    check(world, [[b"PLNT"], [b"PLNT", b"QX"]], [0, 1, 2], [d, d], 30)
    psg, tf = check(world, [[b"PLNT", b"PLNT"]], [0, 2], [d, BIG_DOC], 30)              # a term twice: two slots, both covered
    assert psg["mask"].tolist() == [3, 3] and psg["value"].tolist() == [2.0, 2.0] and tf.tolist() == [[65, 65], [BIG, BIG]]
    # a query with hits and no slots; a query with slots and no hits; the stride is the longest query's
    psg, tf = check(world, [[], [b"PLNT", b"QX", b"a"], [b"QX"]], [0, 2, 2, 4], [d, 5, BIG_DOC, d], 30)
    assert psg[:2].tobytes() == bytes(64) and tf.shape == (4, 3) and tf[2:].tolist() == [[3, 0, 0], [1, 0, 0]]
    psg, tf = check(world, [[], []], [0, 1, 3], [3, 4, 5], 30)                          # no slots at all
    assert tf.shape == (3, 0) and psg.tobytes() == bytes(96)
    psg, tf = check(world, [[b"PLNT"]], [0, 0], [], 30)                                 # no hits at all
    assert psg.size == 0 and tf.shape == (0, 1)
    check(world, [[b"ZZZZQQ", b"QQZZZZ"]], [0, 2], [d, 7], 30)                          # terms, but no rows
    check(world, [[b"PLNT"]], [0, 3], [3, 4, 212], 30)                                  # rows, but none in a hit (212 is empty)


# ---- 3. windows
def test_windows(world):
    one = lambda q, d, w, **kw: check(world, [q], [0, 1], [d], w, **kw)[0][0]
    p = one([b"ALPHA"], 200, 4)                                                         # a byte shorter than the term
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"]), int(p["raw_len"]), int(p["n_occ"])) == (2, 0, 0.0, 4, 1)
    p = one([b"ALPHA"], 200, 5)                                                         # the term's length
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"]), int(p["raw_len"])) == (2, 1, 1.0, 5)
    p = one([b"ALPHA", b"BETA"], 200, 13)                                               # the exact span of both
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"]), int(p["raw_len"])) == (2, 3, 2.0, 13)
    p = one([b"ALPHA", b"BETA"], 200, 12)                                               # one byte less: ALPHA alone, the smaller start
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"])) == (2, 1, 1.0)
    p = one([b"BETA", b"ALPHA"], 200, 1000)                                             # longer than the file: clipped at its last byte
    assert (int(p["raw_off"]), int(p["mask"]), int(p["raw_len"])) == (2, 3, 15)
    p = one([b"EDGE"], 201, 4)                                                          # a file's first bytes ..
    assert (int(p["raw_off"]), int(p["raw_len"]), int(p["n_occ"])) == (0, 4, 2)
    p = one([b"zzz", b"EDGE"], 201, 50, weights=[1.0, 1.0])
    assert int(p["mask"]) == 2
    p = one([b"qrsEDGE", b"EDGE"], 201, 7)                                              # .. and its last: the window ends at the separator
    assert (int(p["raw_off"]), int(p["mask"]), int(p["raw_len"])) == (16, 3, 7)
    # two neighbours, LEFT at the end of one and RIGHT at the start of the next: neither window holds both
    psg, _ = check(world, [[b"LEFT", b"RIGHT"]], [0, 2], [204, 203], 64)
    assert psg["mask"].tolist() == [2, 1] and psg["raw_off"].tolist() == [0, 4] and psg["raw_len"].tolist() == [8, 4]
    for w in (1, 2, 3, 6, 7, 8, 40, (1 << 32) - 1):
        check(world, [[b"EDGE", b"DGE", b"E"], [b"a", b"b", b"\\"]], [0, 2, 6], [201, 202, 3, 4, 5, 6], w)


# ---- 4. ties and the order of the additions
def test_ties_and_order(world):
    one = lambda q, d, w, **kw: check(world, [q], [0, 1], [d], w, **kw)[0][0]
    p = one([b"TIEA"], 205, 10)
    assert (int(p["raw_off"]), float(p["value"]), int(p["n_occ"])) == (0, 1.0, 2)
    p = one([b"AA1", b"BB2", b"CC3"], 206, 8, weights=[1.0, 2.0, 3.0])                  # {0, 1} first, {2} later: equal, the smaller start
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"])) == (0, 3, 3.0)
    p = one([b"AA1", b"BB2", b"CC3"], 207, 8, weights=[1.0, 2.0, 3.0])
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"])) == (0, 4, 3.0)
    p = one([b"CEE", b"DEE", b"DOT"], 208, 9, weights=[1e16, 1.0, -1e16])               # 0.0 in slot order, 1.0 in any other
    assert (int(p["raw_off"]), int(p["mask"]), bits([p["value"]])) == (0, 7, bits([0.0]))
    p = one([b"CEE", b"DOT", b"DEE"], 208, 9, weights=[1e16, -1e16, 1.0])
    assert (int(p["mask"]), float(p["value"])) == (7, 1.0)
    p = one([b"POS", b"NEG"], 209, 8, weights=[1.0, -2.0])                              # the window without NEG wins
    assert (int(p["raw_off"]), int(p["mask"]), float(p["value"])) == (15, 1, 1.0)
    p = one([b"NEG"], 209, 8, weights=[-2.0])                                           # only negative windows: still the best of them
    assert (int(p["raw_off"]), float(p["value"])) == (4, -2.0)


# ---- 5. escapes
def test_escapes(world):
    d = 210                                                 # raw a 00 b ff 0 00 00 c 0 ff: the stream a\0b\f0\0\0c0\f, 15 bytes
    for w in (1, 2, 3, 4, 5, 6, 7, 14, 15):
        check(world, [[b"\x00"], [b"\xff"], [b"a\x00"], [b"0"], [b"\x00", b"\xff", b"a\x00", b"0", b"\x00\x00"]], [0, 1, 2, 3, 4, 5],
              [d] * 5, w)
    p = check(world, [[b"a\x00"]], [0, 1], [d], 5)[0][0]   # the window ends between the two bytes of the \f pair: its raw byte counts
    assert (int(p["raw_off"]), int(p["raw_len"]), int(p["mask"])) == (0, 4, 1)
    p, tf = check(world, [[b"0"]], [0, 1], [d], 1)
    assert tf.tolist() == [[5]] and int(p[0]["raw_off"]) == 1                           # the first 0 is the second byte of raw byte 1's pair
    off, doc, _, _, _ = world[0].rank([[b"\x00", b"\xff"], [b"\\", b"0", b"f"]], top=20)
    check(world, [[b"\x00", b"\xff"], [b"\\", b"0", b"f"]], off, doc, 6)               # the filler's escapes, in the ranking's order


# ---- 6. overlaps
def test_overlapping_occurrences(world):
    for w, want in ((3, (0, 0, 0.0, 3)), (4, (0, 1, 1.0, 4)), (7, (0, 1, 1.0, 7)), (100, (0, 1, 1.0, 7))):
        p, tf = check(world, [[b"EDGE"]], [0, 1], [202], w)
        assert (int(p[0]["raw_off"]), int(p[0]["mask"]), float(p[0]["value"]), int(p[0]["raw_len"])) == want and tf.tolist() == [[2]]


# ---- 7. sets of intervals: case, words, and the two forms of one slot per interval
def test_case_words_and_set_forms(world):
    cs = world[0]
    q = [[b"error", b"Error"], [b"ERROR"]]
    hits = ([0, 2, 3], [211, 5, 211])
    for kw in ({"ignore_case": True}, {"words": True}, {"words": True, "ignore_case": True}):
        psg, tf = check(world, q, hits[0], hits[1], 12, **kw)
    assert tf[0].tolist() == [4, 4] and tf[2].tolist() == [4, 0]                        # whole words, any case: Error, error, ERROR, error.
    psg, tf = check(world, q, hits[0], hits[1], 12)
    assert tf[0].tolist() == [4, 1] and tf[2].tolist() == [1, 0]
    off, doc, _, _, _ = cs.rank([[b"ab", b"e"]], top=10, ignore_case=True)
    check(world, [[b"ab", b"e"]], off, doc, 10, ignore_case=True)
    # set_off = NULL and set_off = 0, 1, .., n_terms: the same bytes
    queries = [[b"PLNT", b"QX"], [b"a", b"b", b"c"]]
    q_off, (sp, ep, so, tl) = cs._query_slots(queries, False, False)
    assert so is None
    h_off, h_doc = [0, 2, 5], [BIG_DOC, CNT_DOC[64], 3, 4, 5]
    a = cs.passages_sets_intervals(sp, ep, None, tl, q_off, h_off, h_doc, window=9)
    b = cs.passages_sets_intervals(sp, ep, np.arange(6, dtype=np.uint64), tl, q_off, h_off, h_doc, window=9)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0]["n_occ"][0] == BIG + 3


# ---- 8. the explanation is an explanation: the counts and the weights reproduce the ranking's score
@pytest.mark.parametrize("match", ["any", "all"])
def test_counts_reproduce_the_score(world, match):
    cs, pr, rr, _ = world
    queries = [[b"PLNT", b"QX", b"q"], [b"ab", b"e", b"\x00"], [b"EDGE", b"DGE"], [b"a"]]
    off, doc, score, df, w, psg, tf = cs.rank_passages(queries, top=10, window=20, match=match)
    assert int(off[-1]) == doc.size > 10 and tf.shape == (doc.size, 3)
    at = 0
    for i, q in enumerate(queries):
        for h in range(int(off[i]), int(off[i + 1])):
            got = rr.score(int(doc[h]), tf[h, :len(q)].tolist(), w[at:at + len(q)].tolist(), 1.2, 0.75)
            assert bits([got]) == bits([score[h]]), (i, h)
        at += len(q)
    recs, rows = pr.run(queries, off, doc, 20, weights=w.tolist())                      # hits in the ranking's score order
    same(psg, tf, recs, rows)
    only = cs.rank(queries, top=10, match=match)
    assert only[1].tobytes() == doc.tobytes() and only[2].tobytes() == score.tobytes()


# ---- 9. max_per: the first rows of every interval, as locate takes them
@pytest.mark.parametrize("max_per", [1, 3, 50])
def test_max_per_takes_the_first_rows_of_every_interval(world, max_per):
    cs, pr, _, _ = world
    queries = [[b"PLNT", b"QX"], [b"e", b"EDGE"]]
    h_off, h_doc = [0, 3, 6], [BIG_DOC, CNT_DOC[257], CNT_DOC[1], 201, 202, 3]
    terms = [t for q in queries for t in q]
    q_off, (sp, ep, _, tl) = cs._query_slots(queries, False, False)
    lo, sa = cs.searcher.locate_intervals(sp, ep, max_per=max_per)
    recs, rows = [], []
    for i, q in enumerate(queries):
        for h in range(h_off[i], h_off[i + 1]):
            occ = []
            for t in range(int(q_off[i]), int(q_off[i + 1])):
                rows_t = sa[int(lo[t]):int(lo[t + 1])]
                if rows_t.size == 0:
                    occ.append([])
                    continue
                e = np.uint64(cs.corpus.stream_len - 1) - rows_t
                d = cs.corpus.map(e)[0]
                occ.append(sorted((e[d == h_doc[h]] - np.uint64(int(tl[t]) - 1)).tolist()))
            rec, tf = pr.passage(h_doc[h], occ, [int(x) for x in tl[int(q_off[i]):int(q_off[i + 1])]], [1.0] * len(q), 30)
            recs.append(rec)
            rows.append(tf)
    psg, tf = cs.passages(queries, h_off, h_doc, window=30, max_per=max_per)
    same(psg, tf, recs, rows)
    assert int(tf.sum()) <= max_per * len(terms)


# ---- 10. the device form, capacity, refusals, captures, the same input twice
def test_dev_form_capacity_and_refusals(world):
    import torch
    cs, pr, _, _ = world
    L = _lib.load()
    vp = ctypes.c_void_p
    queries = [[b"PLNT", b"QX"], [], [b"EDGE"]]
    q_off, (sp, ep, _, tl) = cs._query_slots(queries, False, False)
    sp, ep = np.ascontiguousarray(sp, dtype=np.uint64), np.ascontiguousarray(ep, dtype=np.uint64)
    h_off = np.array([0, 3, 4, 6], dtype=np.uint64)
    h_doc = np.array([CNT_DOC[256], BIG_DOC, CNT_DOC[0], 7, 202, 201], dtype=np.uint32)
    w = np.array([1.0, 4.0, 0.5])
    n_hits, stride, G = 6, 2, 4
    want = cs.passages_sets_intervals(sp, ep, None, tl, q_off, h_off, h_doc, window=9, weights=w)
    recs, rows = pr.run(queries, h_off, h_doc, 9, weights=w.tolist())
    same(want[0], want[1], recs, rows)
    assert cs.passages_sets_intervals(sp, ep, None, tl, q_off, h_off, h_doc, window=9, weights=w)[0].tobytes() == want[0].tobytes()
    last = cs.passages_last()
    assert last["hits"] == 6 and last["rows"] == int((ep - sp).sum()) and last["occurrences"] == int(want[0]["n_occ"].sum())
    assert last["locate_ms"] > 0 and last["window_ms"] > 0 and last["filter_ms"] > 0 and last["sort_ms"] > 0
    prm = _lib.fmx_passage_params(9, 0, 0, 0)

    def host(cap, doc=h_doc, guard=G):
        out = np.full((cap + guard) * 4, 77, dtype=np.uint64)
        tf = np.full((cap + guard) * stride, 77, dtype=np.uint32)
        st = ctypes.c_uint32(99)
        rc = L.fmx_corpus_passages(cs.corpus.handle, cs.searcher.handle, sp.ctypes.data_as(vp), ep.ctypes.data_as(vp), sp.size, None, 3,
                                   tl.ctypes.data_as(vp), q_off.ctypes.data_as(vp), 3, h_off.ctypes.data_as(vp), doc.ctypes.data_as(vp),
                                   w.ctypes.data_as(vp), ctypes.byref(prm), out.ctypes.data_as(vp), tf.ctypes.data_as(vp), cap,
                                   ctypes.byref(st))
        return rc, out, tf, st.value
    rc, out, tf, st = host(n_hits)
    assert rc == 0 and st == stride and out[:24].tobytes() == want[0].tobytes() and tf[:12].tolist() == want[1].reshape(-1).tolist()
    assert (out[24:] == 77).all() and (tf[12:] == 77).all()
    # a capacity one short: overflow, the first cap hits written, nothing behind them
    rc, out2, tf2, st = host(n_hits - 1)
    assert rc == 9 and b"room" in L.fmx_last_error() and st == stride
    assert out2[:20].tobytes() == out[:20].tobytes() and tf2[:10].tolist() == tf[:10].tolist()
    assert (out2[20:] == 77).all() and (tf2[10:] == 77).all()
    # a (query, document) pair twice; a document past the corpus
    bad = h_doc.copy()
    bad[1] = bad[0]
    rc, _, _, _ = host(n_hits, doc=bad)
    assert rc == 3 and b"twice" in L.fmx_last_error() and str(CNT_DOC[256]).encode() in L.fmx_last_error()
    bad = h_doc.copy()
    bad[4] = N_DOCS
    rc, _, _, _ = host(n_hits, doc=bad)
    assert rc == 3 and str(N_DOCS).encode() in L.fmx_last_error()
    bad = h_doc.copy()
    bad[3] = bad[0]                                                                      # the same file in another query: fine
    assert host(n_hits, doc=bad)[0] == 0
    # the device form: the same bytes, guard words behind the records and the counts
    t = lambda a: torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()
    dsp, dep, dtl, dq, dho, dhd, dw = t(sp), t(ep), t(tl), t(q_off), t(h_off), t(h_doc), torch.from_numpy(w).cuda()
    d_out = torch.full(((n_hits + G) * 4,), 77, dtype=torch.int64, device="cuda")
    d_tf = torch.full(((n_hits + G) * stride,), 77, dtype=torch.int32, device="cuda")

    def dev(cap, stream=None):
        st = ctypes.c_uint32(99)
        rc = L.fmx_corpus_passages_dev(cs.corpus.handle, cs.searcher.handle, dsp.data_ptr(), dep.data_ptr(), sp.size, None, 3,
                                       dtl.data_ptr(), dq.data_ptr(), 3, dho.data_ptr(), dhd.data_ptr(), dw.data_ptr(), ctypes.byref(prm),
                                       d_out.data_ptr(), d_tf.data_ptr(), cap, ctypes.byref(st), stream)
        return rc, st.value
    torch.cuda.synchronize()
    assert dev(n_hits) == (0, stride)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().view(np.uint64).tolist() == out.tolist()
    assert d_tf.cpu().numpy().view(np.uint32).tolist() == tf.tolist()
    d_out.fill_(77)
    d_tf.fill_(77)
    torch.cuda.synchronize()
    assert dev(n_hits - 1) == (9, stride)
    torch.cuda.synchronize()
    got_out, got_tf = d_out.cpu().numpy().view(np.uint64), d_tf.cpu().numpy().view(np.uint32)
    assert got_out[:20].tolist() == out[:20].tolist() and got_tf[:10].tolist() == tf[:10].tolist()
    assert (got_out[20:] == 77).all() and (got_tf[10:] == 77).all()
    # under a stream capture the call is refused with a message and the capture stays valid
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        rc, _ = dev(n_hits, stream=s.cuda_stream)
        msg = L.fmx_last_error()
        d_tf.zero_()                                                  # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert rc == 5 and b"stream capture" in msg
    del g
    # an index that is not this corpus' index is refused
    other = findex_amd.HipFMSearcher.from_text(b"abracadabra")
    out3, tf3, st3 = np.zeros(24, dtype=np.uint64), np.zeros(12, dtype=np.uint32), ctypes.c_uint32(0)
    rc = L.fmx_corpus_passages(cs.corpus.handle, other.handle, sp.ctypes.data_as(vp), ep.ctypes.data_as(vp), sp.size, None, 3,
                               tl.ctypes.data_as(vp), q_off.ctypes.data_as(vp), 3, h_off.ctypes.data_as(vp), h_doc.ctypes.data_as(vp),
                               None, ctypes.byref(prm), out3.ctypes.data_as(vp), tf3.ctypes.data_as(vp), 6, ctypes.byref(st3))
    assert rc == 3
    other.close()


def test_same_input_same_bytes(world):
    cs = world[0]
    queries = [[b"PLNT", b"QX", b"q"], SIXTY_FOUR, [b"e", b"a", b"\x00"]]
    a = cs.rank_passages(queries, top=50, window=33)
    b = cs.rank_passages(queries, top=50, window=33)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---- 11. rank_files with a window, and the command line, on the reference's directory
def shown(text):
    return bytes(32 if c < 0x20 else c for c in text)


def test_rank_files_and_cli_on_t1(world, tmp_path):
    cs, pr, _, docs = world
    files = cs.rank_files([b"PLNT", b"QX"], top=4, window=12)
    off, doc, score, _, w = cs.rank([[b"PLNT", b"QX"]], top=4)
    recs, _ = pr.run([[b"PLNT", b"QX"]], off, doc, 12, weights=w.tolist())
    assert files == [(cs.corpus.names[int(d)], float(s), r[0], docs[int(d)][r[0]:r[0] + r[3]]) for d, s, r in zip(doc, score, recs)]
    assert len(files) == 4 and all(b"QX" in f[3] and b"PLNT" in f[3] for f in files)
    assert cs.rank_files([b"PLNT", b"QX"], top=4) == [f[:2] for f in files]              # the default is unchanged
    assert cs.rank_files([b"ZZZZQQ"], window=12) == []
    root = os.path.join(TESTDATA, "t1")
    ref = corpus_ref.RefCorpus.from_dir(root)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = tmp_path / "x"
    from findex_amd import index
    assert index.main(["--dir", root, "--out", str(base)]) == 0                          # (in this process: the test is about `rank`)
    words = ["jerz CCC", "@@ uexm ttnx", "zzzzqq"]
    cmd = [sys.executable, "-m", "findex_amd.rank", str(base)] + words + ["--top", "2"]
    runs = [subprocess.Popen(c, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)       # side by side
            for c in (cmd, cmd + ["--snippets", "40", "--explain"])]
    (plain_out, plain_err), (full_out, full_err) = [p.communicate(timeout=600) for p in runs]
    assert runs[0].returncode == 0 and runs[1].returncode == 0, (plain_err, full_err)
    queries = [[w.encode() for w in q.split()] for q in words]
    t1 = findex_amd.HipCorpusSearcher.open(base)
    off, doc, score, _, w = t1.rank(queries, top=2)
    t1.close()
    recs, rows = passages_ref.PassagesRef(ref).run(queries, off, doc, 40, weights=w.tolist())
    want_plain, want_full = [], []
    for i, q in enumerate(queries):
        if i:
            want_plain.append(b"")
            want_full.append(b"")
        for h in range(int(off[i]), int(off[i + 1])):
            head = repr(float(score[h])).encode() + b"\t" + ref.names[int(doc[h])]
            a, n = recs[h][0], recs[h][3]
            want_plain.append(head)
            want_full += [head, b"\t%d\t" % a + shown(ref.docs[int(doc[h])][a:a + n]),
                          b"\t" + b" ".join(t + b"=%d" % rows[h][s] for s, t in enumerate(q))]
    assert plain_out.split(b"\n") == want_plain + [b""]                                  # without the flags: today's lines
    assert full_out.split(b"\n") == want_full + [b""]
    assert len(want_full) > len(want_plain) >= 4 and any(ln.startswith(b"\t") and b"jerz=" in ln for ln in want_full)
