"""Ranked retrieval on the device (fmx_corpus_rank) through the C ABI against tests/rank_ref.py: the document
frequencies exactly, the default weights within 1e-12 of math.log, and -- given the weights the library returned -- offsets,
documents and the scores' bits exactly, for both match rules, both paths of the selection and the boundary between them, ties at
the threshold, a threshold decided in a key's last byte, the device form, capacity, and the command line."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_ref
import findex_amd
import rank_ref
from findex_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")

# planted words: upper case and digits, which the filler never holds; none is a substring of another
PLANTED = {b"Q09Z": 9, b"Q10Z": 10, b"Q11Z": 11, b"K1023Z": 1023, b"K1024Z": 1024, b"K1025Z": 1025, b"ALLZ": 2900}
N_DOCS, S1_SIZE, S2_SIZE = 3000, 600, 500


def filler(rng, n, escapes=0.1):
    """n raw bytes: letters, backslashes, and a share of the three escaped values (the small_docs recipe of test_gpu_corpus)."""
    b = rng.integers(97, 123, n, dtype=np.uint8)
    b[rng.random(n) < 0.02] = 92
    m = rng.random(n) < escapes
    b[m] = rng.choice(np.array([0, 1, 255], dtype=np.uint8), int(m.sum()))
    return b.tobytes()


def make_docs():
    rng = np.random.default_rng(2026)
    docs = [bytearray(filler(rng, int(n))) for n in rng.integers(0, 41, N_DOCS)]
    inner = np.arange(20, N_DOCS - 4)                               # the first twenty and the last four documents stay out of it
    for word, count in PLANTED.items():
        for d in rng.choice(inner, count, replace=False):
            for _ in range(int(rng.integers(1, 4))):                # tf 1 .. 3
                docs[d] += b" " + word
    both = rng.choice(inner, S1_SIZE + S2_SIZE, replace=False)      # S1, S2: disjoint, each word exactly once per document
    s1, s2 = np.sort(both[:S1_SIZE]), np.sort(both[S1_SIZE:])
    for d in s1:
        docs[d] += b"ONEZ"
    for d in s2:
        docs[d] += b"TWOZ"
    # EDGE: a document's first bytes, its last bytes before the separator, both, and the whole document
    docs[10] = bytearray(b"EDGE") + docs[10]
    docs[11] += b"EDGE"
    docs[12] = bytearray(b"EDGE") + docs[12] + b"EDGE"
    docs[13] = bytearray(b"EDGE")
    docs[14] = bytearray(b"EDGEDGE")                                # overlapping: tf 2
    for d in (0, 1, N_DOCS - 2, N_DOCS - 1):                        # empty documents at the start and at the end
        docs[d] = bytearray()
    return [bytes(d) for d in docs], s1.tolist(), s2.tolist()


@pytest.fixture(scope="module")
def world():
    docs, s1, s2 = make_docs()
    ref = corpus_ref.RefCorpus(docs)
    assert len(ref.stream) < (1 << 20)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    yield cs, rank_ref.RankRef(ref), s1, s2
    cs.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def check(cs, rr, queries, top=10, match="any", weights=None, k1=1.2, b=0.75):
    """One call against the checker: df exactly, the default weights within 1e-12, everything else bit for bit."""
    off, doc, score, df, w = cs.rank(queries, top=top, match=match, weights=weights, k1=k1, b=b)
    post = rr.postings(queries)
    assert df.tolist() == [len(p) for p in post]
    if weights is None:
        for got, want in zip(w.tolist(), rr.weights(post)):
            assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    else:
        assert bits(w) == bits(weights)
    eo, ed, es = rr.rank([len(q) for q in queries], post, w.tolist(), top=top, k1=k1, b=b, match=match)
    assert off.tolist() == eo
    assert doc.tolist() == ed
    assert bits(score) == bits(es)
    return off, doc, score


SIXTY_FOUR = [bytes([97 + i % 26, 97 + (7 * i + i // 26) % 26]) for i in range(64)]
assert len(set(SIXTY_FOUR)) == 64
QUERIES = [[b"ab"], [b"qu", b"x"], SIXTY_FOUR, [b"ab", b"ab"], [b"ab", b"ZZZZQQ"], [], [b"ZZZZQQ"], [b"\x00"], [b"\xff", b"a\x00"],
           [b"\x00\xff", b"\\"], [b"EDGE"], [b"EDGE", b"DGE", b"E"], [b"ALLZ", b"Q10Z", b"e"], [b"\x01"]]


# ---- 1. weights
def test_df_and_default_weights(world):
    cs, rr, _, _ = world
    terms = [b"ab", b"e", b"ALLZ", b"Q09Z", b"K1024Z", b"ZZZZQQ", b"\x00", b"\xff", b"EDGE", b"DGE", b"ONEZ", b"\x01\x00"]
    _, _, _, df, w = cs.rank([terms[:5], terms[5:]])
    want_df = [len(rr.tf(t)) for t in terms]
    assert df.tolist() == want_df
    assert want_df[2:6] == [2900, 9, 1024, 0] and want_df[8] == 5 and want_df[10] == S1_SIZE
    for got, d in zip(w.tolist(), want_df):
        want = math.log(1.0 + (float(N_DOCS - d) + 0.5) / (float(d) + 0.5))
        assert abs(got - want) <= 1e-12 * abs(want)
    # what the bound separates: a df off by one moves a weight by more than 1e-10 at this N
    assert all(abs(rank_ref.default_weight(N_DOCS, d) - rank_ref.default_weight(N_DOCS, d + 1)) > 1e-10 * rank_ref.default_weight(N_DOCS, d)
               for d in want_df)


# ---- 2. scores and order, bit for bit
@pytest.mark.parametrize("match", ["any", "all"])
@pytest.mark.parametrize("top", [1, 10, 1024])
def test_scores_and_order_bit_for_bit(world, match, top):
    cs, rr, _, _ = world
    off, doc, _ = check(cs, rr, QUERIES, top=top, match=match)
    assert off[6] == off[5] == off[4] if match == "all" else off[6] == off[5]       # no slots, no candidates: nothing
    if top == 1024 and match == "any":
        assert int(off[3] - off[2]) == 1024                                            # 64 common pairs: more candidates than top
        assert int(off[11] - off[10]) == 5 and sorted(doc[int(off[10]):int(off[11])].tolist()) == [10, 11, 12, 13, 14]


def test_no_queries_and_no_terms(world):
    cs, rr, _, _ = world
    off, doc, score, df, w = cs.rank([])
    assert off.tolist() == [0] and doc.size == 0 and score.size == 0 and df.size == 0
    off, doc, _, _, _ = cs.rank([[], []])
    assert off.tolist() == [0, 0, 0] and doc.size == 0
    check(cs, rr, [[b"ZZZZQQ"], [b"ZZZZQQ", b"QQZZZZ"]])                              # terms, but no rows at all


def test_other_parameters(world):
    cs, rr, _, _ = world
    for k1, b in ((0.0, 0.75), (2.0, 1.0), (0.9, 0.0), (1.2, 0.3)):
        check(cs, rr, QUERIES[:5] + QUERIES[10:13], top=7, k1=k1, b=b)
    w = [(-1.0) ** t * (0.25 + t) for t in range(sum(len(q) for q in QUERIES))]       # caller weights, negative ones too
    check(cs, rr, QUERIES, top=10, weights=w)
    check(cs, rr, QUERIES, top=10, weights=w, match="all")


# ---- 3. both select paths and the boundary between them
@pytest.mark.parametrize("top", [10, 1024])
def test_candidate_counts_around_top_and_around_1024(world, top):
    cs, rr, _, _ = world
    queries = [[w] for w in PLANTED]
    off, _, _ = check(cs, rr, queries, top=top)
    assert np.diff(off.astype(np.int64)).tolist() == [min(top, c) for c in PLANTED.values()]
    check(cs, rr, queries + [[b"ALLZ", b"e"], [b"K1025Z", b"K1023Z"]], top=top, match="all")
    check(cs, rr, [[b"K1024Z", b"ZZZZQQ"], [b"K1025Z", b"Q09Z"], [b"ALLZ", b"a", b"b"]], top=top)


# ---- 4. ties at the threshold
def test_ties_at_the_threshold_go_by_document():
    same = [b"one and the same text"] * 1500
    for docs, first in ((same, None), (same[:700] + [b"same same"] + same[701:], 700)):
        rr = rank_ref.RankRef(corpus_ref.RefCorpus(docs))
        cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
        _, doc, score = check(cs, rr, [[b"same"], [b"same", b"text"]], top=10)
        if first is None:
            assert doc[:10].tolist() == list(range(10)) and len(set(bits(score[:10]))) == 1
        else:
            assert doc[:10].tolist() == [first] + list(range(9)) and score[0] > score[1] and len(set(bits(score[1:10]))) == 1
        cs.close()


# ---- 5. a threshold decided in the key's last byte
def test_threshold_in_the_last_byte(world):
    cs, rr, s1, s2 = world
    up = math.nextafter(1.0, 2.0)
    assert (1.0 * (1.2 + 1.0)) / (1.0 + 1.2) == 1.0 and len(s1) + len(s2) > 1024
    off, doc, score = check(cs, rr, [[b"ONEZ", b"TWOZ"]], top=len(s2) + 3, weights=[1.0, up], k1=1.2, b=0.0)
    assert doc.tolist() == s2 + s1[:3]
    assert bits(score) == bits([up] * len(s2) + [1.0] * 3)
    # negated: the keys lie on the other side of the map's sign branch, and now S1 is the better set
    off, doc, score = check(cs, rr, [[b"ONEZ", b"TWOZ"]], top=len(s1) + 3, weights=[-1.0, -up], k1=1.2, b=0.0)
    assert doc.tolist() == s1 + s2[:3]
    assert bits(score) == bits([-1.0] * len(s1) + [-up] * 3)


# ---- 6. terms of different lengths in one call; max_per
def test_terms_of_different_lengths_share_a_call(world):
    cs, _, _, _ = world
    terms = [b"e", b"ab", b"ALLZ", b"K1025Z", b"\x00", b"a\x00", b"EDGEDGE"]
    off, doc, score, df, w = cs.rank([[t] for t in terms], top=20)
    for i, t in enumerate(terms):
        o1, d1, s1, df1, w1 = cs.rank([[t]], top=20)
        lo, hi = int(off[i]), int(off[i + 1])
        assert d1.tolist() == doc[lo:hi].tolist() and bits(s1) == bits(score[lo:hi])
        assert int(df1[0]) == int(df[i]) and bits(w1) == bits(w[i:i + 1])


@pytest.mark.parametrize("max_per", [1, 3, 50])
def test_max_per_takes_the_first_rows_of_every_slot(world, max_per):
    cs, rr, _, _ = world
    queries = [[b"e", b"ALLZ"], [b"ab"], [b"EDGE", b"Q11Z"]]
    terms = [t for q in queries for t in q]
    _, sp, ep = cs._intervals(terms)
    lo, sa = cs.searcher.locate_intervals(sp, ep, max_per=max_per)
    post = []
    for t in range(len(terms)):
        rows = sa[int(lo[t]):int(lo[t + 1])]
        d = cs.corpus.map(np.uint64(cs.corpus.stream_len - 1) - rows)[0]
        post.append({int(k): int(v) for k, v in zip(*np.unique(d, return_counts=True))})
        assert rows.size == min(max_per, int(ep[t] - sp[t]))
    off, doc, score, df, w = cs.rank(queries, top=10, max_per=max_per)
    assert df.tolist() == [len(p) for p in post]
    eo, ed, es = rr.rank([len(q) for q in queries], post, w.tolist(), top=10)
    assert off.tolist() == eo and doc.tolist() == ed and bits(score) == bits(es)


def test_rows_without_a_document_are_dropped(world):
    cs, rr, _, _ = world
    _, sp, ep = cs._intervals([b"EDGE"])
    # row 0 is the empty suffix: SA = stream length, no stream position
    sp2, ep2 = np.array([0, sp[0], 0], dtype=np.uint64), np.array([1, ep[0], 2], dtype=np.uint64)
    off, doc, score, df, w = cs.rank_intervals(sp2, ep2, np.array([0, 1, 2, 3], dtype=np.uint64), top=10)
    only = cs.rank([[b"EDGE"]], top=10)
    assert int(df[0]) == 0 and int(off[1]) == 0 and int(df[1]) == 5 and int(df[2]) == 1
    assert doc[int(off[1]):int(off[2])].tolist() == only[1].tolist() and bits(score[int(off[1]):int(off[2])]) == bits(only[2])


# ---- 7. the device form, captures, capacity
def raw_call(L, cs, sp, ep, q_off, prm, cap, guard=4):
    off = np.full(q_off.size + guard, 77, dtype=np.uint64)
    doc = np.full(cap + guard, 77, dtype=np.uint32)
    score = np.full(cap + guard, 77.0, dtype=np.float64)
    df = np.full(sp.size + guard, 77, dtype=np.uint32)
    w = np.full(sp.size + guard, 77.0, dtype=np.float64)
    vp = ctypes.c_void_p
    rc = L.fmx_corpus_rank(cs.corpus.handle, cs.searcher.handle, sp.ctypes.data_as(vp), ep.ctypes.data_as(vp), sp.size,
                           q_off.ctypes.data_as(vp), q_off.size - 1, ctypes.byref(prm), None, off.ctypes.data_as(vp),
                           doc.ctypes.data_as(vp), score.ctypes.data_as(vp), cap, df.ctypes.data_as(vp), w.ctypes.data_as(vp))
    return rc, off, doc, score, df, w


def test_dev_form_capacity_and_captures(world):
    import torch
    cs, rr, _, _ = world
    L = _lib.load()
    queries = [[b"ab", b"e"], [b"ALLZ"], [], [b"EDGE", b"ZZZZQQ"]]
    terms = [t for q in queries for t in q]
    _, sp, ep = cs._intervals(terms)
    sp, ep = np.ascontiguousarray(sp, dtype=np.uint64), np.ascontiguousarray(ep, dtype=np.uint64)
    q_off = np.array([0, 2, 3, 3, 5], dtype=np.uint64)
    prm = _lib.fmx_rank_params(1.2, 0.75, 0, 10, 0)
    total = 10 + 10 + 0 + 5
    rc, off, doc, score, df, w = raw_call(L, cs, sp, ep, q_off, prm, total)
    assert rc == 0 and off[:5].tolist() == [0, 10, 20, 20, 25]
    assert (off[5:] == 77).all() and (doc[total:] == 77).all() and (score[total:] == 77.0).all() and (df[5:] == 77).all() and (w[5:] == 77.0).all()
    h_off, h_doc, h_score, h_df, h_w = cs.rank(queries)
    assert off[:5].tolist() == h_off.tolist() and doc[:total].tolist() == h_doc.tolist() and bits(score[:total]) == bits(h_score)
    assert df[:5].tolist() == h_df.tolist() and bits(w[:5]) == bits(h_w)
    # a capacity too small: overflow, every offset written, nothing past the capacity
    rc2, off2, doc2, score2, _, _ = raw_call(L, cs, sp, ep, q_off, prm, total - 7)
    assert rc2 == 9 and b"room" in L.fmx_last_error()
    assert off2[:5].tolist() == off[:5].tolist() and (off2[5:] == 77).all()
    assert doc2[:total - 7].tolist() == doc[:total - 7].tolist() and bits(score2[:total - 7]) == bits(score[:total - 7])
    assert (doc2[total - 7:] == 77).all() and (score2[total - 7:] == 77.0).all()
    # the device form: the same bytes, guard words behind every buffer
    G = 4
    t = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda()
    dsp, dep, dq = t(sp), t(ep), t(q_off)
    d_off = torch.full((5 + G,), 77, dtype=torch.int64, device="cuda")
    d_doc = torch.full((total + G,), 77, dtype=torch.int32, device="cuda")
    d_score = torch.full((total + G,), 77.0, dtype=torch.float64, device="cuda")
    d_df = torch.full((5 + G,), 77, dtype=torch.int32, device="cuda")
    d_w = torch.full((5 + G,), 77.0, dtype=torch.float64, device="cuda")

    def dev(cap, stream=None, weights=None):
        return L.fmx_corpus_rank_dev(cs.corpus.handle, cs.searcher.handle, dsp.data_ptr(), dep.data_ptr(), 5, dq.data_ptr(), 4,
                                     ctypes.byref(prm), weights, d_off.data_ptr(), d_doc.data_ptr(), d_score.data_ptr(), cap,
                                     d_df.data_ptr(), d_w.data_ptr(), stream)
    torch.cuda.synchronize()
    _lib.check(dev(total))
    torch.cuda.synchronize()
    assert d_off.cpu().numpy().view(np.uint64).tolist() == off.tolist()
    assert d_doc.cpu().numpy().view(np.uint32).tolist() == doc.tolist()
    assert bits(d_score.cpu().numpy()) == bits(score)
    assert d_df.cpu().numpy().view(np.uint32).tolist() == df.tolist() and bits(d_w.cpu().numpy()) == bits(w)
    last = cs.rank_last()
    assert last["rows"] == int(np.where(ep > sp, ep - sp, 0).sum()) and last["postings"] == int(df[:5].sum()) and 0 < last["candidates"] <= last["postings"]
    # too small a capacity in the device form: the total is left in d_out_off for the caller, nothing past cap
    d_doc.fill_(77)
    d_score.fill_(77.0)
    _lib.check(dev(total - 7))
    torch.cuda.synchronize()
    assert d_off.cpu().numpy().view(np.uint64)[:5].tolist() == off[:5].tolist()
    assert d_doc.cpu().numpy().view(np.uint32)[:total - 7].tolist() == doc[:total - 7].tolist()
    assert (d_doc[total - 7:] == 77).all() and (d_score[total - 7:] == 77.0).all()
    # caller weights from device memory; a NaN among them is refused
    d_cw = torch.tensor([2.0, -1.0, 0.5, 3.0, 1.0], dtype=torch.float64, device="cuda")
    _lib.check(dev(total, weights=d_cw.data_ptr()))
    torch.cuda.synchronize()
    want = cs.rank(queries, weights=[2.0, -1.0, 0.5, 3.0, 1.0])
    assert d_doc.cpu().numpy().view(np.uint32)[:total].tolist() == want[1].tolist() and bits(d_score.cpu().numpy()[:total]) == bits(want[2])
    d_cw[2] = float("nan")
    torch.cuda.synchronize()
    assert dev(total, weights=d_cw.data_ptr()) == 3 and b"weights" in L.fmx_last_error()
    # under a stream capture the call is refused with a message and the capture stays valid
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        rc = dev(total, stream=s.cuda_stream)
        msg = L.fmx_last_error()
        d_df.zero_()                                                  # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert rc == 5 and b"stream capture" in msg
    del g
    # an index that is not this corpus' index is refused
    other = findex_amd.HipFMSearcher.from_text(b"abracadabra")
    rc = L.fmx_corpus_rank(cs.corpus.handle, other.handle, sp.ctypes.data, ep.ctypes.data, 5, q_off.ctypes.data, 4, ctypes.byref(prm),
                           None, off.ctypes.data, doc.ctypes.data, score.ctypes.data, total, None, None)
    assert rc == 3
    other.close()


# ---- 8. the document listing after the refactor
def test_doc_list_still_equals_numpy_unique(world):
    cs, rr, _, _ = world
    # (no 255 here: the filler holds backslashes and the letter f, which together read like its escape; occurrences()
    # looks at the raw files.  The filler holds no digits, so a raw 0 or 1 is not ambiguous.)
    queries = [b"ab", b"e", b"ALLZ", b"EDGE", b"\x00", b"a\x00", b"ZZZZQQ", b"K1025Z", b"\x00\x01", b"DGE"]
    off, doc, cnt = cs.list_docs(queries)
    assert off[0] == 0 and off.size == len(queries) + 1
    for i, q in enumerate(queries):
        d, n = np.unique(np.array([o[0] for o in rr.ref.occurrences(q)], dtype=np.uint32), return_counts=True)
        lo, hi = int(off[i]), int(off[i + 1])
        assert doc[lo:hi].tolist() == d.tolist() and cnt[lo:hi].tolist() == n.tolist(), q
    phases = [ctypes.c_double(-1.0) for _ in range(4)]
    _lib.check(_lib.load().fmx_corpus_doc_list_phases(*[ctypes.byref(p) for p in phases]))
    assert all(p.value >= 0.0 for p in phases) and sum(p.value for p in phases) > 0.0


# ---- 9. the same input twice
def test_same_input_same_bytes(world):
    cs, _, _, _ = world
    for match in ("any", "all"):
        a = cs.rank(QUERIES + [[w] for w in PLANTED], top=100, match=match)
        b = cs.rank(QUERIES + [[w] for w in PLANTED], top=100, match=match)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


# ---- 10. rank_files and the command line, on the reference's directory
def test_rank_files_and_cli_on_t1(tmp_path):
    root = os.path.join(TESTDATA, "t1")
    ref = corpus_ref.RefCorpus.from_dir(root)
    rr = rank_ref.RankRef(ref)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = tmp_path / "x"
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", "--dir", root, "--out", str(base)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    words = ["jerz CCC", "@@ uexm ttnx", "zzzzqq", "ab"]
    r = subprocess.run([sys.executable, "-m", "findex_amd.rank", str(base)] + words + ["--top", "2"], cwd=ROOT, env=env,
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split(b"\n")
    want_lines = []
    for i, q in enumerate(words):
        _, doc, score = rr.rank_queries([[w.encode() for w in q.split()]], top=2)
        if i:
            want_lines.append(None)
        want_lines += [(ref.names[d], s) for d, s in zip(doc, score)]
    assert got[-1] == b"" and len(got) - 1 == len(want_lines)
    for ln, want in zip(got, want_lines):
        if want is None:
            assert ln == b""
        else:
            s, name = ln.split(b"\t")
            assert name == want[0] and abs(float(s) - want[1]) <= 1e-12 * abs(want[1])
    assert got[0].endswith(b".txt") and b"" in got[:-1]
    # --all through the command line, and rank_files in this process
    r = subprocess.run([sys.executable, "-m", "findex_amd.rank", str(base), "jerz CCC", "--all"], cwd=ROOT, env=env,
                       capture_output=True, timeout=600)
    assert r.returncode == 0 and [ln.split(b"\t")[1] for ln in r.stdout.split(b"\n") if ln] == \
        [ref.names[d] for d in rr.rank_queries([[b"jerz", b"CCC"]], match="all")[1]]
    cs = findex_amd.HipCorpusSearcher.open(base)
    for terms, match in (([b"jerz", b"CCC"], "any"), ([b"@@", b"uexm", b"ttnx"], "any"), ([b"jerz", b"@"], "all")):
        files = cs.rank_files(terms, top=3, match=match)
        _, doc, score = rr.rank_queries([terms], top=3, match=match)
        assert [f[0] for f in files] == [ref.names[d] for d in doc] and len(files) > 0
        for (_, s), want in zip(files, score):
            assert abs(s - want) <= 1e-12 * abs(want)
    cs.close()
