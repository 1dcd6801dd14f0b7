"""The corpus map and the document listing at hundreds to tens of thousands of documents, bit for bit against
tests/corpus_ref.py: the map at every stream position; the listing of 92 queries; interval lists that take the listing's
radix sort through 2, 3, 4 and 5 passes (keys of 9 to 33 bits), many radix tiles, a scan of two and of three levels and
k_loc_scan through dozens of its 1024-interval chunks; max_per, the capacity rules, rows that are no stream position
(listed as UINT32_MAX), locate_docs and read.  The corpora and the interval lists come from tests/corpus_many.py, whose
shapes tests/test_corpus_cpu.py asserts."""
import ctypes

import numpy as np
import pytest

import corpus_many
import corpus_ref
import findex_amd
from findex_amd import _lib

pytestmark = pytest.mark.gpu

NO_DOC = corpus_many.NO_DOC


class Many:
    """One corpus: its documents, the reference, the device corpus with its index, and the reference's listings."""

    def __init__(self, name):
        self.name = name
        self.docs = corpus_many.documents(name)
        self.ref = corpus_ref.RefCorpus(self.docs)
        self.cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(self.docs))
        self.n = len(self.ref.stream)
        self._counts = {}
        self._table = None

    def doc_counts(self, q):
        if q not in self._counts:
            self._counts[q] = corpus_many.expected_doc_counts(self.ref, q)
        return self._counts[q]

    def table(self):
        """ref.table as an int64 array (n, 3)."""
        if self._table is None:
            self._table = np.array(self.ref.table, dtype=np.int64).reshape(-1, 3)
        return self._table


_made = {}


@pytest.fixture(scope="module")
def corpora():
    def get(name):
        if name not in _made:
            _made[name] = Many(name)
        return _made[name]
    yield get
    for m in _made.values():
        m.cs.close()
    _made.clear()


def assert_csr(got, want, what):
    for g, w, nm in zip(got, want, ("off", "doc", "cnt")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, nm)


# ---- 1. the map
def map_positions(n):
    return np.concatenate([np.arange(n, dtype=np.uint64), np.array([n, n + 5, 2 ** 32 + 5, 2 ** 63], dtype=np.uint64)])


def map_expected(m):
    t = m.table()
    past = np.full(4, -1, dtype=np.int64)
    doc = np.concatenate([t[:, 0], past]).astype(np.uint32)                   # -1 -> UINT32_MAX
    eo = np.concatenate([t[:, 1], past]).view(np.uint64)
    ro = np.concatenate([t[:, 2], past]).view(np.uint64)
    assert doc[-1] == NO_DOC and eo[-1] == 2 ** 64 - 1 and m.ref.map(m.n) == (int(doc[-4]), int(eo[-4]), int(ro[-4]))
    return doc, eo, ro


def assert_map(got, want, what):
    for g, w, nm in zip(got, want, ("doc", "esc_off", "raw_off")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm)


@pytest.mark.parametrize("name", ["D256", "D5000", "D65537"])
def test_map_at_every_position(corpora, name):
    m = corpora(name)
    assert m.cs.corpus.info()[:3] == (len(m.docs), m.n, len(m.ref.esc_pos))
    assert_map(m.cs.corpus.map(map_positions(m.n)), map_expected(m), name)


def test_map_dev_on_a_side_stream_with_guards(corpora):
    import torch
    m = corpora("D5000")
    pos = map_positions(m.n)
    k, guard = pos.size, 64
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dpos = torch.from_numpy(pos.view(np.int64)).cuda()
        doc = torch.full((k + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        eo = torch.full((k + guard,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        ro = torch.full((k + guard,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        m.cs.corpus.map_dev(dpos.data_ptr(), k, doc.data_ptr(), eo.data_ptr(), ro.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    doc, eo, ro = doc.cpu().numpy(), eo.cpu().numpy(), ro.cpu().numpy()
    assert_map((doc[:k].view(np.uint32), eo[:k].view(np.uint64), ro[:k].view(np.uint64)), map_expected(m), "map_dev")
    assert np.all(doc[k:] == 0x5A5A5A5A) and np.all(eo[k:] == 0x5A5A5A5A5A5A) and np.all(ro[k:] == 0x5A5A5A5A5A5A)


def test_map_of_a_corpus_rebuilt_from_its_tables(corpora):
    m = corpora("D5000")
    ds, rl, ep = m.cs.corpus.tables()
    assert ds.tolist() == m.ref.doc_start and rl.tolist() == m.ref.raw_len and ep.tolist() == m.ref.esc_pos
    h = ctypes.c_void_p()
    _lib.check(_lib.load().fmx_corpus_from_tables(ds.ctypes.data, rl.ctypes.data, ep.ctypes.data, rl.size, ep.size, 0, ctypes.byref(h)))
    again = findex_amd.Corpus(h, m.cs.corpus.names)
    assert again.info()[:3] == (len(m.docs), m.n, len(m.ref.esc_pos))
    assert_map(again.map(map_positions(m.n)), map_expected(m), "from tables")
    for a, b in zip(again.tables(), (ds, rl, ep)):
        assert np.array_equal(a, b)
    again.close()


# ---- 2. the listing of the query set
@pytest.mark.parametrize("name", ["D255", "D256", "D257", "D5000"])
def test_list_docs_against_the_reference(corpora, name):
    m = corpora(name)
    Q = corpus_many.QUERIES
    want = corpus_many.csr([m.doc_counts(q) for q in Q])
    got = m.cs.list_docs(Q)
    assert_csr(got, want, name)
    assert_csr(m.cs.list_docs(Q), got, name + ", second call")
    for q in Q:
        assert m.cs.count_docs(q) == len(m.doc_counts(q)), (name, q)


# ---- 3. key widths
def width_lists(m, k):
    """(g, sp, ep, expected CSR, rows) of corpus_many.width_case(ref, k): the intervals from the device's own search."""
    g, tokens, rows = corpus_many.width_case(m.ref, k)
    distinct = sorted({w for kind, w in tokens if kind != "miss"})
    _, dsp, dep = m.cs._intervals(distinct + [b"z" * g])
    at = {w: i for i, w in enumerate(distinct)}
    miss = len(distinct)
    assert dep[miss] <= dsp[miss]
    idx = np.array([miss if kind == "miss" else at[w] for kind, w in tokens], dtype=np.int64)
    inv = np.array([kind == "inverted" for kind, _ in tokens], dtype=bool)
    sp, ep = dsp[idx].copy(), dep[idx].copy()
    sp[inv], ep[inv] = dep[idx][inv], dsp[idx][inv]
    assert np.all(sp[inv] > ep[inv])
    size = np.where(ep > sp, ep - sp, 0).astype(np.uint64)
    assert int(size.sum()) == rows                                # the call has the rows the CPU test sized it for
    # the per-query reference tiled the same way
    per = {w: m.ref.doc_counts(w) for w in distinct}
    per_doc = {w: np.array([d for d, _ in per[w]], dtype=np.uint32) for w in distinct}
    per_cnt = {w: np.array([c for _, c in per[w]], dtype=np.uint32) for w in distinct}
    hits = [w for kind, w in tokens if kind == "hit"]
    off = np.zeros(k + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(per[w]) if kind == "hit" else 0 for kind, w in tokens])
    want = (off, np.concatenate([per_doc[w] for w in hits]), np.concatenate([per_cnt[w] for w in hits]))
    return g, sp, ep, want, rows


@pytest.mark.parametrize("name,k,bits,passes", corpus_many.WIDTH_CASES, ids=["%s-%d" % c[:2] for c in corpus_many.WIDTH_CASES])
def test_listing_key_widths(corpora, name, k, bits, passes):
    m = corpora(name)
    assert corpus_many.lib_bits(m.cs.corpus.n_docs) + corpus_many.lib_bits(k) == bits and (bits + 7) // 8 == passes
    g, sp, ep, want, rows = width_lists(m, k)
    assert sp.size == k and rows <= corpus_many.MAX_ROWS
    got = m.cs._doc_list(sp, ep, g)
    assert_csr(got, want, (name, k))
    if k == 70000:
        # k_loc_scan through 69 chunks, by itself: the offsets, and every position against locate of the expanded rows
        size = np.where(ep > sp, ep - sp, 0).astype(np.uint64)
        loff, lpos = m.cs.searcher.locate_intervals(sp, ep)
        cum = np.zeros(k + 1, dtype=np.uint64)
        cum[1:] = np.cumsum(size)
        assert np.array_equal(loff, cum) and lpos.size == rows
        expanded = np.repeat(sp, size.astype(np.int64)) + (np.arange(rows, dtype=np.uint64) - np.repeat(cum[:-1], size.astype(np.int64)))
        assert np.array_equal(lpos, m.cs.searcher.locate(expanded))


# ---- 4. a head scan of three levels
def test_rows_beyond_the_scans_second_level(corpora):
    m = corpora("D5000")
    counts = {w: sum(c for _, c in m.doc_counts(w)) for w in corpus_many.grams(1)}
    w = max(counts, key=lambda x: (counts[x], x))
    k = (2048 * 2048 + 100000) // counts[w] + 1
    assert counts[w] > 4096 and k * counts[w] > 4.3e6 and k * counts[w] <= corpus_many.MAX_ROWS
    _, sp, ep = m.cs._intervals([w])
    assert int(ep[0] - sp[0]) == counts[w]
    one = corpus_many.csr([m.doc_counts(w)])
    want = corpus_many.csr([m.doc_counts(w)] * k)
    assert want[0][-1] == k * one[0][-1] and one[0][-1] > 256
    assert_csr(m.cs._doc_list(np.repeat(sp, k), np.repeat(ep, k), 1), want, "three scan levels")


# ---- 5. max_per
@pytest.mark.parametrize("max_per", [1, 7, 5000])
def test_max_per_against_the_reference_table(corpora, max_per):
    m = corpora("D5000")
    _, sp, ep = m.cs._intervals(corpus_many.grams(2))
    got = m.cs._doc_list(sp, ep, 2, max_per=max_per)
    loff, sa = m.cs.searcher.locate_intervals(sp, ep, max_per=max_per)
    pos = m.cs.searcher.text_offsets(sa, m.cs.searcher.n, 2)
    per = []
    for i in range(sp.size):
        a, b = int(loff[i]), int(loff[i + 1])
        assert b - a == min(max_per, int(ep[i] - sp[i]))
        per.append(m.ref.list_positions(pos[a:b].tolist()))
        assert sum(c for _, c in per[-1]) == b - a
    assert_csr(got, corpus_many.csr(per), max_per)
    off, _, cnt = got
    for i in range(sp.size):
        assert int(cnt[int(off[i]):int(off[i + 1])].sum()) == min(max_per, int(ep[i] - sp[i]))


# ---- 6. capacity
def test_capacity_at_size(corpora):
    import torch
    m = corpora("D5000")
    L = _lib.load()
    cs = m.cs
    G = corpus_many.grams(2)
    _, sp, ep = cs._intervals(G)
    want = corpus_many.csr([m.doc_counts(q) for q in G])
    off, doc, cnt = cs._doc_list(sp, ep, 2)
    assert_csr((off, doc, cnt), want, "2-grams")
    total = int(off[-1])
    assert total > 16 * 256
    for cap in (total - 1, 0):
        o2 = np.zeros(sp.size + 1, dtype=np.uint64)
        d2 = np.full(total, 77, dtype=np.uint32)
        c2 = np.full(total, 77, dtype=np.uint32)
        rc = L.fmx_corpus_doc_list(cs.corpus.handle, cs.searcher.handle, sp.ctypes.data, ep.ctypes.data, sp.size, 2, 0, o2.ctypes.data,
                                   d2.ctypes.data, c2.ctypes.data, cap)
        assert rc == 9 and b"room" in L.fmx_last_error()
        assert np.array_equal(o2, off)
        assert np.array_equal(d2[:cap], doc[:cap]) and np.array_equal(c2[:cap], cnt[:cap])
        assert np.all(d2[cap:] == 77) and np.all(c2[cap:] == 77)
    # the device form on a side stream: the same, with the total in off[k]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dsp, dep = torch.from_numpy(sp.view(np.int64)).cuda(), torch.from_numpy(ep.view(np.int64)).cuda()
    s.synchronize()
    for cap in (total - 1, 0):
        with torch.cuda.stream(s):
            doff = torch.zeros(sp.size + 1, dtype=torch.int64, device="cuda")
            ddoc = torch.full((total,), 77, dtype=torch.int32, device="cuda")
            dcnt = torch.full((total,), 77, dtype=torch.int32, device="cuda")
        s.synchronize()
        _lib.check(L.fmx_corpus_doc_list_dev(cs.corpus.handle, cs.searcher.handle, dsp.data_ptr(), dep.data_ptr(), sp.size, 2, 0,
                                             doff.data_ptr(), ddoc.data_ptr(), dcnt.data_ptr(), cap, s.cuda_stream))
        s.synchronize()
        o3 = doff.cpu().numpy().view(np.uint64)
        d3, c3 = ddoc.cpu().numpy().view(np.uint32), dcnt.cpu().numpy().view(np.uint32)
        assert np.array_equal(o3, off) and int(o3[-1]) == total
        assert np.array_equal(d3[:cap], doc[:cap]) and np.array_equal(c3[:cap], cnt[:cap])
        assert np.all(d3[cap:] == 77) and np.all(c3[cap:] == 77)


# ---- 7. intervals that are no search result: rows whose position is no stream position
@pytest.mark.parametrize("name", ["D256", "D5000"])
def test_rows_that_are_no_stream_position_list_as_uint32_max(corpora, name):
    m = corpora(name)
    cs, ref, n_docs = m.cs, m.ref, len(m.docs)
    n = cs.searcher.n
    assert n == m.n + 1
    sa = cs.searcher.locate(np.arange(n, dtype=np.uint64))          # (test_gpu_locate.py holds locate to the oracle)
    assert np.array_equal(np.sort(sa), np.arange(n, dtype=np.uint64))
    sp, ep = np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint64)
    # pat_len 1: every stream position once, and the row of SA = stream length falls out in front of the stream
    want = [(d, ref.doc_start[d + 1] - ref.doc_start[d]) for d in range(n_docs)] + [(NO_DOC, 1)]
    assert all(c >= 1 for _, c in want) and want[0] == (0, 1) and want[n_docs - 1] == (n_docs - 1, 1)       # empty documents: their separator
    assert_csr(cs._doc_list(sp, ep, 1), corpus_many.csr([want]), "pat_len 1")
    for pat_len in (3, 0):
        p = m.n - pat_len - sa.astype(np.int64)
        positions = [int(x) if 0 <= x < m.n else None for x in p]
        want = ref.list_positions(positions)
        assert want[-1] == (NO_DOC, 3 if pat_len else 1) and len(want) > n_docs // 2
        assert_csr(cs._doc_list(sp, ep, pat_len), corpus_many.csr([want]), "pat_len %d" % pat_len)
    assert_csr(cs._doc_list(sp, ep, m.n + 5), corpus_many.csr([[(NO_DOC, n)]]), "pat_len past the stream")


# ---- 8. locate_docs and read
def test_locate_docs_at_5000_documents(corpora):
    m = corpora("D5000")
    for q in corpus_many.QUERIES:
        doc, raw = m.cs.locate_docs(q)
        want = corpus_many.expected_occurrences(m.ref, q)
        assert doc.dtype == np.uint32 and raw.dtype == np.uint64
        assert list(zip(doc.tolist(), raw.tolist())) == want, q


def test_read_every_document_in_one_call(corpora):
    m = corpora("D5000")
    n_docs = len(m.docs)
    rl = np.array(m.ref.raw_len, dtype=np.uint64)
    assert m.cs.read(np.arange(n_docs), 0, rl) == m.docs
    assert m.docs[0] == b"" and b"" in m.docs[1:-1]
    m.cs.corpus.drop_stream()                                       # the text comes from the index, not from the stream in HBM
    with pytest.raises(findex_amd.FmxError):
        m.cs.corpus.stream()
    assert m.cs.read(np.arange(n_docs), 0, rl) == m.docs
