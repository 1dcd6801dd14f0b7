"""The corpus index on the device against tests/corpus_ref.py: the stream, doc_start and esc_pos byte for byte on the
reference's directories and on corpora built around the build's tile size; the index of the stream against bwt_from_text; the
position map at every stream position; locate_docs against bytes.find in every raw file; the document listing against
numpy.unique; memory, stream captures and the X.docs round trip."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus_ref
import findex_amd
from findex_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")


def tile_bytes():
    t = ctypes.c_uint32()
    _lib.check(_lib.load().fmx_corpus_info(None, None, None, None, None, None, ctypes.byref(t)))
    assert t.value >= 64 and t.value % 16 == 0
    return int(t.value)


def filler(rng, n, escapes=0.03):
    """n raw bytes: letters, backslashes, and a share of the three escaped values."""
    b = rng.integers(97, 123, n, dtype=np.uint8)
    b[rng.random(n) < 0.02] = 92
    m = rng.random(n) < escapes
    b[m] = rng.choice(np.array([0, 1, 255], dtype=np.uint8), int(m.sum()))
    return b.tobytes()


def with_bytes(raw, at):
    raw = bytearray(raw)
    for i, c in at.items():
        raw[i] = c
    return bytes(raw)


def synthetic_corpora():
    T = tile_bytes()
    rng = np.random.default_rng(41)
    out = {}
    for n in (T - 1, T, T + 1, 3 * T + 1):                        # a single document each
        out["len_%d" % n] = [filler(rng, n)]
    for c in (0, 1, 255):                                         # an escaped byte last in a tile and first in the next
        out["edge_%d" % c] = [with_bytes(filler(rng, 2 * T + 5, 0.0), {T - 1: c, T: c, 2 * T - 1: c})]
    out["edge_mixed"] = [with_bytes(filler(rng, 3 * T + 7), {T - 1: 0, T: 1, 2 * T - 1: 255, 2 * T: 0, 3 * T - 1: 1, 3 * T: 255})]
    out["doc_ends_on_edge"] = [filler(rng, T), filler(rng, 100), filler(rng, T - 100), filler(rng, 7)]
    out["empties_at_edge"] = [filler(rng, T), b"", b"", b"", filler(rng, 50)]
    out["empties_at_start_and_end"] = [b"", b"", b"", filler(rng, 300), b"", b"", b""]
    out["empties_only"] = [b"", b"", b""]
    out["one_byte"] = [b"x"]
    out["one_escaped_byte"] = [b"\x00"]
    out["ff_5000"] = [b"\xff" * 5000]
    out["ff_5000_among_others"] = [filler(rng, 10), b"\xff" * 5000, b"\x01" * (T + 3), filler(rng, 2 * T)]
    out["small_docs"] = [filler(rng, int(n), 0.1) for n in rng.integers(0, 40, 700)]
    # more separators in one tile than the emit pass stages at once (3 T bytes): its second window
    out["many_empties_in_one_tile"] = [filler(rng, T + 9)] + [b""] * (3 * T + 100) + [filler(rng, 20)]
    return out


@pytest.fixture(scope="module")
def synth():
    return {k: (docs, corpus_ref.RefCorpus(docs)) for k, docs in synthetic_corpora().items()}


@pytest.fixture(scope="module")
def tbad():
    ref = corpus_ref.RefCorpus.from_dir(os.path.join(TESTDATA, "tbad"))
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_dir(os.path.join(TESTDATA, "tbad")))
    yield ref, cs
    cs.close()


def check_against_ref(c, ref, what):
    n_docs, stream_len, n_esc = c.info()[:3]
    assert (n_docs, stream_len, n_esc) == (len(ref.docs), len(ref.stream), len(ref.esc_pos)), what
    assert c.stream().tobytes() == ref.stream, what
    ds, rl, ep = c.tables()
    assert ds.tolist() == ref.doc_start, what
    assert ep.tolist() == ref.esc_pos, what
    assert rl.tolist() == ref.raw_len, what


# ---- 1. stream, doc_start, esc_pos
@pytest.mark.parametrize("name", ["t1", "t2", "tbad"])
def test_reference_directories(name):
    ref = corpus_ref.RefCorpus.from_dir(os.path.join(TESTDATA, name))
    c = findex_amd.Corpus.from_dir(os.path.join(TESTDATA, name))
    assert c.names == ref.names
    check_against_ref(c, ref, name)
    if name == "t1":
        assert c.stream_len == 3075 and c.stream()[:2].tolist() == [67, 67]
    if name == "tbad":
        assert c.stream_len == 3 * 1024 + 133 + 3 and c.n_esc == 133
    c.close()


def test_corpora_around_the_tile_size(synth):
    for name, (docs, ref) in synth.items():
        c = findex_amd.Corpus.from_documents(docs)
        check_against_ref(c, ref, name)
        c.close()


def test_two_builds_give_identical_bytes(synth):
    for name in ("edge_mixed", "small_docs", "ff_5000_among_others"):
        docs, _ = synth[name]
        a, b = findex_amd.Corpus.from_documents(docs), findex_amd.Corpus.from_documents(docs)
        assert a.stream().tobytes() == b.stream().tobytes()
        for x, y in zip(a.tables(), b.tables()):
            assert np.array_equal(x, y)
        a.close()
        b.close()


def test_build_from_device_memory_at_any_alignment(synth):
    import torch
    docs, ref = synth["edge_mixed"]
    raw = np.frombuffer(b"".join(docs), dtype=np.uint8)
    ends = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    L = _lib.load()
    for shift in (0, 3):                                          # 3: no 16-byte loads, the same bytes
        buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
        buf[shift:shift + raw.size] = torch.from_numpy(raw.copy()).cuda()
        h = ctypes.c_void_p()
        _lib.check(L.fmx_corpus_build_dev(buf.data_ptr() + shift, raw.size, ends.ctypes.data, ends.size, 0, None, ctypes.byref(h)))
        c = findex_amd.Corpus(h, [b"d"] * len(docs))
        check_against_ref(c, ref, shift)
        p, n = c.stream_dev()
        assert p != 0 and n == len(ref.stream)
        c.close()


# ---- 2. the index
def bwt_of(hip):
    b, _ = hip.lf_walk_batch(np.arange(hip.n, dtype=np.uint64), 1)            # BWT', 0 at the EOF row
    return b.reshape(-1)


def test_index_equals_bwt_from_text_of_the_stream(synth, tbad):
    L = _lib.load()
    for docs, ref in (synth["ff_5000_among_others"], synth["small_docs"], (tbad[0].docs, tbad[0])):
        c = findex_amd.Corpus.from_documents(docs)
        hip = c.build_index()
        bwt, eof, counts = findex_amd.bwt_from_text(ref.stream)
        assert hip.n == bwt.size == len(ref.stream) + 1 and hip.eof == eof
        got = np.zeros(256, dtype=np.int64)
        _lib.check(L.fmx_counts(hip.handle, got.ctypes.data))
        assert np.array_equal(got, counts) and counts[1] == len(docs) and counts[0] == 0 and counts[255] == 0
        want = bwt.copy()
        want[eof] = 0
        assert np.array_equal(bwt_of(hip), want)
        hip.close()
        c.close()


def test_tool_writes_the_stream_and_its_index(tmp_path, tbad):
    ref, _ = tbad
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = tmp_path / "x"
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", "--dir", os.path.join(TESTDATA, "tbad"), "--out", str(out), "--data"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["x.aux", "x.bwt", "x.data", "x.docs"]
    assert (tmp_path / "x.data").read_bytes() == ref.stream
    bwt, eof, counts = findex_amd.bwt_from_text(ref.stream)
    findex_amd.write_bwt(tmp_path / "w.bwt", tmp_path / "w.aux", bwt, eof, counts)
    assert (tmp_path / "x.bwt").read_bytes() == (tmp_path / "w.bwt").read_bytes()
    assert (tmp_path / "x.aux").read_bytes() == (tmp_path / "w.aux").read_bytes()
    ds, rl, ep, names = findex_amd.corpus.read_docs(tmp_path / "x.docs")
    assert ds.tolist() == ref.doc_start and rl.tolist() == ref.raw_len and ep.tolist() == ref.esc_pos and names == ref.names
    # grep -c style counts per file from the files alone
    cs = findex_amd.HipCorpusSearcher.open(out)
    for q in (b"jm", b"\xff", b"t2.txt"):
        doc, _ = cs.locate_docs(q)
        got = {names[d]: int(n) for d, n in zip(*np.unique(doc, return_counts=True))}
        want = {names[d]: raw.count(q) for d, raw in enumerate(ref.docs) if raw.count(q)}         # (no q overlaps itself)
        assert got == want, q
    cs.close()


# ---- 3. the map
def test_map_at_every_position(synth, tbad):
    for ref, c in ((tbad[0], tbad[1].corpus), (synth["edge_mixed"][1], None), (synth["empties_at_start_and_end"][1], None)):
        own = c is None
        if own:
            c = findex_amd.Corpus.from_documents(ref.docs)
        n = len(ref.stream)
        pos = np.concatenate([np.arange(n, dtype=np.uint64), np.array([n, n + 5], dtype=np.uint64)])
        doc, eo, ro = c.map(pos)
        want = [ref.map(int(p)) for p in pos]
        assert doc.tolist() == [w[0] for w in want]
        assert eo.tolist() == [w[1] for w in want]
        assert ro.tolist() == [w[2] for w in want]
        # the cases by name: a separator, the second byte of an escape, past the end
        sep = ref.doc_start[1] - 1
        assert (int(doc[sep]), int(ro[sep])) == (0, ref.raw_len[0])
        if ref.esc_pos:
            e = ref.esc_pos[0]
            assert ro[e] == ro[e + 1] and eo[e + 1] == eo[e] + 1 and doc[e] == doc[e + 1]
        assert doc[n] == 0xFFFFFFFF and doc[n + 1] == 0xFFFFFFFF
        if own:
            c.close()


# ---- 4. locate_docs
def as_pairs(doc, raw):
    return list(zip(doc.tolist(), raw.tolist()))


def test_locate_docs_on_tbad(tbad):
    ref, cs = tbad
    for q in (b"\xff", b"jm", b"t2.txt", b"zzzzqq", b"\xff\xff", b"t"):
        assert as_pairs(*cs.locate_docs(q)) == ref.occurrences(q), q
    assert len(ref.occurrences(b"\xff")) == 133 and len(ref.occurrences(b"jm")) == 4 and ref.occurrences(b"zzzzqq") == []
    # no hit spans two files: the end of one and the start of the next, which occur nowhere else
    for d in range(2):
        tail, head = ref.docs[d][-2:], ref.docs[d + 1][:2]
        assert ref.occurrences(tail + head) == [] and ref.stream.count(tail + b"\x01" + head) == 1
        assert as_pairs(*cs.locate_docs(tail + head)) == []
        assert as_pairs(*cs.locate_docs(tail + b"\x01" + head)) == []           # a raw 1 in a query is the escape, never the separator
    doc, raw = cs.locate_docs(b"\xff", max_hits=10)
    assert doc.size == 10 and set(as_pairs(doc, raw)) <= set(ref.occurrences(b"\xff"))


def test_locate_docs_with_raw_0_and_1():
    docs = [b"hello a\x00\x01b world QZ", b"JX second a\x00\x01b file a\x00\x01b\x00", b"", b"third\xff\xffa\x00\x01", b"\x01\x00"]
    ref = corpus_ref.RefCorpus(docs)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    for q in (b"a\x00\x01b", b"\x00\x01", b"\x01", b"\x00", b"\xff\xff", b"QZJX", b"QZ\x01JX", b"a\x00\x01", b"\x01\x00"):
        assert as_pairs(*cs.locate_docs(q)) == ref.occurrences(q), q
    assert len(ref.occurrences(b"a\x00\x01b")) == 3 and ref.occurrences(b"QZJX") == [] and len(ref.occurrences(b"\x00")) == 6
    cs.close()


def test_the_unescaped_backslash_is_ambiguous_to_the_search_not_to_the_map():
    """The reference's quirk, kept: the backslash is not escaped, so the raw text '\\' '0' and the raw byte 0 are the same
    two stream bytes.  A search for either finds both; the map still gives each hit its own offset in its raw file."""
    docs = [b"x\\0y\x00z", b"\x00"]
    ref = corpus_ref.RefCorpus(docs)
    assert ref.stream == b"x\\0y\\0z\x01\\0\x01" and ref.esc_pos == [4, 8]
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    both = sorted(ref.occurrences(b"\\0") + ref.occurrences(b"\x00"))
    assert both == [(0, 1), (0, 4), (1, 0)]
    assert as_pairs(*cs.locate_docs(b"\x00")) == both
    assert as_pairs(*cs.locate_docs(b"\\0")) == both
    cs.close()


# ---- 5. list_docs / count_docs
QUERIES = [b"t", b"\xff", b".txt", b"mk", b"ab", b"t2.txt", b"\xff\xff", b"zzzzqq"]


def test_list_docs_against_numpy_unique(tbad):
    ref, cs = tbad
    off, doc, cnt = cs.list_docs(QUERIES)
    assert off[0] == 0 and off.size == len(QUERIES) + 1
    seen = []
    for i, q in enumerate(QUERIES):
        occ = ref.occurrences(q)
        d, n = np.unique(np.array([o[0] for o in occ], dtype=np.uint32), return_counts=True)
        lo, hi = int(off[i]), int(off[i + 1])
        assert doc[lo:hi].tolist() == d.tolist() and cnt[lo:hi].tolist() == n.tolist(), q
        assert cs.count_docs(q) == d.size
        seen.append(d.size)
    assert seen[0] == 3 and seen[-1] == 0 and 1 in seen and 2 in seen          # from "in every file" to "in none"


def test_list_docs_capacity_and_max_per(tbad):
    ref, cs = tbad
    L = _lib.load()
    same_len = [b"mk", b"ab", b"jm", b"qx", b"zq"]                # one escaped length: one call
    _, sp, ep = cs._intervals(same_len)
    off, doc, cnt = cs._doc_list(sp, ep, 2)
    total = int(off[-1])
    assert total == doc.size == sum(len({o[0] for o in ref.occurrences(q)}) for q in same_len) and total >= 8
    # a capacity one too small: overflow, every offset written, nothing past the capacity
    o2 = np.zeros(sp.size + 1, dtype=np.uint64)
    d2 = np.full(total, 77, dtype=np.uint32)
    c2 = np.full(total, 77, dtype=np.uint32)
    rc = L.fmx_corpus_doc_list(cs.corpus.handle, cs.searcher.handle, sp.ctypes.data, ep.ctypes.data, sp.size, 2, 0, o2.ctypes.data,
                               d2.ctypes.data, c2.ctypes.data, total - 1)
    assert rc == 9 and b"room" in L.fmx_last_error()
    assert np.array_equal(o2, off)
    assert np.array_equal(d2[:total - 1], doc[:total - 1]) and np.array_equal(c2[:total - 1], cnt[:total - 1])
    assert d2[total - 1] == 77 and c2[total - 1] == 77
    # the device form leaves the total for the caller to compare
    import torch
    dsp, dep = torch.from_numpy(sp.view(np.int64)).cuda(), torch.from_numpy(ep.view(np.int64)).cuda()
    doff = torch.zeros(sp.size + 1, dtype=torch.int64, device="cuda")
    ddoc = torch.full((total,), 77, dtype=torch.int32, device="cuda")
    dcnt = torch.full((total,), 77, dtype=torch.int32, device="cuda")
    _lib.check(L.fmx_corpus_doc_list_dev(cs.corpus.handle, cs.searcher.handle, dsp.data_ptr(), dep.data_ptr(), sp.size, 2, 0,
                                         doff.data_ptr(), ddoc.data_ptr(), dcnt.data_ptr(), total - 1, None))
    torch.cuda.synchronize()
    assert np.array_equal(doff.cpu().numpy().view(np.uint64), off)
    assert np.array_equal(ddoc.cpu().numpy().view(np.uint32)[:total - 1], doc[:total - 1]) and int(ddoc[total - 1]) == 77
    # max_per: the documents of each interval's first max_per rows
    for max_per in (1, 2, 3):
        o3, d3, c3 = cs._doc_list(sp, ep, 2, max_per=max_per)
        lo, pos = cs.searcher.locate_intervals(sp, ep, max_per=max_per)
        for i in range(sp.size):
            text_pos = cs.searcher.text_offsets(pos[int(lo[i]):int(lo[i + 1])], cs.searcher.n, 2)
            d, n = np.unique(cs.corpus.map(text_pos)[0], return_counts=True)
            a, b = int(o3[i]), int(o3[i + 1])
            assert d3[a:b].tolist() == d.tolist() and c3[a:b].tolist() == n.tolist()
            assert int(c3[a:b].sum()) == min(max_per, int(ep[i] - sp[i]) if ep[i] > sp[i] else 0)
    # an index that is not this corpus' index is refused
    other = findex_amd.HipFMSearcher.from_text(b"abracadabra")
    rc = L.fmx_corpus_doc_list(cs.corpus.handle, other.handle, sp.ctypes.data, ep.ctypes.data, sp.size, 2, 0, o2.ctypes.data,
                               d2.ctypes.data, c2.ctypes.data, total)
    assert rc == 3
    other.close()


# ---- 6. housekeeping
def test_memory_comes_back(synth):
    import torch
    docs, _ = synth["ff_5000_among_others"]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    c = findex_amd.Corpus.from_documents(docs)
    assert c.info()[3] >= c.stream_len
    hip = c.build_index()
    held = c.info()[3]
    c.drop_stream()
    assert c.info()[3] == held - c.stream_len
    with pytest.raises(findex_amd.FmxError) as ei:
        c.build_index()
    assert ei.value.code == 3
    doc, _, _ = c.map(np.array([0, c.stream_len - 1], dtype=np.uint64))         # the map outlives the stream
    assert doc.tolist() == [0, len(docs) - 1]
    hip.close()
    c.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 64 << 20


def test_build_refuses_a_stream_capture_and_map_dev_is_capturable(tbad):
    import torch
    ref, cs = tbad
    L = _lib.load()
    raw = np.frombuffer(b"".join(ref.docs), dtype=np.uint8)
    ends = np.cumsum([len(d) for d in ref.docs], dtype=np.uint64)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    n = len(ref.stream)
    pos = torch.arange(0, n + 2, dtype=torch.int64, device="cuda")
    doc = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
    eo = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    ro = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    h = ctypes.c_void_p()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        rc = L.fmx_corpus_build_dev(d_raw.data_ptr(), raw.size, ends.ctypes.data, ends.size, 0, s.cuda_stream, ctypes.byref(h))
        msg = L.fmx_last_error()
        rc2 = L.fmx_corpus_open_index(cs.corpus.handle, s.cuda_stream, ctypes.byref(h))
        doc.zero_()                                               # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert rc == 5 and b"stream capture" in msg and rc2 == 5 and not h.value
    del g
    # the map's device form only enqueues: captured, replayed, compared at every position
    with torch.cuda.stream(s):
        cs.corpus.map_dev(pos.data_ptr(), n + 2, doc.data_ptr(), eo.data_ptr(), ro.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs.corpus.map_dev(pos.data_ptr(), n + 2, doc.data_ptr(), eo.data_ptr(), ro.data_ptr(), stream=s.cuda_stream)
    want = [ref.map(p) for p in range(n + 2)]
    for _ in range(2):
        doc.zero_()
        ro.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert doc.cpu().numpy().view(np.uint32).tolist() == [w[0] for w in want]
        assert ro.cpu().numpy().view(np.uint64).tolist() == [w[2] for w in want]
        assert eo.cpu().numpy().view(np.uint64).tolist() == [w[1] for w in want]
    del g


def test_docs_file_and_bwt_answer_like_the_live_corpus(tbad, tmp_path):
    ref, cs = tbad
    cs.corpus.save(tmp_path / "x.docs")
    bwt, eof, counts = findex_amd.bwt_from_text(ref.stream)
    findex_amd.write_bwt(tmp_path / "x.bwt", tmp_path / "x.aux", bwt, eof, counts)
    again = findex_amd.HipCorpusSearcher.open(tmp_path / "x")
    assert again.corpus.names == cs.corpus.names == ref.names
    for a, b in zip(again.corpus.tables(), cs.corpus.tables()):
        assert np.array_equal(a, b)
    for q in (b"\xff", b"jm", b"t2.txt", b"zzzzqq"):
        assert as_pairs(*again.locate_docs(q)) == as_pairs(*cs.locate_docs(q)) == ref.occurrences(q)
    off, doc, cnt = again.list_docs(QUERIES)
    for a, b in zip((off, doc, cnt), cs.list_docs(QUERIES)):
        assert np.array_equal(a, b)
    with pytest.raises(findex_amd.FmxError) as ei:                # a map without a stream builds no index
        again.corpus.build_index()
    assert ei.value.code == 3
    again.close()
