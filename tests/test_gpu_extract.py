"""Extraction by text position on the device: every (offset, length) of a small text in one batch at four rates, the
row-block edges of both layouts, the goldens against their .txt, the tile edges of the kernel, the step relation of every
batch, the two ways the samples are built, the prepare contract under a stream capture, the device form with guard bytes, the
refusals, and the corpus methods (read, document, snippets) with no stream in HBM and no X.data on disk.

Every expectation is a slice of the text (or of the raw documents); nothing of the library produces one."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import findex_amd
from findex_amd import _lib
from helpers import ends_at_a_fault, synth_bwt
from test_extract_cpu import DOCS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")
T = _lib.FMX_EXTRACT_TILE
LAYOUTS = ("onehot", "bytes")


@pytest.fixture
def layout():
    yield findex_amd.set_layout
    findex_amd.set_layout("auto")


def set_rate(hip, s, via_locate=False):
    """The handle's extract samples at rate s, built anew: by the inversion, or from locate samples at the same rate."""
    hip.config_set("extract_sample", s)
    hip.drop_tables(jump=False, frontier=False, locate=True, extract=True)
    if via_locate:
        hip.config_set("locate_sample", s)
        hip.prepare(ktab=False, locate=True)
    hip.prepare(ktab=False, extract=True)
    rate, nbytes, _ = hip.extract_info()
    m = (hip.n - 1) // s + 1
    assert rate == s and nbytes == m * (8 if hip.n > 1 << 32 else 4)


def check_batch(hip, text, pos, lens, s, note=None):
    """One host call: the bytes are the slices, the steps keep fmx.h's relation, rank_queries grows by exactly the steps."""
    pos = np.asarray(pos, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint64)
    before = hip.stats()["rank_queries"]
    off, data = hip.extract_text_batch(pos, lens)
    ms, steps, requests = hip.extract_last()
    grown = hip.stats()["rank_queries"] - before
    nb = int(lens.sum())
    assert int(off[-1]) == nb == data.size
    want = b"".join(text[int(a):int(a) + int(l)] for a, l in zip(pos.tolist(), lens.tolist()))
    got = data.tobytes()
    if got != want:
        bad = next(i for i in range(nb) if got[i] != want[i])
        q = int(np.searchsorted(off, bad, side="right") - 1)
        pytest.fail("%s: byte %d of the batch (range %d, pos %d, length %d) is %r, expected %r"
                    % (note, bad, q, int(pos[q]), int(lens[q]), got[bad:bad + 1], want[bad:bad + 1]))
    nonempty = int((lens > 0).sum())
    hi = nb + (s - 1) * (nonempty + -(-nb // T) + nb // s + 1)
    print("%s: s=%d, %d ranges, %d bytes: %d steps (<= %d), %d requests, %.3f ms" % (note, s, pos.size, nb, steps, hi, requests, ms))
    if nb:
        assert nb <= steps <= hi, (note, nb, steps, hi)
        assert grown == steps, (note, grown, steps)
        assert 0 < requests <= 4 * steps, (note, requests, steps)
    return data


@ends_at_a_fault
def test_every_range_of_a_small_text_in_one_batch(layout):
    rng = np.random.default_rng(31)
    text = bytes(rng.integers(97, 100, 70, dtype=np.uint8))
    pairs = [(a, ln) for a in range(70) for ln in range(1, 70 - a + 1)]
    assert len(pairs) == 2485
    pos = [a for a, _ in pairs]
    lens = [ln for _, ln in pairs]
    for lay in LAYOUTS:
        layout(lay)
        hip = findex_amd.HipFMSearcher.from_text(text)
        assert hip.stats()["layout"] == (0 if lay == "onehot" else 1)
        for s in (1, 3, 32, 4096):                                # 4096 > n: every piece falls back to row 0
            set_rate(hip, s)
            check_batch(hip, text, pos, lens, s, "%s exhaustive" % lay)
            assert hip.extract_text(0, 70) == text and hip.extract_text(69, 1) == text[69:] and hip.extract_text(70, 0) == b""
        hip.close()


@pytest.mark.parametrize("length", [446, 447, 448, 126, 127, 128])
@ends_at_a_fault
def test_row_block_edges(layout, length):
    """n - 1 = length rows beside the sentinel's: the last row on either side of a block edge of the one-hot layout (448
    rows) and of the bytes layout (128).  2 divides 446, 448, 126, 128; 7 divides 448 and 126; 32 divides 448 and 128."""
    rng = np.random.default_rng(length)
    text = bytes(rng.integers(97, 101, length, dtype=np.uint8))
    for lay in LAYOUTS:
        layout(lay)
        hip = findex_amd.HipFMSearcher.from_text(text)
        for s in (2, 7, 32):
            set_rate(hip, s)
            check_batch(hip, text, [0], [length], s, "%s edges %d whole" % (lay, length))
            check_batch(hip, text, [0, length - 1], [1, 1], s, "%s edges %d ends" % (lay, length))
        hip.close()


def golden_indexes():
    out = [(os.path.basename(p)[:-8], os.path.basename(p)[:-4], False) for p in sorted(glob.glob(os.path.join(TESTDATA, "*.cmp.bwt")))]
    return out + [("words", "words", True)]


@pytest.mark.parametrize("txt,name,be", golden_indexes())
@ends_at_a_fault
def test_goldens_against_their_text(txt, name, be, layout):
    text = open(os.path.join(TESTDATA, txt + ".txt"), "rb").read()
    rng = np.random.default_rng(32)
    lens = rng.integers(0, 301, 2000).clip(max=len(text))
    pos = (rng.random(2000) * (len(text) - lens + 1)).astype(np.uint64)
    for lay in LAYOUTS:
        layout(lay)
        hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, name + ".bwt"), bigEndian=be)
        assert hip.n == len(text) + 1
        assert hip.extract_info()[:2] == (32, 0)                  # the first call builds the samples at the default rate
        check_batch(hip, text, [0], [len(text)], 32, "%s %s whole" % (lay, name))
        assert hip.extract_info()[1] == ((hip.n - 1) // 32 + 1) * 4
        check_batch(hip, text, pos, lens, 32, "%s %s random" % (lay, name))
        hip.close()


@pytest.fixture(scope="module")
def words():
    text = open(os.path.join(TESTDATA, "words.txt"), "rb").read()
    assert len(text) > 4 * T + 16
    return text


@ends_at_a_fault
def test_tile_edges(words, layout):
    text = words
    n1 = len(text)
    for lay in LAYOUTS:
        layout(lay)
        hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
        hip.prepare(ktab=False, extract=True)
        for ln in (T - 1, T, T + 1, 2 * T + 3):
            check_batch(hip, text, [7], [ln], 32, "%s one range of %d" % (lay, ln))
            check_batch(hip, text, [n1 - ln, 3, 0], [ln, 5, ln], 32, "%s three ranges, %d" % (lay, ln))
        check_batch(hip, text, np.arange(100, 100 + T) * 3, np.ones(T), 32, "%s T ranges of one byte" % lay)
        check_batch(hip, text, np.arange(T + 1), np.ones(T + 1), 32, "%s T + 1 ranges of one byte" % lay)
        pos = np.concatenate([[11], np.full(5000, n1), [n1 - 9]])
        lens = np.concatenate([[T - 3], np.zeros(5000), [9]])
        check_batch(hip, text, pos, lens, 32, "%s 5000 empty ranges between two" % lay)
        check_batch(hip, text, [n1 - 1], [1], 32, "%s one byte" % lay)
        check_batch(hip, text, [0, 5, 0], [0, 1, 0], 32, "%s one byte among empty ranges" % lay)
        off, data = hip.extract_text_batch([], [])
        assert off.tolist() == [0] and data.size == 0
        off, data = hip.extract_text_batch([3, n1], [0, 0])
        assert off.tolist() == [0, 0, 0] and data.size == 0
        hip.close()


@ends_at_a_fault
def test_samples_by_inversion_and_by_scatter_agree(words, layout):
    text = words
    rng = np.random.default_rng(33)
    lens = rng.integers(0, 200, 3000)
    pos = (rng.random(3000) * (len(text) - lens + 1)).astype(np.uint64)
    for lay in LAYOUTS:
        layout(lay)
        hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
        for s in (32, 5):
            set_rate(hip, s)                                      # the inversion: no locate samples
            assert hip.locate_info()[1] == 0
            a = check_batch(hip, text, pos, lens, s, "%s inversion" % lay)
            by_inversion = hip.extract_info()[1]
            set_rate(hip, s, via_locate=True)                     # the scatter over the locate samples' marks
            assert hip.locate_info()[:1] == (s,) and hip.locate_info()[1] > 0
            b = check_batch(hip, text, pos, lens, s, "%s scatter" % lay)
            assert np.array_equal(a, b) and hip.extract_info()[1] == by_inversion
            check_batch(hip, text, [0], [len(text)], s, "%s scatter, whole" % lay)
        # different rates: the inversion again, beside locate samples it cannot use
        hip.config_set("locate_sample", 32)
        hip.config_set("extract_sample", 7)
        hip.drop_tables(jump=False, frontier=False, locate=True, extract=True)
        hip.prepare(ktab=False, locate=True, extract=True)
        assert hip.locate_info()[0] == 32 and hip.extract_info()[0] == 7
        c = check_batch(hip, text, pos, lens, 7, "%s rates differ" % lay)
        assert np.array_equal(a, c)
        hip.close()


@ends_at_a_fault
def test_contract(words):
    import torch
    text = words
    L = _lib.load()
    hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
    rng = np.random.default_rng(34)
    k = 4000
    lens = rng.integers(0, 100, k).astype(np.uint64)
    pos = (rng.random(k) * (len(text) - lens + 1)).astype(np.uint64)
    off = np.zeros(k + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    nb = int(off[-1])
    want = b"".join(text[int(a):int(a) + int(l)] for a, l in zip(pos.tolist(), lens.tolist()))
    d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    # search tables and locate samples first: extraction must leave them as they are
    pats = [text[i:i + 4][::-1] for i in rng.integers(0, len(text) - 4, 1000).tolist()]
    pbuf = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    poff = np.arange(0, 4 * len(pats) + 1, 4, dtype=np.uint64)
    hip.prepare(ktab=True, jump=True, locate=True)
    sp0, ep0 = hip.search_batch(pbuf, poff)
    rows = np.arange(0, hip.n, 97, dtype=np.uint64)
    sa0 = hip.locate(rows)
    held0, loc0 = hip.stats()["tables_held_bytes"], hip.locate_info()[:2]
    hip.config_set("extract_sample", 16)                          # not locate's rate: the inversion
    assert hip.extract_info()[:2] == (16, 0)
    # without prepare: FMX_ERR_HIP under a capture, nothing built, the capture valid
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        rc = L.fmx_extract_text_batch_dev(hip.handle, d_pos.data_ptr(), d_off.data_ptr(), k, nb, d_out.data_ptr(), s.cuda_stream)
        msg = L.fmx_last_error()
        d_out.zero_()                                             # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert rc == 5 and b"outside a stream capture" in msg and hip.extract_info()[1] == 0
    del g
    # prepared: the device form only enqueues -- captured, replayed twice
    hip.prepare(ktab=False, extract=True)
    rate, nbytes, ms = hip.extract_info()
    assert rate == 16 and nbytes == ((hip.n - 1) // 16 + 1) * 4 and ms > 0
    with torch.cuda.stream(s):
        hip.extract_text_batch_dev(d_pos.data_ptr(), d_off.data_ptr(), k, nb, d_out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        hip.extract_text_batch_dev(d_pos.data_ptr(), d_off.data_ptr(), k, nb, d_out.data_ptr(), stream=s.cuda_stream)
    for _ in range(2):
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want
    del g
    # two runs give equal bytes; locate and the search tables are as they were
    a = hip.extract_text_batch(pos, lens)[1]
    b = hip.extract_text_batch(pos, lens)[1]
    assert a.tobytes() == b.tobytes() == want
    sp1, ep1 = hip.search_batch(pbuf, poff)
    assert np.array_equal(sp0, sp1) and np.array_equal(ep0, ep1) and np.array_equal(hip.locate(rows), sa0)
    assert hip.stats()["tables_held_bytes"] == held0 and hip.locate_info()[:2] == loc0
    # drop: the samples go, nothing else does
    hip.drop_tables(jump=False, frontier=False, extract=True)
    assert hip.extract_info()[1] == 0 and hip.locate_info()[:2] == loc0 and hip.stats()["tables_held_bytes"] == held0
    assert np.array_equal(hip.locate(rows), sa0)
    sp1, ep1 = hip.search_batch(pbuf, poff)
    assert np.array_equal(sp0, sp1) and np.array_equal(ep0, ep1)
    # argument errors that need a handle
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.extract_text(len(text) - 3, 4)
    assert ei.value.code == 3 and "past the text" in str(ei.value)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.extract_text(len(text) + 1, 0)
    assert ei.value.code == 3
    assert hip.extract_text(len(text), 0) == b""
    assert L.fmx_index_config_set(hip.handle, b"extract_sample", b"0") == 3
    assert L.fmx_index_config_set(hip.handle, b"extract_sample", b"4097") == 3
    assert L.fmx_index_config_set(hip.handle, b"extract_sample", b"text") == 3
    assert L.fmx_index_config_set(hip.handle, b"extract_sample", b"4096") == 0
    assert hip.extract_info()[:2] == (4096, 0)                    # a refused or accepted key builds nothing
    hip.close()


@ends_at_a_fault
def test_device_form_on_a_side_stream_with_guard_bytes(words, layout):
    """64 guard bytes on both sides of d_out stay as they were; a range that runs past the text gets 0 from t = n - 1 on."""
    import torch
    text = words
    n1 = len(text)
    pos = np.array([5, n1 - 40, 0, n1 - 1, n1, n1 + 7, 123], dtype=np.uint64)
    lens = np.array([T + 9, 100, 0, 3, 4, 2, 700], dtype=np.uint64)          # ranges 1, 3, 4 and 5 run past the text
    off = np.zeros(pos.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    nb = int(off[-1])
    want = b"".join((text[int(a):int(a) + int(l)] + bytes(int(l)))[:int(l)] for a, l in zip(pos.tolist(), lens.tolist()))
    assert len(want) == nb and want[T + 9 + 40:T + 9 + 100] == bytes(60)
    for lay in LAYOUTS:
        layout(lay)
        hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
        hip.prepare(ktab=False, extract=True)
        d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        for shift in (0, 3):                                      # 3: the destination allows no 16-byte stores
            buf = torch.full((64 + shift + nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                hip.extract_text_batch_dev(d_pos.data_ptr(), d_off.data_ptr(), pos.size, nb, buf.data_ptr() + 64 + shift, stream=s.cuda_stream)
            s.synchronize()
            got = buf.cpu().numpy()
            assert (got[:64 + shift] == 0xA5).all() and (got[64 + shift + nb:] == 0xA5).all(), (lay, shift)
            assert got[64 + shift:64 + shift + nb].tobytes() == want, (lay, shift)
        hip.close()


@ends_at_a_fault
def test_refusals():
    L = _lib.load()
    # an fmx_open_block handle
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    pos = (ctypes.c_uint64 * 1)(0)
    off = (ctypes.c_uint64 * 2)(0, 1)
    out = (ctypes.c_uint8 * 1)()
    assert L.fmx_extract_text_batch(hip.handle, pos, off, 1, out) == 6
    assert L.fmx_extract_text_batch_dev(hip.handle, pos, off, 1, 1, out, None) == 6
    assert L.fmx_prepare(hip.handle, 128) == 6
    hip.close()
    # a BWT of several LF cycles
    bwt, eof, counts = synth_bwt(20000, 1, 4, seed=21)
    hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.prepare(ktab=False, extract=True)
    assert ei.value.code == 2 and "not the BWT of one text" in str(ei.value)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.extract_text(0, 5)
    assert ei.value.code == 2
    assert hip.extract_info()[1] == 0
    hip.close()


# ---------------------------------------------------------------- the corpus: read, document, snippets
def check_corpus(cs, docs):
    for d, raw in enumerate(docs):
        assert cs.document(d) == raw, d
    # every raw window [a, b) of every document, one call per document
    for d, raw in enumerate(docs):
        wins = [(a, b) for a in range(len(raw) + 1) for b in range(a, len(raw) + 1)]
        got = cs.read(np.full(len(wins), d), [a for a, _ in wins], [b - a for a, b in wins])
        assert got == [raw[a:b] for a, b in wins], d
    # clipping at the document's end, scalars in
    assert cs.read(0, 3, 1000) == [docs[0][3:]] and cs.read(5, len(docs[5]), 4) == [b""] and cs.read(1, 0, 9) == [b""]
    assert cs.read(2, 10 ** 6, 5) == [b""]


@ends_at_a_fault
def test_corpus_read_document_and_snippets_without_the_stream(tmp_path):
    c = findex_amd.Corpus.from_documents(DOCS)
    cs = findex_amd.HipCorpusSearcher(c)
    c.drop_stream()
    check_corpus(cs, DOCS)
    # snippets: hits at a file's first byte ("p" begins document 6, "x" document 3) and last byte ("l" ends document 5, the
    # newline document 6), contexts that hold escaped bytes.  The queries hold no backslash and no escaped byte: the stream
    # does not escape the backslash, so such a query also matches halves of escape pairs (locate_docs' known limit).
    for q, before, after in ((b"p", 3, 4), (b"l", 40, 40), (b"x", 2, 2), (b"\n", 5, 0), (b"t", 0, 0), (b"ab", 1, 3), (b"zzq", 5, 5)):
        doc, raw, snips = cs.snippets(q, before=before, after=after)
        want = [(d, i) for d, t in enumerate(DOCS) for i in range(len(t)) if t.startswith(q, i)]
        assert list(zip(doc.tolist(), raw.tolist())) == want, q
        assert snips == [DOCS[d][max(i - before, 0):i + len(q) + after] for d, i in want], q
    doc, raw, snips = cs.snippets(b"p", before=4, after=4)
    assert (doc.tolist(), raw.tolist(), snips) == ([6], [0], [b"plain"])
    doc, raw, snips = cs.snippets(b"l", before=2, after=2)
    assert (5, len(DOCS[5]) - 1) in list(zip(doc.tolist(), raw.tolist())) and snips == [b"ail", b"plai"]
    doc, raw, snips = cs.snippets(b"x", before=0, after=3)
    assert (doc[0], raw[0], snips[0]) == (3, 0, b"xyz\x00")
    cs.close()
    # the same from files: python -m findex_amd.index --dir, X.data deleted
    src = tmp_path / "src"
    src.mkdir()
    for d, raw in enumerate(DOCS):
        (src / ("d%d" % d)).write_bytes(raw)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = tmp_path / "x"
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", "--dir", str(src), "--out", str(out), "--data", "--no-filter-binary"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    (tmp_path / "x.data").unlink()
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["x.aux", "x.bwt", "x.docs"]
    cs = findex_amd.HipCorpusSearcher.open(out)
    assert cs.corpus.names == [b"d%d" % d for d in range(len(DOCS))]
    for d, raw in enumerate(DOCS):
        assert cs.document(d) == raw, d
    cs.close()
