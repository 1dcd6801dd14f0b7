"""Append on the device (include/fmx.h, "append"): fmx_append_text[_dev], HipFMSearcher.append_text /
.from_text(chunk=), bwt_from_text_chunked, HipCorpusSearcher.append_documents and `python -m findex_amd.index --append`.

Every merged BWT is held, byte for byte with eof and counts, to two references: tests/merge_ref.py (written from the
definitions, given the index of A and B alone) and the product's own bwt_from_text(A + B), which test_gpu_build_text.py
holds to the goldens.  fmx_merge_last's fix-up steps, runs and longest run, its walk steps, the context and the number
of pieces are held to what merge_ref computes for the same segment, warm-up and context.  S, W, T are the header's
constants."""
import functools
import os
import sys

import numpy as np
import pytest

import findex_amd
import merge_ref
import oracle
from findex_amd import _lib
from helpers import ends_at_a_fault

pytestmark = pytest.mark.gpu

S, W, T = _lib.FMX_MERGE_SEGMENT, _lib.FMX_MERGE_WARMUP, _lib.FMX_MERGE_TILE
GUARD = 64


@pytest.fixture(params=["onehot", "bytes"])
def layout(request):
    findex_amd.set_layout(request.param)
    yield request.param
    findex_amd.set_layout("auto")


def rand_text(seed, n, syms):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(bytes(syms), dtype=np.uint8)[rng.integers(0, len(syms), n)])


@functools.lru_cache(maxsize=None)
def index_of(A):
    """(bwt, eof, counts) of A by the numpy suffix sort of merge_ref: what the reference is given instead of A"""
    return merge_ref.bwt_direct(A)


def append_dev(hip, B, shift=0, **opts):
    """fmx_append_text_dev into a buffer with guard bytes on both sides (shift: bytes by which the output is off a 16-byte
    boundary) -> (bwt, eof, counts)"""
    import torch
    dev = torch.device("cuda", 0)
    n_t = hip.n + len(B)
    text = torch.from_numpy(np.frombuffer(B, dtype=np.uint8).copy()).to(dev)
    buf = torch.full((n_t + 2 * GUARD + shift,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[GUARD + shift: GUARD + shift + n_t]
    torch.cuda.synchronize()
    eof, counts = hip.append_text_dev(text.data_ptr(), len(B), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **opts)
    host = buf.cpu().numpy()
    assert (host[: GUARD + shift] == 0xA5).all() and (host[GUARD + shift + n_t:] == 0xA5).all(), "wrote outside n + len bytes"
    return host[GUARD + shift: GUARD + shift + n_t].copy(), eof, counts


def same(got, want, what):
    assert got[1] == want[1], (what, "eof", got[1], want[1])
    assert np.array_equal(got[0], want[0]), (what, "bwt", np.nonzero(got[0] != want[0])[0][:8])
    assert np.array_equal(got[2], want[2]), (what, "counts")


def check(hip, A, B, index=None, product=True, shift=0, **opts):
    """One append through the device form, held to merge_ref (given the index of A only) and to bwt_from_text(A + B)."""
    got = append_dev(hip, B, shift=shift, **opts)
    st = hip.merge_last()
    ref = merge_ref.merge_ref(None, B, segment=opts.get("segment") or S, warmup=W if opts.get("warmup") is None else opts["warmup"],
                              context=opts.get("context") or _lib.FMX_MERGE_CONTEXT, index=index if index is not None else index_of(A))
    same(got, (ref["bwt"], ref["eof"], ref["counts"]), "merge_ref")
    if product:
        same(got, findex_amd.bwt_from_text(A + B), "bwt_from_text(A + B)")
    for key in ("walk_steps", "fixup_steps", "longest_run", "runs", "context", "rounds"):
        assert st[key] == ref[key], (key, st[key], ref[key])
    assert min(st["piece_ms"], st["walk_ms"], st["fixup_ms"], st["emit_ms"]) >= 0
    return got, ref, st


# ---------------------------------------------------------------- fixtures and one-byte cases
@ends_at_a_fault
def test_fixture_handle_without_text(testdata, layout):
    """A opened from .bwt / .aux: the tail of A comes from the handle's Psi walk"""
    A = open(os.path.join(testdata, "test1024.txt"), "rb").read()
    B = open(os.path.join(testdata, "test2048.txt"), "rb").read()
    hip = findex_amd.HipFMSearcher(os.path.join(testdata, "test1024.cmp.bwt"), bigEndian=False)
    gbwt, size, geof = oracle.load_bwt_file(os.path.join(testdata, "test1024.cmp.bwt"), bigEndian=False)
    gaux = oracle.load_aux_file(os.path.join(testdata, "test1024.cmp.aux"), bigEndian=False)
    assert size == len(A) + 1 and hip.n == size
    check(hip, A, B, index=(np.asarray(gbwt, dtype=np.uint8), geof, np.asarray(gaux, dtype=np.int64)))
    check(hip, A, B[:777], shift=3)                          # an output off the 16-byte boundary
    hip.close()


@ends_at_a_fault
def test_from_text_and_one_byte_cases(layout):
    A = rand_text(1, 3000, b"acgt")
    hip = findex_amd.HipFMSearcher.from_text(A)
    check(hip, A, rand_text(2, 1500, b"acgt"))
    for B in (b"a", b"t", b"x", b"\x01", b"\xff"):            # B of one byte
        check(hip, A, B)
    hip.close()
    for A1 in (b"a", b"\xff"):                               # A of one byte
        h1 = findex_amd.HipFMSearcher.from_text(A1)
        for B in (b"a", b"b", rand_text(3, 700, b"ab")):
            check(h1, A1, B)
        h1.close()


# ---------------------------------------------------------------- segment edges
@ends_at_a_fault
@pytest.mark.parametrize("b", [S - 1, S, S + 1, 3 * S + 5])
def test_segment_edges(layout, b):
    A = rand_text(4, 3000, b"acgt")
    B = rand_text(5 + b, b, b"acgt")
    hip = findex_amd.HipFMSearcher.from_text(A)
    _, ref, _ = check(hip, A, B)
    _, ref1, _ = check(hip, A, B, segment=1, warmup=0)
    assert ref1["walk_steps"] == b and ref1["runs"] >= 1     # one step from the full range resolves nothing A holds
    hip.close()


# ---------------------------------------------------------------- unresolved runs
def planted(kind):
    """sigma = 2 texts where B holds a copy of a stretch of A; positions are B's, a segment covers S positions of
    reverse(B) counted from B's end"""
    A = rand_text(11, 6000, b"ab")
    bg = lambda seed, n: rand_text(seed, n, b"ab")
    b = 5 * S + 17
    if kind == "short":                     # shorter than the warm-up
        return A, bg(12, 600) + A[1000:1008] + bg(13, 401)
    if kind == "two_borders":               # 2 S + 3 bytes
        L = 2 * S + 3
        return A, bg(14, 300) + A[2000:2000 + L] + bg(15, b - 300 - L)
    if kind == "three_segments":            # 3 S + 40 bytes: a run over two segment borders at the header's S and W
        L = 3 * S + 40
        return A, bg(22, 200) + A[100:100 + L] + bg(23, b - 200 - L)
    if kind == "ends_on_border":            # S + 100 bytes whose first byte is a segment's last position: the run it
        L = S + 100                         # causes in the segment before starts at that border
        i0 = b - 2 * S
        return A, bg(16, i0) + A[3000:3000 + L] + bg(17, b - i0 - L)
    if kind == "starts_on_border":          # S + 100 bytes whose last byte is a segment's first position: that segment is
        L = S + 100                         # unresolved throughout and the run ends on its border
        i0 = b - 3 * S - 100
        return A, bg(18, i0) + A[3500:3500 + L] + bg(19, b - i0 - L)
    if kind == "at_end":
        return A, bg(20, b - 400) + A[4000:4400]
    if kind == "at_start":
        return A, A[5000:5400] + bg(21, b - 400)
    raise KeyError(kind)


@ends_at_a_fault
@pytest.mark.parametrize("kind", ["short", "two_borders", "three_segments", "ends_on_border", "starts_on_border", "at_end", "at_start"])
def test_unresolved_runs(layout, kind):
    A, B = planted(kind)
    hip = findex_amd.HipFMSearcher.from_text(A)
    _, ref, st = check(hip, A, B)
    if kind == "short":
        assert ref["fixup_steps"] == 0 and st["runs"] == 0
    else:
        assert ref["fixup_steps"] > 0
    # A run begins at a segment border that lies at least about W positions inside the stretch (else the warm-up has
    # emptied the interval), so at the header's S and W a stretch of 2 S + 3 bytes gives a run over ONE border, 3 S + 40
    # bytes one over two; with segment = 64 the 2 S + 3 bytes cross many.
    if kind == "two_borders":
        assert ref["longest_run"] > S
    if kind == "three_segments":
        assert ref["longest_run"] > 2 * S
    if kind == "starts_on_border":
        assert ref["longest_run"] >= S                       # a whole segment and the stretch's rest right of it
    _, ref64, _ = check(hip, A, B, segment=64, warmup=4)     # the same with more borders and hardly any warm-up
    if kind == "two_borders":
        assert ref64["longest_run"] > 2 * 64 + 4
    hip.close()


# ---------------------------------------------------------------- context
def retry_case():
    """B begins with A's last 4096 + 5 bytes.  The order of two new suffixes needs more of A only where B holds
    tail(A, M) followed by B's own first byte, so that copy is followed by B[0]: the piece of M = 4096 then fails, 8192
    passes."""
    A = rand_text(31, 9000, b"acgt")
    tail = A[-(4096 + 5):]
    return A, tail + tail[:1] + rand_text(32, 200, b"acgt")


@ends_at_a_fault
def test_context_retry(layout):
    A, B = retry_case()
    hip = findex_amd.HipFMSearcher.from_text(A)
    _, ref, st = check(hip, A, B)
    assert (ref["rounds"], ref["context"]) == (2, 8192)
    assert (st["rounds"], st["context"]) == (2, 8192)
    _, _, st = check(hip, A, B, context=8192)
    assert st["rounds"] == 1
    hip.close()


@ends_at_a_fault
def test_b_equal_a(layout):
    A = rand_text(33, 3000, b"acgt")
    hip = findex_amd.HipFMSearcher.from_text(A)
    _, ref, st = check(hip, A, A)
    exact_from = min(lo for lo in range(0, len(A), S) if min(lo + S, len(A)) + W >= len(A))        # a segment whose warm-up is clipped at b starts exact
    assert st["context"] == len(A) and st["runs"] == 1 and st["longest_run"] == st["fixup_steps"] == exact_from
    hip.close()
    P = rand_text(34, 100, b"acgt") * 30                     # periodic: every context short of all of A fails
    hp = findex_amd.HipFMSearcher.from_text(P)
    _, ref, st = check(hp, P, P, context=64)
    assert st["context"] == len(P) and st["rounds"] == 7 and st["runs"] == 1      # 64, 128, .., 2048 fail; 4096 -> a
    hp.close()


@ends_at_a_fault
def test_max_context_below_the_need():
    import torch
    A, B = retry_case()
    hip = findex_amd.HipFMSearcher.from_text(A)
    q = A[100:108][::-1]
    before = hip.search(q)
    with pytest.raises(findex_amd.FmxError):                 # (first use: the select directory an append builds, the runtime's own
        hip.append_text(B, max_context=4096)                 # allocations for a stream and for kernels not launched before)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(findex_amd.FmxError) as e:
        hip.append_text(B, max_context=4096)
    assert e.value.code == 6 and "8192" in str(e.value) and "max_context" in str(e.value)
    assert torch.cuda.mem_get_info()[0] == free0
    assert hip.search(q) == before
    new = hip.append_text(B, max_context=8192)
    assert new.n == hip.n + len(B)
    new.close()
    hip.close()


# ---------------------------------------------------------------- symbols
@ends_at_a_fault
def test_symbols_a_lacks(layout):
    A = rand_text(41, 2000, b"bd")
    hip = findex_amd.HipFMSearcher.from_text(A)
    for B in (b"a", b"e", b"c", rand_text(42, 900, b"abcde"), rand_text(43, 600, b"\x01\xff")):
        check(hip, A, B)
    hip.close()


@ends_at_a_fault
def test_eof_rows_of_a(layout):
    for A, want in ((rand_text(44, 1500, b"bcd") + b"z", "last"), (rand_text(45, 1500, b"bcd") + b"a", "row1")):
        hip = findex_amd.HipFMSearcher.from_text(A)
        assert hip.eof == (hip.n - 1 if want == "last" else 1)
        for B in (rand_text(46, 500, b"abcdz"), b"z", b"a", b"c"):
            check(hip, A, B)
        hip.close()


@ends_at_a_fault
@pytest.mark.parametrize("row", [T, T - 1])
def test_new_eof_row_on_a_tile_edge(layout, row):
    """A + B ends with "za", z nowhere else and a the smallest letter: reverse(A + B) is the largest suffix that begins with
    a, so the new eof row is the number of a's -- a tile's first row, or a tile's last."""
    rng = np.random.default_rng(47 + row)
    n = 3 * T
    body = np.full(n - 2, ord("b"), dtype=np.uint8)
    body[rng.choice(n - 2, row - 1, replace=False)] = ord("a")
    text = bytes(body) + b"za"
    A, B = text[:7000], text[7000:]
    hip = findex_amd.HipFMSearcher.from_text(A)
    got, ref, _ = check(hip, A, B)
    assert ref["eof"] == row and got[1] == row
    hip.close()


# ---------------------------------------------------------------- emit edges
@ends_at_a_fault
@pytest.mark.parametrize("n_a", [T - 1, T, T + 1, 3 * T + 5])
def test_emit_edges(layout, n_a):
    """A over {a, c}, B of b's alone: all new suffixes lie between A's a-rows and c-rows, 2 T + 904 rows in a row -- a tile of
    new suffixes only, and neighbours on a tile's last and the next tile's first row."""
    A = rand_text(50 + n_a, n_a - 1, b"ac")
    B = b"b" * (2 * T + 904)
    hip = findex_amd.HipFMSearcher.from_text(A)
    assert hip.n == n_a
    _, ref, _ = check(hip, A, B)
    rows = ref["rows"]
    assert np.all(np.diff(rows) == 1)
    first_tile = -(-int(rows[0]) // T)
    assert (first_tile + 1) * T - 1 <= rows[-1]              # tile first_tile holds new suffixes only
    hip.close()
    if n_a == 3 * T + 5:                                     # new suffixes scattered through every tile
        A2 = rand_text(60, n_a - 1, b"acgt")
        h2 = findex_amd.HipFMSearcher.from_text(A2)
        check(h2, A2, rand_text(61, 2 * T + 11, b"acgt"))
        h2.close()


# ---------------------------------------------------------------- chunking
CHUNK_TEXT = rand_text(70, 5000, b"acgt")


@ends_at_a_fault
@pytest.mark.parametrize("chunk", [1, 7, S, len(CHUNK_TEXT) - 1, len(CHUNK_TEXT)])
def test_chunked_construction(chunk):
    """chunk = 1 is 4999 appends, 1.2 ms each: the slowest case of this module, 5.9 s"""
    want = findex_amd.bwt_from_text(CHUNK_TEXT)
    same(findex_amd.bwt_from_text_chunked(CHUNK_TEXT, chunk), want, "chunk %d" % chunk)


@ends_at_a_fault
def test_two_appends_and_two_runs(layout):
    t = CHUNK_TEXT
    h0 = findex_amd.HipFMSearcher.from_text(t[:2000])
    h1 = h0.append_text(t[2000:3100])
    h2 = h1.append_text(t[3100:])
    want = findex_amd.bwt_from_text(t)
    same((h2.bwt_bytes(), h2.eof, h2.counts()), want, "two appends")
    again = h1.append_text(t[3100:])
    same((again.bwt_bytes(), again.eof, again.counts()), want, "second run")
    a = append_dev(h1, t[3100:])
    b = append_dev(h1, t[3100:])
    same(a, b, "device form twice")
    same(a, want, "device form")
    for h in (h0, h1, h2, again):
        h.close()


# ---------------------------------------------------------------- the merged handle works
@ends_at_a_fault
def test_merged_handle_answers_as_the_rebuilt_one(layout):
    A, B = rand_text(80, 4000, b"acgt"), rand_text(81, 3000, b"acgt")
    text = A + B
    old = findex_amd.HipFMSearcher.from_text(A)
    rng = np.random.default_rng(82)
    pats = [text[i:i + m][::-1] for i, m in zip(rng.integers(0, len(text) - 12, 300), rng.integers(1, 12, 300))]
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    buf = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    old_sp, old_ep = old.search_batch(buf, off)
    seen = old.stats()["patterns_seen"]
    merged = old.append_text(B)
    assert old.stats()["patterns_seen"] == seen              # the append searched nothing on the old handle
    rebuilt = findex_amd.HipFMSearcher.from_text(text)
    assert (merged.n, merged.eof) == (rebuilt.n, rebuilt.eof) and np.array_equal(merged.bucketStarts, rebuilt.bucketStarts)
    sp, ep = merged.search_batch(buf, off)
    wsp, wep = rebuilt.search_batch(buf, off)
    assert np.array_equal(sp, wsp) and np.array_equal(ep, wep) and np.all(sp < ep)
    for q in (text[3990:4010], text[100:104], B[-5:], b"acgtacgtacgtacgtacgt"):      # one across the seam
        assert np.array_equal(np.sort(merged.locate_text(q)), np.sort(rebuilt.locate_text(q)))
    assert len(merged.locate_text(text[3990:4010])) >= 1
    sp2, ep2 = old.search_batch(buf, off)
    assert np.array_equal(sp2, old_sp) and np.array_equal(ep2, old_ep)
    for h in (old, merged, rebuilt):
        h.close()


# ---------------------------------------------------------------- device form
@ends_at_a_fault
def test_refused_under_a_capture_that_still_ends_validly():
    import torch
    dev = torch.device("cuda", 0)
    A = rand_text(90, 2000, b"acgt")
    hip = findex_amd.HipFMSearcher.from_text(A)
    text = torch.full((512,), 97, dtype=torch.uint8, device=dev)
    out = torch.empty(hip.n + 512, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            hip.append_text_dev(text.data_ptr(), 512, out.data_ptr(), stream=s.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        out.zero_()                                          # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert err is not None and err.code == 5 and "stream capture" in str(err)
    torch.cuda.synchronize()
    new = hip.append_text(b"a" * 512)                        # the handle and the device go on working
    assert new.n == hip.n + 512
    new.close()
    hip.close()


@ends_at_a_fault
def test_block_handles_are_refused():
    bwt, eof, counts = findex_amd.bwt_from_text(rand_text(91, 500, b"ab"))
    bs = np.zeros(256, dtype=np.int64)
    blk = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    with pytest.raises(findex_amd.FmxError) as e:
        blk.append_text(b"ab")
    assert e.value.code == 6 and "fmx_open_block" in str(e.value)
    blk.close()


@ends_at_a_fault
def test_device_memory_returns():
    import torch
    dev = torch.device("cuda", 0)
    A = rand_text(92, 1 << 20, b"acgt")
    b = 1 << 22
    hip = findex_amd.HipFMSearcher.from_text(A)
    g = torch.Generator(device=dev)
    g.manual_seed(93)
    text = torch.randint(1, 5, (b,), generator=g, device=dev, dtype=torch.uint8)
    out = torch.empty(hip.n + b, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hip.append_text_dev(text.data_ptr(), 1 << 16, out.data_ptr(), stream=stream)      # first-use allocations happen here
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    eof, counts = hip.append_text_dev(text.data_ptr(), b, out.data_ptr(), stream=stream)
    new = hip.append_text(rand_text(94, 1 << 18, b"acgt"))
    new.close()
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 64 << 20
    assert int(counts.sum()) == len(A) + b and eof < hip.n + b
    assert hip.merge_last()["need_bytes"] > 47 * (1 << 18)
    hip.close()


@ends_at_a_fault
def test_refused_when_free_memory_is_below_the_need():
    """Free HBM held below the need (some 47 bytes per piece byte and 17 per new byte: 2^24 bytes need about 1 GB): refused
    with the need in the message, nothing allocated, the handle still good."""
    import time
    import torch
    dev = torch.device("cuda", 0)
    A = rand_text(95, 1 << 16, b"acgt")
    b = 1 << 24
    hip = findex_amd.HipFMSearcher.from_text(A)
    text = torch.randint(1, 5, (b,), device=dev, dtype=torch.uint8)
    out = torch.empty(hip.n + b, dtype=torch.uint8, device=dev)
    hip.append_text_dev(text.data_ptr(), 1 << 12, out.data_ptr())
    need = hip.merge_last()["need_bytes"]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.time()
    hog = torch.empty(free0 - (256 << 20), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    print("holding %d MiB took %.1f s" % ((free0 - (256 << 20)) >> 20, time.time() - t0))
    free1 = torch.cuda.mem_get_info()[0]
    assert need < free1 < (1 << 30)
    with pytest.raises(findex_amd.FmxError) as e:
        hip.append_text_dev(text.data_ptr(), b, out.data_ptr())
    assert e.value.code == 4 and "needs" in str(e.value) and "are free" in str(e.value)
    assert torch.cuda.mem_get_info()[0] == free1
    hip.append_text_dev(text.data_ptr(), 1 << 12, out.data_ptr())            # what fits still runs
    del hog
    torch.cuda.empty_cache()
    hip.close()


# ---------------------------------------------------------------- corpus
@ends_at_a_fault
def test_corpus_append_documents(tmp_path):
    from test_gpu_repeats import corpus_documents
    docs = corpus_documents()
    names = [b"doc%d.txt" % d for d in range(len(docs))]
    whole = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs, names))
    first = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs[:5], names[:5]))
    both = first.append_documents(docs[5:], names[5:])
    same((both.searcher.bwt_bytes(), both.searcher.eof, both.searcher.counts()),
         (whole.searcher.bwt_bytes(), whole.searcher.eof, whole.searcher.counts()), "corpus index")
    for got, want in zip(both.corpus.tables(), whole.corpus.tables()):
        assert np.array_equal(got, want)
    assert both.corpus.names == whole.corpus.names and both.corpus.n_docs == 8
    assert first.corpus.n_docs == 5 and first.searcher.n == first.corpus.stream_len + 1      # the old one is untouched
    for q in (b"best of times", b"raw zero \x00 raw", docs[6][3:11], docs[1][:9]):
        for a, b in zip(both.locate_docs(q), whole.locate_docs(q)):
            assert np.array_equal(a, b)
        assert len(both.locate_docs(q)[0]) >= 1
    for got, want in zip(both.list_docs([b"times", b"raw one \x01", docs[5][:6]]), whole.list_docs([b"times", b"raw one \x01", docs[5][:6]])):
        assert np.array_equal(got, want)
    for d in (1, 6, 7):
        assert both.document(d) == docs[d]
    # default names go on counting
    more = first.append_documents(docs[5:])
    assert more.corpus.names[5:] == [b"5", b"6", b"7"]
    more.close()
    for h in (whole, first, both):
        h.close()


class Ran:
    pass


def run_index(capsys, *argv):
    """python -m findex_amd.index with these arguments, in this process (the module's main is what the command runs)"""
    from findex_amd import index
    capsys.readouterr()
    r = Ran()
    r.returncode = index.main(list(argv))
    r.stdout, r.stderr = capsys.readouterr()
    return r


@ends_at_a_fault
def test_cli_append_to_a_corpus(tmp_path, capsys):
    """--append on disk: a corpus index written from four files with X.sa and X.lcp, three more files appended with --sa:
    X.bwt / X.aux / X.docs / X.sa describe all seven, the stale X.lcp is gone."""
    from test_gpu_repeats import corpus_documents
    plain = [d for d in corpus_documents() if d]             # (a directory listing keeps no empty file apart)
    src, src2 = tmp_path / "four", tmp_path / "three"
    src.mkdir()
    src2.mkdir()
    content = {}
    for d, raw in enumerate(plain):
        ((src if d < 4 else src2) / ("f%d.txt" % d)).write_bytes(raw)
        content[b"f%d.txt" % d] = raw
    base = str(tmp_path / "idx")
    r = run_index(capsys, "--dir", str(src), "--out", base, "--no-filter-binary", "--sa", "--lcp")
    assert r.returncode == 0, r.stderr
    assert os.path.exists(base + ".lcp")
    r = run_index(capsys, "--append", base, "--dir", str(src2), "--no-filter-binary", "--sa")
    assert r.returncode == 0, r.stderr
    assert os.path.exists(base + ".sa") and not os.path.exists(base + ".lcp") and "idx.lcp" in r.stderr
    opened = findex_amd.HipCorpusSearcher.open(base)
    assert sorted(opened.corpus.names) == sorted(content) and set(opened.corpus.names[:4]) == {b"f%d.txt" % d for d in range(4)}
    every = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents([content[nm] for nm in opened.corpus.names], opened.corpus.names))
    same((opened.searcher.bwt_bytes(), opened.searcher.eof, opened.searcher.counts()),
         (every.searcher.bwt_bytes(), every.searcher.eof, every.searcher.counts()), "--append")
    for got, want in zip(opened.corpus.tables(), every.corpus.tables()):
        assert np.array_equal(got, want)
    sa = np.frombuffer(open(base + ".sa", "rb").read(), dtype=">u4")
    assert sa.size == opened.searcher.n and np.array_equal(sa[:50], opened.searcher.locate(np.arange(50, dtype=np.uint64)))
    for h in (opened, every):
        h.close()


@ends_at_a_fault
def test_cli_append_to_a_text_and_chunk(tmp_path, capsys):
    """X.bwt / X.aux of a text with a second file appended, and of the whole text with --chunk: the same files."""
    t1, t2 = tmp_path / "t.txt", tmp_path / "u.txt"
    t1.write_bytes(CHUNK_TEXT[:3000])
    t2.write_bytes(CHUNK_TEXT[3000:])
    r = run_index(capsys, str(t1), "--sa")
    assert r.returncode == 0, r.stderr
    r = run_index(capsys, "--append", str(tmp_path / "t"), str(t2))
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(str(tmp_path / "t.sa")) and "t.sa" in r.stderr
    full = tmp_path / "full.txt"
    full.write_bytes(CHUNK_TEXT)
    r = run_index(capsys, str(full), "--chunk", "1024")
    assert r.returncode == 0, r.stderr
    for ext in (".bwt", ".aux"):
        assert (tmp_path / ("t" + ext)).read_bytes() == (tmp_path / ("full" + ext)).read_bytes()
    hb = findex_amd.HipFMSearcher(str(full))
    same((hb.bwt_bytes(), hb.eof, hb.counts()), findex_amd.bwt_from_text(CHUNK_TEXT), "--chunk")
    hb.close()
