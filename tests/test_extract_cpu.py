"""The corpus map backwards, without a GPU: Corpus.to_stream (the inverse of the position map) and the map-driven unescape
in numpy, against the per-position table of corpus_ref.py.  The cases of the device side of extraction (symbols, argument
errors, the "extract_sample" key) belong in this file too, once that side exists."""
import types

import numpy as np

from corpus_ref import RefCorpus
from findex_amd.corpus import Corpus, stream_positions, unescape_ranges

# raw 0, 1 and 255, lone backslashes, a file's own backslash-zero (no escape: the reference does not escape the backslash),
# an empty document, a document that ends in an escape, one that begins with one
DOCS = [b"ab\x00c\\d\\0e", b"", b"\x01\xff\\", b"xyz\x00", b"\\0\\1\\f", b"\xff\xff\x00\x00\x01\x01 tail", b"plain text\n"]


def test_to_stream_inverts_the_map_at_every_position():
    ref = RefCorpus(DOCS)
    esc = set(ref.esc_pos)
    # Corpus.to_stream is stream_positions over the handle's tables: a stand-in supplies them without a device
    stub = types.SimpleNamespace(tables=lambda: (np.array(ref.doc_start, dtype=np.uint64), np.array(ref.raw_len, dtype=np.uint64),
                                                 np.array(ref.esc_pos, dtype=np.uint64)))
    docs = np.array([t[0] for t in ref.table])
    raws = np.array([t[2] for t in ref.table])
    got = Corpus.to_stream(stub, docs, raws)
    assert got.dtype == np.uint64 and got.size == len(ref.stream)
    assert np.array_equal(got, stream_positions(ref.doc_start, ref.esc_pos, docs, raws))
    for p, (d, _, ro) in enumerate(ref.table):
        s = int(got[p])
        # the position of the byte itself, or of its backslash when p is the second byte of an escape pair
        assert s == (p - 1 if (p - 1) in esc else p), (p, s)
        assert ref.map(s)[0] == d and ref.map(s)[2] == ro
    # every (doc, raw_off), the separator (raw_off == raw_len) included, by the definition
    for d, raw in enumerate(ref.docs):
        for ro in range(len(raw) + 1):
            want = ref.doc_start[d] + ro + sum(1 for c in raw[:ro] if c in (0, 1, 255))
            assert int(Corpus.to_stream(stub, [d], [ro])[0]) == want, (d, ro)
        assert ref.stream[int(Corpus.to_stream(stub, d, len(raw))[0])] == 1


def test_unescape_by_the_map():
    ref = RefCorpus(DOCS)
    ds = np.array(ref.doc_start, dtype=np.uint64)
    # whole documents, in one call
    starts = ds[:-1]
    lens = ds[1:] - 1 - ds[:-1]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = b"".join(ref.stream[int(a):int(a + n)] for a, n in zip(starts, lens))
    assert unescape_ranges(data, off, starts, ref.esc_pos) == ref.docs
    assert ref.docs[0].count(b"\\0") == 1 and ref.docs[4] == b"\\0\\1\\f"        # pattern matching would get these wrong
    # every raw window of every document
    for d, raw in enumerate(ref.docs):
        for a in range(len(raw) + 1):
            for b in range(a, len(raw) + 1):
                s0, s1 = (int(x) for x in stream_positions(ref.doc_start, ref.esc_pos, [d, d], [a, b]))
                got = unescape_ranges(ref.stream[s0:s1], [0, s1 - s0], [s0], ref.esc_pos)
                assert got == [raw[a:b]], (d, a, b)



def test_unescape_refuses_data_that_disagrees_with_the_map():
    import pytest
    ref = RefCorpus(DOCS)
    e = ref.esc_pos[0]
    for bad in (ref.stream[:e] + b"x" + ref.stream[e + 1:], ref.stream[:e + 1] + b"7" + ref.stream[e + 2:]):
        with pytest.raises(ValueError):
            unescape_ranges(bad, [0, len(bad)], [0], ref.esc_pos)
    with pytest.raises(ValueError):                                   # a range that ends inside a pair
        unescape_ranges(ref.stream[:e + 1], [0, e + 1], [0], ref.esc_pos)
    assert unescape_ranges(bytearray(ref.stream[:e]), [0, e], [0], ref.esc_pos) == [ref.docs[0][:e]]
