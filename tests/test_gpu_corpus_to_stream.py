"""Corpus.to_stream against the device's own map: map(to_stream(doc, raw_off)) gives (doc, raw_off) back at every raw offset,
the separator included, on a corpus with escapes at every edge and on golden directory tbad."""
import os

import numpy as np
import pytest

import corpus_ref
import findex_amd
from test_extract_cpu import DOCS

pytestmark = pytest.mark.gpu

TESTDATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testdata")


@pytest.mark.parametrize("which", ["synthetic", "tbad"])
def test_to_stream_round_trips_with_the_device_map(which):
    if which == "synthetic":
        ref = corpus_ref.RefCorpus(DOCS)
        c = findex_amd.Corpus.from_documents(DOCS)
    else:
        ref = corpus_ref.RefCorpus.from_dir(os.path.join(TESTDATA, "tbad"))
        c = findex_amd.Corpus.from_dir(os.path.join(TESTDATA, "tbad"))
    docs = np.concatenate([np.full(len(raw) + 1, d, dtype=np.int64) for d, raw in enumerate(ref.docs)])
    raws = np.concatenate([np.arange(len(raw) + 1, dtype=np.int64) for raw in ref.docs])
    pos = c.to_stream(docs, raws)
    assert pos.dtype == np.uint64 and np.all(np.diff(pos.astype(np.int64)) >= 1)          # strictly increasing: no two alike
    doc, eo, ro = c.map(pos)
    assert np.array_equal(doc.astype(np.int64), docs) and np.array_equal(ro.astype(np.int64), raws)
    assert [ref.map(int(p)) for p in pos] == list(zip(doc.tolist(), eo.tolist(), ro.tolist()))
    stream = c.stream()
    sep = pos[raws == np.array([len(ref.docs[d]) for d in docs])]
    assert np.all(stream[sep.astype(np.int64)] == 1) and sep.size == len(ref.docs)
    # whole documents back from the stream by the map
    ds, _, ep = c.tables()
    starts = ds[:-1]
    lens = (ds[1:] - np.uint64(1) - ds[:-1]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = b"".join(stream[int(a):int(a) + int(n)].tobytes() for a, n in zip(starts, lens))
    assert findex_amd.corpus.unescape_ranges(data, off, starts, ep) == ref.docs
    c.close()
