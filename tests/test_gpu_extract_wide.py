"""Extraction by text position on an index of more than 2^32 rows, in both layouts: k_extract<true, kLayoutOneHot> starts
only when n > 2^32, the samples are u64 only then, and below this size no row or SA value of 2^32 or more ever passed
through the kernel.

The text is 'b' x p + 'a' x q with p = 2^29 + 77 and q = 2^32 + 1000, n = p + q + 1 rows.  Its BWT is written directly into
device memory (s = reverse(text) + sentinel = a^q b^p $; the closed form was held to a brute-force suffix sort for small p and q):
eof = 1; row 0 is 'b'; rows 2 .. q are 'a'; rows q + 1 .. q + p - 1 are 'b'; row q + p is 'a'; slot 1 is a filler.  Row r in
1 .. q has SA r - 1 and row q + i has SA n - 1 - i.  So text[t] is 'b' iff t < p, the 'b' rows lie above 2^32, and SA values above
2^32 belong to small t.  Every expectation is that rule; nothing of the library produces one.

Seconds on the MI355X: the slowest test is the first to touch the device -- 1.4 s with the start of torch when
the module runs alone; the fixture (the BWT and both handles) is 0.3 s, a layout's samples 0.4 / 0.7 s and its five batches
0.1 s -- SLOWEST_S; the limit of a test is three times that, the margin tests/test_gpu_search_forms.py takes for the machine's
load.
"""
import gc
import time

import numpy as np
import pytest

import findex_amd
from findex_amd import _lib
from helpers import ends_at_a_fault

SLOWEST_S = 2
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
P = (1 << 29) + 77
Q = LINE + 1000
N = P + Q + 1
T = _lib.FMX_EXTRACT_TILE
LAYOUTS = ("onehot", "bytes")


def closed_form_bwt(p, q):
    """(bwt, eof) of 'b' x p + 'a' x q as the header defines it, on the host: for the brute-force check of small sizes."""
    bwt = np.full(p + q + 1, ord("a"), dtype=np.uint8)
    bwt[0] = ord("b")
    bwt[q + 1:q + p] = ord("b")
    return bwt, 1


def test_closed_form_against_a_suffix_sort():
    from helpers import bwt_of_text
    for p, q in ((1, 1), (1, 5), (4, 1), (3, 7), (6, 2), (9, 9)):
        want, weof, _ = bwt_of_text((b"b" * p + b"a" * q)[::-1])
        got, eof = closed_form_bwt(p, q)
        keep = np.arange(p + q + 1) != eof
        assert weof == eof and np.array_equal(got[keep], want[keep]), (p, q)


class Wide:
    pass


@pytest.fixture(scope="module")
def wide():
    import torch
    w = Wide()
    t0 = time.time()
    gc.collect()
    torch.cuda.empty_cache()
    bwt = torch.full((N,), ord("a"), dtype=torch.uint8, device="cuda")
    bwt[0] = ord("b")
    bwt[Q + 1:Q + P] = ord("b")
    counts = np.zeros(256, dtype=np.int64)
    counts[ord("a")], counts[ord("b")] = Q, P
    torch.cuda.synchronize()
    w.hip = {}
    try:
        for layout in LAYOUTS:
            findex_amd.set_layout(layout)
            w.hip[layout] = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), N, 1, counts)
    finally:
        findex_amd.set_layout("auto")
    del bwt
    for layout in LAYOUTS:
        assert w.hip[layout].stats()["layout"] == (0 if layout == "onehot" else 1) and w.hip[layout].n == N > LINE
    print("wide extract: index of %d rows in both layouts, %.1f s" % (N, time.time() - t0))
    yield w
    for h in w.hip.values():
        h.close()
    gc.collect()
    torch.cuda.empty_cache()


def batches():
    """(name, pos, lens) of every batch."""
    rng = np.random.default_rng(41)
    out = []
    pos, lens = [], []
    for al in range(32):                                          # straddling t = p at every alignment mod 32
        for ln in (1, 33, T + 5, 3 * T):
            pos += [P - 1 - al, P + al, P - ln + (al % ln)]
            lens += [ln, ln, ln]
    pos += [P, P - 1]
    lens += [1, 1]
    out.append(("around t = p", pos, lens))
    out.append(("at t = 0", [0, 0, 0, 1, 31, 32], [1, 77, 3 * T, T, T + 1, 2]))
    ends = (1, 31, 32, 33, T, 3 * T)
    out.append(("ending at n - 1", [N - 1 - ln for ln in ends] + [N - 1], list(ends) + [0]))
    t0 = N - 1 - LINE                                             # SA == 2^32 there
    pos, lens = [t0 - 1, t0, t0 + 1], [1, 1, 1]
    for al in range(0, 32, 3):
        pos += [t0 - 3 * T // 2 - al, t0 - al, t0 - 33 + al]
        lens += [3 * T, T + 1, 66]
    out.append(("around SA = 2^32", pos, lens))
    out.append(("2^20 single bytes", rng.integers(0, N - 1, 1 << 20, dtype=np.uint64), np.ones(1 << 20, dtype=np.uint64)))
    return out


def expected(pos, lens):
    """text[t] = 'b' iff t < p, range after range."""
    pos = np.asarray(pos, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    t = np.repeat(pos - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
    return np.where(t < P, ord("b"), ord("a")).astype(np.uint8)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_extract_above_two_to_the_32(wide, layout):
    hip = wide.hip[layout]
    t0 = time.time()
    hip.prepare(ktab=False, extract=True)
    rate, nbytes, ms = hip.extract_info()
    print("%s: samples built in %.1f s (%.0f ms inside the build)" % (layout, time.time() - t0, ms))
    assert rate == 32 and nbytes == ((N - 1) // 32 + 1) * 8      # u64 samples above 2^32 rows
    for name, pos, lens in batches():
        want = expected(pos, lens)
        if name in ("around t = p", "2^20 single bytes"):
            assert want.min() == ord("a") and want.max() == ord("b"), name
        off, got = hip.extract_text_batch(pos, lens)
        kms, steps, requests = hip.extract_last()
        print("%s %s: %d ranges, %d bytes, %d steps, %d requests, %.3f ms" % (layout, name, len(lens), want.size, steps, requests, kms))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (layout, name, int(bad[0]), int(np.searchsorted(off, bad[0], side="right") - 1))
        assert want.size <= steps and 0 < requests <= 4 * steps
