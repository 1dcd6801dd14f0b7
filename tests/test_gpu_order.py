"""What the shared order kernels promise on behalf of a caller that never exercised it: the CSR offsets of an
approximate search whose last offset is answered without a search and whose key array may be missing, and the class maxima
of repeats and n-grams where a repeated class ends at the last row.  Against tests/approx_ref.py, tests/repeats_ref.py and
tests/ngrams_ref.py; nothing of the library produces an expectation."""
import numpy as np
import pytest

import approx_ref
import findex_amd
import ngrams_ref
import repeats_ref
from findex_amd import _lib
from helpers import bwt_of_text, pack_patterns

pytestmark = pytest.mark.gpu

HIT = findex_amd.HipFMSearcher.APPROX_HIT
T = _lib.FMX_REPEATS_TILE


@pytest.mark.parametrize("k", [1, 3])
def test_approx_offsets_without_hits_and_with_hits_in_the_last_pattern_only(k):
    """k patterns, first none of them with a hit (no key is ever sorted: every offset is 0), then only the last with hits:
    out_off[0 .. k - 1] are searched for in the keys, all of which lie behind them, and out_off[k] is the row count."""
    rng = np.random.default_rng(250)
    s = bytes(rng.integers(97, 101, 3000, dtype=np.uint8))
    absent = [b"zzzz", b"zzzzzz", b"zazz"][:k]
    last = s[10:16]
    hip = findex_amd.HipFMSearcher.from_mem(*bwt_of_text(s))
    for pats in (absent, absent[:k - 1] + [last]):
        per = [approx_ref.window_hits(s, p, 1) for p in pats]
        assert all(not h for h in per[:k - 1]) and bool(per[-1]) == (pats[-1] == last)
        off, rows = approx_ref.expected_csr(per)
        buf, poff = pack_patterns(pats)
        got_off, got = hip.search_approx_batch(buf, poff, 1)
        assert got_off.tolist() == off and got_off.size == k + 1
        want = np.array(rows, dtype=HIT) if rows else np.zeros(0, dtype=HIT)
        assert got.tobytes() == want.tobytes()
        assert got.size == 0 or (got["pattern"] == k - 1).all()
    hip.close()


def test_repeats_and_ngrams_where_a_repeated_class_ends_at_the_last_row():
    """A text of 2 T + 3 bytes with a stop byte: three scan blocks, and at L = 1 the class of the largest byte is repeated
    and its last row is row n - 1, the one row whose LCP entry stands for no neighbour."""
    rng = np.random.default_rng(251)
    a = rng.integers(97, 101, 2 * T + 3, dtype=np.uint8)
    a[rng.choice(a.size, 40, replace=False)] = 10               # the stop byte, smaller than every letter
    a[[T - 1, T, 2 * T - 1, 2 * T, a.size - 1]] = 100            # the largest byte at the blocks' edges and at the end
    text = a.tobytes()
    n = len(text) + 1
    assert len(text) == 2 * T + 3 and text.count(bytes([max(text)])) >= 2 and 10 in text
    rec, _ = ngrams_ref.hashed(text, 1, min_count=2, order="row", stop=10)
    assert int(rec["sp"][-1] + rec["count"][-1]) == n and int(rec["count"][-1]) >= 2      # a repeated class ends at row n - 1
    levels = [1, 2, 7]
    hip = findex_amd.HipFMSearcher.from_text(text)
    for later in (False, True):
        got = hip.repeats(levels, keep_first=later, stop=10)
        for L, (ranges, summary) in zip(levels, got):
            want_r, want_s = repeats_ref.hashed(text, L, later, 10)
            assert summary == want_s, (L, later, summary, want_s)
            assert ranges.shape == want_r.shape and np.array_equal(ranges, want_r), (L, later)
    for order in ("row", "count"):
        got = hip.ngrams(levels, min_count=2, order=order, stop=10)
        for L, (records, summary) in zip(levels, got):
            want_rec, want_s = ngrams_ref.hashed(text, L, min_count=2, order=order, stop=10)
            assert {f: summary[f] for f in ngrams_ref.FIELDS} == want_s, (L, order, summary, want_s)
            assert records.shape == want_rec.shape and records.tobytes() == want_rec.tobytes(), (L, order)
    hip.close()
