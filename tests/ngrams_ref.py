"""The yardsticks of the n-grams feature (fmx.h: n-grams).

A window is text[t : t + L]; with a stop byte a window that holds it does not count.  A class is the set of the windows with
the same bytes, its count their number, its first position the smallest t.  Its sp is the first row of the suffix array of
s = reverse(text) + sentinel whose suffix begins with reverse(window).  A call lists the classes with count >= min_count by
sp ("row") or by descending count, ties by sp ("count"), the first `top` of them (0: all), and sums up: records, selected,
distinct, windows, singletons, largest_count, largest_sp, largest_pos and, with bins = B, the spectrum (entry c the classes
of count c, entry 0 those of count >= B).

brute:  a Counter of windows in text coordinates, first positions by scanning t upward, sp from a naive sort of the
        suffixes of s -- the definition itself, for small texts.
hashed: the same classes from np.unique over packed windows of s padded with L zero bytes, the way tests/repeats_ref.py
        finds its classes but with ids that keep the lexicographic order: the padded windows at positions 0 .. m ARE the
        suffixes cut at L bytes, so the sorted groups are the runs of rows and a group's sp is the number of windows in the
        groups before it.  A window that reaches into the padding is a suffix with fewer than L bytes: a group of one, no class."""
from collections import Counter

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

FIELDS = ("records", "selected", "distinct", "windows", "singletons", "largest_count", "largest_sp", "largest_pos")
RECORD = np.dtype([("sp", np.uint64), ("count", np.uint64), ("first_pos", np.uint64)])


def result(classes, min_count, order, top, bins):
    """classes: [(sp, count, first_pos)] of every eligible class, or the three as arrays -> (records, summary)"""
    if isinstance(classes, tuple):
        sp, cnt, pos = (np.asarray(x, dtype=np.int64).reshape(-1) for x in classes)
    else:
        c = np.array(classes, dtype=np.int64).reshape(-1, 3)
        sp, cnt, pos = c[:, 0], c[:, 1], c[:, 2]
    sel = np.nonzero(cnt >= min_count)[0]
    sel = sel[np.argsort(sp[sel])] if order == "row" else sel[np.lexsort((sp[sel], -cnt[sel]))]
    kept = sel[:top] if top else sel
    records = np.zeros(kept.size, dtype=RECORD)
    records["sp"], records["count"], records["first_pos"] = sp[kept], cnt[kept], pos[kept]
    largest = int(cnt.max()) if cnt.size else 0
    lsp = lpos = 0
    if cnt.size:
        big = np.nonzero(cnt == largest)[0]
        at = big[np.argmin(sp[big])]
        lsp, lpos = int(sp[at]), int(pos[at])
    summary = dict(records=int(kept.size), selected=int(sel.size), distinct=int(cnt.size), windows=int(cnt.sum()),
                   singletons=int((cnt == 1).sum()), largest_count=largest, largest_sp=lsp, largest_pos=lpos)
    if bins:
        summary["spectrum"] = np.bincount(np.where(cnt < bins, cnt, 0), minlength=bins).astype(np.uint64)
    return records, summary


def suffix_rows(text):
    """the suffix array of s = reverse(text) + sentinel by a naive sort, and s"""
    s = bytes(text)[::-1] + b"\0"
    return sorted(range(len(s)), key=lambda i: s[i:]), s


def brute(text, L, min_count=2, order="count", top=0, stop=0, bins=0):
    """-> (records, summary dict; "spectrum" with bins)"""
    text = bytes(text)
    m = len(text)
    assert L >= 1 and 0 not in text
    count, first = Counter(), {}
    for t in range(m - L + 1):
        w = text[t:t + L]
        if stop and stop in w:
            continue
        count[w] += 1
        first.setdefault(w, t)
    rows, s = suffix_rows(text)
    sp = {}
    for r, i in enumerate(rows):
        pre = s[i:i + L]
        if len(pre) == L and 0 not in pre:
            sp.setdefault(pre[::-1], r)
    return result([(sp[w], c, first[w]) for w, c in count.items()], min_count, order, top, bins)


def heads(text, L):
    """the runs of rows of s = reverse(text) + sentinel whose suffixes agree in their first L bytes"""
    s = bytes(text)[::-1] + b"\0"
    return len({s[i:i + L] for i in range(len(s))})


class _Chain:
    """ids[c][p] = the lexicographic rank of a[p : p + c] among all windows of c bytes, for c = 1 .. 8 on demand and 16, 32, ..."""

    def __init__(self, a):
        self.a = a
        self.ids = {}

    def _pair(self, c, step):
        """the ranks of the windows of c + step bytes from those of c bytes (step <= c): (first c bytes, last c bytes)"""
        x = self.get(c)
        k = int(x.max()) + 1 if x.size else 1
        rec = sliding_window_view(x, step + 1)[:, [0, step]].astype(np.uint64)
        return np.unique(rec[:, 0] * np.uint64(k) + rec[:, 1], return_inverse=True)[1].reshape(-1)

    def get(self, c):
        if c not in self.ids:
            if c <= 8:
                rec = np.zeros((self.a.size - c + 1, 8), dtype=np.uint8)
                rec[:, :c] = sliding_window_view(self.a, c)
                self.ids[c] = np.unique(rec.view(">u8").reshape(-1), return_inverse=True)[1].reshape(-1)
            else:
                assert c & (c - 1) == 0
                self.ids[c] = self._pair(c // 2, c // 2)
        return self.ids[c]

    def classes(self, L):
        if L <= 8:
            return self.get(L)
        c = 8
        while 2 * c <= L:
            c *= 2
        return self.get(c) if c == L else self._pair(c, L - c)


def hashed(text, L, min_count=2, order="count", top=0, stop=0, bins=0):
    """-> (records, summary), as brute"""
    text = bytes(text)
    m = len(text)
    assert L >= 1
    if L > m:
        return result([], min_count, order, top, bins)
    a = np.frombuffer(text, dtype=np.uint8)
    padded = np.concatenate([a[::-1], np.zeros(L, dtype=np.uint8)])
    ids = _Chain(padded).classes(L)
    assert ids.size == m + 1
    by_row = np.argsort(ids, kind="stable")                   # positions of s by row: equal windows ascending
    cnt = np.bincount(ids)
    sp = np.cumsum(cnt) - cnt
    p_max = by_row[sp + cnt - 1].astype(np.int64)               # the largest position of every group
    window = p_max <= m - L                                     # (a group of a short suffix has that suffix alone)
    first = (m - L) - p_max
    if stop:
        hits = np.concatenate(([0], np.cumsum(a == stop)))
        t = np.clip(first, 0, m - L)
        window &= hits[t + L] == hits[t]
    return result((sp[window], cnt[window], first[window]), min_count, order, top, bins)
