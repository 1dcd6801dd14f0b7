"""The yardsticks of the repeats feature (fmx.h: repeats), written from the definition in TEXT coordinates: no suffix array,
no LCP array, no reversed text.

A window is text[t : t + L]; with a stop byte a window that holds it does not count.  A class is the set of the windows with
the same bytes; it is repeated when it has two windows or more.  Mode ALL flags every window of a repeated class, mode LATER
every one but the first.  The result is the union of [t, t + L) over the flagged windows as maximal ranges, and the summary
(ranges, covered_bytes, classes, windows, largest_class, largest_class_pos).

brute:  a dictionary of windows, pure Python -- the definition itself, for small texts.
hashed: the same classes from np.unique over sliding_window_view records, for texts around 2^20 bytes.  The records are the
        windows themselves up to 8 bytes (one u64 each); a longer window is the pair (class of its first c bytes, class of its
        last c bytes), c doubling -- two windows are equal iff both halves are, so the classes are exact, not hashes that may
        collide.  The doubling chain depends on the text alone and is kept per text."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

FIELDS = ("ranges", "covered_bytes", "classes", "windows", "largest_class", "largest_class_pos")


def _summary(ranges, classes, windows, largest, pos):
    covered = sum(b - a for a, b in ranges)
    return dict(ranges=len(ranges), covered_bytes=covered, classes=classes, windows=windows, largest_class=largest,
                largest_class_pos=pos)


def brute(text, L, later=False, stop=0):
    """-> (ranges uint64[r, 2], summary dict)"""
    text = bytes(text)
    m = len(text)
    assert L >= 1
    groups = {}
    for t in range(m - L + 1):
        w = text[t:t + L]
        if stop and stop in w:
            continue
        groups.setdefault(w, []).append(t)
    covered = [False] * m
    classes = windows = largest = pos = 0
    for ts in groups.values():                     # (each list ascending: ts[0] is the first copy)
        if len(ts) < 2:
            continue
        classes += 1
        if len(ts) > largest or (len(ts) == largest and ts[0] < pos):
            largest, pos = len(ts), ts[0]
        for t in (ts[1:] if later else ts):
            windows += 1
            for j in range(t, t + L):
                covered[j] = True
    ranges, t = [], 0
    while t < m:
        if covered[t]:
            a = t
            while t < m and covered[t]:
                t += 1
            ranges.append((a, t))
        else:
            t += 1
    return np.array(ranges, dtype=np.uint64).reshape(-1, 2), _summary(ranges, classes, windows, largest, pos)


class _Chain:
    """ids[c][t] = the class of text[t : t + c] among all windows of c bytes, for c = 1 .. 8 on demand and 16, 32, ..."""

    def __init__(self, text):
        self.a = np.frombuffer(bytes(text), dtype=np.uint8)
        self.ids = {}
        self.groups = {}

    def _pair(self, c, step):
        """the classes of the windows of c + step bytes from those of c bytes (step <= c)"""
        x = self.get(c)
        k = int(x.max()) + 1 if x.size else 1
        rec = sliding_window_view(x, step + 1)[:, [0, step]].astype(np.uint64)
        return np.unique(rec[:, 0] * np.uint64(k) + rec[:, 1], return_inverse=True)[1].reshape(-1)

    def get(self, c):
        if c not in self.ids:
            if c <= 8:
                rec = np.zeros((self.a.size - c + 1, 8), dtype=np.uint8)
                rec[:, :c] = sliding_window_view(self.a, c)
                self.ids[c] = np.unique(rec.view(np.uint64).reshape(-1), return_inverse=True)[1].reshape(-1)
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


_chains = {}


def hashed(text, L, later=False, stop=0):
    """-> (ranges uint64[r, 2], summary dict), as brute"""
    text = bytes(text)
    m = len(text)
    assert L >= 1
    empty = np.zeros((0, 2), dtype=np.uint64)
    if L > m:
        return empty, _summary([], 0, 0, 0, 0)
    key = (len(text), hash(text))
    if key not in _chains:
        _chains.clear()                            # (one text at a time: the chain of a 2^20-byte text is tens of megabytes)
        _chains[key] = _Chain(text)
    chain = _chains[key]
    if (L, stop) not in chain.groups:              # (both modes share the classes of one threshold and stop byte)
        ids = chain.classes(L)
        t = np.arange(m - L + 1, dtype=np.int64)
        if stop:
            hits = np.concatenate(([0], np.cumsum(chain.a == stop)))
            ok = hits[t + L] == hits[t]            # no stop byte in [t, t + L)
            ids, t = ids[ok], t[ok]
        _, idx, inv, cnt = np.unique(ids, return_index=True, return_inverse=True, return_counts=True)
        chain.groups = {(L, stop): (t, t[idx] if t.size else t, inv.reshape(-1), cnt)}      # (t ascends: idx names the first copy)
    t, first, inv, cnt = chain.groups[(L, stop)]
    if t.size == 0:
        return empty, _summary([], 0, 0, 0, 0)
    rep = cnt >= 2
    if not rep.any():
        return empty, _summary([], 0, 0, 0, 0)
    flagged = rep[inv] & ((t != first[inv]) if later else True)
    starts = t[flagged]
    delta = np.bincount(starts, minlength=m + 1) - np.bincount(starts + L, minlength=m + 1)
    cov = np.cumsum(delta[:m]) > 0
    edge = np.diff(np.concatenate(([0], cov.astype(np.int8), [0])))
    ranges = np.stack([np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]], axis=1).astype(np.uint64)
    largest = int(cnt[rep].max())
    pos = int(first[rep & (cnt == largest)].min())
    return ranges, dict(ranges=int(ranges.shape[0]), covered_bytes=int(cov.sum()), classes=int(rep.sum()),
                        windows=int(starts.size), largest_class=largest, largest_class_pos=pos)
