"""Reference for the append of new text to an index (include/fmx.h, "append"), written from the definitions:
no kernel's code is restated here, and nothing is shared with the library but the constants' meaning.

A is the indexed text (a bytes), s_A = reverse(A) + sentinel with n_A = a + 1 rows; B the new text (b bytes, no 0 byte),
R = reverse(B); s_T = R . s_A.  X_j = R[j..] . s_A are the b new suffixes.

    bwt_direct(text)     the (bwt, eof, counts) fmx_bwt_from_text gives, by a direct suffix sort
    merge_ref(A, B, ..)  the same for A + B from the index of A alone and B: gap ranks by segments with warm-up and fix-up
                         runs, the order of the new suffixes from a piece with its LCP check and context retry, the emit.
"""
import numpy as np


def _bytes(x):
    return bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else np.asarray(x, dtype=np.uint8).tobytes()


def suffix_array(s):
    """SA of the byte string s whose last byte is a unique smallest sentinel: prefix doubling in numpy."""
    a = np.frombuffer(s, dtype=np.uint8).astype(np.int64)
    n = a.size
    rank = a.copy()
    k = 1
    while True:
        second = np.full(n, -1, dtype=np.int64)
        if k < n:
            second[: n - k] = rank[k:]
        order = np.lexsort((second, rank))
        key = np.stack([rank[order], second[order]], axis=1)
        diff = np.any(key[1:] != key[:-1], axis=1)
        new = np.zeros(n, dtype=np.int64)
        new[order] = np.concatenate([[0], np.cumsum(diff)])
        rank = new
        if rank.max() == n - 1:
            return order
        k *= 2


def naive_suffix_array(s):
    return np.array(sorted(range(len(s)), key=lambda i: s[i:]), dtype=np.int64)


def bwt_of(s, sa):
    """bwt[i] = the byte before suffix sa[i]; the eof row (sa == 0) is filled with the byte of the row above, of the row
    below when it is row 0 (sa2BWT, bwtmerger.scala:799-806)."""
    n = len(s)
    a = np.frombuffer(s, dtype=np.uint8)
    bwt = a[(sa - 1) % n].copy()
    eof = int(np.nonzero(sa == 0)[0][0])
    if n > 1:
        bwt[eof] = bwt[eof - 1] if eof else bwt[1]
    return bwt, eof


def bwt_direct(text, sort=suffix_array):
    t = _bytes(text)
    s = t[::-1] + b"\0"
    bwt, eof = bwt_of(s, sort(s))
    counts = np.bincount(np.frombuffer(t, dtype=np.uint8), minlength=256).astype(np.int64)
    return bwt, eof, counts


def lcp_below(s, sa):
    """LCP[r] = lcp of the suffixes of rows r and r + 1, LCP[n - 1] = 0 (Kasai over the successor)."""
    n = len(s)
    inv = np.empty(n, dtype=np.int64)
    inv[sa] = np.arange(n)
    lcp = np.zeros(n, dtype=np.int64)
    h = 0
    for i in range(n):
        r = inv[i]
        if r + 1 < n:
            j = int(sa[r + 1])
            while i + h < n and j + h < n and s[i + h] == s[j + h]:
                h += 1
            lcp[r] = h
            h = max(h - 1, 0)
        else:
            h = 0
    return lcp


class RankA:
    """C[] and occ of A's index from (bwt, eof, counts) alone: BWT' holds the sentinel symbol 0 at the eof slot."""

    def __init__(self, bwt, eof, counts):
        b = np.asarray(bwt, dtype=np.uint8).astype(np.int64)
        b[eof] = 0
        self.n, self.eof = b.size, int(eof)
        self.C = np.zeros(257, dtype=np.int64)
        c = np.asarray(counts, dtype=np.int64).copy()
        c[0] = 1
        self.C[1:] = np.cumsum(c)
        self.pre = {}
        self.bp = b

    def rank(self, c, x):
        """#{p < x : BWT'[p] == c}"""
        if c not in self.pre:
            self.pre[c] = np.concatenate([[0], np.cumsum(self.bp == c)])
        return int(self.pre[c][x])

    def step(self, c, x):
        return int(self.C[c]) + self.rank(c, x)

    def tail_reversed(self, m):
        """s_A[0 .. m): the first bytes of the rows eof, Psi eof, .. -- from the index alone."""
        out = bytearray()
        row = self.eof
        for _ in range(m):
            c = int(np.searchsorted(self.C, row, side="right")) - 1       # the symbol whose bucket holds the row
            out.append(c)
            j = row - int(self.C[c])                                       # Psi: the j-th occurrence of c in BWT'
            row = int(np.nonzero(self.bp == c)[0][j])
        return bytes(out)


def gap_ranks(ra, B, segment, warmup):
    """r_j for j = 0 .. b - 1 as the segments, their warm-up and the fix-up runs compute them, and what the fix-up does."""
    R = _bytes(B)[::-1]
    b = len(R)
    S, W = int(segment), int(warmup)
    rank = [None] * b
    walk_steps = 0
    for lo in range(0, b, S):
        hi = min(lo + S, b)
        start = min(hi + W, b)
        sp, ep = (ra.eof, ra.eof) if start == b else (0, ra.n)
        for j in range(start - 1, lo - 1, -1):
            c = R[j]
            sp, ep = ra.step(c, sp), ra.step(c, ep)
            walk_steps += 1
            if j < hi and sp == ep:
                rank[j] = sp
    unresolved = [r is None for r in rank]
    for lo in range(0, b, S):              # the unresolved positions of a segment are its right end
        hi = min(lo + S, b)
        seg = unresolved[lo:hi]
        assert seg == sorted(seg)
    runs, j = [], b - 1
    while j >= 0:                          # maximal runs, each walked from the exact rank to its right
        if not unresolved[j]:
            j -= 1
            continue
        assert j + 1 < b and rank[j + 1] is not None
        r, length = rank[j + 1], 0
        while j >= 0 and unresolved[j]:
            r = ra.step(R[j], r)
            rank[j] = r
            length += 1
            j -= 1
        runs.append(length)
    return rank, {"walk_steps": walk_steps, "fixup_steps": sum(runs), "longest_run": max(runs) if runs else 0, "runs": len(runs)}


def new_order(ra, B, context, max_context=None):
    """The new suffixes' positions j in their order among themselves, from the piece tail(A, M) + B; (order, M, rounds).
    ValueError when the context would have to pass max_context."""
    Bb = _bytes(B)
    b, a = len(Bb), ra.n - 1
    rounds = 0
    while True:
        M = min(a, context)
        s = Bb[::-1] + ra.tail_reversed(M) + b"\0"            # R . s_A[0 .. M) . sentinel
        sa = suffix_array(s)
        rounds += 1
        rows = np.nonzero(sa < b)[0]
        if M == a:
            return sa[rows], M, rounds
        lcp = lcp_below(s, sa)
        above = np.where(rows > 0, lcp[rows - 1], 0)
        if np.all(sa[rows] + np.maximum(above, lcp[rows]) < b + M):
            return sa[rows], M, rounds
        context = max(1, 2 * context)
        if max_context is not None and context > max_context:
            raise ValueError("context %d needed, max_context %d" % (context, max_context))


def merge_ref(A, B, segment=256, warmup=32, context=4096, max_context=None, index=None):
    """-> dict: bwt, eof, counts of A + B; rows (output row of every new suffix, in their order), ranks (r_j by j) and the
    statistics fmx_merge_last reports.  `index` = (bwt, eof, counts) of A when A itself is not at hand."""
    Bb = _bytes(B)
    bwt_a, eof_a, counts_a = index if index is not None else bwt_direct(A)
    ra = RankA(bwt_a, eof_a, counts_a)
    b = len(Bb)
    R = Bb[::-1]
    rank, stats = gap_ranks(ra, Bb, segment, warmup)
    order, M, rounds = new_order(ra, Bb, context, max_context)
    rows = np.array([rank[int(j)] + q for q, j in enumerate(order)], dtype=np.int64)
    assert np.all(np.diff(rows) > 0)
    n_t = ra.n + b
    out = np.zeros(n_t, dtype=np.uint8)
    is_new = np.zeros(n_t, dtype=bool)
    is_new[rows] = True
    old = np.asarray(bwt_a, dtype=np.uint8).copy()
    old[eof_a] = R[b - 1]                                      # A's eof row now stands before R's last byte
    out[~is_new] = old
    eof = None
    for q, j in enumerate(order):
        if j == 0:
            eof = int(rows[q])
        else:
            out[rows[q]] = R[int(j) - 1]
    out[eof] = out[eof - 1] if eof else out[1]
    counts = np.asarray(counts_a, dtype=np.int64) + np.bincount(np.frombuffer(Bb, dtype=np.uint8), minlength=256)
    res = {"bwt": out, "eof": eof, "counts": counts, "rows": rows, "ranks": np.array(rank, dtype=np.int64), "context": M,
           "rounds": rounds}
    res.update(stats)
    return res
