"""Two independent expectations for the approximate search (fmx_search_approx_batch), window_hits and dfs_hits, and walk,
the kernel's own walk restated with the backward steps it makes; none uses the library.

A hit of pattern P with budget e and substitution range [lo, hi] is a string Q of len(P) bytes that differs from P in
d <= e positions, holds a byte of the range at each of them and occurs in the index; it is reported as (sp, ep, d) with
(sp, ep) the interval the exact search gives for Q.  The hits for a budget e are the hits for a larger budget with d <= e."""
import numpy as np

import helpers
import oracle

_indexes = {}        # text -> (oracle searcher, the text as an array, {window content: interval})


def index_of(s):
    """The oracle's searcher over helpers.bwt_of_text(s), made once per text."""
    s = bytes(s)
    if s not in _indexes:
        bwt, eof, counts = helpers.bwt_of_text(s)
        _indexes[s] = (oracle.NaiveFMSearcher.from_mem(bwt, eof, counts), np.frombuffer(s + b"\0", dtype=np.uint8), {})
    return _indexes[s]


def window_hits(s, P, e, lo=1, hi=255):
    """Slides a window of len(P) over the text s, keeps the windows within distance e of P whose differing bytes lie in
    [lo, hi], groups them by content and takes each distinct content's interval from the oracle's exact search.  The
    text is taken as the index holds it: with the sentinel 0 behind it, and cyclic -- the reference's loop steps from
    the row of the whole text to the sentinel's row, so a pattern that holds byte 0 finds the end of the text followed by
    its beginning.  Patterns without byte 0 see the plain text.  -> sorted list of (sp, ep, d)."""
    orc, arr, found = index_of(s)
    P = np.frombuffer(bytes(P), dtype=np.uint8)
    m = P.size
    if m == 0:
        return [(0, orc.n, 0)]
    if m > arr.size:
        return []
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([arr, arr[:m - 1]]), m)
    diff = win != P
    d = diff.sum(axis=1)
    ok = (d <= e) & ~(diff & ((win < lo) | (win > hi))).any(axis=1)
    out = {}
    for i in np.nonzero(ok)[0].tolist():
        w = win[i].tobytes()
        if w in out:
            continue
        if w not in found:
            r = orc.search(w)
            assert r is not None, w
            found[w] = (int(r[0]), int(r[1]))
        out[w] = found[w] + (int(d[i]),)
    return sorted(out.values())


def dfs_hits(orc, P, e, lo=1, hi=255):
    """A recursive walk over the oracle's getPrevRange that tries every symbol of the range at every position with budget
    left (one prev_range_batch call per node: getPrevRange for all of them) and prunes empty intervals; no shortcut for
    intervals of one row.  Rests on cf / occ alone, so it holds for a synthetic BWT that is not the BWT of a text.
    -> sorted list of (sp, ep, d)."""
    P = bytes(P)
    out = []
    syms = np.arange(lo, hi + 1, dtype=np.uint8)

    def walk(i, d, sp, ep):
        if i == 0:
            out.append((int(sp), int(ep), d))
            return
        pc = P[i - 1]
        r = orc.getPrevRange(sp, ep, pc)
        if r is not None:
            walk(i - 1, d, r[0], r[1])
        if d < e:
            a, b = orc.prev_range_batch(np.full(syms.size, sp, dtype=np.uint64), np.full(syms.size, ep, dtype=np.uint64), syms)
            for j in np.nonzero((a < b) & (syms != pc))[0].tolist():
                walk(i - 1, d + 1, int(a[j]), int(b[j]))

    walk(len(P), 0, 0, orc.n)
    return sorted(out)


def occurring(orc, lo=0, hi=255):
    """The symbols of [lo, hi] that occur in the index (occ over all rows; the filler byte of the EOF slot is no occurrence),
    ascending; kept on the searcher."""
    memo = orc.__dict__.setdefault("_approx_occurring", {})
    if (lo, hi) not in memo:
        memo[(lo, hi)] = np.array([c for c in range(lo, hi + 1) if orc.occ(c, orc.n - 1) > 0], dtype=np.uint8)
    return memo[(lo, hi)]


def row_symbol(orc, row):
    """BWT'[row]: the symbol of the row, 0 on the EOF row.  From bwt_read where the searcher has it, else from occ alone:
    the one symbol whose count grows at the row."""
    if hasattr(orc, "bwt_read"):
        return int(orc.bwt_read(row))
    for c in occurring(orc, 1, 255).tolist():
        if orc.occ(c, row) != orc.occ(c, row - 1):
            return c
    return 0


def walk(orc, P, e, lo=1, hi=255):
    """The walk of fmx_approx.hip as DESIGN.md 15 describes it, restated over the oracle, with the backward steps it makes.
    The candidates are the symbols of [lo, hi] that occur in the index.  A node (i bytes left, d mismatches, sp, ep):
      * with d < e and more than one row: one step per candidate c != P[i - 1], every non-empty one a child with d + 1;
        then the match step with P[i - 1];
      * with d < e and exactly one row (the one-row rule): it tries BWT'[sp] alone, and only if that differs from P[i - 1]
        and is a candidate -- one step, and no match child; otherwise it makes the match step;
      * with d == e (an exact tail, or e = 0): the match step only, until the interval is empty or the pattern is through.
    Every step counts, the one that empties an interval included.  -> (sorted list of (sp, ep, d), steps)."""
    P = bytes(P)
    cand = occurring(orc, lo, hi)
    is_cand = set(cand.tolist())
    hits = []
    steps = 0

    def node(i, d, sp, ep):
        nonlocal steps
        while i > 0:                                         # the match child is the continuation of the loop
            pc = P[i - 1]
            if d < e:
                if ep - sp == 1:
                    b = row_symbol(orc, sp)
                    if b != pc and b in is_cand:
                        steps += 1
                        r = orc.getPrevRange(sp, ep, b)
                        if r is not None:
                            node(i - 1, d + 1, int(r[0]), int(r[1]))
                        return
                else:
                    cs = cand[cand != pc]
                    if cs.size:
                        a, b = orc.prev_range_batch(np.full(cs.size, sp, dtype=np.uint64), np.full(cs.size, ep, dtype=np.uint64), cs)
                        steps += int(cs.size)
                        for j in np.nonzero(a < b)[0].tolist():
                            node(i - 1, d + 1, int(a[j]), int(b[j]))
            steps += 1
            r = orc.getPrevRange(sp, ep, pc)
            if r is None:
                return
            sp, ep = int(r[0]), int(r[1])
            i -= 1
        hits.append((sp, ep, d))

    node(len(P), 0, 0, orc.n)
    return sorted(hits), steps


def within(hits, e):
    """The hits of a smaller budget among those of a larger one."""
    return [h for h in hits if h[2] <= e]


def expected_csr(per_pattern):
    """What the library returns for per-pattern lists of (sp, ep, d): (off, rows) with rows = (pattern, d, sp, ep), each
    pattern's by ascending sp."""
    off, rows = [0], []
    for q, hits in enumerate(per_pattern):
        rows += [(q, d, sp, ep) for sp, ep, d in sorted(hits)]
        off.append(len(rows))
    return off, rows
