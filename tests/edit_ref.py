"""Three expectations for the edit-distance search (fmx_search_edit_batch); none uses the library.

A hit of pattern P (m bytes) with budget e and symbol range A = [lo, hi] is a byte string Q with d = d_A(Q, P) <= e whose
exact search ends non-empty.  d_A is the cheapest alignment of Q with P: equal bytes cost 0; a Q byte of A standing for a
different P byte, or for nothing, costs 1; a P byte standing for nothing costs 1; a Q byte outside A may only stand for an
equal P byte.  Every function here reports a pattern's hits as a sorted list of (sp, len, ep, d): the library's order.

brute_hits : the distinct substrings of the plain text with the full DP table, intervals from the oracle's exact search.
dfs_hits   : the walk over getPrevRange with all 256 symbols and the full row at every node, depth by depth.
walk       : the walk of fmx_edit.hip restated -- the band, the tried sets, the one-row rule -- with the steps it makes."""
import numpy as np

import approx_ref

INF = 1 << 20


def d_a(Q, P, lo=1, hi=255):
    """d_A(Q, P) by the full table."""
    Q, P = bytes(Q), bytes(P)
    row = list(range(len(P) + 1))
    for q in Q:
        in_a = lo <= q <= hi
        new = [row[0] + 1 if in_a else INF]
        for j in range(1, len(P) + 1):
            sub = row[j - 1] + (0 if q == P[j - 1] else 1 if in_a else INF)
            ins = row[j] + 1 if in_a else INF
            new.append(min(sub, ins, new[j - 1] + 1, INF))
        row = new
    return row[len(P)]


def brute_strings(s, P, e, lo=1, hi=255):
    """{Q: d_A(Q, P)} over the distinct substrings Q of s of len(P) - e .. len(P) + e bytes with d_A(Q, P) <= e."""
    s, P = bytes(s), bytes(P)
    m = len(P)
    out = {}
    for ln in range(max(0, m - e), m + e + 1):
        for Q in {s[i:i + ln] for i in range(len(s) - ln + 1)}:
            d = d_a(Q, P, lo, hi)
            if d <= e:
                out[Q] = d
    return out


def brute_hits(s, P, e, lo=1, hi=255):
    """brute_strings over the plain text s, each string with the interval the oracle's exact search gives it."""
    orc = approx_ref.index_of(s)[0]
    out = []
    for Q, d in brute_strings(s, P, e, lo, hi).items():
        sp, ep = orc.search(Q) if Q else (0, orc.n)
        out.append((int(sp), len(Q), int(ep), d))
    return sorted(out)


def dfs_hits(orc, P, e, lo=1, hi=255):
    """The walk without shortcuts: every node tries all 256 symbols (getPrevRange for each, one prev_range_batch call per
    depth for all nodes of that depth), keeps the full row R[0 .. m] against the reversed pattern, and is pruned only when
    its whole row exceeds e.  No one-row rule, no band, no candidate list."""
    P = np.frombuffer(bytes(P), dtype=np.uint8)
    m = P.size
    rev = P[::-1].astype(np.int64)                           # rev[j - 1] = P_j, the j-th byte from the end
    idx = np.arange(m + 1, dtype=np.int64)
    cost = np.where((np.arange(256) >= lo) & (np.arange(256) <= hi), 1, INF).astype(np.int64)
    out = []
    sp, ep, R, t = np.array([0], dtype=np.uint64), np.array([orc.n], dtype=np.uint64), idx[None, :].copy(), 0
    while sp.size:
        for i in np.nonzero(R[:, m] <= e)[0].tolist():
            out.append((int(sp[i]), t, int(ep[i]), int(R[i, m])))
        a, b = orc.prev_range_batch(np.repeat(sp, 256), np.repeat(ep, 256), np.tile(np.arange(256, dtype=np.uint8), sp.size))
        kid = np.nonzero(a < b)[0]
        par, c = kid // 256, kid % 256
        x = np.empty((kid.size, m + 1), dtype=np.int64)
        x[:, 0] = R[par, 0] + cost[c]
        x[:, 1:] = np.minimum(R[par, :-1] + np.where(rev[None, :] == c[:, None], 0, cost[c][:, None]), R[par, 1:] + cost[c][:, None])
        x = np.minimum(np.minimum.accumulate(x - idx, axis=1) + idx, INF)        # the deletions: R'[j] <= R'[j - 1] + 1
        keep = x.min(axis=1) <= e
        sp, ep, R, t = a[kid][keep], b[kid][keep], x[keep], t + 1
    return sorted(out)


def walk(orc, P, e, lo=1, hi=255):
    """The walk of fmx_edit.hip.  A node is (t, sp, ep, band): band[b] = min(R[t - e + b], e + 1) for b = 0 .. 2 e, e + 1
    where t - e + b lies outside 0 .. m.  At a node:
      1. R[m] <= e: a hit (sp, t, ep, R[m]).
      2. M = the P_j with R[j - 1] <= e, by ascending j, each once.
           min R == e                  : the tried symbols are M;
           min R <  e, several rows    : the candidates (the symbols of A that occur, ascending), then M's others;
           min R <  e, one row         : BWT'[sp] (0 on the EOF row) if it is a candidate or in M, else none.
      3. One backward step per tried symbol, the steps that come back empty included; every non-empty child is a node.
    -> (sorted hits, steps)."""
    P = bytes(P)
    m = len(P)
    cand = approx_ref.occurring(orc, lo, hi).tolist()
    is_cand = set(cand)
    dead = e + 1
    hits = []
    steps = 0

    def child_band(t, band, c):
        in_a = lo <= c <= hi
        new = []
        for b in range(2 * e + 1):
            j = t + 1 - e + b
            v = dead
            if 0 <= j <= m:
                if in_a and b + 1 <= 2 * e:
                    v = min(v, band[b + 1] + 1)                          # R[j] + ins
                if j >= 1:
                    if c == P[m - j]:
                        v = min(v, band[b])                              # R[j - 1], equal bytes
                    elif in_a:
                        v = min(v, band[b] + 1)                          # R[j - 1] + sub
                    if b >= 1:
                        v = min(v, new[b - 1] + 1)                       # R'[j - 1] + 1
            new.append(v)
        return new

    def node(t, sp, ep, band):
        nonlocal steps
        jm = m - t + e                                                   # the band slot of R[m]
        if 0 <= jm <= 2 * e and band[jm] <= e:
            hits.append((sp, t, ep, band[jm]))
        M = []
        for b in range(2 * e + 1):
            j = t - e + b + 1                                            # band[b] = R[j - 1]
            if band[b] <= e and 1 <= j <= m and P[m - j] not in M:
                M.append(P[m - j])
        if min(band) == e:
            tried = M
        elif ep - sp == 1:
            c = approx_ref.row_symbol(orc, sp)
            tried = [c] if c in is_cand or c in M else []
        else:
            tried = cand + [c for c in M if c not in is_cand]
        if not tried:
            return
        cs = np.array(tried, dtype=np.uint8)
        a, b = orc.prev_range_batch(np.full(cs.size, sp, dtype=np.uint64), np.full(cs.size, ep, dtype=np.uint64), cs)
        steps += len(tried)
        for i in np.nonzero(a < b)[0].tolist():
            node(t + 1, int(a[i]), int(b[i]), child_band(t, band, tried[i]))

    node(0, 0, orc.n, [min(t_j, dead) if t_j >= 0 else dead for t_j in range(-e, e + 1)])
    return sorted(hits), steps


def within(hits, e):
    """The hits of a smaller budget among those of a larger one (same range)."""
    return [h for h in hits if h[3] <= e]


def expected_csr(per_pattern):
    """What the library returns for per-pattern lists of (sp, len, ep, d): (off, rows), rows = (pattern, d, len, sp, ep),
    a pattern's by ascending (sp, len)."""
    off, rows = [0], []
    for q, hits in enumerate(per_pattern):
        rows += [(q, d, ln, sp, ep) for sp, ln, ep, d in sorted(hits)]
        off.append(len(rows))
    return off, rows
