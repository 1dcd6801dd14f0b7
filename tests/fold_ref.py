"""Three independent expectations for the search under a fold map (fmx_search_fold_batch): window_hits and
dfs_hits, and walk, the kernel's own walk restated with the backward steps it makes and the stack it needs; none uses the
library.

A fold map sends a byte to the representative of its class.  A hit of pattern P is a string Q of len(P) bytes with
fold[Q[j]] == fold[P[j]] at every j that occurs in the index; it is reported as (sp, ep), the interval the exact search gives
for Q.  Patterns are given as the exact search takes them: matched last byte first."""
import numpy as np

import approx_ref

IDENTITY = bytes(range(256))
ASCII = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def make_map(classes):
    """A fold map from lists of members; the representative is the smallest member."""
    fold = bytearray(range(256))
    for members in classes:
        members = sorted(bytes(members))
        for c in members:
            fold[c] = members[0]
    return bytes(fold)


def mixed_case(s, seed=7, p=0.3):
    """s with each lower-case letter upper-cased with probability p (numpy.random.RandomState(seed))."""
    a = np.frombuffer(bytes(s), dtype=np.uint8).copy()
    up = np.random.RandomState(seed).random_sample(a.size) < p
    a[up & (a >= 97) & (a <= 122)] -= 32
    return a.tobytes()


def window_hits(s, P, fold):
    """Slides a window of len(P) over the text s, keeps the windows that equal P under the map, groups them by content and
    takes each distinct content's interval from the oracle's exact search.  The text is taken as the index holds it: with
    the sentinel 0 behind it, and cyclic (approx_ref.window_hits says why); byte 0 is alone in its class, so a pattern without
    it sees the plain text.  -> sorted list of (sp, ep)."""
    orc, arr, found = approx_ref.index_of(s)
    f = np.frombuffer(bytes(fold), dtype=np.uint8)
    P = np.frombuffer(bytes(P), dtype=np.uint8)
    m = P.size
    if m == 0:
        return [(0, orc.n)]
    if m > arr.size:
        return []
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([arr, arr[:m - 1]]), m)
    ok = (f[win] == f[P]).all(axis=1)
    out = {}
    for i in np.nonzero(ok)[0].tolist():
        w = win[i].tobytes()
        if w in out:
            continue
        if w not in found:
            r = orc.search(w)
            assert r is not None, w
            found[w] = (int(r[0]), int(r[1]))
        out[w] = found[w]
    return sorted(out.values())


def _step(orc, sp, ep, c):
    """getPrevRange by symbol c for arrays of intervals (one prev_range_batch call); an empty one has sp >= ep."""
    a, b = orc.prev_range_batch(sp, ep, np.full(sp.size, c, dtype=np.uint8))
    return np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)


def dfs_hits(orc, P, fold):
    """A walk over the oracle's getPrevRange that tries EVERY member of the class of P[i - 1] at every position, present in
    the index or not, and prunes empty intervals; no shortcut for intervals of one row and none for singleton classes.  The
    tree is expanded a level at a time (one prev_range_batch call per level and member), so that 2^16 spellings of one
    pattern cost 32 calls.  Rests on cf / occ alone, so it holds for a synthetic BWT.  -> sorted list of (sp, ep)."""
    P = bytes(P)
    fold = bytes(fold)
    members = {}
    for c in range(256):
        members.setdefault(fold[c], []).append(c)
    sp, ep = np.array([0], dtype=np.uint64), np.array([orc.n], dtype=np.uint64)
    for i in range(len(P), 0, -1):
        parts = []
        for c in members[fold[P[i - 1]]]:
            a, b = _step(orc, sp, ep, c)
            parts.append((a[a < b], b[a < b]))
        sp, ep = np.concatenate([x for x, _ in parts]), np.concatenate([y for _, y in parts])
        if not sp.size:
            return []
    return sorted(zip(sp.tolist(), ep.tolist()))


def walk(orc, P, fold, lead=0):
    """The walk of fmx_fold.hip as DESIGN.md 28 describes it, restated over the oracle.  A node (i bytes left, sp, ep):
      * P[i - 1]'s class is a singleton in the map, or the step is one of the first `lead` (exact whatever the map says):
        the one step with P[i - 1], as the exact search makes it;
      * otherwise, with exactly one row (the one-row rule): BWT'[sp] (0 on the EOF row) -- in the class, the one step with
        it; else the node dies without a step;
      * otherwise one step per member of the class that occurs in the index, none for an absent member; the walk goes on
        with the non-empty child of the smallest symbol and pushes the others.
    At i == 0 the node is a hit and the next entry is popped (the last pushed first).  Every step made counts, the ones that
    come back empty included.  The steps and the hits do not depend on the order in which nodes are visited, so the tree is
    expanded a level at a time (prev_range_batch) with every node's children kept in symbol order; the stack is then played
    through on that tree.  -> (sorted list of (sp, ep), steps, the largest number of entries on the stack)."""
    P = bytes(P)
    fold = bytes(fold)
    m = len(P)
    occurring = approx_ref.occurring(orc, 1, 255).tolist()
    size = [0] * 256
    for c in range(256):
        size[fold[c]] += 1
    folded = np.frombuffer(fold, dtype=np.uint8)
    children = [[]]                                          # node -> its non-empty children, ascending symbol
    ids = np.array([0], dtype=np.int64)
    sp, ep = np.array([0], dtype=np.uint64), np.array([orc.n], dtype=np.uint64)
    steps = 0
    for i in range(m, 0, -1):
        pc = P[i - 1]
        rep = fold[pc]
        kids = []                                            # (parents, sp, ep) per symbol tried, ascending
        if size[rep] <= 1 or i + lead > m:
            steps += sp.size
            kids.append((ids,) + _step(orc, sp, ep, pc))
        else:
            one = ep - sp == 1
            if one.any():                                    # the row's symbol: the one whose step is not empty, 0 on the EOF row
                s1, e1 = sp[one], ep[one]
                sym = np.zeros(s1.size, dtype=np.uint8)
                ra, rb = np.zeros_like(s1), np.zeros_like(s1)
                for c in occurring:
                    a, b = _step(orc, s1, e1, c)
                    sym[a < b], ra[a < b], rb[a < b] = c, a[a < b], b[a < b]
                take = folded[sym] == rep
                steps += int(take.sum())
                kids.append((ids[one][take], ra[take], rb[take]))
            if not one.all():
                s2, e2 = sp[~one], ep[~one]
                for c in occurring:
                    if fold[c] == rep:
                        steps += s2.size
                        kids.append((ids[~one],) + _step(orc, s2, e2, c))
        nsp, nep = [], []
        first = len(children)
        for parents, a, b in kids:
            ok = a < b
            for p, x, y in zip(parents[ok].tolist(), a[ok].tolist(), b[ok].tolist()):
                children[p].append(len(children))
                children.append([])
                nsp.append(x)
                nep.append(y)
        sp, ep = np.array(nsp, dtype=np.uint64), np.array(nep, dtype=np.uint64)
        ids = np.arange(first, len(children), dtype=np.int64)
        if not sp.size:
            break
    hits = sorted(zip(sp.tolist(), ep.tolist()))             # (an empty frontier: the pattern does not occur in any spelling)
    stack, depth, v = [], 0, 0
    while True:
        if children[v]:
            stack.extend(children[v][1:])
            depth = max(depth, len(stack))
            v = children[v][0]
        elif stack:
            v = stack.pop()
        else:
            break
    return hits, steps, depth


def expected_csr(pats, per_pattern):
    """What the library returns for per-pattern lists of (sp, ep): (off, rows) with rows = (pattern, len, sp, ep), each
    pattern's by ascending sp."""
    off, rows = [0], []
    for q, (p, hits) in enumerate(zip(pats, per_pattern)):
        rows += [(q, len(p), sp, ep) for sp, ep in sorted(hits)]
        off.append(len(rows))
    return off, rows
