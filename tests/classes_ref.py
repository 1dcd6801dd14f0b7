"""Three independent expectations for the search under string classes (fmx_search_classes_batch): window_hits,
dfs_hits, and walk, the kernel's own walk restated with the backward steps it makes and the stack it needs; none uses the
library.

A TABLE is a list of classes, a class a list of members, a member a bytes object of 1 .. 4 bytes.  A pattern is a list of
ELEMENTS: an int < 256 is that byte, an int >= 256 class (element - 256).  Both are given as the exact search takes a pattern:
strings of the indexed text s, matched last element first and a member's bytes last first.  A hit is a string Q = m_1 .. m_e
(m_j the j-th literal or a member of the j-th class) that occurs; it is reported as (len(Q), sp, ep) with the interval the exact
search gives for Q."""
import numpy as np

import approx_ref


def abi(table):
    """(cls_off, mem_off, mem_bytes) of a table, as fmx_class_table takes them."""
    cls_off, mem_off, data = [0], [0], bytearray()
    for members in table:
        for m in members:
            data += bytes(m)
            mem_off.append(len(data))
        cls_off.append(len(mem_off) - 1)
    return (np.array(cls_off, dtype=np.uint64), np.array(mem_off, dtype=np.uint64), np.frombuffer(bytes(data), dtype=np.uint8))


def pack(patterns):
    """(el, off): the uint16 elements of the patterns one behind the other, and their k + 1 offsets."""
    off = np.zeros(len(patterns) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in patterns])
    return np.array([e for p in patterns for e in p], dtype=np.uint16), off


def unpack(el, off):
    """The patterns of pack()'s arrays, as lists of ints."""
    el, off = np.asarray(el).tolist(), np.asarray(off).tolist()
    return [el[a:b] for a, b in zip(off[:-1], off[1:])]


def table_of(cls_off, mem_off, mem_bytes):
    """The table of abi()'s arrays."""
    data = np.asarray(mem_bytes, dtype=np.uint8).tobytes()
    cls_off, mem_off = np.asarray(cls_off).tolist(), np.asarray(mem_off).tolist()
    return [[data[mem_off[j]:mem_off[j + 1]] for j in range(a, b)] for a, b in zip(cls_off[:-1], cls_off[1:])]


def literals(b):
    """A byte string as a pattern of literal elements."""
    return list(bytes(b))


def fold_table(fold):
    """A fold map (256 bytes) as a table: every class of two or more, its single-byte members ascending.
    -> (table, class id of every byte or None)."""
    groups = {}
    for c in range(256):
        groups.setdefault(fold[c], []).append(c)
    table, cid = [], [None] * 256
    for members in groups.values():
        if len(members) >= 2:
            for c in members:
                cid[c] = len(table)
            table.append([bytes([c]) for c in members])
    return table, cid


def folded(P, cid):
    """The byte pattern P under a fold map as elements: a byte with a class is that class."""
    return [c if cid[c] is None else 256 + cid[c] for c in bytes(P)]


def window_hits(s, elements, table):
    """Tries the element sequence at every start of the text s -- as the index holds it: with the sentinel 0 behind it, and
    cyclic (approx_ref.window_hits says why) -- an element after the other, a class by whichever member stands there (no member
    is a prefix of another, so at most one does); groups the matched strings by content and takes each distinct one's interval
    from the oracle's exact search.  -> sorted list of (len, sp, ep)."""
    orc, arr, found = approx_ref.index_of(s)
    if not elements:
        return [(0, 0, orc.n)]
    full = arr.tobytes()
    t = full + full[:4 * len(elements)]
    out = {}
    for p in range(len(full)):
        at = p
        for e in elements:
            if e < 256:
                if t[at] != e:
                    break
                at += 1
            else:
                for m in table[e - 256]:
                    if t.startswith(m, at):
                        at += len(m)
                        break
                else:
                    break
        else:
            if at - p > len(full):
                continue
            w = t[p:at]
            if w not in out:
                if w not in found:
                    r = orc.search(w)
                    assert r is not None, w
                    found[w] = (int(r[0]), int(r[1]))
                out[w] = (len(w),) + found[w]
    return sorted(out.values())


def _step(orc, sp, ep, c):
    a, b = orc.prev_range_batch(sp, ep, np.full(sp.size, c, dtype=np.uint8))
    return np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)


def dfs_hits(orc, elements, table):
    """A walk over the oracle's getPrevRange that tries EVERY member of the class at every class element, byte after byte from
    the member's last, and prunes empty intervals; no shortcut for intervals of one row and none for classes of one.  The tree
    is expanded an element at a time (one prev_range_batch call per member byte).  Rests on cf / occ alone, so it holds for a
    synthetic BWT.  -> sorted list of (len, sp, ep)."""
    sp, ep = np.array([0], dtype=np.uint64), np.array([orc.n], dtype=np.uint64)
    ln = np.array([0], dtype=np.int64)
    for e in reversed(list(elements)):
        parts = []
        for m in ([bytes([e])] if e < 256 else table[e - 256]):
            a, b, l = sp, ep, ln
            for c in reversed(bytes(m)):
                a, b = _step(orc, a, b, c)
                ok = a < b
                a, b, l = a[ok], b[ok], l[ok]
            parts.append((a, b, l + len(m)))
        sp, ep, ln = (np.concatenate([p[j] for p in parts]) for j in range(3))
        if not sp.size:
            return []
    return sorted(zip(ln.tolist(), sp.tolist(), ep.tolist()))


def walk(orc, elements, table, deaths=None, one_rows=None):
    """The walk of fmx_classes.hip as DESIGN.md 30 describes it, restated over the oracle.  A node (elements left, sp, ep, bytes
    matched):
      * a literal, or a class of one member: its bytes as plain steps, from the last, until the interval is empty;
      * otherwise every member, in rounds of as many as the layout has lane groups (16 or 8; the rounds change neither the
        steps nor what is pushed), makes its steps from its last byte until its interval is empty -- on a node of exactly one
        row only the members whose last byte is BWT'[sp] (0 on the EOF row), and with none of those the node dies without a
        step; the walk goes on with the non-empty child of the smallest member index and pushes the others.
    With no element left the node is a hit and the next entry is popped (the last pushed first).  Every step made counts, the
    ones that come back empty included.  -> (sorted list of (len, sp, ep), steps, the largest number of entries on the stack).
    deaths (a dict, or None): deaths[(bytes of the member, j)] counts the members of branching nodes whose interval became empty
    at their j-th step, j = 1 .. ; (bytes, 0) those that went through.  one_rows (a list, or None): gets the row of every
    branching node of exactly one row."""
    elements = list(elements)
    one = np.zeros(1, dtype=np.uint64)

    def step(sp, ep, c):
        a, b = orc.prev_range_batch(one + np.uint64(sp), one + np.uint64(ep), np.array([c], dtype=np.uint8))
        return int(a[0]), int(b[0])

    hits, stack, steps, depth = [], [], 0, 0
    node = (len(elements), 0, orc.n, 0)
    while node is not None:
        i, sp, ep, ln = node
        while True:
            if i == 0:
                hits.append((ln, sp, ep))
                break
            e = elements[i - 1]
            members = [bytes([e])] if e < 256 else [bytes(m) for m in table[e - 256]]
            if len(members) == 1:
                for c in reversed(members[0]):
                    sp, ep = step(sp, ep, c)
                    steps += 1
                    if sp >= ep:
                        break
                if sp >= ep:
                    break
                i, ln = i - 1, ln + len(members[0])
                continue
            row = approx_ref.row_symbol(orc, sp) if ep - sp == 1 else None
            if row is not None and one_rows is not None:
                one_rows.append(sp)
            kids = []
            for m in members:
                if row is not None and m[-1] != row:
                    continue
                s, t = sp, ep
                made = 0
                for c in reversed(m):
                    s, t = step(s, t, c)
                    steps += 1
                    made += 1
                    if s >= t:
                        break
                if deaths is not None:
                    key = (len(m), made if s >= t else 0)
                    deaths[key] = deaths.get(key, 0) + 1
                if s < t:
                    kids.append((i - 1, s, t, ln + len(m)))
            if not kids:
                break
            stack.extend(kids[1:])
            depth = max(depth, len(stack))
            i, sp, ep, ln = kids[0]
        node = stack.pop() if stack else None
    return sorted(hits), steps, depth


def expected_csr(per_pattern):
    """What the library returns for per-pattern lists of (len, sp, ep): (off, rows) with rows = (pattern, len, sp, ep), each
    pattern's by ascending sp."""
    off, rows = [0], []
    for q, hits in enumerate(per_pattern):
        rows += [(q, ln, sp, ep) for ln, sp, ep in sorted(hits, key=lambda h: h[1])]
        off.append(len(rows))
    return off, rows
