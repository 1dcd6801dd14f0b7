"""UTF-8 case folding as string classes (fmx_search_classes_batch): the classes of code points that differ in
case only, and the class table of a batch of patterns as the library takes it.

A class is a set of code points; its members are their UTF-8 encodings, 1 .. 4 bytes each.  case_classes() are the connected
components of "c ~ c.lower(), c ~ c.upper()" over images of one code point, plus the three pairs re.IGNORECASE equates on top
(U+0390/U+1FD3, U+03B0/U+1FE3, U+FB05/U+FB06): {K, k, U+212A}, {S, s, U+017F}, {Σ, σ, ς}.  Foldings to several code points
(ß/ss, İ) and decomposed text (a base letter followed by a combining mark) are out of scope."""
import unicodedata

import numpy as np

from . import _lib

_EXTRA_PAIRS = ((0x0390, 0x1FD3), (0x03B0, 0x1FE3), (0xFB05, 0xFB06))
_cache = {}


def _components(pairs):
    """{code point: sorted tuple of its component} for the components of two members or more."""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for x in parent:
        groups.setdefault(find(x), []).append(x)
    out = {}
    for members in groups.values():
        if len(members) >= 2:
            members = tuple(sorted(members))
            for x in members:
                out[x] = members
    return out


def _case_pairs():
    for c in range(0x110000):
        if 0xD800 <= c <= 0xDFFF:
            continue
        ch = chr(c)
        for other in (ch.lower(), ch.upper()):
            if len(other) == 1 and other != ch:
                yield c, ord(other)
    yield from _EXTRA_PAIRS


def case_classes():
    """{code point: its class, a sorted tuple of code points} for every code point whose class has two members or more.
    Built on the first call (about half a second) and kept."""
    if "case" not in _cache:
        _cache["case"] = _components(_case_pairs())
    return _cache["case"]


def _base(c):
    """The base letter of a precomposed code point: the first code point of its NFD form when the rest are combining marks."""
    d = unicodedata.normalize("NFD", chr(c))
    if len(d) > 1 and all(unicodedata.combining(x) for x in d[1:]) and not unicodedata.combining(d[0]):
        return ord(d[0])
    return c


def mark_classes():
    """case_classes() widened: a class holds every precomposed code point whose NFD base letter folds to the same base (e, E,
    é, É, ê ..).  Decomposed text is not matched.  A class may have more than 16 members; class_table refuses it unless the
    members that occur are few enough."""
    if "marks" not in _cache:
        pairs = list(_case_pairs())
        for c in range(0x80, 0x110000):
            if 0xD800 <= c <= 0xDFFF:
                continue
            b = _base(c)
            if b != c:
                pairs.append((c, b))
        _cache["marks"] = _components(pairs)
    return _cache["marks"]


def tokens(q):
    """The raw byte string q as UTF-8: a list of (code point, its bytes); a byte that does not decode is (None, that byte)."""
    q = bytes(q)
    out, i = [], 0
    while i < len(q):
        b = q[i]
        n = 1 if b < 0x80 else 2 if 0xC2 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF4 else 0
        if n:
            try:
                ch = q[i:i + n].decode("utf-8")
                out.append((ord(ch), q[i:i + n]))
                i += n
                continue
            except UnicodeDecodeError:
                pass
        out.append((None, q[i:i + 1]))
        i += 1
    return out


def members_of(patterns, classes):
    """The distinct member byte strings (UTF-8, text order) of the classes the patterns' code points have: what a caller
    searches once to learn which occur."""
    seen = {}
    for q in patterns:
        for cp, _ in tokens(q):
            for m in classes.get(cp, ()) if cp is not None else ():
                seen.setdefault(chr(m).encode("utf-8"), None)
    return list(seen)


def class_table(patterns, classes=None, occurring=None):
    """The ABI arrays of a batch of text strings under `classes` (default case_classes()).
    -> (el, el_off, cls_off, mem_off, mem_bytes): uint16 elements with uint64 offsets[k + 1], and the table.  A pattern is
    tokenised as UTF-8; a byte that does not decode is a literal element, a code point with a class of two or more is an
    element of that class, any other code point its bytes as literals.  Both the elements of a pattern and the bytes of a member
    are REVERSED, as search_batch takes the reverse of a text string.
    occurring (a container of member byte strings, text order, or None: all): members outside it are dropped; a class left
    with one member is inlined as literals, one left with none keeps the query's own bytes.  A class that still has more than
    16 members is a ValueError that names the character."""
    if classes is None:
        classes = case_classes()
    ids, table = {}, []                                        # members (tuple of bytes) -> class id
    el, el_off = [], [0]
    for q in patterns:
        row = []
        for cp, raw in tokens(q):
            members = classes.get(cp) if cp is not None else None
            if members:
                enc = [chr(m).encode("utf-8") for m in members]
                if occurring is not None:
                    enc = [m for m in enc if m in occurring]
                if len(enc) == 1:
                    raw = enc[0]
                elif len(enc) > _lib.FMX_CLASS_MAX_MEMBERS:
                    raise ValueError("the class of %r has %d members that occur, at most %d" % (chr(cp), len(enc), _lib.FMX_CLASS_MAX_MEMBERS))
                elif len(enc) >= 2:
                    key = tuple(enc)
                    if key not in ids:
                        if len(table) >= _lib.FMX_CLASS_MAX_CLASSES:
                            raise ValueError("more than %d classes in one table" % _lib.FMX_CLASS_MAX_CLASSES)
                        ids[key] = len(table)
                        table.append(key)
                    row.append(256 + ids[key])
                    continue
            row.extend(raw)
        el.extend(reversed(row))
        el_off.append(len(el))
    cls_off, mem_off, mem_bytes = [0], [0], bytearray()
    for members in table:
        for m in members:
            mem_bytes += m[::-1]
            mem_off.append(len(mem_bytes))
        cls_off.append(len(mem_off) - 1)
    return (np.array(el, dtype=np.uint16), np.array(el_off, dtype=np.uint64), np.array(cls_off, dtype=np.uint64),
            np.array(mem_off, dtype=np.uint64), np.frombuffer(bytes(mem_bytes), dtype=np.uint8))


def fold_map_table(fold):
    """The class table of a fold map (256 bytes): every class of two or more its single-byte members, ascending.
    -> (class id of every byte or -1, cls_off, mem_off, mem_bytes)."""
    fold = bytes(fold)
    groups = {}
    for c in range(256):
        groups.setdefault(fold[c], []).append(c)
    cid = [-1] * 256
    cls_off, mem = [0], []
    for members in groups.values():
        if len(members) >= 2:
            for c in members:
                cid[c] = len(cls_off) - 1
            mem += members
            cls_off.append(len(mem))
    return (cid, np.array(cls_off, dtype=np.uint64), np.arange(len(mem) + 1, dtype=np.uint64), np.array(mem, dtype=np.uint8))
