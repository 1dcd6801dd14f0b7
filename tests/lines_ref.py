"""The line table, its lookups and the occurrence-lines reduction in numpy, written from the definitions of include/fmx.h
(DESIGN.md 23): the breaks by np.isin, line(p) by np.searchsorted, the reduction from the (group, line) pairs of sorted
occurrences.  The corpus expectation stands on corpus_ref.RefCorpus's stream and per-position table."""
import numpy as np

LINE_HIT = np.dtype([("group", np.uint32), ("doc", np.uint32), ("line_no", np.uint64), ("start", np.uint64), ("len", np.uint32),
                     ("n_hits", np.uint32), ("raw_off", np.uint64), ("raw_len", np.uint32), ("first", np.uint32)])
NONE = np.uint64(2 ** 64 - 1)
NO_DOC = 0xFFFFFFFF


class Lines:
    """brk[] of a text for a break set, and line / start / end over it."""

    def __init__(self, text, breaks=b"\n"):
        T = np.frombuffer(bytes(text), dtype=np.uint8)
        self.len = int(T.size)
        self.brk = np.flatnonzero(np.isin(T, np.frombuffer(bytes(breaks), dtype=np.uint8))).astype(np.int64)
        self.n_brk = int(self.brk.size)

    def line(self, p):
        """#{ j : brk[j] < p }"""
        return np.searchsorted(self.brk, np.asarray(p, dtype=np.int64), side="left").astype(np.int64)

    def start(self, L):
        L = np.asarray(L, dtype=np.int64)
        before = np.concatenate([[-1], self.brk])            # before[L] = brk[L - 1], -1 for L = 0
        return before[L] + 1

    def end(self, L):
        L = np.asarray(L, dtype=np.int64)
        return np.concatenate([self.brk, [self.len]])[L]

    def lookup(self, pos):
        """(line, start, end) as uint64, NONE in all three for p >= len: what fmx_lines_batch returns."""
        pos = np.asarray(pos, dtype=np.uint64).reshape(-1)
        ok = pos < np.uint64(self.len)
        L = self.line(np.where(ok, pos, 0).astype(np.int64))
        return tuple(np.where(ok, a.astype(np.uint64), NONE) for a in (L, self.start(L), self.end(L)))

    def spans(self, lines):
        """(start, end) as uint64, NONE for L > n_brk: what fmx_line_spans returns."""
        lines = np.asarray(lines, dtype=np.uint64).reshape(-1)
        ok = lines <= np.uint64(self.n_brk)
        L = np.where(ok, lines, 0).astype(np.int64)
        return tuple(np.where(ok, a.astype(np.uint64), NONE) for a in (self.start(L), self.end(L)))

    def directory(self, shift):
        """dir[i] = #{ j : brk[j] < i << shift }, i = 0 .. (len >> shift) + 1 (len = n - 1)."""
        i = np.arange((self.len >> shift) + 2, dtype=np.int64)
        return np.searchsorted(self.brk, i << shift, side="left").astype(np.uint32)


def occurrence_lines(lines, off, occ, docs=None):
    """(line_off, LINE_HIT array) of the CSR occurrence list (off, occ), records ascending by pos inside a group.  docs: the
    corpus_ref.RefCorpus whose stream `lines` was made of (with the break set {10, 1})."""
    off = np.asarray(off, dtype=np.int64)
    out, line_off = [], [0]
    for g in range(off.size - 1):
        pos = occ["pos"][off[g]:off[g + 1]].astype(np.int64)
        L, first, count = np.unique(lines.line(pos), return_index=True, return_counts=True)
        rec = np.zeros(L.size, dtype=LINE_HIT)
        start, end = lines.start(L), lines.end(L)
        rec["group"], rec["doc"], rec["line_no"], rec["start"], rec["len"] = g, NO_DOC, L + 1, start, end - start
        rec["n_hits"], rec["first"], rec["raw_off"], rec["raw_len"] = count, first, start, end - start
        if docs is not None:
            for r, s, e, l_ in zip(rec, start.tolist(), end.tolist(), L.tolist()):
                d, _, ro = docs.table[s]
                assert docs.table[e][0] == d, "a line spans two documents"
                r["doc"], r["raw_off"], r["raw_len"] = d, ro, docs.table[e][2] - ro
                r["line_no"] = l_ - int(lines.line(docs.doc_start[d])) + 1
        out.append(rec)
        line_off.append(line_off[-1] + L.size)
    return np.array(line_off, dtype=np.uint64), np.concatenate(out) if out else np.zeros(0, dtype=LINE_HIT)


def python_grep(docs, needle):
    """[(doc, 1-based line number, line)] of the lines that hold `needle`, file by file: split on newlines, `in`.  The empty
    piece behind a final newline is no line."""
    out = []
    for d, raw in enumerate(docs):
        pieces = raw.split(b"\n")
        if raw.endswith(b"\n") or not raw:
            pieces = pieces[:-1]
        out += [(d, i + 1, ln) for i, ln in enumerate(pieces) if needle in ln]
    return out


def wc_l(raw):
    """Lines as the issue counts them: the newlines, plus the last unterminated line."""
    return raw.count(b"\n") + (not raw.endswith(b"\n") and len(raw) > 0)
