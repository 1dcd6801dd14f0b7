"""References of tests/test_gpu_top_bit.py that need the text itself, in plain torch on whatever device the text tensor lies
on: the break positions of a break set, a stand-in for lines_ref.Lines over them, and the table of the distinct windows of
1 .. 3 bytes.  Nothing of the library is used.  Every pass walks the text `step` bytes at a time, so no temporary holds more
than `step` int64 (2^28 in the device test); tests/test_top_bit_ref_cpu.py holds all of it to lines_ref.Lines,
linequery_ref.line_query and ngrams_ref.brute on a text of 12 419 bytes, with a step that cuts it into many pieces."""
import numpy as np
import torch

import linequery_ref
from lines_ref import LINE_HIT, NO_DOC

STEP = 1 << 28
M32 = 0xFFFFFFFF


def _is_break(chunk, breaks):
    mask = torch.zeros(chunk.numel(), dtype=torch.bool, device=chunk.device)
    for b in sorted(set(bytes(breaks))):
        mask |= chunk == b
    return mask


def break_positions(text, breaks, step=STEP):
    """The ascending positions (int64) of the bytes of `text` (uint8) that belong to the break set: counted first, so the
    result is allocated once."""
    m = text.numel()
    counts = [int(_is_break(text[a:a + step], breaks).sum()) for a in range(0, m, step)]
    out = torch.empty(sum(counts), dtype=torch.int64, device=text.device)
    at = 0
    for a, c in zip(range(0, m, step), counts):
        out[at:at + c] = torch.nonzero(_is_break(text[a:a + step], breaks)).reshape(-1) + a
        at += c
    return out


class Lines:
    """lines_ref.Lines' line / start / end / lookup / spans over break_positions.  An argument that is a tensor is answered
    with tensors on the breaks' device (int64; -1 holds NO_LINE's bits), anything else with numpy arrays as lines_ref.Lines
    gives them -- which is what lines_ref.occurrence_lines and linequery_ref.line_query ask for."""

    def __init__(self, text, breaks=b"\n", step=STEP):
        self.len = int(text.numel())
        self.brk = break_positions(text, breaks, step)
        self.n_brk = int(self.brk.numel())

    def _in(self, x):
        if torch.is_tensor(x):
            return x.to(self.brk.device, torch.int64), True
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))).to(self.brk.device), False

    @staticmethod
    def _out(t, as_tensor):
        return t if as_tensor else t.cpu().numpy()

    def _line(self, p):
        return torch.searchsorted(self.brk, p.contiguous(), right=False)      # #{ j : brk[j] < p }

    def _start(self, L):
        if not self.n_brk:
            return torch.zeros_like(L)
        return torch.where(L > 0, self.brk[(L - 1).clamp(0, self.n_brk - 1)] + 1, torch.zeros_like(L))

    def _end(self, L):
        if not self.n_brk:
            return torch.full_like(L, self.len)
        return torch.where(L < self.n_brk, self.brk[L.clamp(0, self.n_brk - 1)], torch.full_like(L, self.len))

    def line(self, p):
        p, t = self._in(p)
        return self._out(self._line(p), t)

    def start(self, L):
        L, t = self._in(L)
        return self._out(self._start(L), t)

    def end(self, L):
        L, t = self._in(L)
        return self._out(self._end(L), t)

    def _answer(self, x, limit, fields):
        """x below `limit` (unsigned) -> fields(x), everything else NO_LINE"""
        as_tensor = torch.is_tensor(x)
        if as_tensor:
            x = x.to(self.brk.device, torch.int64).reshape(-1)
            ok = (x >= 0) & (x < limit)                          # a negative int64 is an unsigned value of 2^63 and more
        else:
            u = np.asarray(x, dtype=np.uint64).reshape(-1)
            ok_np = u < np.uint64(limit)
            x = torch.from_numpy(np.where(ok_np, u, 0).astype(np.int64)).to(self.brk.device)
            ok = torch.from_numpy(ok_np).to(self.brk.device)
        safe = torch.where(ok, x, torch.zeros_like(x))
        out = tuple(torch.where(ok, f, torch.full_like(f, -1)) for f in fields(safe))
        return out if as_tensor else tuple(f.cpu().numpy().view(np.uint64) for f in out)

    def lookup(self, pos):
        """(line, start, end), NO_LINE in all three for p >= len: what fmx_lines_batch returns."""
        def fields(p):
            L = self._line(p)
            return L, self._start(L), self._end(L)
        return self._answer(pos, self.len, fields)

    def spans(self, lines):
        """(start, end), NO_LINE for L > n_brk: what fmx_line_spans returns."""
        return self._answer(lines, self.n_brk + 1, lambda L: (self._start(L), self._end(L)))

    def directory_crossings(self, shift, line=1 << 31):
        """The text positions [first, last] of the directory entries b, b + 1 between which dir[] = #{ j : brk[j] < i << shift }
        crosses `line`: b is the last entry whose value is below it."""
        assert self.n_brk > line
        b = int(self.brk[line - 1].item()) >> shift               # dir[b] <= line - 1 < dir[b + 1], as brk[line - 1] >= b << shift
        return [b << shift, min(((b + 1) << shift) - 1, self.len - 1), min((b + 1) << shift, self.len - 1), min(((b + 2) << shift) - 1, self.len - 1)]


def line_records(lines, L):
    """The LINE_HIT records linequery_ref.real_lines gives for the global lines L (int64, ascending), the real ones of them."""
    L = np.asarray(L, dtype=np.int64)
    L = L[(L >= 0) & (L <= lines.n_brk)]
    start, end = lines.start(L), lines.end(L)
    real = start != lines.len
    L, start, end = L[real], start[real], end[real]
    rec = np.zeros(L.size, dtype=LINE_HIT)
    rec["doc"], rec["line_no"], rec["start"], rec["len"] = NO_DOC, L + 1, start, end - start
    rec["n_hits"], rec["first"], rec["raw_off"], rec["raw_len"] = 0, 0xFFFFFFFF, start, end - start
    return rec


def line_query(off, hits, queries, lines):
    """linequery_ref.line_query for a text whose real lines cannot be listed (more than 2^31 of them).  A query whose anchor
    is ALL_LINES must have a positive term with a line window w: a line satisfies that term only if it lies within w lines of
    one of the term's hits, so the candidates of the query are cut down to those lines -- appended to (off, hits) as a group of
    their own, which becomes the query's anchor -- and the reference decides every term on them as it does on any anchor."""
    off = np.asarray(off, dtype=np.uint64).copy()
    parts, asked = [hits], []
    for anchor, terms in queries:
        if anchor is not None:
            asked.append((anchor, terms))
            continue
        g, w = next((g, int(w)) for g, w, neg in terms if not neg and w != "file")
        at = hits["line_no"][int(off[g]):int(off[g + 1])].astype(np.int64) - 1
        near = np.unique((at[:, None] + np.arange(-w, w + 1, dtype=np.int64)[None, :]).reshape(-1))
        parts.append(line_records(lines, near))
        asked.append((off.size - 1, terms))
        off = np.concatenate([off, [off[-1] + np.uint64(parts[-1].size)]]).astype(np.uint64)
    return linequery_ref.line_query(off, np.concatenate(parts), asked)


HEAD = 1 << 16


def _scatter(table, code, value, how):
    """table[code] = min or max (how: "amin", "amax") of itself and value, a scatter-reduce in two steps: the first HEAD
    elements, then those of the rest that still improve on the table.  A window that fills a quarter of the text would send a
    quarter of a plain scatter's elements to one address; after the first step all but a few of them have nothing to add."""
    table.scatter_reduce_(0, code[:HEAD], value[:HEAD], how)
    now = table[code]
    left = torch.nonzero(value < now if how == "amin" else value > now).reshape(-1)
    table.scatter_reduce_(0, code[left], value[left], how)


def _codes(text, L, a, e):
    code = torch.zeros(e - a, dtype=torch.int64, device=text.device)
    for i in range(L):
        code = (code << 8) | text[a + i:e + i].to(torch.int64)
    return code


def gram_table(text, L, row_of=None, step=STEP):
    """The distinct windows of L <= 3 bytes of `text`: a dict of int64 tensors, one entry per window that occurs, ascending by
    the packed code (text[t] << 8 (L - 1) | ..):  code;  first, the smallest t, a scatter-min over the codes;  count, a
    torch.bincount over the codes' ranks among the codes that occur (a table of a few hundred bins, not of 2^24);  and with
    row_of -- the inverse of the suffix array of s = reverse(text) + sentinel, int64 or the u32 bits in int32 -- sp, the
    smallest row among the window's occurrences (the window at t is the prefix of the suffix at m - t - L), a scatter-min as
    well, with the check that the largest row is sp + count - 1: the occurrences are one run of rows."""
    assert 1 <= L <= 3 and text.dtype == torch.uint8
    m, dev = text.numel(), text.device
    K = 1 << (8 * L)
    big = 1 << 62
    first = torch.full((K,), big, dtype=torch.int64, device=dev)
    lo = torch.full((K,), big, dtype=torch.int64, device=dev)
    hi = torch.full((K,), -1, dtype=torch.int64, device=dev)
    chunks = [(a, min(m - L + 1, a + step)) for a in range(0, m - L + 1, step)]
    for a, e in chunks:
        code = _codes(text, L, a, e)
        _scatter(first, code, torch.arange(a, e, dtype=torch.int64, device=dev), "amin")
        if row_of is not None:
            rows = row_of[m - e - L + 1:m - a - L + 1].to(torch.int64).flip(0) & M32      # row_of[m - t - L], t = a .. e - 1
            _scatter(lo, code, rows, "amin")
            _scatter(hi, code, rows, "amax")
            del rows
        del code
    keep = torch.nonzero(first != big).reshape(-1)
    count = torch.zeros(keep.numel(), dtype=torch.int64, device=dev)
    for a, e in chunks:
        rank = torch.searchsorted(keep, _codes(text, L, a, e))
        count += torch.bincount(rank, minlength=keep.numel())
    out = {"code": keep, "count": count, "first": first[keep]}
    if row_of is not None:
        out["sp"] = lo[keep]
        assert bool(torch.equal(hi[keep] - out["sp"] + 1, out["count"])), "the rows of a window are not one run"
    return out
