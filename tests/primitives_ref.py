"""The plain reference for the primitive kernels (rank, step, LF, Psi): everything straight from the BWT bytes with one
stable sort -- numpy only, no GPU, no oracle.  tests/test_primitives_ref_cpu.py pins every function here against the
oracle and the reference's known answers; the GPU tests use nothing that file has not pinned.

B is the BWT with slot eof read as symbol 0.  Sorting the positions of B by symbol, ties by position, lists for row
cf[c] + j the position of the j-th c: that is Psi (the reference's inverted list), and LF is its inverse."""
import numpy as np


class PlainIndex:
    def __init__(self, bwt, eof):
        B = np.array(bwt, dtype=np.uint8, copy=True).reshape(-1)
        B[eof] = 0
        self.B, self.n, self.eof = B, int(B.size), int(eof)
        self.psi = np.argsort(B, kind="stable").astype(np.int64)
        self.lf = np.empty(self.n, dtype=np.int64)
        self.lf[self.psi] = np.arange(self.n, dtype=np.int64)
        cnt = np.bincount(B, minlength=256).astype(np.int64)
        self.cf = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        self._pos = {}

    def positions(self, c):
        """Where symbol c stands in B, ascending."""
        c = int(c)
        if c not in self._pos:
            self._pos[c] = np.nonzero(self.B == c)[0]
        return self._pos[c]

    def occ(self, c, i):
        """#{p <= i : B[p] == c}; i < 0 gives 0, i >= n is read as n - 1."""
        c = np.asarray(c, dtype=np.uint8).reshape(-1)
        i = np.asarray(i, dtype=np.int64).reshape(-1)
        key = np.minimum(i, self.n - 1)
        out = np.zeros(c.size, dtype=np.int64)
        order = np.argsort(c, kind="stable")
        syms, first = np.unique(c[order], return_index=True)
        for sym, a, b in zip(syms.tolist(), first.tolist(), first.tolist()[1:] + [c.size]):
            q = order[a:b]
            out[q] = np.searchsorted(self.positions(sym), key[q], side="right")
        out[i < 0] = 0
        return out

    def prev_range(self, sp, ep, c):
        """getPrevRange: (cf[c] + occ(c, sp - 1), cf[c] + occ(c, ep - 1))."""
        c = np.asarray(c, dtype=np.uint8).reshape(-1)
        sp = np.asarray(sp).astype(np.int64).reshape(-1)
        ep = np.asarray(ep).astype(np.int64).reshape(-1)
        base = self.cf[c.astype(np.int64)]
        return base + self.occ(c, sp - 1), base + self.occ(c, ep - 1)

    def interval_prev_range(self, sp, ep, c0, c1):
        """getIntervalPrevRange: the non-empty steps of the symbols c0 .. c1, in descending c."""
        if c1 < c0:
            return []
        c = np.arange(c0, c1 + 1, dtype=np.int64)
        a, b = self.prev_range(np.full(c.size, sp), np.full(c.size, ep), c.astype(np.uint8))
        return [(int(a[j]), int(b[j])) for j in range(c.size - 1, -1, -1) if a[j] < b[j]]

    def prev_substr(self, rows, length):
        """prevSubstr / the LF walk: `length` times emit B[row], row = lf[row] -> (bytes [k, length], end rows)."""
        rows = np.asarray(rows).astype(np.int64).reshape(-1).copy()
        out = np.zeros((rows.size, int(length)), dtype=np.uint8)
        for s in range(int(length)):
            out[:, s] = self.B[rows]
            rows = self.lf[rows]
        return out, rows

    def next_substr(self, rows, length):
        """nextSubstr in WALK order (the device form): up to `length` times emit B[psi[row]], stop after a 0, row =
        psi[row] -> (bytes [k, length], lengths); bytes behind a walk's length are 0 here and mean nothing."""
        rows = np.asarray(rows).astype(np.int64).reshape(-1).copy()
        out = np.zeros((rows.size, int(length)), dtype=np.uint8)
        ln = np.zeros(rows.size, dtype=np.uint32)
        live = np.ones(rows.size, dtype=bool)
        for s in range(int(length)):
            nxt = self.psi[rows]
            b = self.B[nxt]
            out[live, s] = b[live]
            ln[live] += 1
            rows = np.where(live, nxt, rows)
            live &= b != 0
        return out, ln

    def next_substr_host(self, rows, length):
        """nextSubstr as the host form returns it: each walk's bytes reversed, as a list of bytes objects."""
        out, ln = self.next_substr(rows, length)
        return [bytes(out[q, :ln[q]][::-1]) for q in range(ln.size)]
