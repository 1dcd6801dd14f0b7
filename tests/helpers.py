"""Shared test helpers (CPU only, numpy)."""
import functools

import numpy as np
import pytest

_table_keys = {}        # the table keys table_default has set for the running test, and their values


@pytest.fixture
def table_default():
    """fmx_config_set for a table key ("jump_pairs", "search_lanes", ...): the default that handles opened afterwards copy.
    Call it as table_default(key, value); every key it set is "auto" again after the test."""
    import findex_amd

    def set_key(key, value):
        findex_amd.config_set(key, value)
        _table_keys[key] = value
    yield set_key
    for key in list(_table_keys):
        findex_amd.config_set(key, "auto")
        del _table_keys[key]


def table_key(key):
    """The value table_default gave `key` in the running test ("auto" when it set none)."""
    return _table_keys.get(key, "auto")


def bwt_of_text(text: bytes):
    """BWT of `text` + EOF in the layout findex's merger writes to .bwt/.aux
    (reference: bwtmerger.scala:782-810 sa2BWT, :841-856 aux): row i holds the
    byte before suffix SA[i]; the row whose suffix is the whole text is the EOF
    slot (filled with a neighbour's byte); counts exclude the EOF symbol.
    The text must not contain byte 0 (the readers escape it,
    bwtreader.scala:136-155).  Naive O(n^2 log n) sort: small inputs only.
    Returns (bwt uint8[n+1], eof, counts int64[256])."""
    assert 0 not in text
    s = bytes(text) + b"\0"
    n = len(s)
    sa = sorted(range(n), key=lambda i: s[i:])
    bwt = np.zeros(n, dtype=np.uint8)
    eof = -1
    for i, p in enumerate(sa):
        if p == 0:
            eof = i
        else:
            bwt[i] = s[p - 1]
    if eof > 0:
        bwt[eof] = bwt[eof - 1]
    elif n != 1:
        bwt[eof] = bwt[eof + 1]
    counts = np.bincount(np.frombuffer(bytes(text), dtype=np.uint8), minlength=256).astype(np.int64)
    return bwt, eof, counts


def synth_bwt(n, sigma_lo, sigma_hi, seed, eof=None):
    """i.i.d. uniform symbols in [sigma_lo, sigma_hi]; any byte string is a valid
    BWT for rank / backward-search purposes.  Returns (bwt, eof, counts)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bwt = rng.integers(sigma_lo, sigma_hi + 1, size=n, dtype=np.uint8 if sigma_hi < 256 else np.int64).astype(np.uint8)
    if eof is None:
        eof = n // 3
    counts = np.bincount(bwt, minlength=256).astype(np.int64)
    counts[bwt[eof]] -= 1
    return bwt, eof, counts


def lf_walk_patterns(sa, rng, k, m, mutate_frac=0.1, alphabet=None):
    """Hit patterns by LF walk: from a random row take c=L[r],
    r=LF(r) m times and emit the bytes reversed, so every backward step has a
    non-empty interval; `mutate_frac` of them get one random byte replaced."""
    pats = []
    for _ in range(k):
        r = int(rng.integers(0, sa.n))
        cs = []
        for _ in range(m):
            cs.append(sa.bwt_read(r))
            r = sa.getPrevI(r)
        p = bytearray(reversed(cs))
        if rng.random() < mutate_frac and m > 0:
            j = int(rng.integers(0, m))
            p[j] = int(rng.choice(alphabet)) if alphabet is not None else int(rng.integers(1, 256))
        pats.append(bytes(p))
    return pats


def pack_patterns(pats):
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    for i, p in enumerate(pats):
        off[i + 1] = off[i] + len(p)
    buf = np.frombuffer(b"".join(pats), dtype=np.uint8).copy() if pats and int(off[-1]) else np.zeros(0, dtype=np.uint8)
    return buf, off


# ---------------------------------------------------------------- designed indexes (tests/test_gpu_primitives.py)
ONEHOT_BLOCK = 448      # BWT positions per block of the one-hot layout
BYTES_BLOCK = 128       # ... of the bytes layout


def index_of_bwt(bwt, eof):
    """(bwt, eof, counts) for given BWT bytes: counts exclude the filler at slot eof, as synth_bwt does it."""
    bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
    counts = np.bincount(bwt, minlength=256).astype(np.int64)
    counts[bwt[eof]] -= 1
    return bwt, int(eof), counts


def clustered_bwt(eof, n=200_000):
    """Symbol 1 in the first and the last quarter, symbol 2 between them: every S-th occurrence of symbol 1 is sampled
    at the density of n/2 occurrences in n rows, so the sample that spans the gap covers n/2 rows of blocks.  Symbol 200
    at both ends and around the first one-hot block edge, symbol 7 once in the middle."""
    bwt = np.full(n, 2, dtype=np.uint8)
    bwt[: n // 4] = 1
    bwt[3 * n // 4:] = 1
    bwt[[0, 447, 448, 449, n - 1]] = 200
    bwt[100_000] = 7
    return index_of_bwt(bwt, eof)


def one_symbol_bwt(n, eof=None):
    """Density 1: every row holds symbol 97."""
    return index_of_bwt(np.full(n, 97, dtype=np.uint8), n // 3 if eof is None else eof)


def geometric_bwt(n=300_007, seed=5):
    """Symbol c with probability about 2^-c, c = 1..16: densities from 1/2 down to 2^-16."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return index_of_bwt(np.minimum(rng.geometric(0.5, size=n), 16).astype(np.uint8), n // 3)


def sparse_alphabet_bwt(n=50_001, seed=6):
    """Symbols {1, 3, 128, 254, 255} with absent ones between them.  1 and 128 share the rows; 254 occurs once, at the
    first position of a block, and 255 once, at the last position of a block (multiples of 896 begin a block of both
    sizes); 3 sits on both sides of the first block edge of either size and in the last row."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bwt = np.where(rng.random(n) < 0.5, 1, 128).astype(np.uint8)
    bwt[[BYTES_BLOCK - 1, BYTES_BLOCK, ONEHOT_BLOCK - 1, ONEHOT_BLOCK, n - 1]] = 3
    bwt[896 * 5] = 254
    bwt[896 * 20 - 1] = 255
    return index_of_bwt(bwt, n // 3)


# ---------------------------------------------------------------- regex oracles shared by the GPU regex modules
class _OIdx:
    """What oracle.engines and oracle.retree ask of an index: .n and getPrevRange."""

    def __init__(self, sa):
        self.sa, self.n = sa, sa.n

    def getPrevRange(self, sp, ep, c):
        return self.sa.getPrevRange(sp, ep, c)


def oracle_results_capped(bwt, eof, counts, re, max_len):
    """All matches of length <= max_len: breadth-first over the oracle's getPrevRange."""
    import oracle
    from oracle import retree as R
    orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
    t = R.ReTree(R.re2post(re)).tables()
    front = [(0, 0, orc.n, s) for s in t["firsts"]]
    out = []
    while front:
        nxt = []
        for ln, sp, ep, s in front:
            r = orc.getPrevRange(sp, ep, t["c"][s])
            if r is None:
                continue
            if t["isLast"][s]:
                out.append((ln + 1, r[0], r[1]))
            elif ln + 1 < max_len:
                nxt += [(ln + 1, r[0], r[1], f) for f in t["follows"][s]]
        front = nxt
    return out


FRONTIER_DTYPE = np.dtype([("regex", np.uint32), ("len", np.uint32), ("sp", np.uint64), ("ep", np.uint64)])


def frontier_oracle(orc, tables, max_len=0, **batch_kw):
    """oracle_results_capped for a whole batch of regexes (`tables`: a list of ReTree.tables() dicts) with one
    orc.prev_range_batch call per level: every frontier element of the level is stepped by its state's byte, a non-empty
    range is emitted when the state isLast and else expanded into the state's follows while len + 1 < max_len (0: no cap),
    multiplicity kept.  -> (structured array of (regex, len, sp, ep) sorted by those four, getPrevRange evaluations made,
    whether the cap cut an element that had follows).  `batch_kw` goes to prev_range_batch (threads=)."""
    st_c, st_last, st_regex, fol_off, fol, firsts = [], [], [], [0], [], []
    for j, t in enumerate(tables):
        base = len(st_c)
        st_c += t["c"]
        st_last += [bool(x) for x in t["isLast"]]
        st_regex += [j] * len(t["c"])
        for f in t["follows"]:
            fol += [base + x for x in f]
            fol_off.append(len(fol))
        firsts += [base + x for x in t["firsts"]]
    st_c = np.asarray(st_c, dtype=np.uint8)
    st_last = np.asarray(st_last, dtype=bool)
    st_regex = np.asarray(st_regex, dtype=np.uint32)
    fol_off = np.asarray(fol_off, dtype=np.int64)
    fol = np.asarray(fol, dtype=np.int64)
    st = np.asarray(firsts, dtype=np.int64)
    sp = np.zeros(st.size, dtype=np.uint64)
    ep = np.full(st.size, orc.n, dtype=np.uint64)
    parts, calls, level, truncated = [], 0, 0, False
    while st.size:
        a, b = orc.prev_range_batch(sp, ep, st_c[st], **batch_kw)
        calls += int(st.size)
        level += 1
        ok = a < b
        emit = ok & st_last[st]
        part = np.zeros(int(emit.sum()), dtype=FRONTIER_DTYPE)
        part["regex"], part["len"], part["sp"], part["ep"] = st_regex[st[emit]], level, a[emit], b[emit]
        parts.append(part)
        grow = ok & ~st_last[st]
        src = st[grow]
        cnt = fol_off[src + 1] - fol_off[src]
        if max_len and level >= max_len:
            truncated = truncated or bool((cnt > 0).any())
            break
        total = int(cnt.sum())
        first = np.repeat(fol_off[src] - (np.cumsum(cnt) - cnt), cnt)      # follows of one element are consecutive
        st = fol[first + np.arange(total, dtype=np.int64)]
        sp = np.repeat(a[grow], cnt)
        ep = np.repeat(b[grow], cnt)
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=FRONTIER_DTYPE)
    return out[np.lexsort((out["ep"], out["sp"], out["len"], out["regex"]))], calls, truncated


# ---------------------------------------------------------------- shared by the modules that open an index above 2^32 rows
def forward_string(orc, row, length, syms=b"abcd"):
    """The first `length` bytes of the suffix of `row`, from cf and occ alone: the first byte is the bucket the row lies
    in, the next row is the position of that byte's (row - cf + 1)-th occurrence in the BWT (binary search over occ).
    `syms`: the symbols the index holds."""
    syms = [0] + list(syms)
    cf = {c: orc.cf(c) for c in syms}
    out = bytearray()
    for _ in range(length):
        c = max(s for s in syms if cf[s] <= row)
        assert c != 0, "the walk reached the end of the text"
        out.append(c)
        k = row - cf[c] + 1
        lo, hi = 0, orc.n - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if orc.occ(c, mid) >= k:
                hi = mid
            else:
                lo = mid + 1
        row = lo
    return bytes(out)


_fault = []


def ends_at_a_fault(test):
    """A HIP error in one case ends the work on the device there: the cases after it, of this module and of every other
    that uses this guard, fail without touching the device again."""
    @functools.wraps(test)
    def run(*args, **kw):
        import findex_amd
        if _fault:
            pytest.fail("an earlier case ended with a HIP error, nothing more is started on the device: " + _fault[0])
        try:
            return test(*args, **kw)
        except findex_amd.FmxError as e:
            if e.code == 5:      # FMX_ERR_HIP
                _fault.append(str(e))
            raise
    return run
