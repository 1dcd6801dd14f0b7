"""HipFMSearcher: the drop-in for findex's NaiveFMSearcher (bwtmerger.scala:335-421) and the
SuffixAlgo / SuffixWalkingAlgo traits it implements (findex.scala:9-57), served by libfmx.so."""
import ctypes
import os

import numpy as np

from . import _lib


# the bytes of a word: 0-9 A-Z a-z _ and 0x80 .. 0xFF, so that a UTF-8 letter is no word boundary.  The boundary class is the
# complement: it holds 0 (the ends of the text) and 1 (the corpus separator), so no file boundary needs a special case.
WORD_BYTES = bytes(sorted(set(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_") | set(range(0x80, 0x100))))


def class_words(members):
    """The 256-bit set fmx_context_filter and fmx_context_opts take, as uint64[4]: bit c of word c // 64 for every byte value of
    `members` (bytes or an iterable of ints; 0 stands for an end of the text)."""
    w = [0, 0, 0, 0]
    for c in bytes(members):
        w[c >> 6] |= 1 << (c & 63)
    return np.array(w, dtype=np.uint64)


def boundary_class(word=WORD_BYTES):
    """The bytes that may stand next to a word: every byte that is not in `word`, 0 (an end of the text) included."""
    word = set(bytes(word))
    return bytes(c for c in range(256) if c not in word)


# ASCII case folding as a fold map (fmx_fold_opts.fold): A..Z fold to a..z, every other byte to itself -- what the
# library uses when it is given no map
ASCII_FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def check_fold(fold):
    """The 256 bytes of a valid fold map, or ValueError: fold[fold[c]] == fold[c], byte 0 alone in its class, at most 8 members
    per class (the library's own checks, made here for the callers that never reach it)."""
    fold = bytes(fold)
    if len(fold) != 256:
        raise ValueError("a fold map has 256 bytes")
    size = [0] * 256
    for c in range(256):
        r = fold[c]
        if fold[r] != r:
            raise ValueError("fold map: fold[fold[%d]] != fold[%d]" % (c, c))
        if (r == 0) != (c == 0):
            raise ValueError("fold map: byte 0 folds to itself and no other byte folds to 0")
        size[r] += 1
        if size[r] > _lib.FMX_FOLD_MAX_CLASS:
            raise ValueError("fold map: a class of more than %d members" % _lib.FMX_FOLD_MAX_CLASS)
    return fold


def fold_map(pairs):
    """A fold map from equivalences: every item of `pairs` is a bytes object or a sequence of byte values (ints or one-byte
    strings) that are all to be equal; classes that share a member merge.  The representative of a class is its smallest
    member.  fold_map([b"aA", b"bB"]), fold_map([(0x61, 0x41)]).  ValueError for byte 0 or a class of more than 8."""
    parent = list(range(256))

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    for item in pairs:
        members = [m if isinstance(m, int) else bytes(m)[0] if len(bytes(m)) == 1 else -1 for m in (item if not isinstance(item, (bytes, bytearray)) else bytes(item))]
        if any(not 0 <= m < 256 for m in members):
            raise ValueError("fold_map: members are byte values or one-byte strings")
        if len(members) > 1 and 0 in members:
            raise ValueError("fold_map: byte 0 is equal to nothing else")
        for m in members[1:]:
            a, b = find(members[0]), find(m)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return check_fold(bytes(find(c) for c in range(256)))


def _swap_ext(filename, ext):
    """BWTTempStorage.gen*Filename, bwtmerger.scala:17-48"""
    return os.path.splitext(filename)[0] + ext


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def _dp(x):
    return ctypes.c_void_p(int(x) if x else 0)


class _NfaSource:
    """What regex.NFA() reads of a PostfixRe: the regex as text and lineOnly, without the postfix string."""

    def __init__(self, src, lineOnly):
        self.src, self.lineOnly = src, bool(lineOnly)


class PinnedArray:
    """A numpy view of page-locked host memory from fmx_host_alloc (freed with the object): batch buffers that the
    host-pointer entry points move by DMA at link speed."""

    def __init__(self, shape, dtype):
        self._L = _lib.load()
        self.dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        self._p = ctypes.c_void_p()
        _lib.check(self._L.fmx_host_alloc(max(n, 1) * self.dtype.itemsize, ctypes.byref(self._p)))
        buf = (ctypes.c_uint8 * (max(n, 1) * self.dtype.itemsize)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=n).reshape(shape)

    def __del__(self):
        try:
            if self._p:
                self.array = None
                self._L.fmx_host_free(self._p)
                self._p = None
        except Exception:
            pass


class HipFMSearcher:
    """`new NaiveFMSearcher(filename, bigEndian)`: opens X.bwt and X.aux next to `filename` and
    builds the rank dictionary in HBM.  The reference's X.fm is not needed; when it is there it must
    pass FMLoader's checks and hold the .bwt's n rows (fmx_open), or the open fails as the reference's does.

    Scalar methods keep the reference's names and Option-like results (tuple or None); each
    `*_batch` method is the batched form the kernels are built for.  Positions are Python ints /
    uint64 arrays."""

    def __init__(self, filename=None, bigEndian=True, device=0, _handle=None):
        self._L = _lib.load()
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _lib.check(self._L.fmx_open(_swap_ext(filename, ".bwt").encode(), _swap_ext(filename, ".aux").encode(),
                                        1 if bigEndian else 0, int(device), ctypes.byref(self._h)))
        v = ctypes.c_uint64()
        _lib.check(self._L.fmx_n(self._h, ctypes.byref(v)))
        self.n = int(v.value)
        _lib.check(self._L.fmx_eof(self._h, ctypes.byref(v)))
        self.eof = int(v.value)
        self.K = 256
        cf = np.zeros(256, dtype=np.uint64)
        for c in range(256):
            _lib.check(self._L.fmx_cf(self._h, c, ctypes.byref(v)))
            cf[c] = v.value
        self.bucketStarts = cf

    # ---- alternative constructors
    @classmethod
    def from_mem(cls, bwt, eof, counts, device=0):
        """fmx_open_mem: BWT bytes (filler at slot eof) + the .aux counts, from host memory."""
        L = _lib.load()
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if counts.size != 256:
            raise ValueError("counts must have 256 entries")
        h = ctypes.c_void_p()
        _lib.check(L.fmx_open_mem(_ptr(bwt), bwt.size, int(eof), _ptr(counts), int(device), ctypes.byref(h)))
        return cls(_handle=h)

    @classmethod
    def from_device(cls, d_bwt_ptr, n, eof, counts=None, device=0, stream=0):
        """fmx_open_dev: BWT bytes already resident in HBM (e.g. tensor.data_ptr())."""
        L = _lib.load()
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
        h = ctypes.c_void_p()
        _lib.check(L.fmx_open_dev(_dp(d_bwt_ptr), int(n), int(eof), _ptr(c), int(device), _dp(stream),
                                  ctypes.byref(h)))
        return cls(_handle=h)

    @classmethod
    def from_text(cls, text, device=0, chunk=None):
        """fmx_open_text: the index BWTMerger2.merge(FileBWTReader) would write for this text (the BWT of the reversed
        text, so that search(reversed pattern) counts the pattern's occurrences), built on the device.  With `chunk` the
        first `chunk` bytes are built that way and the rest is appended chunk by chunk (append_text): the same index, and
        the way to a text beyond the suffix sort's 2^32 - 2 bytes, for which chunking is forced."""
        L = _lib.load()
        t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(text, dtype=np.uint8).reshape(-1)
        if chunk is None and t.size > _lib.MAX_TEXT_LEN:
            chunk = 1 << 30
        if chunk is not None:
            chunk = int(chunk)
            if chunk < 1:
                raise ValueError("chunk must be at least 1 byte")
        if chunk is None or chunk >= t.size:
            h = ctypes.c_void_p()
            _lib.check(L.fmx_open_text(_ptr(t), t.size, int(device), ctypes.byref(h)))
            return cls(_handle=h)
        cur = cls.from_text(t[:chunk], device=device)
        # a piece is not made much longer than what it appends: the first context follows the chunk (a retry doubles it)
        context = min(_lib.FMX_MERGE_CONTEXT, max(64, chunk))
        for lo in range(chunk, t.size, chunk):
            nxt = cur.append_text(t[lo: lo + chunk], context=context)
            cur.close()
            cur = nxt
        return cur

    # ---- append (fmx.h, "append")
    @staticmethod
    def _merge_opts(context=None, max_context=None, segment=None, warmup=None):
        if context is None and max_context is None and segment is None and warmup is None:
            return None
        o = _lib.fmx_merge_opts()
        o.context = int(context or 0)
        o.max_context = int(max_context or 0)
        if segment is not None or warmup is not None:
            o.segment = int(_lib.FMX_MERGE_SEGMENT if segment is None else segment)
            o.warmup = int(_lib.FMX_MERGE_WARMUP if warmup is None else warmup)
            if o.segment < 1:
                raise ValueError("segment must be at least 1")
        return o

    def append_text(self, text, context=None, max_context=None, segment=None, warmup=None):
        """fmx_append_text: a NEW searcher over (this index's text) + text, byte for byte the index from_text of the
        whole would give, merged on the device without rebuilding this one.  This searcher is untouched and stays valid.
        `context`: bytes of the indexed text's tail sorted together with the new text (doubled while the new text
        repeats them, up to `max_context`); `segment`, `warmup`: the rank walk's cut (fmx.h)."""
        t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(text, dtype=np.uint8).reshape(-1)
        o = self._merge_opts(context, max_context, segment, warmup)
        h = ctypes.c_void_p()
        _lib.check(self._L.fmx_append_text(self._h, _ptr(t), t.size, ctypes.byref(o) if o is not None else None,
                                           ctypes.byref(h)))
        return type(self)(_handle=h)

    def append_text_dev(self, d_text, length, d_bwt_out, context=None, max_context=None, segment=None, warmup=None, stream=0):
        """fmx_append_text_dev: device pointers -- text[length] in, the merged BWT (n + length bytes) out, ready for
        from_device.  Synchronises `stream`.  Returns (eof, counts int64[256])."""
        o = self._merge_opts(context, max_context, segment, warmup)
        counts = np.zeros(256, dtype=np.int64)
        eof = ctypes.c_uint64()
        _lib.check(self._L.fmx_append_text_dev(self._h, _dp(d_text), int(length), ctypes.byref(o) if o is not None else None,
                                               _dp(d_bwt_out), ctypes.byref(eof), _ptr(counts), _dp(stream)))
        return int(eof.value), counts

    @staticmethod
    def merge_last():
        """fmx_merge_last: this thread's last append -- device ms of its phases, the steps of the segment walk, steps,
        number and longest of the fix-up runs, the context that passed and the pieces built."""
        st = _lib.fmx_merge_stats()
        _lib.check(_lib.load().fmx_merge_last(ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def bwt_bytes(self, batch=1 << 22):
        """The index's BWT as fmx_bwt_from_text writes it: BWTLoader.read of every row, and at the eof slot the filler
        of sa2BWT (bwtmerger.scala:799-806: the byte of the row above, of the row below for eof == 0)."""
        out = np.empty(self.n, dtype=np.uint8)
        for lo in range(0, self.n, batch):
            rows = np.arange(lo, min(lo + batch, self.n), dtype=np.uint64)
            b, _ = self.lf_walk_batch(rows, 1)
            out[lo: lo + rows.size] = np.asarray(b, dtype=np.uint8).reshape(-1)
        if self.n > 1:
            out[self.eof] = out[self.eof - 1] if self.eof else out[1]
        return out

    def counts(self):
        """fmx_counts: the .aux counts (occurrences of every byte in the text)."""
        c = np.zeros(256, dtype=np.int64)
        _lib.check(self._L.fmx_counts(self._h, _ptr(c)))
        return c

    @classmethod
    def from_block(cls, bwt, bucketStarts, rk0, device=0):
        """`new NaiveBWTSearcher(bwt, bucketStarts, rk0)` (findex.scala:459-506): one merge block's BWT, the caller's
        bucket starts, row rk0 skipped."""
        L = _lib.load()
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        bs = np.ascontiguousarray(bucketStarts, dtype=np.int64)
        if bs.size != 256:
            raise ValueError("bucketStarts must have 256 entries")
        h = ctypes.c_void_p()
        _lib.check(L.fmx_open_block(_ptr(bwt), bwt.size, _ptr(bs), int(rk0), int(device), ctypes.byref(h)))
        return cls(_handle=h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.fmx_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- SuffixAlgo (findex.scala:9-52)
    def cf(self, c):
        if not 0 <= int(c) < 256:
            raise IndexError("symbol %r (reference: ArrayIndexOutOfBoundsException)" % (c,))
        return int(self.bucketStarts[int(c)])

    def occ(self, c, i):
        if not 0 <= int(c) < 256:
            raise IndexError("symbol %r (reference: ArrayIndexOutOfBoundsException)" % (c,))
        return int(self.occ_batch(np.array([c], dtype=np.uint8), np.array([i], dtype=np.int64))[0])

    def search(self, pat):
        pat = bytes(pat)
        sp, ep = self.search_batch(np.frombuffer(pat, dtype=np.uint8), np.array([0, len(pat)], dtype=np.uint64))
        return (int(sp[0]), int(ep[0])) if sp[0] < ep[0] else None

    def getPrevRange(self, sp, ep, c):
        if not 0 <= int(c) < 256:
            raise IndexError("symbol %r (reference: ArrayIndexOutOfBoundsException)" % (c,))
        a, b = self.prev_range_batch(np.array([sp], dtype=np.uint64), np.array([ep], dtype=np.uint64),
                                     np.array([c], dtype=np.uint8))
        return (int(a[0]), int(b[0])) if a[0] < b[0] else None

    def getIntervalPrevRange(self, sp, ep, cstart, cend):
        k = max(int(cend) - int(cstart) + 1, 1)
        osp = np.zeros(k, dtype=np.uint64)
        oep = np.zeros(k, dtype=np.uint64)
        n_out = ctypes.c_size_t()
        _lib.check(self._L.fmx_interval_prev_range(self._h, int(sp), int(ep), int(cstart), int(cend), _ptr(osp),
                                                   _ptr(oep), None, ctypes.byref(n_out)))
        return [(int(osp[j]), int(oep[j])) for j in range(n_out.value)]

    # ---- NaiveFMSearcher walkers (bwtmerger.scala:376-419)
    def getPrevI(self, i):
        _, end = self.lf_walk_batch(np.array([i], dtype=np.uint64), 1, want_bytes=False)
        return int(end[0])

    def getNextI(self, i):
        return int(self.psi_batch(np.array([i], dtype=np.uint64))[0])

    def bwt_read(self, i):
        """BWTLoader.read (bwtmerger.scala:155-162): 0 at the EOF slot."""
        b, _ = self.lf_walk_batch(np.array([i], dtype=np.uint64), 1)
        return int(b[0, 0])

    def nextSubstr(self, sp, length):
        out = np.zeros(max(int(length), 1), dtype=np.uint8)
        w = ctypes.c_uint32()
        _lib.check(self._L.fmx_next_substr(self._h, int(sp), int(length), _ptr(out), ctypes.byref(w)))
        return bytes(out[: w.value])

    def nextSubstr_batch(self, rows, length):
        """nextSubstr for many rows in one call -> list of bytes (what SAResult.toString prints per result)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros((rows.size, max(int(length), 1)), dtype=np.uint8)
        w = np.zeros(max(rows.size, 1), dtype=np.uint32)
        _lib.check(self._L.fmx_next_substr_batch(self._h, _ptr(rows), rows.size, int(length), _ptr(out), _ptr(w)))
        if int(length) == 0:
            return [b""] * rows.size
        flat = out.reshape(-1)
        return [bytes(flat[q * int(length): q * int(length) + int(w[q])]) for q in range(rows.size)]

    def prevSubstr(self, sp, length):
        out = np.zeros(max(int(length), 1), dtype=np.uint8)
        _lib.check(self._L.fmx_prev_substr(self._h, int(sp), int(length), _ptr(out)))
        return bytes(out[: int(length)])

    @staticmethod
    def search_batch_multi(searchers, pat, off):
        """fmx_search_batch_multi: one process, one replica handle per GPU; the batch is cut by pattern bytes."""
        pat = np.ascontiguousarray(pat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = off.size - 1
        sp = np.zeros(max(k, 0), dtype=np.uint64)
        ep = np.zeros(max(k, 0), dtype=np.uint64)
        arr = (ctypes.c_void_p * len(searchers))(*[s._h for s in searchers])
        _lib.check(_lib.load().fmx_search_batch_multi(arr, len(searchers), _ptr(pat), _ptr(off), _ptr(sp), _ptr(ep), max(k, 0)))
        return sp, ep

    def extract(self, row, length, direction=1):
        """fmx_extract: direction > 0 = nextSubstr, < 0 = prevSubstr."""
        out = np.zeros(max(int(length), 1), dtype=np.uint8)
        w = ctypes.c_uint32()
        _lib.check(self._L.fmx_extract(self._h, int(row), int(length), int(direction), _ptr(out), ctypes.byref(w)))
        return bytes(out[: w.value])

    def write_fm(self, path):
        """FMCreator.create (bwtmerger.scala:452-532): write the reference's .fm file."""
        _lib.check(self._L.fmx_write_fm(self._h, str(path).encode()))

    # ---- locate: SALoader / SACreator (bwtmerger.scala:214-249,535-556), Util.bwtFm2sa (util.scala:213-224)
    def locate(self, rows):
        """fmx_locate_batch: SA[row] for each row (the position in reverse(text) + sentinel of the row's suffix)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(rows.size, dtype=np.uint64)
        _lib.check(self._L.fmx_locate_batch(self._h, _ptr(rows), rows.size, _ptr(out)))
        return out

    def locate_dev(self, d_rows, k, d_out, stream=0):
        """fmx_locate_batch_dev: device pointers; a row >= n gets UINT64_MAX."""
        _lib.check(self._L.fmx_locate_batch_dev(self._h, _dp(d_rows), int(k), _dp(d_out), _dp(stream)))

    def locate_intervals(self, sp, ep, max_per=None):
        """fmx_locate_intervals: (off, pos) -- interval i's positions are pos[off[i]:off[i + 1]], rows sp[i] ..
        sp[i] + min(ep[i] - sp[i], max_per) - 1 in row order."""
        sp = np.ascontiguousarray(sp, dtype=np.uint64)
        ep = np.ascontiguousarray(ep, dtype=np.uint64)
        if sp.size != ep.size:
            raise ValueError("sp and ep differ in length")
        cnt = np.where(ep > sp, ep - sp, 0).astype(np.uint64)
        if max_per is not None:
            cnt = np.minimum(cnt, np.uint64(max_per))
        cap = int(cnt.sum())
        off = np.zeros(sp.size + 1, dtype=np.uint64)
        pos = np.zeros(max(cap, 1), dtype=np.uint64)
        _lib.check(self._L.fmx_locate_intervals(self._h, _ptr(sp), _ptr(ep), sp.size, int(max_per or 0), _ptr(off),
                                                _ptr(pos), cap))
        return off, pos[:cap]

    def locate_intervals_dev(self, d_sp, d_ep, k, d_off, d_pos, cap, max_per=None, stream=0):
        """fmx_locate_intervals_dev: d_off gets k + 1 offsets (d_off[k] = the total, which may exceed cap)."""
        _lib.check(self._L.fmx_locate_intervals_dev(self._h, _dp(d_sp), _dp(d_ep), int(k), int(max_per or 0), _dp(d_off),
                                                    _dp(d_pos), int(cap), _dp(stream)))

    @staticmethod
    def text_offsets(sa, n, m):
        """Where a text string of length m begins in the indexed text, for the SA values of the rows a search for its
        reverse found: n - 1 - SA - m (the index holds reverse(text) + sentinel, n = len(text) + 1 rows)."""
        sa = np.asarray(sa, dtype=np.uint64)
        return (np.uint64(n - 1 - m) - sa).astype(np.uint64) if sa.size else sa.astype(np.uint64)

    def locate_text(self, q, max_hits=None):
        """Sorted text offsets of the occurrences of q (overlapping ones included) -- at most max_hits of them."""
        q = bytes(q)
        if not q:
            raise ValueError("empty pattern")
        r = self.search(q[::-1])
        if r is None:
            return np.zeros(0, dtype=np.uint64)
        sp, ep = r
        if max_hits is not None:
            ep = min(ep, sp + int(max_hits))
        pos = self.locate(np.arange(sp, ep, dtype=np.uint64))
        return np.sort(self.text_offsets(pos, self.n, len(q)))

    def locate_info(self):
        """fmx_locate_info: (rate, device bytes, build ms) of the locate samples; 0 bytes when not built."""
        rate, nbytes, ms = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
        _lib.check(self._L.fmx_locate_info(self._h, ctypes.byref(rate), ctypes.byref(nbytes), ctypes.byref(ms)))
        return int(rate.value), int(nbytes.value), float(ms.value)

    def write_sa(self, path):
        """SACreator.create (bwtmerger.scala:535-556): write the reference's X.sa (n big-endian int32)."""
        _lib.check(self._L.fmx_write_sa(self._h, str(path).encode()))

    # ---- LCP: LCPSuffixWalkingAlgo.getLCP (findex.scala:59-62), LCPLoader / LCPCreator (bwtmerger.scala:176-211,558-652)
    def getLCP(self, i):
        """LCPSuffixWalkingAlgo.getLCP(i): the longest common prefix of the suffixes of rows i and i + 1 (0 for the last row)."""
        return int(self.lcp([int(i)])[0])

    def lcp(self, rows=None):
        """fmx_lcp_batch: LCP[row] for each row (uint32); rows=None: the whole array (fmx_lcp_range, LCPLoader.readAll)."""
        if rows is None:
            out = np.zeros(self.n, dtype=np.uint32)
            _lib.check(self._L.fmx_lcp_range(self._h, 0, self.n, _ptr(out)))
            return out
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(rows.size, dtype=np.uint32)
        _lib.check(self._L.fmx_lcp_batch(self._h, _ptr(rows), rows.size, _ptr(out)))
        return out

    def lcp_dev(self, d_rows, k, d_out, stream=0):
        """fmx_lcp_batch_dev: device pointers (u64 rows, u32 out); a row >= n gets UINT32_MAX."""
        _lib.check(self._L.fmx_lcp_batch_dev(self._h, _dp(d_rows), int(k), _dp(d_out), _dp(stream)))

    def lcp_range_dev(self, first, count, d_out, stream=0):
        """fmx_lcp_range_dev: LCP[first .. first + count) into device memory (u32)."""
        _lib.check(self._L.fmx_lcp_range_dev(self._h, int(first), int(count), _dp(d_out), _dp(stream)))

    def lcp_info(self):
        """fmx_lcp_info: (device bytes, build ms, largest entry, the first row that holds it, sum of all entries); 0 bytes
        when the array is not built."""
        nbytes, ms, mx, row, total = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_lcp_info(self._h, ctypes.byref(nbytes), ctypes.byref(ms), ctypes.byref(mx), ctypes.byref(row),
                                        ctypes.byref(total)))
        return int(nbytes.value), float(ms.value), int(mx.value), int(row.value), int(total.value)

    def write_lcp(self, path):
        """LCPCreator.create (bwtmerger.scala:558-652): write the reference's X.lcp (n - 1 big-endian int32)."""
        _lib.check(self._L.fmx_write_lcp(self._h, str(path).encode()))

    @staticmethod
    def _csr_hits(entry, args, k, dtype, cap):
        """entry(*args, out_off, hits, cap, &n_out) -> (out_off[k + 1], hits[:n_out]).  cap=None: a counting call with no room
        at all first; FMX_ERR_OVERFLOW then leaves the exact total in n_out, which sizes the buffer of the second call."""
        n_out = ctypes.c_size_t()
        out_off = np.zeros(k + 1, dtype=np.uint64)
        if cap is None:
            rc = entry(*args, _ptr(out_off), None, 0, ctypes.byref(n_out))
            if rc != _lib.FMX_ERR_OVERFLOW:
                _lib.check(rc)
                return out_off, np.zeros(0, dtype=dtype)
            cap = int(n_out.value)
        hits = np.zeros(max(int(cap), 1), dtype=dtype)
        _lib.check(entry(*args, _ptr(out_off), _ptr(hits), int(cap), ctypes.byref(n_out)))
        return out_off, hits[: int(n_out.value)]

    # ---- approximate search: up to three substituted bytes (fmx_search_approx_batch)
    APPROX_HIT = np.dtype([("pattern", np.uint32), ("mismatches", np.uint32), ("sp", np.uint64), ("ep", np.uint64)])

    @staticmethod
    def _approx_opts(max_mismatches, sub):
        lo, hi = (int(sub[0]), int(sub[1]))
        if not (0 <= lo <= 255 and 0 <= hi <= 255 and 0 <= int(max_mismatches) < 2 ** 32):
            raise ValueError("max_mismatches or sub out of range")
        return _lib.fmx_approx_opts(int(max_mismatches), lo, hi, 0)

    def search_approx_batch(self, pat, off, max_mismatches, sub=(1, 255), cap=None):
        """fmx_search_approx_batch: every string within max_mismatches (0 .. 3) substitutions of each pattern that occurs,
        the substituted bytes taken from sub = (lo, hi).  -> (off[k + 1], hits): pattern q's hits are
        hits[off[q]:off[q + 1]], a structured array (pattern, mismatches, sp, ep) by ascending sp.  cap=None: a counting
        call sizes the buffer; with a cap that is too small the library's FMX_ERR_OVERFLOW is raised."""
        pat = np.ascontiguousarray(pat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = max(off.size - 1, 0)
        opts = self._approx_opts(max_mismatches, sub)
        return self._csr_hits(self._L.fmx_search_approx_batch, (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts)), k,
                              self.APPROX_HIT, cap)

    def search_approx(self, pat, max_mismatches, sub=(1, 255)):
        """One pattern: the list of (sp, ep, mismatches), by ascending sp."""
        pat = bytes(pat)
        _, hits = self.search_approx_batch(np.frombuffer(pat, dtype=np.uint8), np.array([0, len(pat)], dtype=np.uint64),
                                           max_mismatches, sub)
        return [(int(h["sp"]), int(h["ep"]), int(h["mismatches"])) for h in hits]

    def search_approx_batch_dev(self, d_pat, d_off, k, max_mismatches, d_out_off, d_out, cap, sub=(1, 255), stream=0):
        """fmx_search_approx_batch_dev: device pointers (u8 patterns, u64 offsets[k + 1], u64 out_off[k + 1], 24-byte hit
        records); allocates and synchronises.  -> the exact number of hits (FMX_ERR_OVERFLOW is raised when it exceeds cap)."""
        opts = self._approx_opts(max_mismatches, sub)
        n_out = ctypes.c_size_t()
        _lib.check(self._L.fmx_search_approx_batch_dev(self._h, _dp(d_pat), _dp(d_off), int(k), ctypes.byref(opts), _dp(d_out_off),
                                                       _dp(d_out), int(cap), ctypes.byref(n_out), _dp(stream)))
        return int(n_out.value)

    def approx_last(self):
        """fmx_approx_last: (search kernel ms, ordering ms, backward steps, rank-dictionary requests) of this thread's last
        approximate search."""
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_approx_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return float(a.value), float(b.value), int(c.value), int(d.value)

    # ---- approximate search with insertions and deletions: edit distance up to two (fmx_search_edit_batch)
    EDIT_HIT = np.dtype([("pattern", np.uint32), ("edits", np.uint16), ("len", np.uint16), ("sp", np.uint64), ("ep", np.uint64)])

    @staticmethod
    def _edit_opts(max_edits, sub):
        lo, hi = (int(sub[0]), int(sub[1]))
        if not (0 <= lo <= 255 and 0 <= hi <= 255 and 0 <= int(max_edits) < 2 ** 32):
            raise ValueError("max_edits or sub out of range")
        return _lib.fmx_edit_opts(int(max_edits), lo, hi, 0)

    def search_edit_batch(self, pat, off, max_edits, sub=(1, 255), cap=None):
        """fmx_search_edit_batch: every string within max_edits (0 .. 2) substitutions, insertions and deletions of each
        pattern (at most 255 bytes) that occurs, the substituted and inserted bytes taken from sub = (lo, hi).
        -> (off[k + 1], hits): pattern q's hits are hits[off[q]:off[q + 1]], a structured array (pattern, edits, len, sp,
        ep) by ascending (sp, len); len is the length of the string that occurs.  cap=None: a counting call sizes the
        buffer; with a cap that is too small the library's FMX_ERR_OVERFLOW is raised."""
        pat = np.ascontiguousarray(pat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = max(off.size - 1, 0)
        opts = self._edit_opts(max_edits, sub)
        return self._csr_hits(self._L.fmx_search_edit_batch, (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts)), k,
                              self.EDIT_HIT, cap)

    def search_edit(self, pat, max_edits, sub=(1, 255)):
        """One pattern: the list of (sp, ep, len, edits), by ascending (sp, len)."""
        pat = bytes(pat)
        _, hits = self.search_edit_batch(np.frombuffer(pat, dtype=np.uint8), np.array([0, len(pat)], dtype=np.uint64),
                                         max_edits, sub)
        return [(int(h["sp"]), int(h["ep"]), int(h["len"]), int(h["edits"])) for h in hits]

    def search_edit_batch_dev(self, d_pat, d_off, k, max_edits, d_out_off, d_out, cap, sub=(1, 255), stream=0):
        """fmx_search_edit_batch_dev: device pointers (u8 patterns, u64 offsets[k + 1], u64 out_off[k + 1], 24-byte hit
        records); allocates and synchronises.  -> the exact number of hits (FMX_ERR_OVERFLOW is raised when it exceeds cap)."""
        opts = self._edit_opts(max_edits, sub)
        n_out = ctypes.c_size_t()
        _lib.check(self._L.fmx_search_edit_batch_dev(self._h, _dp(d_pat), _dp(d_off), int(k), ctypes.byref(opts), _dp(d_out_off),
                                                     _dp(d_out), int(cap), ctypes.byref(n_out), _dp(stream)))
        return int(n_out.value)

    def edit_last(self):
        """fmx_edit_last: (search kernel ms, ordering ms, backward steps, rank-dictionary requests) of this thread's last
        edit-distance search."""
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_edit_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return float(a.value), float(b.value), int(c.value), int(d.value)

    def locate_text_edits(self, q, max_edits, max_hits=None):
        """Where strings within max_edits edits of the text string q stand in the indexed text: rows (text offset, len,
        edits) of a uint64 array sorted by (offset, len) -- the reverse of q is searched and every hit's rows are located
        with the hit's own len (text_offsets); max_hits bounds the rows taken of every distinct matching string.  A stretch
        of the text may appear with several lengths."""
        q = bytes(q)
        _, hits = self.search_edit_batch(np.frombuffer(q[::-1], dtype=np.uint8), np.array([0, len(q)], dtype=np.uint64), max_edits)
        off, sa = self.locate_intervals(hits["sp"], hits["ep"], max_per=max_hits)
        per = np.diff(off).astype(np.int64)
        out = np.zeros((sa.size, 3), dtype=np.uint64)
        out[:, 1] = np.repeat(hits["len"], per)
        out[:, 2] = np.repeat(hits["edits"], per)
        out[:, 0] = np.uint64(self.n - 1) - out[:, 1] - sa
        return out[np.lexsort((out[:, 1], out[:, 0]))]

    # ---- occurrences: (group, len, sp, ep) intervals as text positions (fmx_occurrences)
    RESULT = np.dtype([("regex", np.uint32), ("len", np.uint32), ("sp", np.uint64), ("ep", np.uint64)])
    OCCURRENCE = np.dtype([("group", np.uint32), ("len", np.uint32), ("pos", np.uint64), ("doc", np.uint32), ("raw_len", np.uint32),
                           ("raw_off", np.uint64)])
    OCC_MODES = {"all": _lib.FMX_OCC_ALL, "longest": _lib.FMX_OCC_LONGEST, "disjoint": _lib.FMX_OCC_DISJOINT}

    @classmethod
    def _occ_opts(cls, mode, max_per):
        if mode not in cls.OCC_MODES:
            raise ValueError("mode: all, longest or disjoint")
        if max_per is not None and not 0 < int(max_per) < 2 ** 64:
            raise ValueError("max_per out of range")
        return _lib.fmx_occ_opts(cls.OCC_MODES[mode], 0, int(max_per or 0))

    @classmethod
    def pack_records(cls, group, length, sp, ep):
        """The record array fmx_occurrences takes, from four arrays (or scalars for the first two)."""
        sp = np.asarray(sp, dtype=np.uint64).reshape(-1)
        rec = np.zeros(sp.size, dtype=cls.RESULT)
        rec["regex"], rec["len"], rec["sp"], rec["ep"] = group, length, sp, ep
        return rec

    def occurrences(self, records, n_groups=None, mode="all", max_per=None, corpus=None, cap=None):
        """fmx_occurrences: the text occurrences of (group, len, sp, ep) records (a RESULT array: what RegexBatch.match_raw
        returns, or pack_records of other hits), at most max_per rows of each, reduced by mode ("all": every distinct (pos,
        len) of a group, "longest": the longest at every pos, "disjoint": the leftmost non-overlapping reading of those).
        -> (off[n_groups + 1], occ): group g's occurrences are occ[off[g]:off[g + 1]], an OCCURRENCE array ascending by
        (pos, len).  corpus (a Corpus whose stream this index is of): occurrences that do not lie inside one document are
        dropped and the others carry doc, raw_off and raw_len.  n_groups=None: the largest group + 1.  cap=None: a counting
        call sizes the buffer; with a cap that is too small the library's FMX_ERR_OVERFLOW is raised."""
        rec = np.ascontiguousarray(records, dtype=self.RESULT).reshape(-1)
        if n_groups is None:
            n_groups = int(rec["regex"].max()) + 1 if rec.size else 1
        opts = self._occ_opts(mode, max_per)
        args = (self._h, corpus.handle if corpus is not None else None, _ptr(rec), rec.size, int(n_groups), ctypes.byref(opts))
        return self._csr_hits(self._L.fmx_occurrences, args, int(n_groups), self.OCCURRENCE, cap)

    def occurrences_dev(self, d_rec, k, n_groups, d_out_off, d_out, cap, mode="all", max_per=None, corpus=None, stream=0, grow=False):
        """fmx_occurrences_dev: device pointers (24-byte records, u64 out_off[n_groups + 1], 32-byte occurrences); allocates and
        synchronises.  -> the exact number of occurrences.  cap = 0 is the counting call; with any other cap that is too
        small FMX_ERR_OVERFLOW is raised -- unless grow is set: then the total comes back all the same, for the caller to
        compare with cap and call again."""
        opts = self._occ_opts(mode, max_per)
        n_out = ctypes.c_size_t()
        rc = self._L.fmx_occurrences_dev(self._h, corpus.handle if corpus is not None else None, _dp(d_rec), int(k), int(n_groups),
                                         ctypes.byref(opts), _dp(d_out_off), _dp(d_out), int(cap), ctypes.byref(n_out), _dp(stream))
        if not (rc == _lib.FMX_ERR_OVERFLOW and (int(cap) == 0 or grow)):
            _lib.check(rc)
        return int(n_out.value)

    def occurrences_last(self):
        """fmx_occurrences_last: (locate ms, keys and sort ms, selection ms, compaction ms, rows located) of this thread's
        last occurrences call."""
        t = [ctypes.c_double() for _ in range(4)]
        rows = ctypes.c_uint64()
        _lib.check(self._L.fmx_occurrences_last(*[ctypes.byref(x) for x in t], ctypes.byref(rows)))
        return tuple(float(x.value) for x in t) + (int(rows.value),)

    # ---- context: rows whose neighbouring text bytes are in a class -- whole words (fmx_context_filter)
    CTX_START = _lib.FMX_CTX_START

    def search_context_batch(self, pat, off, left, right, cap=None, fold=None, classes=None):
        """fmx_search_context_batch: the patterns as search_batch takes them (strings of reverse(text)), left / right = the byte
        values (bytes; 0 = the text begins / ends there) that may stand in front of / behind an occurrence in the TEXT.
        -> (off[k + 1], runs): pattern i's rows are the disjoint ranges runs[off[i]:off[i + 1]], a RESULT array {i, length,
        sp, ep} in ascending sp.  cap=None: a counting call sizes the buffer.  fold (a fold map, e.g. ASCII_FOLD):
        fmx_search_context_fold_batch -- every variant of a pattern under the map, the neighbours still compared as they are.
        classes (a class table (cls_off, mem_off, mem_bytes); pat then holds uint16 elements as search_classes_batch takes them):
        fmx_search_context_classes_batch -- every spelling under the table; a run's length is that of its spelling."""
        if fold is not None and classes is not None:
            raise ValueError("fold and classes do not combine")
        pat = np.ascontiguousarray(pat, dtype=np.uint16 if classes is not None else np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = off.size - 1
        if k < 0:
            raise ValueError("off needs at least one entry")
        opts = _lib.fmx_context_opts()
        for j, (lw, rw) in enumerate(zip(class_words(left), class_words(right))):
            opts.left[j], opts.right[j] = int(lw), int(rw)
        if fold is not None:
            fopts = self._fold_opts(fold)
            args = (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts), ctypes.byref(fopts))
            return self._csr_hits(self._L.fmx_search_context_fold_batch, args, k, self.RESULT, cap)
        if classes is not None:
            tab, keep = self._class_table(classes)
            args = (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts), ctypes.byref(tab))
            out = self._csr_hits(self._L.fmx_search_context_classes_batch, args, k, self.RESULT, cap)
            del keep
            return out
        args = (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts))
        return self._csr_hits(self._L.fmx_search_context_batch, args, k, self.RESULT, cap)

    def context_filter(self, records, right, mode=None, cap=None):
        """fmx_context_filter: the runs of rows of every (group, len, sp, ep) record whose following text byte is in `right`
        (byte values; 0 = the text ends there).  mode: None or one byte per record, lead | CTX_START.  -> (off[k + 1], runs):
        record j's runs are runs[off[j]:off[j + 1]], a RESULT array {group, len - lead, run_sp, run_ep}."""
        rec = np.ascontiguousarray(records, dtype=self.RESULT).reshape(-1)
        if mode is not None:
            mode = np.ascontiguousarray(mode, dtype=np.uint8).reshape(-1)
            if mode.size != rec.size:
                raise ValueError("mode: one byte per record")
        rw = class_words(right)
        args = (self._h, _ptr(rec), _ptr(mode) if mode is not None else None, rec.size, _ptr(rw))
        return self._csr_hits(self._L.fmx_context_filter, args, rec.size, self.RESULT, cap)

    def context_filter_dev(self, d_rec, d_mode, k, right, d_out_off, d_out, cap, stream=0, grow=False):
        """fmx_context_filter_dev: device pointers (24-byte records in and out, k mode bytes or 0, u64 out_off[k + 1]); allocates
        and synchronises.  -> the exact number of runs; cap = 0 is the counting call, grow as occurrences_dev."""
        rw = class_words(right)
        n_out = ctypes.c_size_t()
        rc = self._L.fmx_context_filter_dev(self._h, _dp(d_rec), _dp(d_mode), int(k), _ptr(rw), _dp(d_out_off), _dp(d_out), int(cap),
                                            ctypes.byref(n_out), _dp(stream))
        if not (rc == _lib.FMX_ERR_OVERFLOW and (int(cap) == 0 or grow)):
            _lib.check(rc)
        return int(n_out.value)

    def context_last(self):
        """fmx_context_last: (search ms, chain ms, ranges + count + scans + emit ms, rows tested, runs found) of this thread's
        last context call."""
        t = [ctypes.c_double() for _ in range(3)]
        rows, runs = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_context_last(*[ctypes.byref(x) for x in t], ctypes.byref(rows), ctypes.byref(runs)))
        return tuple(float(x.value) for x in t) + (int(rows.value), int(runs.value))

    def search_words(self, pats, word=WORD_BYTES, cap=None, fold=None, classes=None, keep=None):
        """The whole-word occurrences of text strings `pats` (bytes each): search_context_batch over their reverses with the
        boundary class of `word` on both sides.  -> (off[k + 1], runs).  fold: a fold map the strings are matched under.
        classes ("unicode", "marks", or a mapping code point -> members as unicode_fold.class_table takes): the strings are read
        as UTF-8 and matched in every spelling under the classes that occurs (unicode_table; keep: its filter on members)."""
        pats = [bytes(q) for q in pats]
        if classes is not None:
            if fold is not None:
                raise ValueError("fold and classes do not combine")
            el, el_off, table = self.unicode_table(pats, classes == "marks", keep, None if isinstance(classes, str) else classes)
            cls = boundary_class(word)
            return self.search_context_batch(el, el_off, cls, cls, cap, classes=table)
        off = np.zeros(len(pats) + 1, dtype=np.uint64)
        np.cumsum([len(q) for q in pats], out=off[1:])
        pat = np.frombuffer(b"".join(q[::-1] for q in pats), dtype=np.uint8)
        cls = boundary_class(word)
        return self.search_context_batch(pat, off, cls, cls, cap, fold=fold)

    def locate_words(self, q, max_hits=None, word=WORD_BYTES, fold=None, classes=None):
        """Sorted text offsets of the whole-word occurrences of q -- of at most max_hits rows.  fold: a fold map q is matched
        under.  classes (as search_words takes it): -> (offsets, lengths) sorted by both, every occurrence with the bytes of
        its spelling."""
        q = bytes(q)
        if not q:
            raise ValueError("empty pattern")
        if classes is not None:
            _, runs = self.search_words([q], word, classes=classes)
            return self.locate_spellings(runs, max_hits)
        _, runs = self.search_words([q], word, fold=fold)
        sp, ep = runs["sp"].copy(), runs["ep"].copy()
        if max_hits is not None:
            left = int(max_hits)
            for j in range(sp.size):
                ep[j] = min(int(ep[j]), int(sp[j]) + left)
                left -= int(ep[j]) - int(sp[j])
        _, pos = self.locate_intervals(sp, ep)
        return np.sort(self.text_offsets(pos, self.n, len(q)))

    # ---- case folding: literal search under a byte map (fmx_search_fold_batch)
    @staticmethod
    def _fold_opts(fold):
        opts = _lib.fmx_fold_opts()
        ctypes.memmove(opts.fold, check_fold(fold), 256)
        return opts

    def search_fold_batch(self, pat, off, fold=ASCII_FOLD, cap=None):
        """fmx_search_fold_batch: every string that equals a pattern under the fold map (256 bytes: a byte -> the representative
        of its class) and occurs.  The patterns are given as search_batch takes them.  -> (off[k + 1], hits): pattern q's
        hits are hits[off[q]:off[q + 1]], a RESULT array {q, length, sp, ep} by ascending sp -- disjoint row intervals.
        cap=None: a counting call sizes the buffer; with a cap that is too small the library's FMX_ERR_OVERFLOW is raised."""
        pat = np.ascontiguousarray(pat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = max(off.size - 1, 0)
        opts = self._fold_opts(fold)
        return self._csr_hits(self._L.fmx_search_fold_batch, (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts)), k, self.RESULT, cap)

    def search_fold(self, q, fold=ASCII_FOLD):
        """One pattern (as search takes it): the list of (sp, ep) of its variants under the map, by ascending sp."""
        q = bytes(q)
        _, hits = self.search_fold_batch(np.frombuffer(q, dtype=np.uint8), np.array([0, len(q)], dtype=np.uint64), fold)
        return [(int(h["sp"]), int(h["ep"])) for h in hits]

    def search_fold_batch_dev(self, d_pat, d_off, k, d_out_off, d_out, cap, fold=ASCII_FOLD, stream=0):
        """fmx_search_fold_batch_dev: device pointers (u8 patterns, u64 offsets[k + 1], u64 out_off[k + 1], 24-byte records);
        allocates and synchronises.  -> the exact number of hits (FMX_ERR_OVERFLOW is raised when it exceeds cap)."""
        opts = self._fold_opts(fold)
        n_out = ctypes.c_size_t()
        _lib.check(self._L.fmx_search_fold_batch_dev(self._h, _dp(d_pat), _dp(d_off), int(k), ctypes.byref(opts), _dp(d_out_off),
                                                     _dp(d_out), int(cap), ctypes.byref(n_out), _dp(stream)))
        return int(n_out.value)

    def fold_last(self):
        """fmx_fold_last: (search kernel ms, ordering ms, backward steps, rank-dictionary requests) of this thread's last
        fold search."""
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_fold_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return float(a.value), float(b.value), int(c.value), int(d.value)

    def locate_fold(self, q, max_hits=None, fold=ASCII_FOLD):
        """Sorted text offsets of the occurrences of the text string q under the map (overlapping ones included) -- of at most
        max_hits rows, taken in row order."""
        q = bytes(q)
        if not q:
            raise ValueError("empty pattern")
        hits = self.search_fold(q[::-1], fold)
        sp = np.array([h[0] for h in hits], dtype=np.uint64)
        ep = np.array([h[1] for h in hits], dtype=np.uint64)
        if max_hits is not None:
            left = int(max_hits)
            for j in range(sp.size):
                ep[j] = min(int(ep[j]), int(sp[j]) + left)
                left -= int(ep[j]) - int(sp[j])
        _, pos = self.locate_intervals(sp, ep)
        return np.sort(self.text_offsets(pos, self.n, len(q)))

    # ---- string classes: a pattern position as a set of byte strings, UTF-8 case folding (fmx_search_classes_batch)
    @staticmethod
    def _class_table(table):
        """fmx_class_table of (cls_off, mem_off, mem_bytes) -- None: no classes -- and the arrays it points into."""
        if table is None:
            return None, ()
        cls_off, mem_off, mem_bytes = table
        keep = (np.ascontiguousarray(cls_off, dtype=np.uint64), np.ascontiguousarray(mem_off, dtype=np.uint64),
                np.ascontiguousarray(mem_bytes, dtype=np.uint8))
        if keep[0].size < 1 or keep[1].size < 1:
            raise ValueError("a class table has at least one offset in cls_off and in mem_off")
        tab = _lib.fmx_class_table()
        tab.cls_off, tab.mem_off, tab.mem_bytes = (a.ctypes.data for a in keep)
        tab.n_classes = keep[0].size - 1
        return tab, keep

    def search_classes_batch(self, el, off, table, cap=None):
        """fmx_search_classes_batch: patterns of uint16 elements (< 256: that byte, else class element - 256 of the table) with
        offsets off[k + 1]; table = (cls_off, mem_off, mem_bytes) or None.  Elements and member bytes are given as search_batch
        takes a pattern: for a text string, reversed (unicode_fold.class_table does both).  -> (off[k + 1], hits): pattern q's
        hits are hits[off[q]:off[q + 1]], a RESULT array {q, bytes of the spelling, sp, ep} by ascending sp -- disjoint row
        intervals.  cap=None: a counting call sizes the buffer."""
        el = np.ascontiguousarray(el, dtype=np.uint16)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = max(off.size - 1, 0)
        tab, keep = self._class_table(table)
        args = (self._h, _ptr(el), _ptr(off), k, ctypes.byref(tab) if tab is not None else None)
        out = self._csr_hits(self._L.fmx_search_classes_batch, args, k, self.RESULT, cap)
        del keep
        return out

    def search_classes(self, elements, table):
        """One pattern of elements: the list of (bytes of the spelling, sp, ep) of its spellings that occur, by ascending sp."""
        el = np.ascontiguousarray(elements, dtype=np.uint16).reshape(-1)
        _, hits = self.search_classes_batch(el, np.array([0, el.size], dtype=np.uint64), table)
        return [(int(h["len"]), int(h["sp"]), int(h["ep"])) for h in hits]

    def search_classes_batch_dev(self, d_el, d_off, k, d_out_off, d_out, cap, table, stream=0):
        """fmx_search_classes_batch_dev: device pointers (u16 elements, u64 offsets[k + 1], u64 out_off[k + 1], 24-byte records),
        the table in host memory as search_classes_batch takes it; allocates and synchronises.  -> the exact number of hits
        (FMX_ERR_OVERFLOW is raised when it exceeds cap)."""
        tab, keep = self._class_table(table)
        n_out = ctypes.c_size_t()
        _lib.check(self._L.fmx_search_classes_batch_dev(self._h, _dp(d_el), _dp(d_off), int(k), ctypes.byref(tab) if tab is not None else None,
                                                        _dp(d_out_off), _dp(d_out), int(cap), ctypes.byref(n_out), _dp(stream)))
        del keep
        return int(n_out.value)

    def classes_last(self):
        """fmx_classes_last: (search kernel ms, ordering ms, backward steps, rank-dictionary requests) of this thread's last
        class search."""
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_classes_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return float(a.value), float(b.value), int(c.value), int(d.value)

    def unicode_table(self, patterns, ignore_marks=False, keep=None, classes=None):
        """unicode_fold.class_table of text strings under UTF-8 case folding (ignore_marks: precomposed accented letters too),
        pruned for this index: the distinct members are searched once with search_batch, and those that do not occur -- or that
        `keep` (member bytes -> bool) turns down -- are dropped.  -> (el, el_off, (cls_off, mem_off, mem_bytes))."""
        from . import unicode_fold
        if classes is None:
            classes = unicode_fold.mark_classes() if ignore_marks else unicode_fold.case_classes()
        members = [m for m in unicode_fold.members_of(patterns, classes) if keep is None or keep(m)]
        occurring = set()
        if members:
            off = np.zeros(len(members) + 1, dtype=np.uint64)
            np.cumsum([len(m) for m in members], out=off[1:])
            sp, ep = self.search_batch(np.frombuffer(b"".join(m[::-1] for m in members), dtype=np.uint8), off)
            occurring = {m for m, a, b in zip(members, sp.tolist(), ep.tolist()) if a < b}
        el, el_off, cls_off, mem_off, mem_bytes = unicode_fold.class_table(patterns, classes, occurring)
        return el, el_off, (cls_off, mem_off, mem_bytes)

    def locate_classes(self, q, max_hits=None, ignore_marks=False):
        """Sorted text offsets of the occurrences of the text string q (raw bytes, read as UTF-8) in every case spelling that
        occurs -- of at most max_hits rows, taken in row order.  -> (offsets, lengths): a spelling may be longer or shorter
        than q (k / U+212A), so every occurrence comes with its bytes."""
        q = bytes(q)
        if not q:
            raise ValueError("empty pattern")
        el, el_off, table = self.unicode_table([q], ignore_marks)
        _, hits = self.search_classes_batch(el, el_off, table)
        return self.locate_spellings(hits, max_hits)

    def locate_spellings(self, hits, max_hits=None):
        """Where the strings of RESULT records {.., len, sp, ep} of different lengths begin in the indexed text: the rows located
        (at most max_hits of them, taken in record order) and each position worked out with its record's own len.
        -> (offsets, lengths), sorted by both."""
        sp, ep = hits["sp"].copy(), hits["ep"].copy()
        if max_hits is not None:
            left = int(max_hits)
            for j in range(sp.size):
                ep[j] = min(int(ep[j]), int(sp[j]) + left)
                left -= int(ep[j]) - int(sp[j])
        off, pos = self.locate_intervals(sp, ep)
        lens = np.repeat(hits["len"].astype(np.uint64), np.diff(off.astype(np.int64)))
        at = (np.uint64(self.n - 1) - pos - lens).astype(np.uint64) if pos.size else pos.astype(np.uint64)
        order = np.lexsort((lens, at))
        return at[order], lens[order]

    def _finditer_words(self, regexes, word, mode, max_steps, max_per, lineOnly, corpus, match_cap, occ_cap):
        """finditer(words=True): one batch of 2k.  Regex i becomes (cls)(re) -- cls = the boundary bytes >= 1 that occur in the
        index (counts()), each backslash-quoted, as an alternation: neither engine of fmx_regex.cpp has a case for a [..] set
        in front of a group, and none has a negated class -- and regex k + i becomes (re), for a match at text offset 0.  They
        are compiled by REParser.createNFA: ReTree has no case for a group behind an alternation either (ConcatPoint,
        retree.scala:240-295), and its paths stop at their first accepting state, so that a+n? would never reach the n.
        The records of the 2k go to HBM, lead 1 for the first k and CTX_START for the rest, the group folded to i; then the
        context filter (the byte behind), then the occurrences."""
        import torch
        from .regex import NFA, RegexBatch

        res = [r if isinstance(r, str) else bytes(r).decode("latin-1") for r in regexes]
        k = len(res)
        counts = self.counts()
        bnd = boundary_class(word)
        cls = "|".join("\\" + chr(c) for c in bnd if c >= 1 and counts[c] > 0)
        both = (["(" + cls + ")(" + r + ")" for r in res] if cls else []) + ["(" + r + ")" for r in res]
        n_lead = k if cls else 0
        batch = RegexBatch(self, [NFA(_NfaSource(r, lineOnly)) for r in both])
        dev = ctypes.c_int()
        _lib.check(self._L.fmx_device(self._h, ctypes.byref(dev)))
        dev = torch.device("cuda", dev.value)
        cap = int(match_cap)
        while True:
            d_res = torch.empty(3 * cap, dtype=torch.int64, device=dev)
            try:
                n_res = batch.match_dev(d_res.data_ptr(), cap, max_steps=max_steps + 1 if max_steps else 0)
                break
            except _lib.FmxError as e:
                if e.code != _lib.FMX_ERR_OVERFLOW or "result buffer" not in str(e) or cap >= 1 << 28:
                    raise
                cap *= 4
        kk = max(k, 1)
        rec = d_res[: 3 * n_res].view(n_res, 3)
        grp = rec[:, 0] & 0xFFFFFFFF
        lead = grp < n_lead
        d_mode = torch.where(lead, 1, self.CTX_START).to(torch.uint8).contiguous()
        rec[:, 0] += (grp % kk) - grp if n_res else 0             # the group folded to i: every block of k is the k regexes
        torch.cuda.synchronize(dev)
        d_roff = torch.empty(n_res + 1, dtype=torch.int64, device=dev)
        room = max(n_res, 1)
        d_run = torch.empty(3 * room, dtype=torch.int64, device=dev)
        n_run = self.context_filter_dev(d_res.data_ptr(), d_mode.data_ptr(), n_res, bnd, d_roff.data_ptr(), d_run.data_ptr(), room, grow=True)
        if n_run > room:
            d_run = torch.empty(3 * n_run, dtype=torch.int64, device=dev)
            self.context_filter_dev(d_res.data_ptr(), d_mode.data_ptr(), n_res, bnd, d_roff.data_ptr(), d_run.data_ptr(), n_run)
        d_off = torch.empty(kk + 1, dtype=torch.int64, device=dev)
        room = int(occ_cap)
        d_occ = torch.empty(4 * max(room, 1), dtype=torch.int64, device=dev)
        total = self.occurrences_dev(d_run.data_ptr(), n_run, kk, d_off.data_ptr(), d_occ.data_ptr(), room, mode, max_per, corpus, grow=True)
        if total > room:
            d_occ = torch.empty(4 * total, dtype=torch.int64, device=dev)
            self.occurrences_dev(d_run.data_ptr(), n_run, kk, d_off.data_ptr(), d_occ.data_ptr(), total, mode, max_per, corpus)
        off = d_off.cpu().numpy().view(np.uint64)
        occ = d_occ[: 4 * total].cpu().numpy().view(self.OCCURRENCE)
        return off, occ, bool(batch.truncated)

    def finditer(self, regexes, mode="disjoint", max_steps=0, max_per=None, lineOnly=False, corpus=None, match_cap=1 << 20,
                 occ_cap=1 << 20, words=False, word=WORD_BYTES, ignore_case=False):
        """Where a batch of regexes matches the indexed text: (off, occ, truncated) -- regex i's matches are
        occ[off[i]:off[i + 1]] (an OCCURRENCE array ascending by (pos, len)), truncated = the match was cut at max_steps
        (FMX_TRUNCATED).  regexes: strings (compiled here; lineOnly as ReTree.compile_batch), a CompiledRegexes set or a
        resident RegexBatch of this searcher.  The batch is matched into device memory (fmx_regex_batch_match_dev; match_cap
        records to begin with, four times as many after every overflow), fmx_occurrences_dev reads the results there (with room for
        occ_cap occurrences, and once more with the exact room when that was too little), and offsets and occurrences come down
        in one copy each: between the two calls only counts cross the link.  The device
        buffers are torch tensors.  words=True (regex strings only): whole-word matches -- the bytes next to a match are not
        in `word`, or the text ends there; the neighbours are not part of the match.  ignore_case=True (regex strings only):
        every regex is rewritten by regex.fold_regex under ASCII_FOLD and compiled by REParser.createNFA (ReTree has no case
        for a set next to a group), so that it is read as Python's re reads it under re.IGNORECASE | re.ASCII -- but for \\w,
        \\d and '.', which keep re2post's meaning (the bytes A .. y, 0 .. 8 and 2 .. 254; \\w gets z, the image of Z, beside it);
        a construct re reads differently is refused with ValueError.  ignore_case="unicode" (regex strings as str): rewritten by
        regex.fold_regex_unicode instead -- UTF-8 case folding, a character as the alternation of its class's byte strings."""
        import torch
        from .regex import CompiledRegexes, NFA, RegexBatch, ReTree, fold_regex, fold_regex_unicode
        if ignore_case:
            if isinstance(regexes, (RegexBatch, CompiledRegexes)):
                raise ValueError("finditer(ignore_case=True) takes regex strings: it rewrites each before it is compiled")
            regexes = [fold_regex_unicode(r) if ignore_case == "unicode" else fold_regex(r, ASCII_FOLD) for r in regexes]
            if not words:
                regexes = RegexBatch(self, [NFA(_NfaSource(r, lineOnly)) for r in regexes])
        if words:
            if isinstance(regexes, (RegexBatch, CompiledRegexes)):
                raise ValueError("finditer(words=True) takes regex strings: it compiles each with its left context")
            return self._finditer_words(list(regexes), word, mode, max_steps, max_per, lineOnly, corpus, match_cap, occ_cap)
        if isinstance(regexes, RegexBatch):
            batch = regexes
        else:
            batch = RegexBatch(self, regexes if isinstance(regexes, CompiledRegexes) else ReTree.compile_batch(list(regexes), lineOnly))
        dev = ctypes.c_int()
        _lib.check(self._L.fmx_device(self._h, ctypes.byref(dev)))
        dev = torch.device("cuda", dev.value)
        k, cap = max(batch.k, 1), int(match_cap)
        while True:
            d_res = torch.empty(3 * cap, dtype=torch.int64, device=dev)
            try:
                n_res = batch.match_dev(d_res.data_ptr(), cap, max_steps=max_steps)
                break
            except _lib.FmxError as e:
                if e.code != _lib.FMX_ERR_OVERFLOW or "result buffer" not in str(e) or cap >= 1 << 28:
                    raise
                cap *= 4
        d_off = torch.empty(k + 1, dtype=torch.int64, device=dev)
        room = int(occ_cap)
        d_occ = torch.empty(4 * max(room, 1), dtype=torch.int64, device=dev)
        total = self.occurrences_dev(d_res.data_ptr(), n_res, k, d_off.data_ptr(), d_occ.data_ptr(), room, mode, max_per, corpus, grow=True)
        if total > room:                                 # too little room: the call said how much it takes
            d_occ = torch.empty(4 * total, dtype=torch.int64, device=dev)
            self.occurrences_dev(d_res.data_ptr(), n_res, k, d_off.data_ptr(), d_occ.data_ptr(), total, mode, max_per, corpus)
        off = d_off.cpu().numpy().view(np.uint64)
        occ = d_occ[: 4 * total].cpu().numpy().view(self.OCCURRENCE)
        return off, occ, bool(batch.truncated)

    # ---- lines: text position -> line, occurrences -> the distinct lines that hold them (fmx_lines_batch)
    LINE_HIT = np.dtype(_lib.LINE_HIT)
    NO_LINE = (1 << 64) - 1

    def lines_prepare(self, breaks=b"\n"):
        """fmx_lines_prepare: build the line table for the break set `breaks` (1 .. 4 distinct non-zero bytes); an equal set
        does nothing, another set rebuilds."""
        b = np.frombuffer(bytes(breaks), dtype=np.uint8)
        _lib.check(self._L.fmx_lines_prepare(self._h, _ptr(b) if b.size else None, b.size))

    def lines_info(self):
        """fmx_lines_info: (breaks found, break set as bytes, shift S, device bytes, build ms) of the line table; 0 breaks,
        0 bytes and the default set when not built."""
        nb, ns, sh, by, ms = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
        st = (ctypes.c_uint8 * 4)()
        _lib.check(self._L.fmx_lines_info(self._h, ctypes.byref(nb), ctypes.cast(st, ctypes.c_void_p), ctypes.byref(ns), ctypes.byref(sh),
                                          ctypes.byref(by), ctypes.byref(ms)))
        return int(nb.value), bytes(st[: ns.value]), int(sh.value), int(by.value), float(ms.value)

    def line_of(self, pos):
        """fmx_lines_batch: (line, start, end) arrays for text positions: the 0-based global line index and the line's
        [start, end) without its break byte; NO_LINE in all three for a position at or past the text's end."""
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        out = [np.zeros(pos.size, dtype=np.uint64) for _ in range(3)]
        _lib.check(self._L.fmx_lines_batch(self._h, _ptr(pos), pos.size, *[_ptr(o) for o in out]))
        return tuple(out)

    def line_of_dev(self, d_pos, k, d_line=0, d_start=0, d_end=0, stream=0):
        """fmx_lines_batch_dev: device pointers (u64 throughout; an output of 0 is left out); with the table built it only
        enqueues."""
        _lib.check(self._L.fmx_lines_batch_dev(self._h, _dp(d_pos), int(k), _dp(d_line), _dp(d_start), _dp(d_end), _dp(stream)))

    def line_spans(self, lines):
        """fmx_line_spans: (start, end) arrays for global line indices; NO_LINE past the last line."""
        lines = np.ascontiguousarray(lines, dtype=np.uint64).reshape(-1)
        out = [np.zeros(lines.size, dtype=np.uint64) for _ in range(2)]
        _lib.check(self._L.fmx_line_spans(self._h, _ptr(lines), lines.size, *[_ptr(o) for o in out]))
        return tuple(out)

    def line_spans_dev(self, d_line, k, d_start=0, d_end=0, stream=0):
        """fmx_line_spans_dev: device pointers; with the table built it only enqueues."""
        _lib.check(self._L.fmx_line_spans_dev(self._h, _dp(d_line), int(k), _dp(d_start), _dp(d_end), _dp(stream)))

    def occurrence_lines(self, off, occ, corpus=None, cap=None):
        """fmx_occurrence_lines: (off, occ) as occurrences or finditer return them -> (line_off[n_groups + 1], hits): group
        g's distinct lines are hits[line_off[g]:line_off[g + 1]], a LINE_HIT array ascending by line, each with the number
        of occurrences that begin on it.  cap=None: a counting call sizes the buffer."""
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        occ = np.ascontiguousarray(occ, dtype=self.OCCURRENCE).reshape(-1)
        if off.size < 2 or int(off[-1]) > occ.size:
            raise ValueError("off: n_groups + 1 offsets into occ")
        args = (self._h, corpus.handle if corpus is not None else None, _ptr(off), _ptr(occ) if occ.size else None, off.size - 1)
        return self._csr_hits(self._L.fmx_occurrence_lines, args, off.size - 1, self.LINE_HIT, cap)

    def occurrence_lines_dev(self, d_occ_off, d_occ, n_occ, n_groups, d_out_off, d_out, cap, corpus=None, stream=0, grow=False):
        """fmx_occurrence_lines_dev: device pointers (u64 offsets, 32-byte occurrences in, 48-byte line hits out); allocates
        and synchronises.  -> the exact number of lines; cap = 0 is the counting call, grow as occurrences_dev."""
        n_out = ctypes.c_size_t()
        rc = self._L.fmx_occurrence_lines_dev(self._h, corpus.handle if corpus is not None else None, _dp(d_occ_off), _dp(d_occ),
                                              int(n_occ), int(n_groups), _dp(d_out_off), _dp(d_out), int(cap), ctypes.byref(n_out),
                                              _dp(stream))
        if not (rc == _lib.FMX_ERR_OVERFLOW and (int(cap) == 0 or grow)):
            _lib.check(rc)
        return int(n_out.value)

    def lines_last(self):
        """fmx_lines_last: (locate ms, keys + sort + directory ms) of this thread's last table build, (lookup ms, compaction
        ms) of its last lookup or occurrence-lines call."""
        t = [ctypes.c_double() for _ in range(4)]
        _lib.check(self._L.fmx_lines_last(*[ctypes.byref(x) for x in t]))
        return tuple(float(x.value) for x in t)

    # ---- line queries: all-of, none-of, near and inverted matches over line-hit lists (fmx_line_query)
    ALL_LINES = None                # the anchor "every real line of the text"
    LINE_TERM = np.dtype([("group", "<u4"), ("window", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])

    @classmethod
    def _line_queries(cls, queries):
        """[(anchor, [(group, window, negate), ..]), ..] -> (q_off, anchor, terms) as fmx_line_query takes them."""
        queries = list(queries)
        q_off = np.zeros(len(queries) + 1, dtype=np.uint64)
        anchor = np.zeros(len(queries), dtype=np.uint32)
        rows = []
        for i, (a, terms) in enumerate(queries):
            if a is not None and not 0 <= int(a) < _lib.FMX_LQ_ALL_LINES:
                raise ValueError("anchor: a group number, or None for all lines")
            anchor[i] = _lib.FMX_LQ_ALL_LINES if a is None else int(a)
            for g, w, neg in terms:
                w = _lib.FMX_LQ_ALL_LINES if isinstance(w, str) and w == "file" else int(w)
                if not (0 <= int(g) < 2 ** 32 and 0 <= w < 2 ** 32):
                    raise ValueError("term: (group, window, negate), window an int below 2^32 or 'file'")
                rows.append((int(g), w, _lib.FMX_LQ_NOT if neg else 0, 0))
            q_off[i + 1] = len(rows)
        return q_off, anchor, np.array(rows, dtype=cls.LINE_TERM).reshape(-1)

    def line_query(self, off, hits, queries, corpus=None, cap=None):
        """fmx_line_query: (off, hits) as occurrence_lines returns them, queries = [(anchor, terms), ..] -> (out_off[n_queries
        + 1], records): query q's lines are records[out_off[q]:out_off[q + 1]], a LINE_HIT array with group == q.  anchor: a
        group number, or None (ALL_LINES) for every real line of the text; terms: [(group, window, negate), ..], window an
        int (lines on either side, 0 = the same line) or "file" (anywhere in the same document).  The result is the anchor's
        records that satisfy every term, in order.  cap=None: a counting call sizes the buffer."""
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        hits = np.ascontiguousarray(hits, dtype=self.LINE_HIT).reshape(-1)
        if off.size < 2 or int(off[-1]) > hits.size:
            raise ValueError("off: n_groups + 1 offsets into hits")
        q_off, anchor, terms = self._line_queries(queries)
        args = (self._h, corpus.handle if corpus is not None else None, _ptr(off), _ptr(hits) if hits.size else None, off.size - 1,
                _ptr(q_off), _ptr(anchor) if anchor.size else None, _ptr(terms) if terms.size else None, anchor.size)
        return self._csr_hits(self._L.fmx_line_query, args, anchor.size, self.LINE_HIT, cap)

    def line_query_dev(self, d_hit_off, d_hits, n_hits, n_groups, queries, d_out_off, d_out, cap, corpus=None, stream=0, grow=False):
        """fmx_line_query_dev: device pointers (u64 offsets, 48-byte line hits in and out), the queries from the host;
        allocates and synchronises.  -> the exact number of records; cap = 0 is the counting call, grow as occurrences_dev."""
        q_off, anchor, terms = self._line_queries(queries)
        n_out = ctypes.c_size_t()
        rc = self._L.fmx_line_query_dev(self._h, corpus.handle if corpus is not None else None, _dp(d_hit_off), _dp(d_hits), int(n_hits),
                                        int(n_groups), _ptr(q_off), _ptr(anchor) if anchor.size else None,
                                        _ptr(terms) if terms.size else None, anchor.size, _dp(d_out_off), _dp(d_out), int(cap),
                                        ctypes.byref(n_out), _dp(stream))
        if not (rc == _lib.FMX_ERR_OVERFLOW and (int(cap) == 0 or grow)):
            _lib.check(rc)
        return int(n_out.value)

    def line_query_last(self):
        """fmx_line_query_last: (key packing ms, flags ms, scan + emit + offsets ms, candidates, keys probed) of this thread's
        last line query."""
        t = [ctypes.c_double() for _ in range(3)]
        n = [ctypes.c_uint64() for _ in range(2)]
        _lib.check(self._L.fmx_line_query_last(*[ctypes.byref(x) for x in t + n]))
        return tuple(float(x.value) for x in t) + tuple(int(x.value) for x in n)

    # ---- matching statistics and maximal exact matches (fmx_match_stats_batch, fmx_mems_batch)
    MEM_HIT =np.dtype([("pattern", np.uint32), ("len", np.uint32), ("end", np.uint64), ("sp", np.uint64), ("ep", np.uint64)])

    @staticmethod
    def _mstat_opts(max_len, min_len=0):
        max_len, min_len = int(max_len or 0), int(min_len or 0)
        if not (0 <= max_len < 2 ** 32 and 0 <= min_len < 2 ** 32):
            raise ValueError("max_len or min_len out of range")
        return _lib.fmx_mstat_opts(max_len, min_len, (0, 0))

    @staticmethod
    def _mstat_batch(pat, off):
        pat = np.ascontiguousarray(pat, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        k = off.size - 1
        if k < 0:
            raise ValueError("off needs k+1 entries")
        if k and int(off[-1]) != pat.size:
            raise ValueError("the offsets must cover the pattern buffer: off[k] == len(pat)")
        return pat, off, k

    def match_stats_batch(self, pat, off, max_len=None, intervals=True):
        """fmx_match_stats_batch: (len, sp, ep), parallel to `pat` -- for byte j of pattern q the number of backward steps
        over pat[j], pat[j - 1], .. that keep a non-empty interval (at most min(j - off[q] + 1, max_len); max_len=None:
        4096) and the interval after them.  intervals=False: sp and ep are None."""
        pat, off, k = self._mstat_batch(pat, off)
        opts = self._mstat_opts(max_len)
        ln = np.zeros(pat.size, dtype=np.uint32)
        sp = np.zeros(pat.size, dtype=np.uint64) if intervals else None
        ep = np.zeros(pat.size, dtype=np.uint64) if intervals else None
        _lib.check(self._L.fmx_match_stats_batch(self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts), _ptr(ln),
                                                 _ptr(sp) if intervals else None, _ptr(ep) if intervals else None))
        return ln, sp, ep

    def match_stats_batch_dev(self, d_pat, d_off, k, n_bytes, d_len, d_sp=0, d_ep=0, max_len=None, stream=0):
        """fmx_match_stats_batch_dev: device pointers (u8 patterns, u64 offsets[k + 1], u32 len[n_bytes], u64 sp / ep or 0);
        only enqueues on `stream`."""
        opts = self._mstat_opts(max_len)
        _lib.check(self._L.fmx_match_stats_batch_dev(self._h, _dp(d_pat), _dp(d_off), int(k), int(n_bytes), ctypes.byref(opts),
                                                     _dp(d_len), _dp(d_sp), _dp(d_ep), _dp(stream)))

    def mems_batch(self, pat, off, min_len, max_len=None, cap=None):
        """fmx_mems_batch: (off[k + 1], hits) -- pattern q's maximal exact matches of min_len bytes and more are
        hits[off[q]:off[q + 1]], a structured array (pattern, len, end, sp, ep) by ascending end; the match is
        P[end - len : end].  A hit with len == max_len is saturated.  cap=None: a counting call sizes the buffer; with a
        cap that is too small the library's FMX_ERR_OVERFLOW is raised."""
        pat, off, k = self._mstat_batch(pat, off)
        opts = self._mstat_opts(max_len, min_len)
        return self._csr_hits(self._L.fmx_mems_batch, (self._h, _ptr(pat), _ptr(off), k, ctypes.byref(opts)), k, self.MEM_HIT, cap)

    def mems_batch_dev(self, d_pat, d_off, k, n_bytes, min_len, d_out_off, d_out, cap, max_len=None, stream=0):
        """fmx_mems_batch_dev: device pointers (u64 out_off[k + 1], 32-byte hit records); allocates and synchronises.  -> the
        exact number of hits (FMX_ERR_OVERFLOW is raised when it exceeds cap)."""
        opts = self._mstat_opts(max_len, min_len)
        n_out = ctypes.c_size_t()
        _lib.check(self._L.fmx_mems_batch_dev(self._h, _dp(d_pat), _dp(d_off), int(k), int(n_bytes), ctypes.byref(opts),
                                              _dp(d_out_off), _dp(d_out), int(cap), ctypes.byref(n_out), _dp(stream)))
        return int(n_out.value)

    def mstat_last(self):
        """fmx_mstat_last: (walk kernel ms, compaction ms, backward steps, rank-dictionary requests) of this thread's last
        host or MEM call."""
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_mstat_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return float(a.value), float(b.value), int(c.value), int(d.value)

    # ---- extract: the text by position, from inverse-SA samples (fmx.h: extract)
    def extract_text_batch(self, pos, lengths):
        """fmx_extract_text_batch: (off, data) -- range q, the lengths[q] text bytes from text offset pos[q], is
        data[off[q]:off[q + 1]] (data a uint8 array); the handle indexes reverse(text) as from_text has it."""
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
        if pos.size != lengths.size:
            raise ValueError("pos and lengths differ in length")
        off = np.zeros(pos.size + 1, dtype=np.uint64)
        np.cumsum(lengths, out=off[1:])
        out = np.zeros(int(off[-1]), dtype=np.uint8)
        _lib.check(self._L.fmx_extract_text_batch(self._h, _ptr(pos), off.ctypes.data_as(ctypes.c_void_p), pos.size, _ptr(out)))
        return off, out

    def extract_text(self, pos, length):
        """The `length` text bytes from text offset `pos`."""
        return self.extract_text_batch([int(pos)], [int(length)])[1].tobytes()

    def extract_text_batch_dev(self, d_pos, d_off, k, n_bytes, d_out, stream=0):
        """fmx_extract_text_batch_dev: device pointers (u64 pos[k], u64 off[k + 1], n_bytes = off[k] bytes out); with the
        samples prepared it only enqueues."""
        _lib.check(self._L.fmx_extract_text_batch_dev(self._h, _dp(d_pos), _dp(d_off), int(k), int(n_bytes), _dp(d_out), _dp(stream)))

    def extract_info(self):
        """fmx_extract_info: (rate, device bytes, build ms) of the inverse-SA samples; 0 bytes when not built."""
        rate, nbytes, ms = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
        _lib.check(self._L.fmx_extract_info(self._h, ctypes.byref(rate), ctypes.byref(nbytes), ctypes.byref(ms)))
        return int(rate.value), int(nbytes.value), float(ms.value)

    def extract_last(self):
        """fmx_extract_last: (kernel ms, LF steps, memory requests) of this thread's last host-pointer extract call."""
        a, b, c = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.fmx_extract_last(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return float(a.value), int(b.value), int(c.value)

    # ---- repeats: the stretches of the indexed text that occur more than once (fmx_repeats)
    REPEAT_SUMMARY = ("ranges", "covered_bytes", "classes", "windows", "largest_class", "largest_class_pos")

    @staticmethod
    def _repeat_args(min_len, keep_first, stop):
        single = np.ndim(min_len) == 0
        levels = [int(x) for x in ([min_len] if single else min_len)]
        if any(not 0 <= x < 2 ** 32 for x in levels) or not 0 <= int(stop) <= 255:
            raise ValueError("min_len or stop out of range")
        lv = np.array(levels, dtype=np.uint32)
        opts = _lib.fmx_repeat_opts(_lib.FMX_REPEATS_LATER if keep_first else _lib.FMX_REPEATS_ALL, int(stop), (0, 0, 0))
        return single, lv, opts

    def repeats(self, min_len, keep_first=False, stop=0):
        """fmx_repeats: the stretches of the text whose every window of min_len bytes occurs at least twice ->
        (ranges, summary): ranges a uint64[r, 2] array of [start, end) text offsets, ascending and maximal, summary a dict
        (ranges, covered_bytes, classes, windows, largest_class, largest_class_pos).  keep_first: the first occurrence of
        every repeated window is left out ("every copy but the first").  stop != 0: a window that holds that byte does not
        count, so no range covers it.  min_len a sequence: one call for all thresholds (the suffix array is made once) and
        a list of such pairs.  The handle indexes reverse(text) as from_text has it.  A counting call sizes the buffer."""
        single, lv, opts = self._repeat_args(min_len, keep_first, stop)
        k = lv.size
        n_out = ctypes.c_size_t()
        off = np.zeros(k + 1, dtype=np.uint64)
        sums = (_lib.fmx_repeat_summary * max(k, 1))()
        rc = self._L.fmx_repeats(self._h, _ptr(lv), k, ctypes.byref(opts), _ptr(off), None, 0, ctypes.byref(n_out), sums)
        total = int(n_out.value)
        out = np.zeros((max(total, 1), 2), dtype=np.uint64)
        if rc == _lib.FMX_ERR_OVERFLOW:
            rc = self._L.fmx_repeats(self._h, _ptr(lv), k, ctypes.byref(opts), _ptr(off), _ptr(out), total, ctypes.byref(n_out), sums)
        _lib.check(rc)
        res = [(out[int(off[j]):int(off[j + 1])].copy(), {f: int(getattr(sums[j], f)) for f in self.REPEAT_SUMMARY})
               for j in range(k)]
        return res[0] if single else res

    def repeats_dev(self, min_len, d_out_off, d_out, cap, keep_first=False, stop=0, stream=0):
        """fmx_repeats_dev: u64 out_off[k + 1] and 16-byte (start, end) records in device memory; allocates and
        synchronises.  -> (the exact number of ranges, the list of summaries); FMX_ERR_OVERFLOW is raised when the ranges
        exceed cap."""
        _, lv, opts = self._repeat_args(min_len, keep_first, stop)
        n_out = ctypes.c_size_t()
        sums = (_lib.fmx_repeat_summary * max(lv.size, 1))()
        _lib.check(self._L.fmx_repeats_dev(self._h, _ptr(lv), lv.size, ctypes.byref(opts), _dp(d_out_off), _dp(d_out), int(cap),
                                           ctypes.byref(n_out), sums, _dp(stream)))
        return int(n_out.value), [{f: int(getattr(sums[j], f)) for f in self.REPEAT_SUMMARY} for j in range(lv.size)]

    def repeats_last(self):
        """fmx_repeats_last: (inversion ms, class passes ms, coverage passes ms, compaction ms) of this thread's last call."""
        v = [ctypes.c_double() for _ in range(4)]
        _lib.check(self._L.fmx_repeats_last(*[ctypes.byref(x) for x in v]))
        return tuple(float(x.value) for x in v)

    # ---- n-grams: the distinct windows of a length, their counts and the spectrum of the counts (fmx_ngrams)
    NGRAM = np.dtype([("sp", np.uint64), ("count", np.uint64), ("first_pos", np.uint64)])
    NGRAM_SUMMARY = ("records", "selected", "distinct", "windows", "singletons", "largest_count", "largest_sp", "largest_pos")
    NO_POS = 2 ** 64 - 1                # first_pos and largest_pos of a call without positions

    @staticmethod
    def _ngram_args(length, min_count, top, order, stop, spectrum, positions):
        single = np.ndim(length) == 0
        levels = [int(x) for x in ([length] if single else length)]
        if order not in ("row", "count"):
            raise ValueError("order: 'row' or 'count'")
        top, spectrum = int(top or 0), int(spectrum or 0)
        if any(not 0 <= x < 2 ** 32 for x in levels) or not 0 <= int(stop) <= 255 or not 0 <= int(min_count) < 2 ** 64 or \
                not 0 <= top < 2 ** 64 or not 0 <= spectrum < 2 ** 32:
            raise ValueError("length, min_count, top, stop or spectrum out of range")
        lv = np.array(levels, dtype=np.uint32)
        opts = _lib.fmx_ngram_opts(_lib.FMX_NGRAMS_BY_COUNT if order == "count" else _lib.FMX_NGRAMS_BY_ROW,
                                   0 if positions else _lib.FMX_NGRAMS_NO_POS, int(min_count), top, spectrum, int(stop), (0, 0, 0))
        return single, lv, opts

    def _ngram_summaries(self, sums, spec, k, bins):
        out = []
        for j in range(k):
            s = {f: int(getattr(sums[j], f)) for f in self.NGRAM_SUMMARY}
            if bins:
                s["spectrum"] = spec[j * bins:(j + 1) * bins].copy()
            out.append(s)
        return out

    def ngrams(self, length, min_count=2, top=None, order="count", stop=0, spectrum=0, positions=True):
        """fmx_ngrams: the distinct windows of `length` bytes that occur min_count times and more -> (records, summary):
        records a structured array (sp, count, first_pos) -- the window's interval is [sp, sp + count), what
        search(reverse(window)) returns, first_pos its first text offset -- by descending count (ties by sp; order="row":
        by sp), the first `top` of them; summary a dict (records, selected, distinct, windows, singletons, largest_count,
        largest_sp, largest_pos) and, with spectrum=B, "spectrum": a uint64[B] array, entry c the number of windows'
        classes of count c, entry 0 those of count >= B.  stop != 0: a window that holds that byte does not count.
        positions=False: first_pos and largest_pos are NO_POS and no suffix array is made (min_count >= 2, no stop byte).
        length a sequence: one call for all lengths and a list of such pairs.  The handle indexes reverse(text) as
        from_text has it.  A counting call sizes the buffer."""
        single, lv, opts = self._ngram_args(length, min_count, top, order, stop, spectrum, positions)
        k, bins = lv.size, int(opts.spectrum_bins)
        n_out = ctypes.c_size_t()
        off = np.zeros(k + 1, dtype=np.uint64)
        sums = (_lib.fmx_ngram_summary * max(k, 1))()
        spec = np.zeros(max(k * bins, 1), dtype=np.uint64)
        rc = self._L.fmx_ngrams(self._h, _ptr(lv), k, ctypes.byref(opts), _ptr(off), None, 0, ctypes.byref(n_out), sums, _ptr(spec))
        total = int(n_out.value)
        out = np.zeros(max(total, 1), dtype=self.NGRAM)
        if rc == _lib.FMX_ERR_OVERFLOW:
            rc = self._L.fmx_ngrams(self._h, _ptr(lv), k, ctypes.byref(opts), _ptr(off), _ptr(out), total, ctypes.byref(n_out), sums,
                                    _ptr(spec))
        _lib.check(rc)
        summaries = self._ngram_summaries(sums, spec, k, bins)
        res = [(out[int(off[j]):int(off[j + 1])].copy(), summaries[j]) for j in range(k)]
        return res[0] if single else res

    def ngrams_dev(self, length, d_out_off, d_out, cap, min_count=2, top=None, order="count", stop=0, spectrum=0, positions=True,
                   stream=0):
        """fmx_ngrams_dev: u64 out_off[k + 1] and 24-byte (sp, count, first_pos) records in device memory; allocates and
        synchronises.  -> (the exact number of records, the list of summaries); FMX_ERR_OVERFLOW is raised when the records
        exceed cap."""
        _, lv, opts = self._ngram_args(length, min_count, top, order, stop, spectrum, positions)
        bins = int(opts.spectrum_bins)
        n_out = ctypes.c_size_t()
        sums = (_lib.fmx_ngram_summary * max(lv.size, 1))()
        spec = np.zeros(max(lv.size * bins, 1), dtype=np.uint64)
        _lib.check(self._L.fmx_ngrams_dev(self._h, _ptr(lv), lv.size, ctypes.byref(opts), _dp(d_out_off), _dp(d_out), int(cap),
                                          ctypes.byref(n_out), sums, _ptr(spec), _dp(stream)))
        return int(n_out.value), self._ngram_summaries(sums, spec, lv.size, bins)

    def ngrams_last(self):
        """fmx_ngrams_last: (inversion ms, class passes ms, selection ms, sort ms) of this thread's last call."""
        v = [ctypes.c_double() for _ in range(4)]
        _lib.check(self._L.fmx_ngrams_last(*[ctypes.byref(x) for x in v]))
        return tuple(float(x.value) for x in v)

    def ngram_texts(self, records, length):
        """The bytes of the windows of `records` (as ngrams gave them for `length`, with positions) -> a list of bytes:
        extract_text_batch(first_pos, length)."""
        rec = np.ascontiguousarray(records, dtype=self.NGRAM).reshape(-1)
        if rec.size and (rec["first_pos"] == np.uint64(self.NO_POS)).any():
            raise ValueError("the records carry no positions (positions=False)")
        off, data = self.extract_text_batch(rec["first_pos"], np.full(rec.size, int(length), dtype=np.uint64))
        return [data[int(off[q]):int(off[q + 1])].tobytes() for q in range(rec.size)]

    def match_stats_text(self, q, max_len=None):
        """ms[i] = the length of the longest prefix of q[i:] that occurs in the indexed text (capped at max_len), for a handle
        that indexes reverse(text) as from_text and locate_text have it: the statistics of reverse(q), flipped."""
        q = bytes(q)
        ln, _, _ = self.match_stats_batch(np.frombuffer(q[::-1], dtype=np.uint8), np.array([0, len(q)], dtype=np.uint64),
                                          max_len, intervals=False)
        return ln[::-1].copy()

    def mems_text(self, q, min_len, max_len=None, max_per=None):
        """The maximal exact matches of q with the indexed text, as rows (q_off, len, text_off) of a uint64 array sorted by
        (q_off, text_off): q[q_off : q_off + len] stands at text_off; at most max_per text positions per match.  The MEMs of
        reverse(q), located, each with its own length (text_offsets)."""
        q = bytes(q)
        _, hits = self.mems_batch(np.frombuffer(q[::-1], dtype=np.uint8), np.array([0, len(q)], dtype=np.uint64), min_len, max_len)
        off, sa = self.locate_intervals(hits["sp"], hits["ep"], max_per=max_per)
        cnt = np.diff(off).astype(np.int64)
        ln = np.repeat(hits["len"].astype(np.uint64), cnt)
        q_off = np.repeat(np.uint64(len(q)) - hits["end"], cnt)
        out = np.zeros((sa.size, 3), dtype=np.uint64)
        if sa.size:
            out[:, 0], out[:, 1], out[:, 2] = q_off, ln, np.uint64(self.n - 1) - ln - sa
            out = out[np.lexsort((out[:, 2], out[:, 0]))]
        return out

    # ---- batched forms (host arrays in, host arrays out)
    def occ_batch(self, c, i):
        c = np.ascontiguousarray(c, dtype=np.uint8)
        i = np.ascontiguousarray(i, dtype=np.int64)
        if c.size != i.size:
            raise ValueError("c and i differ in length")
        out = np.zeros(c.size, dtype=np.uint64)
        _lib.check(self._L.fmx_occ_batch(self._h, _ptr(c), _ptr(i), _ptr(out), c.size))
        return out

    def search_batch(self, pat, off, out=None):
        """out = (sp, ep) uint64 arrays to fill (e.g. PinnedArray views), else new ones."""
        pat = np.ascontiguousarray(pat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        k = off.size - 1
        if k < 0:
            raise ValueError("off needs k+1 entries")
        if k and int(off[-1]) > pat.size:
            raise ValueError("offsets run past the pattern buffer")
        if out is not None:
            sp, ep = out
            if sp.size != k or ep.size != k or sp.dtype != np.uint64 or ep.dtype != np.uint64:
                raise ValueError("out arrays must be uint64 of length k")
        else:
            sp = np.zeros(k, dtype=np.uint64)
            ep = np.zeros(k, dtype=np.uint64)
        _lib.check(self._L.fmx_search_batch(self._h, _ptr(pat), _ptr(off), _ptr(sp), _ptr(ep), k))
        return sp, ep

    def search_batch_ex(self, pat, off=None, fixed_len=0, packed=False, escape_cap=0, miss_none=False):
        """fmx_search_batch_ex: the lean forms of search_batch -- `fixed_len` > 0: k = len(pat) // fixed_len patterns of
        that length, no offsets travel; `packed`: the intervals come back in the 8-byte form (one uint64 array of
        fmx_packed_words(k, escape_cap) words: unpack_intervals).  Returns (sp, ep) or the packed array."""
        pat = np.ascontiguousarray(pat, dtype=np.uint8)
        if fixed_len:
            if pat.size % int(fixed_len):
                raise ValueError("the pattern buffer is not a whole number of patterns")
            k, offp = pat.size // int(fixed_len), None
        else:
            off = np.ascontiguousarray(off, dtype=np.uint64)
            k, offp = off.size - 1, _ptr(off)
            if k and int(off[-1]) > pat.size:
                raise ValueError("offsets run past the pattern buffer")
        opts = _lib.fmx_search_opts(int(fixed_len), (1 if packed else 0) | (2 if miss_none else 0), int(escape_cap))
        if packed:
            out = np.zeros(int(self._L.fmx_packed_words(k, int(escape_cap))), dtype=np.uint64)
            _lib.check(self._L.fmx_search_batch_ex(self._h, _ptr(pat), offp, _ptr(out), None, k, ctypes.byref(opts)))
            return out
        sp = np.zeros(k, dtype=np.uint64)
        ep = np.zeros(k, dtype=np.uint64)
        _lib.check(self._L.fmx_search_batch_ex(self._h, _ptr(pat), offp, _ptr(sp), _ptr(ep), k, ctypes.byref(opts)))
        return sp, ep

    def unpack_intervals(self, packed, k, escape_cap=0):
        """fmx_unpack_intervals (host): the 8-byte form -> (sp, ep); raises FMX_ERR_OVERFLOW when more intervals were wide
        than the escape list holds."""
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        sp = np.zeros(int(k), dtype=np.uint64)
        ep = np.zeros(int(k), dtype=np.uint64)
        _lib.check(self._L.fmx_unpack_intervals(_ptr(packed) if packed.size else None, int(k), int(escape_cap), _ptr(sp), _ptr(ep)))
        return sp, ep

    def prev_range_batch(self, sp, ep, c):
        sp = np.ascontiguousarray(sp, dtype=np.uint64)
        ep = np.ascontiguousarray(ep, dtype=np.uint64)
        c = np.ascontiguousarray(c, dtype=np.uint8)
        if not (sp.size == ep.size == c.size):
            raise ValueError("sp, ep and c differ in length")
        sp1 = np.zeros(sp.size, dtype=np.uint64)
        ep1 = np.zeros(sp.size, dtype=np.uint64)
        _lib.check(self._L.fmx_prev_range_batch(self._h, _ptr(sp), _ptr(ep), _ptr(c), _ptr(sp1), _ptr(ep1), sp.size))
        return sp1, ep1

    def lf_walk_batch(self, rows, length, want_bytes=True):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros((rows.size, int(length)), dtype=np.uint8) if want_bytes else None
        end = np.zeros(rows.size, dtype=np.uint64)
        _lib.check(self._L.fmx_lf_walk_batch(self._h, _ptr(rows), rows.size, int(length),
                                             _ptr(out) if want_bytes else None, _ptr(end)))
        return out, end

    def psi_batch(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(rows.size, dtype=np.uint64)
        _lib.check(self._L.fmx_psi_batch(self._h, _ptr(rows), _ptr(out), rows.size))
        return out

    # ---- device-pointer forms (inputs resident in HBM; only enqueue on `stream`)
    def search_batch_dev(self, d_pat, d_off, d_sp, d_ep, k, stream=0):
        _lib.check(self._L.fmx_search_batch_dev(self._h, _dp(d_pat), _dp(d_off), _dp(d_sp), _dp(d_ep), int(k),
                                                _dp(stream)))

    def search_batch_ex_dev(self, d_pat, d_off, d_sp, d_ep, k, stream=0, fixed_len=0, packed=False, escape_cap=0, miss_none=False):
        """fmx_search_batch_ex_dev: d_off may be 0 with fixed_len; with `packed` d_sp receives the packed words (it needs
        fmx_packed_words(k, escape_cap) of them) and d_ep is k words of scratch."""
        opts = _lib.fmx_search_opts(int(fixed_len), (1 if packed else 0) | (2 if miss_none else 0), int(escape_cap))
        _lib.check(self._L.fmx_search_batch_ex_dev(self._h, _dp(d_pat), _dp(d_off), _dp(d_sp), _dp(d_ep), int(k),
                                                   ctypes.byref(opts), _dp(stream)))

    def packed_words(self, k, escape_cap=0):
        return int(self._L.fmx_packed_words(int(k), int(escape_cap)))

    def pack_intervals_dev(self, d_sp, d_ep, k, d_packed, escape_cap=0, stream=0):
        _lib.check(self._L.fmx_pack_intervals_dev(self._h, _dp(d_sp), _dp(d_ep), int(k), int(escape_cap), _dp(d_packed), _dp(stream)))

    def unpack_intervals_dev(self, d_packed, k, d_sp, d_ep, escape_cap=0, stream=0):
        _lib.check(self._L.fmx_unpack_intervals_dev(self._h, _dp(d_packed), int(k), int(escape_cap), _dp(d_sp), _dp(d_ep), _dp(stream)))

    def occ_batch_dev(self, d_c, d_i, d_out, k, stream=0):
        _lib.check(self._L.fmx_occ_batch_dev(self._h, _dp(d_c), _dp(d_i), _dp(d_out), int(k), _dp(stream)))

    def prev_range_batch_dev(self, d_sp, d_ep, d_c, d_sp1, d_ep1, k, stream=0):
        _lib.check(self._L.fmx_prev_range_batch_dev(self._h, _dp(d_sp), _dp(d_ep), _dp(d_c), _dp(d_sp1), _dp(d_ep1),
                                                    int(k), _dp(stream)))

    def lf_walk_batch_dev(self, d_rows, k, length, d_out_bytes, d_end_rows, stream=0):
        _lib.check(self._L.fmx_lf_walk_batch_dev(self._h, _dp(d_rows), int(k), int(length), _dp(d_out_bytes),
                                                 _dp(d_end_rows), _dp(stream)))

    def psi_batch_dev(self, d_rows, d_out, k, stream=0):
        _lib.check(self._L.fmx_psi_batch_dev(self._h, _dp(d_rows), _dp(d_out), int(k), _dp(stream)))

    def next_substr_batch_dev(self, d_rows, k, length, d_out, d_out_len, stream=0):
        _lib.check(self._L.fmx_next_substr_batch_dev(self._h, _dp(d_rows), int(k), int(length), _dp(d_out),
                                                     _dp(d_out_len), _dp(stream)))

    # ---- BWTMerger2.calcGaps' rank loop (bwtmerger.scala:981-1023): one dependent chain, answered on the host
    def occ_host(self, c, i):
        """fmx_occ_host: occ(c, i) from the host-side copy of the dictionary (same answer as occ)."""
        if not 0 <= int(c) < 256:
            raise IndexError("symbol %r (reference: ArrayIndexOutOfBoundsException)" % (c,))
        v = ctypes.c_uint64()
        _lib.check(self._L.fmx_occ_host(self._h, int(c), int(i), ctypes.byref(v)))
        return int(v.value)

    def calc_gaps_chain(self, text, rank0=0, last_char=-1, rklst=0):
        """fmx_calc_gaps_chain: (ranks, done) -- ranks[j] = calcGaps' curRank after byte j; done < len(text) when the
        chain stopped at a rank equal to rklst for the caller to decide (bwtmerger.scala:1004-1010)."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        ranks = np.zeros(max(text.size, 1), dtype=np.uint64)
        done = ctypes.c_size_t()
        _lib.check(self._L.fmx_calc_gaps_chain(self._h, _ptr(text), text.size, int(rank0), int(last_char), int(rklst),
                                               _ptr(ranks), ctypes.byref(done)))
        return ranks[: text.size], int(done.value)

    def prepare(self, ktab=True, select=False, jump=False, frontier=False, search=False, budget_bytes=0, locate=False,
                lcp=False, extract=False, lines=False):
        """fmx_prepare[_ex]: build the k-mer jump table / the select directory / the literal search's row tables (J, R3) / the
        regex frontier's row table / the locate samples / the LCP array / the extract samples / the line table (break set {10}) now instead of at the threshold or at first use, and calibrate the
        search kernel they select (`search` alone: only that).  budget_bytes != 0: the handle's "table_budget" first
        (fmx_prepare_ex)."""
        what = (1 if ktab else 0) | (2 if select else 0) | (4 if jump else 0) | (8 if frontier else 0) | (16 if search else 0) \
            | (32 if locate else 0) | (64 if lcp else 0) | (128 if extract else 0) | (256 if lines else 0)
        if budget_bytes:
            _lib.check(self._L.fmx_prepare_ex(self._h, what, int(budget_bytes)))
        else:
            _lib.check(self._L.fmx_prepare(self._h, what))

    def drop_tables(self, jump=True, frontier=True, ktab=False, locate=False, lcp=False, extract=False, lines=False):
        """fmx_drop_tables: free the row jump table and the three-step row table / the frontier's row table / the k-mer table /
        the locate samples / the LCP array / the extract samples / the line table."""
        _lib.check(self._L.fmx_drop_tables(self._h, (4 if jump else 0) | (8 if frontier else 0) | (1 if ktab else 0)
                                           | (32 if locate else 0) | (64 if lcp else 0) | (128 if extract else 0) | (256 if lines else 0)))

    def config_set(self, key, value):
        """fmx_index_config_set: this handle's own table policy ("ktab", "jump", "jump_pairs", "search_lanes", "jump_chars", "tables_after",
        "table_budget", "locate_sample", "extract_sample", "lines_shift"); tables that exist stay until drop_tables."""
        _lib.check(self._L.fmx_index_config_set(self._h, key.encode(), str(value).encode()))

    # ---- statistics
    def stats(self):
        s = _lib.fmx_stats_t()
        _lib.check(self._L.fmx_stats(self._h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def last_kernel_ms(self):
        v = ctypes.c_double()
        _lib.check(self._L.fmx_last_kernel_ms(self._h, ctypes.byref(v)))
        return float(v.value)

    def stats_reset(self):
        _lib.check(self._L.fmx_stats_reset(self._h))
