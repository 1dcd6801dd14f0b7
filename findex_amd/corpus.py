"""A directory of files as one index -- the drop-in for findex's DirBWTReader (bwtreader.scala:17-173), the input side of the
reference's IndexerApp -- and, beyond the reference, the way back from a hit to (file, offset).

The STREAM that gets indexed: the files of a directory first, then its subdirectories recursively (recursiveListFiles,
:44-62); files that look binary dropped (Util.isBinary, util.scala:20-44); in every file raw byte 0 -> '\\' '0', raw 1 ->
'\\' '1', raw 255 -> '\\' 'f' (:144-155; the backslash itself is NOT escaped, the reference's quirk); one separator byte 1
after every file, the last included (:133-137).  File.listFiles has no defined order; this package fixes one: names compared
as bytes, ascending, a directory's files before its subdirectories.

Walking the tree is host work and lives here; escaping, the map and the document listing run on the device (libfmx:
fmx_corpus_*, csrc/fmx_corpus.hip).  There is no CPU fallback."""
import ctypes
import os
import struct

import numpy as np

from . import _lib
from .searcher import ASCII_FOLD, HipFMSearcher, _dp, _ptr

MAGIC = b"FMXDOCS1"
SEPARATOR = 1
NO_DOC = 0xFFFFFFFF


def is_binary(path):
    """Util.isBinary (util.scala:20-44) as DirBWTReader uses it: a 0 among the first 1024 bytes, an empty file (an empty read
    is None, which the reader treats as binary) or a file that cannot be opened."""
    try:
        with open(path, "rb") as f:
            head = f.read(1024)
    except OSError:
        return True
    return not head or b"\0" in head


def list_files(root, filter_binary=True):
    """The files under `root` in stream order: a directory's files (names as bytes, ascending), then its subdirectories
    (likewise) recursively.  Returns paths relative to `root`, '/'-separated, as bytes."""
    root_b = os.fsencode(root)
    out = []

    def walk(d, rel):
        try:
            names = sorted(os.listdir(d))
        except OSError:
            return
        dirs = []
        for nm in names:
            p = os.path.join(d, nm)
            if os.path.isdir(p):
                dirs.append(nm)
            elif os.path.isfile(p) and not (filter_binary and is_binary(p)):
                out.append(rel + nm)
        for nm in dirs:
            walk(os.path.join(d, nm), rel + nm + b"/")

    walk(root_b, b"")
    return out


def escape(b):
    """fmx_corpus_escape: `b` as it stands in the stream (0, 1 and 255 become two bytes each)."""
    L = _lib.load()
    src = np.frombuffer(bytes(b), dtype=np.uint8)
    out = np.zeros(max(2 * src.size, 1), dtype=np.uint8)
    n = ctypes.c_size_t()
    _lib.check(L.fmx_corpus_escape(_ptr(src), src.size, _ptr(out), out.size, ctypes.byref(n)))
    return out[: n.value].tobytes()


def write_docs(path, doc_start, raw_len, esc_pos, names):
    """X.docs, little-endian: magic FMXDOCS1; u64 n_docs, n_esc, stream_len; doc_start[n_docs + 1], raw_len[n_docs],
    esc_pos[n_esc] as u64; name offsets [n_docs + 1] as u64; the name bytes (paths relative to the root, '/'-separated)."""
    doc_start, raw_len, esc_pos = (np.asarray(a, dtype=np.uint64).reshape(-1) for a in (doc_start, raw_len, esc_pos))
    names = [bytes(nm) for nm in names]
    if doc_start.size != raw_len.size + 1 or len(names) != raw_len.size or raw_len.size < 1:
        raise ValueError("doc_start, raw_len and names disagree about the number of documents")
    off = np.zeros(raw_len.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(nm) for nm in names])
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<QQQ", raw_len.size, esc_pos.size, int(doc_start[-1])))
        for a in (doc_start, raw_len, esc_pos, off):
            f.write(a.astype("<u8").tobytes())
        f.write(b"".join(names))


def read_docs(path):
    """(doc_start, raw_len, esc_pos, names) of an X.docs file; ValueError for a wrong magic or a truncated file."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 32 or blob[:8] != MAGIC:
        raise ValueError("%s: not an FMXDOCS1 file" % path)
    n_docs, n_esc, stream_len = struct.unpack_from("<QQQ", blob, 8)
    words = (n_docs + 1) + n_docs + n_esc + (n_docs + 1)
    if n_docs < 1 or len(blob) < 32 + 8 * words:
        raise ValueError("%s: truncated (%d documents, %d escapes need %d bytes of tables)" % (path, n_docs, n_esc, 8 * words))
    a = np.frombuffer(blob, dtype="<u8", count=words, offset=32).astype(np.uint64)
    doc_start, raw_len = a[: n_docs + 1], a[n_docs + 1: 2 * n_docs + 1]
    esc_pos, name_off = a[2 * n_docs + 1: 2 * n_docs + 1 + n_esc], a[2 * n_docs + 1 + n_esc:]
    names_at = 32 + 8 * words
    if int(name_off[0]) != 0 or np.any(np.diff(name_off.astype(np.int64)) < 0) or len(blob) != names_at + int(name_off[-1]):
        raise ValueError("%s: truncated or trailing bytes (the name table does not end with the file)" % path)
    if int(doc_start[-1]) != stream_len:
        raise ValueError("%s: doc_start does not end at the stream length" % path)
    names = [blob[names_at + int(name_off[d]): names_at + int(name_off[d + 1])] for d in range(n_docs)]
    return doc_start, raw_len, esc_pos, names


def stream_positions(doc_start, esc_pos, doc, raw_off):
    """The inverse of the map, in numpy over the map's tables: where raw byte raw_off of document doc stands in the stream
    -- the backslash where the byte is escaped; raw_off == raw_len[doc] is the document's separator.
    stream = doc_start[d] + raw_off + #{escapes of d whose raw offset < raw_off}; the i-th escape of d, at stream position e,
    has raw offset e - doc_start[d] - i, so with key[j] = esc_pos[j] - j (strictly increasing over all escapes) and lo = the
    index of d's first escape, the count is #{j >= lo : key[j] < doc_start[d] + raw_off - lo}.
    Not validated: a doc outside 0 .. n_docs - 1 raises numpy's IndexError, and a raw_off beyond raw_len[doc] silently gives
    a position in a later document."""
    ds = np.asarray(doc_start, dtype=np.uint64).astype(np.int64)
    ep = np.asarray(esc_pos, dtype=np.uint64).astype(np.int64)
    d = np.asarray(doc, dtype=np.int64).reshape(-1)
    ro = np.asarray(raw_off, dtype=np.uint64).astype(np.int64).reshape(-1)
    lo = np.searchsorted(ep, ds[d], side="left")
    hi = np.searchsorted(ep, ds[d + 1], side="left")
    key = ep - np.arange(ep.size, dtype=np.int64)
    upto = np.minimum(np.searchsorted(key, ds[d] + ro - lo, side="left"), hi)
    return (ds[d] + ro + (upto - lo)).astype(np.uint64)


_ESC_CODE = np.zeros(256, dtype=np.uint8)           # the second byte of an escape pair -> the raw byte it stands for
_ESC_CODE[ord("1")] = 1
_ESC_CODE[ord("f")] = 255
_ESC_SECOND = np.zeros(256, dtype=bool)             # ... and which second bytes there are: '0', '1', 'f'
_ESC_SECOND[[ord("0"), ord("1"), ord("f")]] = True


def unescape_ranges(data, off, starts, esc_pos):
    """The raw bytes of stream ranges (pieces of Corpus.stream() or of X.data), unescaped BY THE MAP: range q is
    data[off[q]:off[q + 1]], the stream from position starts[q] on; every escape of esc_pos inside it loses its backslash
    and its second byte becomes the raw byte.  No pattern matching: the reference does not escape the backslash, so a
    file's own backslash-zero reads like an escape and is none.  The ranges begin and end between pairs (stream_positions
    gives such positions).  ValueError when the data and esc_pos disagree: no backslash at an escape, or a second byte
    that is not '0', '1' or 'f'.  -> a list of bytes."""
    buf = np.array(np.frombuffer(data, dtype=np.uint8))          # the one copy: the second bytes are rewritten in it
    off = np.asarray(off, dtype=np.uint64).astype(np.int64)
    st = np.asarray(starts, dtype=np.uint64).astype(np.int64).reshape(-1)
    ep = np.asarray(esc_pos, dtype=np.uint64).astype(np.int64)
    lens = np.diff(off)
    lo = np.searchsorted(ep, st, side="left")
    cnt = np.searchsorted(ep, st + lens, side="left") - lo
    which = np.repeat(np.arange(st.size, dtype=np.int64), cnt)
    j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    at = ep[j] - st[which] + off[which]                      # the backslashes in `data`
    if at.size and np.any(at + 1 >= off[which + 1]):
        raise ValueError("a range ends inside an escape pair")
    if at.size and (np.any(buf[at] != 0x5C) or not np.all(_ESC_SECOND[buf[at + 1]])):
        raise ValueError("the data and esc_pos disagree: no escape pair where the map has one")
    keep = np.ones(buf.size, dtype=bool)
    keep[at] = False
    buf[at + 1] = _ESC_CODE[buf[at + 1]]
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    raw = buf[keep]
    return [raw[before[off[q]]:before[off[q + 1]]].tobytes() for q in range(st.size)]


class Corpus:
    """fmx_corpus: the stream of a list of documents in HBM (until drop_stream) and the map from stream positions to
    (document, offset).  `names[d]` is document d's path relative to the root, as bytes."""

    def __init__(self, handle, names, device=0):
        self._L = _lib.load()
        self._c = handle
        self.names = list(names)
        self.device = int(device)
        self.n_docs, self.stream_len, self.n_esc = self.info()[:3]
        if len(self.names) != self.n_docs:
            raise ValueError("%d names for %d documents" % (len(self.names), self.n_docs))

    # ---- constructors
    @classmethod
    def from_documents(cls, docs, names=None, device=0):
        """fmx_corpus_build over the given raw documents (a list of bytes), in their order."""
        L = _lib.load()
        docs = [bytes(d) for d in docs]
        raw = np.frombuffer(b"".join(docs), dtype=np.uint8)
        ends = np.cumsum([len(d) for d in docs], dtype=np.uint64) if docs else np.zeros(0, dtype=np.uint64)
        h = ctypes.c_void_p()
        _lib.check(L.fmx_corpus_build(_ptr(raw), raw.size, _ptr(ends), ends.size, int(device), ctypes.byref(h)))
        return cls(h, names if names is not None else [b"%d" % d for d in range(len(docs))], device)

    @classmethod
    def from_dir(cls, root, filter_binary=True, device=0):
        """DirBWTReader over `root`: list_files, read, build.  A file that vanishes or cannot be read between the listing and
        the read is dropped like one that cannot be opened."""
        names, docs = [], []
        for rel in list_files(root, filter_binary=filter_binary):
            try:
                with open(os.path.join(os.fsencode(root), *rel.split(b"/")), "rb") as f:
                    docs.append(f.read())
                names.append(rel)
            except OSError:
                continue
        if not docs:
            raise ValueError("%s: no files to index" % (root,))
        return cls.from_documents(docs, names, device)

    @classmethod
    def load(cls, path, device=0):
        """The map alone from an X.docs side file (fmx_corpus_from_tables): no stream, so no build_index."""
        L = _lib.load()
        doc_start, raw_len, esc_pos, names = read_docs(path)
        h = ctypes.c_void_p()
        _lib.check(L.fmx_corpus_from_tables(_ptr(doc_start), _ptr(raw_len), _ptr(esc_pos), raw_len.size, esc_pos.size,
                                            int(device), ctypes.byref(h)))
        return cls(h, names, device)

    def close(self):
        if getattr(self, "_c", None):
            self._L.fmx_corpus_free(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._c

    # ---- what it holds
    def info(self):
        """fmx_corpus_info: (n_docs, stream_len, n_esc, device bytes, build ms, tile bytes)."""
        a, b, c, d = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        ms, tile = ctypes.c_double(), ctypes.c_uint32()
        _lib.check(self._L.fmx_corpus_info(self._c, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d),
                                           ctypes.byref(ms), ctypes.byref(tile)))
        return int(a.value), int(b.value), int(c.value), int(d.value), float(ms.value), int(tile.value)

    def stream(self):
        """fmx_corpus_stream: the escaped stream as a uint8 array (what X.data holds)."""
        out = np.empty(self.stream_len, dtype=np.uint8)
        _lib.check(self._L.fmx_corpus_stream(self._c, _ptr(out), out.size))
        return out

    def stream_dev(self):
        """fmx_corpus_stream_dev: (device pointer, length)."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self._L.fmx_corpus_stream_dev(self._c, ctypes.byref(p), ctypes.byref(n)))
        return int(p.value), int(n.value)

    def drop_stream(self):
        _lib.check(self._L.fmx_corpus_drop_stream(self._c))

    def tables(self):
        """fmx_corpus_tables: (doc_start[n_docs + 1], raw_len[n_docs], esc_pos[n_esc]) as uint64 arrays."""
        ds = np.zeros(self.n_docs + 1, dtype=np.uint64)
        rl = np.zeros(self.n_docs, dtype=np.uint64)
        ep = np.zeros(self.n_esc, dtype=np.uint64)
        _lib.check(self._L.fmx_corpus_tables(self._c, _ptr(ds), _ptr(rl), _ptr(ep)))
        return ds, rl, ep

    def build_index(self, stream=0):
        """fmx_corpus_open_index: the stream's index, built on the device from the stream in HBM -> HipFMSearcher."""
        h = ctypes.c_void_p()
        _lib.check(self._L.fmx_corpus_open_index(self._c, _dp(stream), ctypes.byref(h)))
        return HipFMSearcher(_handle=h)

    def map(self, pos):
        """fmx_corpus_map: (doc uint32, esc_off uint64, raw_off uint64) per stream position; doc = 0xFFFFFFFF at or past the
        end of the stream."""
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        doc = np.zeros(pos.size, dtype=np.uint32)
        eo = np.zeros(pos.size, dtype=np.uint64)
        ro = np.zeros(pos.size, dtype=np.uint64)
        _lib.check(self._L.fmx_corpus_map(self._c, _ptr(pos), pos.size, _ptr(doc), _ptr(eo), _ptr(ro)))
        return doc, eo, ro

    def map_dev(self, d_pos, k, d_doc, d_esc_off, d_raw_off, stream=0):
        """fmx_corpus_map_dev: device pointers; only enqueues."""
        _lib.check(self._L.fmx_corpus_map_dev(self._c, _dp(d_pos), int(k), _dp(d_doc), _dp(d_esc_off), _dp(d_raw_off), _dp(stream)))

    def to_stream(self, doc, raw_off):
        """The inverse of map: the stream position (uint64) of raw byte raw_off of document doc (arrays or scalars);
        raw_off == raw_len[doc] is the separator.  stream_positions over tables()."""
        ds, _, ep = self.tables()
        return stream_positions(ds, ep, doc, raw_off)

    @classmethod
    def from_tables(cls, doc_start, raw_len, esc_pos, names, device=0):
        """The map alone from its three tables (fmx_corpus_from_tables), as load() makes it from an X.docs file."""
        L = _lib.load()
        doc_start, raw_len, esc_pos = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (doc_start, raw_len, esc_pos))
        h = ctypes.c_void_p()
        _lib.check(L.fmx_corpus_from_tables(_ptr(doc_start), _ptr(raw_len), _ptr(esc_pos), raw_len.size, esc_pos.size,
                                            int(device), ctypes.byref(h)))
        return cls(h, names, device)

    def extended(self, more):
        """The map of this corpus followed by the documents of the corpus `more`: the tables concatenated, the new documents'
        starts and escapes shifted by this stream's length (every document ends with its separator, so the streams simply
        follow each other).  No stream."""
        ds, rl, ep = self.tables()
        ds2, rl2, ep2 = more.tables()
        shift = np.uint64(self.stream_len)
        return Corpus.from_tables(np.concatenate([ds, ds2[1:] + shift]), np.concatenate([rl, rl2]),
                                  np.concatenate([ep, ep2 + shift]), self.names + more.names, self.device)

    def save(self, path):
        """X.docs (write_docs) from the device's tables."""
        ds, rl, ep = self.tables()
        write_docs(path, ds, rl, ep, self.names)


class HipCorpusSearcher:
    """A corpus and the searcher of its stream: where does q occur, in which files?"""

    def __init__(self, corpus, searcher=None):
        self.corpus = corpus
        self.searcher = searcher if searcher is not None else corpus.build_index()
        if self.searcher.n != corpus.stream_len + 1:
            raise ValueError("the index has %d rows, the corpus stream %d bytes" % (self.searcher.n, corpus.stream_len))
        self._L = _lib.load()
        self._doc_start = None                  # doc_start[n_docs + 1], fetched by the first lines call

    @classmethod
    def open(cls, base, bigEndian=True, device=0):
        """X.bwt / X.aux / X.docs as `python -m findex_amd.index --dir D --out X` writes them."""
        return cls(Corpus.load(str(base) + ".docs", device=device), HipFMSearcher(str(base) + ".bwt", bigEndian=bigEndian, device=device))

    def close(self):
        self.searcher.close()
        self.corpus.close()

    def append_documents(self, docs, names=None, context=None):
        """A NEW HipCorpusSearcher over this corpus followed by the raw documents `docs`: their stream (fmx_corpus_build) is
        appended to the index on the device (HipFMSearcher.append_text) and the document tables are concatenated -- what
        Corpus.from_documents of all the documents and its index would be, without sorting the old stream again.  This
        searcher is untouched; the caller closes both.  Default names go on counting from this corpus's documents."""
        docs = [bytes(d) for d in docs]
        if not docs:
            raise ValueError("no documents to append")
        if names is None:
            names = [b"%d" % (self.corpus.n_docs + d) for d in range(len(docs))]
        more = Corpus.from_documents(docs, names, self.corpus.device)
        try:
            stream = more.stream()
            more.drop_stream()
            searcher = self.searcher.append_text(stream, context=context)
            try:
                return HipCorpusSearcher(self.corpus.extended(more), searcher)
            except Exception:
                searcher.close()
                raise
        finally:
            more.close()

    def locate_docs(self, q, max_hits=None, max_mismatches=0, words=False, ignore_case=False, ignore_marks=False):
        """(doc, raw_off) arrays of the occurrences of the raw bytes q, sorted by (doc, raw_off): q is escaped, its reverse
        searched, the rows located (locate_text's arithmetic with the escaped length) and the positions mapped.

        max_mismatches > 0 (up to 3): the windows of the stream within that many substituted bytes of the escaped q as well,
        as (doc, raw_off, mismatches) sorted by (doc, raw_off); max_hits then bounds the rows taken of every distinct matching
        string.  Bytes are substituted from 2 .. 254 only, so the separator byte 1 is never one of them and no hit spans two
        files.  One known limit: q is compared in its escaped form, so a substitution may fall on one half of an escape pair
        (the backslash or the digit that stand for a raw 0, 1 or 255) -- such a window counts one mismatch although its raw
        bytes differ otherwise, and a window whose raw bytes differ in an escaped byte may be missed.

        words=True (exact search only): whole-word occurrences, HipFMSearcher.locate_words on the escaped stream -- a raw
        byte 0, 1 or 255 next to q shows the second byte of its escape pair there, which is a word byte.

        ignore_case=True (exact search only): q in every ASCII case spelling that occurs (HipFMSearcher.locate_fold, or
        locate_words(fold=ASCII_FOLD) with words=True).

        ignore_case="unicode" (exact search; with words=True whole words, HipFMSearcher.search_words(classes=..)): q, read as UTF-8, in every case spelling that occurs, classes
        of several bytes included (HipFMSearcher.search_classes_batch, DESIGN.md 30: k / U+212A, s / U+017F); ignore_marks=True
        adds the precomposed accented forms of every letter.  A spelling may have another length than q, so the result is
        (doc, raw_off, stream_len) sorted by (doc, raw_off, stream_len)."""
        if ignore_marks and ignore_case != "unicode":
            raise ValueError('ignore_marks=True goes with ignore_case="unicode"')
        if ignore_case == "unicode":
            if max_mismatches:
                raise ValueError('ignore_case="unicode" goes with max_mismatches=0')
            esc = escape(q)
            if not esc:
                raise ValueError("empty pattern")
            keep = lambda m: escape(m) == m
            if words:
                _, hits = self.searcher.search_words([esc], classes="marks" if ignore_marks else "unicode", keep=keep)
            else:
                el, el_off, table = self.searcher.unicode_table([esc], ignore_marks, keep=keep)
                _, hits = self.searcher.search_classes_batch(el, el_off, table)
            pos, lens = self.searcher.locate_spellings(hits, max_hits)
            doc, _, raw = self.corpus.map(pos)
            order = np.lexsort((lens, raw, doc))
            return doc[order], raw[order], lens[order]
        if words and max_mismatches:
            raise ValueError("words=True goes with max_mismatches=0")
        if ignore_case and max_mismatches:
            raise ValueError("ignore_case=True goes with max_mismatches=0")
        if not max_mismatches:
            if ignore_case:
                pos = (self.searcher.locate_words(escape(q), max_hits=max_hits, fold=ASCII_FOLD) if words else
                       self.searcher.locate_fold(escape(q), max_hits=max_hits))
            else:
                pos = (self.searcher.locate_words if words else self.searcher.locate_text)(escape(q), max_hits=max_hits)
            doc, _, raw = self.corpus.map(pos)
            order = np.lexsort((raw, doc))
            return doc[order], raw[order]
        esc = escape(q)
        if not esc:
            raise ValueError("empty pattern")
        _, hits = self.searcher.search_approx_batch(np.frombuffer(esc[::-1], dtype=np.uint8), np.array([0, len(esc)], dtype=np.uint64),
                                                    int(max_mismatches), sub=(2, 254))
        off, sa = self.searcher.locate_intervals(hits["sp"], hits["ep"], max_per=max_hits)
        mism = np.repeat(hits["mismatches"], np.diff(off).astype(np.int64))
        doc, _, raw = self.corpus.map(HipFMSearcher.text_offsets(sa, self.searcher.n, len(esc)))
        order = np.lexsort((raw, doc))
        return doc[order], raw[order], mism[order]

    def locate_docs_edits(self, q, max_edits, max_hits=None):
        """Where strings within max_edits (0 .. 2) substitutions, insertions and deletions of the raw bytes q stand in the
        files: (doc, raw_off, stream_len, edits) arrays sorted by (doc, raw_off, stream_len).  q is escaped and its reverse
        searched (HipFMSearcher.search_edit_batch), every hit's rows located with the hit's own length and the positions
        mapped; stream_len is the length of the string that stands there, in stream (escaped) bytes; max_hits bounds the
        rows taken of every distinct matching string.  Bytes are substituted and inserted from 2 .. 254 only, so the
        separator byte 1 is never one of them and no hit spans two files.  One known limit, that of locate_docs: q is compared
        in its escaped form, so an edit may fall on one half of an escape pair (the backslash or the digit that stand for a
        raw 0, 1 or 255) -- such a stretch counts one edit although its raw bytes differ otherwise, and a stretch whose raw
        bytes differ in an escaped byte may be missed."""
        esc = escape(q)
        if not esc:
            raise ValueError("empty pattern")
        _, hits = self.searcher.search_edit_batch(np.frombuffer(esc[::-1], dtype=np.uint8), np.array([0, len(esc)], dtype=np.uint64),
                                                  int(max_edits), sub=(2, 254))
        off, sa = self.searcher.locate_intervals(hits["sp"], hits["ep"], max_per=max_hits)
        per = np.diff(off).astype(np.int64)
        ln = np.repeat(hits["len"], per).astype(np.uint64)
        edits = np.repeat(hits["edits"], per).astype(np.uint32)
        doc, _, raw = self.corpus.map(np.uint64(self.searcher.n - 1) - ln - sa)
        order = np.lexsort((ln, raw, doc))
        return doc[order], raw[order], ln[order], edits[order]

    def shared_passages(self, q, min_len, max_len=None, max_per=None):
        """Which stretches of the raw bytes q stand in the corpus, and where: rows (q_off, len, doc, raw_off) of a uint64
        array sorted by (q_off, doc, raw_off) -- the passage that begins at byte q_off of q begins at byte raw_off of
        document doc.  q is escaped and its maximal exact matches with the stream of min_len stream bytes and more are
        taken (HipFMSearcher.mems_text; at most max_per positions per match), the positions mapped by the corpus and q_off
        mapped back to the raw query by the escape's own prefix counts.  `len` is in stream (escaped) bytes.  The escaped q
        never holds the separator byte 1, so no passage spans two files.  One known limit: the query is compared in its
        escaped form, so a match may begin or end inside an escape pair (the backslash or the digit that stand for a raw
        0, 1 or 255); its q_off and raw_off are then those of the byte the pair stands for."""
        raw = np.frombuffer(bytes(q), dtype=np.uint8)
        special = (raw == 0) | (raw == 1) | (raw == 255)
        first = np.arange(raw.size, dtype=np.int64) + np.cumsum(special) - special      # where raw byte i begins in the escaped q
        esc = escape(q)
        to_raw = np.zeros(len(esc), dtype=np.uint64)
        to_raw[first] = np.arange(raw.size, dtype=np.uint64)
        to_raw[first[special] + 1] = np.nonzero(special)[0].astype(np.uint64)
        rows = self.searcher.mems_text(esc, min_len, max_len, max_per)
        out = np.zeros((rows.shape[0], 4), dtype=np.uint64)
        if rows.shape[0]:
            doc, _, raw_off = self.corpus.map(rows[:, 2])
            out[:, 0], out[:, 1], out[:, 2], out[:, 3] = to_raw[rows[:, 0].astype(np.int64)], rows[:, 1], doc, raw_off
            out = out[np.lexsort((out[:, 3], out[:, 2], out[:, 0]))]
        return out

    # ---- the corpus against itself: which passages stand in it more than once (HipFMSearcher.repeats)
    def duplicate_passages(self, min_len, keep_first=True):
        """The stretches of the files whose every window of min_len stream bytes occurs more than once in the corpus: rows
        (doc, raw_start, raw_end) of a uint64 array sorted by (doc, raw_start).  keep_first: the first occurrence of every
        repeated window (in stream order: the documents' order) is left out, so the rows are what a reader may delete and
        still find every passage once.  The repeats of the stream with the separator byte 1 as the stop byte, so no row
        spans two files; the two ends of a range are mapped by the corpus.  min_len is in stream (escaped) bytes.  One known
        limit: the stream is compared in its escaped form, so a range may begin or end inside an escape pair (the backslash
        or the digit that stand for a raw 0, 1 or 255); its offsets are then those of the byte the pair stands for."""
        ranges, _ = self.searcher.repeats(int(min_len), keep_first=keep_first, stop=1)
        out = np.zeros((ranges.shape[0], 3), dtype=np.uint64)
        if ranges.shape[0]:
            doc, _, lo = self.corpus.map(ranges[:, 0])
            _, _, hi = self.corpus.map(ranges[:, 1] - np.uint64(1))
            out[:, 0], out[:, 1], out[:, 2] = doc, lo, hi + np.uint64(1)
            out = out[np.lexsort((out[:, 1], out[:, 0]))]
        return out

    def duplicate_bytes(self, min_len, keep_first=True):
        """The raw bytes of every document that duplicate_passages covers (uint64[n_docs])."""
        rows = self.duplicate_passages(min_len, keep_first)
        out = np.zeros(self.corpus.n_docs, dtype=np.uint64)
        np.add.at(out, rows[:, 0].astype(np.int64), rows[:, 2] - rows[:, 1])
        return out

    # ---- the most frequent phrases of the corpus (HipFMSearcher.ngrams)
    def frequent_phrases(self, length, min_count=2, top=100):
        """The windows of `length` stream bytes that occur min_count times and more in the corpus, the `top` most frequent
        of them: a list of rows (text, count, n_docs, first_doc, first_raw_off) by descending count -- the phrase's raw
        bytes, how often it occurs, in how many documents, and the document and raw offset of its first occurrence (in
        stream order: the documents' order).  The n-grams of the stream with the separator byte 1 as the stop byte, so no
        phrase spans two files; the bytes come from the index (extract_text_batch) and are unescaped by the map, the
        documents from fmx_corpus_doc_list over the phrase's interval, the first occurrence from the map.  `length` is in
        stream (escaped) bytes.  One known limit: the stream is compared in its escaped form, so a window may begin or end
        inside an escape pair (the backslash or the digit that stand for a raw 0, 1 or 255); its text is then that of the raw
        bytes the first occurrence touches, and its offset that of the byte the pair stands for."""
        length = int(length)
        rec, _ = self.searcher.ngrams(length, min_count=min_count, top=top, order="count", stop=1)
        if not rec.size:
            return []
        _, _, ep = self.corpus.tables()
        lo = rec["first_pos"].copy()
        hi = lo + np.uint64(length)
        if ep.size:                      # a window that begins on a pair's second byte or ends on its backslash: the whole pair
            at = np.minimum(np.searchsorted(ep, lo - np.uint64(1)), ep.size - 1)
            lo = np.where((lo > 0) & (ep[at] == lo - np.uint64(1)), lo - np.uint64(1), lo)
            at = np.minimum(np.searchsorted(ep, hi - np.uint64(1)), ep.size - 1)
            hi = np.where(ep[at] == hi - np.uint64(1), hi + np.uint64(1), hi)
        off, data = self.searcher.extract_text_batch(lo, hi - lo)
        texts = unescape_ranges(data, off, lo, ep)
        doc_off, _, _ = self._doc_list(rec["sp"], rec["sp"] + rec["count"], length)
        n_docs = np.diff(doc_off.astype(np.int64))
        doc, _, raw = self.corpus.map(rec["first_pos"])
        return [(texts[i], int(rec["count"][i]), int(n_docs[i]), int(doc[i]), int(raw[i])) for i in range(rec.size)]

    # ---- the text itself, from the index alone (HipFMSearcher.extract_text_batch): no stream in HBM, no X.data on disk
    def read(self, doc, raw_off, length):
        """The raw bytes [raw_off, raw_off + length) of document doc, clipped at the document's end (arrays or scalars) -> a
        list of bytes.  The map backwards gives the stream range (stream_positions), the index its bytes, the map the raw
        bytes again (unescape_ranges)."""
        ds, rl, ep = self.corpus.tables()
        d = np.asarray(doc, dtype=np.int64).reshape(-1)
        a = np.asarray(raw_off, dtype=np.uint64).reshape(-1)
        ln = np.asarray(length, dtype=np.uint64).reshape(-1)
        d, a, ln = np.broadcast_arrays(d, a, ln)
        if d.size and (d.min() < 0 or d.max() >= self.corpus.n_docs):
            raise IndexError("document out of range")
        a = np.minimum(a, rl[d])
        b = a + np.minimum(ln, rl[d] - a)
        s0 = stream_positions(ds, ep, d, a)
        s1 = stream_positions(ds, ep, d, b)
        off, data = self.searcher.extract_text_batch(s0, s1 - s0)
        return unescape_ranges(data, off, s0, ep)

    def document(self, d):
        """The whole file d, as it was on disk."""
        _, rl, _ = self.corpus.tables()
        return self.read(int(d), 0, int(rl[int(d)]))[0]

    def snippets(self, q, before=40, after=40, max_hits=None, max_mismatches=0):
        """(doc, raw_off, [bytes]): each hit of locate_docs(q, max_hits, max_mismatches) with `before` raw bytes in front of
        it and `after` behind its len(q) bytes, clipped at the file's ends."""
        q = bytes(q)
        doc, raw = self.locate_docs(q, max_hits=max_hits, max_mismatches=max_mismatches)[:2]
        a = raw - np.minimum(raw, np.uint64(before))
        return doc, raw, self.read(doc, a, raw - a + np.uint64(len(q) + int(after)))

    # ---- regexes over the files (HipFMSearcher.finditer)
    def grep(self, regexes, mode="disjoint", max_steps=0, max_per=None, text=False, lineOnly=False, words=False, ignore_case=False):
        """Where a batch of regexes matches inside the files: (off, occ, truncated) as HipFMSearcher.finditer gives them, with
        the corpus -- a match that does not lie inside one file is dropped before the reduction, and every occurrence carries
        doc, raw_off and raw_len (offset and length in the file on disk).  text=True: a fourth value, the matched raw bytes
        of every occurrence (read).  The regexes are matched against the escaped stream: a raw 0, 1 or 255 stands there as its
        escape pair, and an end that falls inside a pair maps to the byte the pair stands for.  words=True: whole-word
        matches only (grep -w; HipFMSearcher.finditer(words=True)); the separator between two files is a word boundary.
        ignore_case=True: grep -i, HipFMSearcher.finditer(ignore_case=True)."""
        off, occ, truncated = self.searcher.finditer(regexes, mode=mode, max_steps=max_steps, max_per=max_per, lineOnly=lineOnly,
                                                     corpus=self.corpus, words=words, ignore_case=ignore_case)
        if not text:
            return off, occ, truncated
        return off, occ, truncated, self.read(occ["doc"], occ["raw_off"], occ["raw_len"]) if occ.size else []

    # ---- lines (HipFMSearcher.line_of / occurrence_lines): the break set holds 10 and 1, so no line spans two files
    def _lines_table(self):
        """The searcher's line table with the separator in its set: {10, 1} is built unless the handle has a table whose set
        holds byte 1 already (a call on the bare searcher would build {10}, under which a line runs across files)."""
        _, bset, _, nbytes, _ = self.searcher.lines_info()
        if not nbytes or 1 not in bset:
            self.searcher.lines_prepare(b"\n\x01")

    def _doc_lines(self, docs=None):
        """(g0, count) of the documents `docs` (all when None): the global index of a document's first line and its number of
        lines as `wc -l` counts them, the last unterminated line counted.  Two lookups per document asked for: at its first
        position and at its separator."""
        self._lines_table()
        if self._doc_start is None:
            self._doc_start = self.corpus.tables()[0]        # (a corpus never changes: extended() makes a new one)
        ds = self._doc_start
        d = np.arange(self.corpus.n_docs) if docs is None else np.asarray(docs, dtype=np.int64).reshape(-1)
        if d.size and (d.min() < 0 or d.max() >= self.corpus.n_docs):
            raise IndexError("document out of range")
        sep = ds[d + 1] - np.uint64(1)
        line, start, _ = self.searcher.line_of(np.concatenate([ds[d], sep]))
        g0 = line[:d.size].astype(np.int64)
        count = line[d.size:].astype(np.int64) - g0 + (start[d.size:] < sep)
        return g0, count

    def line_count(self, doc=None):
        """The lines of document doc (an int64 array over all documents when None): its newlines, plus one when the file does
        not end in one."""
        if doc is None:
            return self._doc_lines()[1]
        return int(self._doc_lines([int(doc)])[1][0])

    def _span_texts(self, start, end):
        """The raw bytes of the stream ranges [start, end) -- whole lines, so both ends map exactly -> a list of bytes."""
        start = np.asarray(start, dtype=np.uint64).reshape(-1)
        if not start.size:
            return []
        doc, _, ro = self.corpus.map(start)
        ro2 = self.corpus.map(end)[2]
        return self.read(doc, ro, ro2 - ro)

    def line(self, doc, line_no):
        """Line line_no (1-based) of document doc, without its newline."""
        g0, count = self._doc_lines([int(doc)])
        if not 1 <= int(line_no) <= int(count[0]):
            raise IndexError("document %d has %d lines" % (int(doc), int(count[0])))
        start, end = self.searcher.line_spans([int(g0[0]) + int(line_no) - 1])
        return self._span_texts(start, end)[0]

    def grep_lines(self, regexes, mode="disjoint", max_steps=0, max_per=None, text=False, before=0, after=0, lineOnly=False,
                   max_line=None, words=False, ignore_case=False):
        """grep, reduced to lines: (off, hits, truncated) -- regex i's matching lines are hits[off[i]:off[i + 1]], a
        HipFMSearcher.LINE_HIT array in (file, line) order, each with its 1-based line_no in the file, its raw_off / raw_len
        there and n_hits, the matches that begin on it.  text=True (or any context): a fourth value, the lines' raw bytes; a
        line longer than max_line (when given) is cut to that many bytes around its first match.  before / after > 0: a
        fifth value, per hit ([lines before], [lines after]), at most that many, clipped to the file."""
        self._lines_table()
        off, occ, truncated = self.grep(regexes, mode=mode, max_steps=max_steps, max_per=max_per, lineOnly=lineOnly, words=words,
                                        ignore_case=ignore_case)
        loff, hits = self.searcher.occurrence_lines(off, occ, corpus=self.corpus)
        return self._lines_result(loff, hits, truncated, off, occ, hits["group"], text, before, after, max_line)

    def _lines_result(self, loff, hits, truncated, off, occ, occ_group, text, before, after, max_line):
        """What grep_lines returns for the line hits (loff, hits): the texts and the context when asked for.  occ_group: per
        hit the group of (off, occ) its `first` counts in; a hit without a first match (first == UINT32_MAX) is cut from
        the line's beginning."""
        before, after = int(before), int(after)
        if not (text or before or after):
            return loff, hits, truncated
        a, ln = hits["raw_off"].copy(), hits["raw_len"].astype(np.uint64)
        if max_line is not None and hits.size:
            has = hits["first"] != np.uint32(0xFFFFFFFF)
            at = np.where(has, off[np.where(has, occ_group, 0)].astype(np.int64) + hits["first"].astype(np.int64), 0)
            first = np.where(has, occ["raw_off"][at] if occ.size else a, a)
            cut = ln > np.uint64(max_line)
            lead = np.minimum(first - a, np.uint64(int(max_line) // 2))
            a = np.where(cut, first - lead, a)
            ln = np.where(cut, np.minimum(np.uint64(max_line), hits["raw_off"] + ln - a), ln)
        lines = self.read(hits["doc"], a, ln) if hits.size else []
        if not (before or after):
            return loff, hits, truncated, lines
        docs, d = np.unique(hits["doc"].astype(np.int64), return_inverse=True)      # the documents with hits alone
        g0, count = self._doc_lines(docs)
        no = hits["line_no"].astype(np.int64)
        nb = np.minimum(no - 1, before)
        na = np.maximum(np.minimum(count[d] - no, after), 0)
        want = [np.arange(g - b, g + 1 + x) for g, b, x in zip((g0[d] + no - 1).tolist(), nb.tolist(), na.tolist())]
        texts = self._span_texts(*self.searcher.line_spans(np.concatenate(want))) if want else []
        context, at = [], 0
        for b, x in zip(nb.tolist(), na.tolist()):
            context.append((texts[at:at + b], texts[at + b + 1:at + b + 1 + x]))
            at += b + 1 + x
        return loff, hits, truncated, lines, context

    def grep_lines_where(self, queries, mode="disjoint", max_steps=0, max_per=None, text=False, before=0, after=0, lineOnly=False,
                         max_line=None, words=False, ignore_case=False):
        """Line queries over regexes (HipFMSearcher.line_query): queries = [(anchor_regex_or_None, [(regex,
        window, negate), ..]), ..] -> what grep_lines returns, with groups equal to query indices.  Query q's lines are the
        lines that hold its anchor regex (every line of every file when None) and satisfy all its terms: a term asks for a
        line with `regex` within `window` lines in the same file (0: the same line, "file": anywhere in the file), or with
        negate for none.  The distinct regexes of all queries are matched in one grep and reduced to lines once; the algebra
        runs on the device.  A line "holds" a regex when a match begins on it (lineOnly, or mode "all" / "longest", for
        grep's strict sense)."""
        queries = [(a, list(terms)) for a, terms in queries]
        regexes, number = [], {}
        for r in [a for a, _ in queries if a is not None] + [t[0] for _, terms in queries for t in terms]:
            if r not in number:
                number[r] = len(regexes)
                regexes.append(r)
        self._lines_table()
        if regexes:
            off, occ, truncated = self.grep(regexes, mode=mode, max_steps=max_steps, max_per=max_per, lineOnly=lineOnly, words=words,
                                            ignore_case=ignore_case)
            loff, hits = self.searcher.occurrence_lines(off, occ, corpus=self.corpus)
        else:                                                # only anchors without terms: one empty group
            off, occ, truncated = np.zeros(2, dtype=np.uint64), np.zeros(0, dtype=self.searcher.OCCURRENCE), False
            loff, hits = np.zeros(2, dtype=np.uint64), np.zeros(0, dtype=self.searcher.LINE_HIT)
        lq = [(None if a is None else number[a], [(number[r], w, neg) for r, w, neg in terms]) for a, terms in queries]
        qoff, out = self.searcher.line_query(loff, hits, lq, corpus=self.corpus)
        anchors = np.array([0 if a is None else a for a, _ in lq], dtype=np.int64)
        return self._lines_result(qoff, out, truncated, off, occ, anchors[out["group"].astype(np.int64)], text, before, after, max_line)

    def grep_lines_inverted(self, regexes, mode="disjoint", max_steps=0, max_per=None, text=False, before=0, after=0, lineOnly=False,
                            max_line=None, words=False, ignore_case=False):
        """grep -v: per regex the lines of all files on which no match of it begins; returns what grep_lines returns."""
        return self.grep_lines_where([(None, [(r, 0, True)]) for r in regexes], mode=mode, max_steps=max_steps, max_per=max_per,
                                     text=text, before=before, after=after, lineOnly=lineOnly, max_line=max_line, words=words,
                                     ignore_case=ignore_case)

    def _intervals(self, queries):
        esc = [escape(q)[::-1] for q in queries]
        if any(not e for e in esc):
            raise ValueError("empty pattern")
        off = np.zeros(len(esc) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(e) for e in esc])
        sp, ep = self.searcher.search_batch(np.frombuffer(b"".join(esc), dtype=np.uint8), off)
        return esc, sp, ep

    def list_docs(self, queries, max_per=None, cap=None):
        """fmx_corpus_doc_list per query: the CSR triple (off[k + 1], doc[], cnt[]) -- query i occurs cnt[j] times in
        document doc[j] for off[i] <= j < off[i + 1], documents ascending.  Queries of one escaped length share a call."""
        queries = [bytes(q) for q in queries]
        esc, sp, ep = self._intervals(queries)
        lens = np.array([len(e) for e in esc], dtype=np.uint64)
        per = [(np.zeros(0, np.uint32), np.zeros(0, np.uint32))] * len(queries)
        for m in sorted(set(lens.tolist())):
            sel = np.nonzero(lens == m)[0]
            o, d, c = self._doc_list(sp[sel], ep[sel], m, max_per, cap)
            for t, i in enumerate(sel.tolist()):
                per[i] = (d[int(o[t]):int(o[t + 1])], c[int(o[t]):int(o[t + 1])])
        off = np.zeros(len(queries) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([p[0].size for p in per])
        cat = (lambda j: np.concatenate([p[j] for p in per]) if per else np.zeros(0, np.uint32))
        return off, cat(0), cat(1)

    def _doc_list(self, sp, ep, pat_len, max_per=None, cap=None):
        sp = np.ascontiguousarray(sp, dtype=np.uint64)
        ep = np.ascontiguousarray(ep, dtype=np.uint64)
        if cap is None:
            cnt = np.where(ep > sp, ep - sp, 0).astype(np.uint64)
            if max_per is not None:
                cnt = np.minimum(cnt, np.uint64(max_per))
            cap = int(np.minimum(cnt, np.uint64(self.corpus.n_docs + 1)).sum())
        off = np.zeros(sp.size + 1, dtype=np.uint64)
        doc = np.zeros(max(cap, 1), dtype=np.uint32)
        cnt = np.zeros(max(cap, 1), dtype=np.uint32)
        _lib.check(self._L.fmx_corpus_doc_list(self.corpus.handle, self.searcher.handle, _ptr(sp), _ptr(ep), sp.size, int(pat_len),
                                               int(max_per or 0), _ptr(off), _ptr(doc), _ptr(cnt), int(cap)))
        m = min(int(cap), int(off[-1]))
        return off, doc[:m], cnt[:m]

    def count_docs(self, q):
        """In how many documents q occurs."""
        off, _, _ = self.list_docs([q])
        return int(off[1])

    # ---- ranked retrieval (fmx_corpus_rank)
    def rank(self, queries, top=10, k1=1.2, b=0.75, match="any", weights=None, max_per=None, words=False, ignore_case=False,
             ignore_marks=False):
        """fmx_corpus_rank: the `top` best files of every query by BM25.  `queries` is a list of lists of raw byte strings
        (terms; substrings, as everywhere in this index), escaped and searched here.  match="any": a file that holds at
        least one term of a query is a candidate; "all": only a file that holds every term.  weights: one float per term in
        the order given (default: the BM25 idf from the document frequencies).  -> (off, doc, score, df, weight): query i's
        files are doc[off[i]:off[i + 1]], best first (equal scores by document number), with their scores; df and weight per
        term.  Terms of any lengths share the one call.  words=True: a term counts only where it stands as a whole word
        (HipFMSearcher.search_words on the escaped stream; a term slot is then the set of row ranges that pass, fmx_corpus_rank_sets).
        ignore_case=True: a term counts in every ASCII case spelling (HipFMSearcher.search_fold_batch, or search_words(fold=
        ASCII_FOLD) with words=True): a term slot is the set of the intervals of the spellings that occur.
        ignore_case="unicode": every UTF-8 case spelling, classes of several bytes included (HipFMSearcher.search_classes_batch,
        or search_words(classes=..) with words=True); ignore_marks=True: precomposed accented forms as well."""
        if match not in ("any", "all"):
            raise ValueError("match is 'any' or 'all'")
        q_off, (sp, ep, set_off, _) = self._query_slots(queries, words, ignore_case, ignore_marks)
        return self._rank_slots(sp, ep, set_off, q_off, top=top, k1=k1, b=b, match=match, weights=weights, max_per=max_per)

    def _query_slots(self, queries, words, ignore_case, ignore_marks=False, same_len=False):
        queries = [[bytes(t) for t in q] for q in queries]
        q_off = np.zeros(len(queries) + 1, dtype=np.uint64)
        q_off[1:] = np.cumsum([len(q) for q in queries])
        return q_off, self._term_slots([t for q in queries for t in q], words, ignore_case, ignore_marks, same_len)

    def _term_slots(self, terms, words=False, ignore_case=False, ignore_marks=False, same_len=False):
        """The one term search of rank() and passages(): (sp, ep, set_off, term_len) of the raw byte strings `terms`, one slot
        each.  set_off is None where a slot is one interval (exact substrings); with words / ignore_case a slot is the set of
        row ranges sp / ep[set_off[t]:set_off[t + 1]].  term_len[t]: the escaped length, which every interval of slot t shares.
        ignore_case="unicode": the spellings of a slot may differ in length; term_len[t] is the length of slot t's spellings
        where they agree, the escaped length for a slot without one or with spellings that do not agree -- which with same_len
        is a ValueError that names the term and two of the lengths."""
        esc = [escape(t) for t in terms]
        term_len = np.array([len(e) for e in esc], dtype=np.uint32)
        if ignore_marks and ignore_case != "unicode":
            raise ValueError('ignore_marks=True goes with ignore_case="unicode"')
        if ignore_case == "unicode":
            if not terms:
                return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(1, dtype=np.uint64), term_len
            if any(not e for e in esc):
                raise ValueError("empty pattern")
            keep = lambda m: escape(m) == m
            if words:
                set_off, hits = self.searcher.search_words(esc, classes="marks" if ignore_marks else "unicode", keep=keep)
            else:
                el, el_off, table = self.searcher.unicode_table(esc, ignore_marks, keep=keep)
                try:                                             # a first guess at the room spares the counting call's search
                    set_off, hits = self.searcher.search_classes_batch(el, el_off, table, cap=64 * len(esc) + 1024)
                except _lib.FmxError as e:
                    if e.code != _lib.FMX_ERR_OVERFLOW:
                        raise
                    set_off, hits = self.searcher.search_classes_batch(el, el_off, table)
            for t in range(len(esc)):
                lens = hits["len"][int(set_off[t]):int(set_off[t + 1])]
                if lens.size:
                    if same_len and int(lens.min()) != int(lens.max()):
                        raise ValueError("the spellings of %r differ in length (%d and %d bytes): passages take one length per term"
                                         % (terms[t], int(lens.min()), int(lens.max())))
                    if int(lens.min()) == int(lens.max()):
                        term_len[t] = int(lens[0])
            return hits["sp"], hits["ep"], set_off, term_len
        if terms and words:
            if any(not e for e in esc):
                raise ValueError("empty pattern")
            set_off, runs = self.searcher.search_words(esc, fold=ASCII_FOLD if ignore_case else None)
            return runs["sp"], runs["ep"], set_off, term_len
        if terms and ignore_case:
            esc = [e[::-1] for e in esc]
            if any(not e for e in esc):
                raise ValueError("empty pattern")
            off = np.zeros(len(esc) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(e) for e in esc])
            pat = np.frombuffer(b"".join(esc), dtype=np.uint8)
            try:                                                 # a first guess at the room spares the counting call's search
                set_off, hits = self.searcher.search_fold_batch(pat, off, ASCII_FOLD, cap=64 * len(esc) + 1024)
            except _lib.FmxError as e:
                if e.code != _lib.FMX_ERR_OVERFLOW:
                    raise
                set_off, hits = self.searcher.search_fold_batch(pat, off, ASCII_FOLD)
            return hits["sp"], hits["ep"], set_off, term_len
        if terms:
            _, sp, ep = self._intervals(terms)
        else:
            sp = ep = np.zeros(0, dtype=np.uint64)
        return sp, ep, None, term_len

    def _rank_slots(self, sp, ep, set_off, q_off, **kw):
        if set_off is None:
            return self.rank_intervals(sp, ep, q_off, **kw)
        return self.rank_sets_intervals(sp, ep, set_off, q_off, **kw)

    def rank_intervals(self, sp, ep, q_off, top=10, k1=1.2, b=0.75, match="any", weights=None, max_per=None, cap=None):
        """rank() for term slots given as row intervals of the index; q_off[n_queries + 1] cuts them into queries."""
        sp = np.ascontiguousarray(sp, dtype=np.uint64).reshape(-1)
        ep = np.ascontiguousarray(ep, dtype=np.uint64).reshape(-1)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64).reshape(-1)
        n_queries = q_off.size - 1
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if weights.size != sp.size:
                raise ValueError("%d weights for %d terms" % (weights.size, sp.size))
        prm = _lib.fmx_rank_params(float(k1), float(b), int(max_per or 0), int(top), _lib.FMX_RANK_ALL if match == "all" else 0)
        if cap is None:
            cap = max(n_queries, 0) * max(int(top), 0)
        off = np.zeros(max(n_queries, 0) + 1, dtype=np.uint64)
        doc = np.zeros(max(cap, 1), dtype=np.uint32)
        score = np.zeros(max(cap, 1), dtype=np.float64)
        df = np.zeros(max(sp.size, 1), dtype=np.uint32)
        w = np.zeros(max(sp.size, 1), dtype=np.float64)
        _lib.check(self._L.fmx_corpus_rank(self.corpus.handle, self.searcher.handle, _ptr(sp), _ptr(ep), sp.size, _ptr(q_off),
                                           n_queries, ctypes.byref(prm), _ptr(weights) if weights is not None else None,
                                           _ptr(off), _ptr(doc), _ptr(score), int(cap), _ptr(df), _ptr(w)))
        m = int(off[-1])
        return off, doc[:m], score[:m], df[:sp.size], w[:sp.size]

    def rank_sets_intervals(self, sp, ep, set_off, q_off, top=10, k1=1.2, b=0.75, match="any", weights=None, max_per=None, cap=None):
        """fmx_corpus_rank_sets: rank_intervals where term slot t is the SET of intervals sp / ep[set_off[t]:set_off[t + 1]]
        (disjoint row ranges: what search_words leaves); weights, df and weight are per slot."""
        sp = np.ascontiguousarray(sp, dtype=np.uint64).reshape(-1)
        ep = np.ascontiguousarray(ep, dtype=np.uint64).reshape(-1)
        set_off = np.ascontiguousarray(set_off, dtype=np.uint64).reshape(-1)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64).reshape(-1)
        n_queries, n_terms = q_off.size - 1, set_off.size - 1
        if sp.size != ep.size or n_terms < 0:
            raise ValueError("sp and ep differ in length, or set_off is empty")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if weights.size != n_terms:
                raise ValueError("%d weights for %d terms" % (weights.size, n_terms))
        prm = _lib.fmx_rank_params(float(k1), float(b), int(max_per or 0), int(top), _lib.FMX_RANK_ALL if match == "all" else 0)
        if cap is None:
            cap = max(n_queries, 0) * max(int(top), 0)
        off = np.zeros(max(n_queries, 0) + 1, dtype=np.uint64)
        doc = np.zeros(max(cap, 1), dtype=np.uint32)
        score = np.zeros(max(cap, 1), dtype=np.float64)
        df = np.zeros(max(n_terms, 1), dtype=np.uint32)
        w = np.zeros(max(n_terms, 1), dtype=np.float64)
        _lib.check(self._L.fmx_corpus_rank_sets(self.corpus.handle, self.searcher.handle, _ptr(sp), _ptr(ep), sp.size,
                                                set_off.ctypes.data_as(ctypes.c_void_p), n_terms, _ptr(q_off), n_queries,
                                                ctypes.byref(prm), _ptr(weights) if weights is not None else None, _ptr(off),
                                                _ptr(doc), _ptr(score), int(cap), _ptr(df), _ptr(w)))
        m = int(off[-1])
        return off, doc[:m], score[:m], df[:n_terms], w[:n_terms]

    def rank_files(self, query_terms, top=10, k1=1.2, b=0.75, match="any", weights=None, max_per=None, words=False, ignore_case=False,
                   window=None, ignore_marks=False):
        """The `top` best files of ONE query (a list of raw byte strings): [(name, score)], best first.  With `window`:
        [(name, score, raw_off, text)], text = the raw bytes of the file's best passage of `window` stream bytes (rank_passages)."""
        if window is None:
            _, doc, score, _, _ = self.rank([list(query_terms)], top=top, k1=k1, b=b, match=match, weights=weights, max_per=max_per,
                                            words=words, ignore_case=ignore_case, ignore_marks=ignore_marks)
            return [(self.corpus.names[int(d)], float(s)) for d, s in zip(doc, score)]
        _, doc, score, _, _, psg, _ = self.rank_passages([list(query_terms)], top=top, window=window, k1=k1, b=b, match=match, weights=weights,
                                                         max_per=max_per, words=words, ignore_case=ignore_case, ignore_marks=ignore_marks)
        texts = self.read(doc, psg["raw_off"], psg["raw_len"]) if doc.size else []
        return [(self.corpus.names[int(d)], float(s), int(o), t) for d, s, o, t in zip(doc, score, psg["raw_off"], texts)]

    def rank_last(self):
        """fmx_corpus_rank_last: {locate_ms, postings_ms, score_ms, select_ms, rows, postings, candidates} of this thread's
        last ranking."""
        ms = [ctypes.c_double() for _ in range(4)]
        n = [ctypes.c_uint64() for _ in range(3)]
        _lib.check(self._L.fmx_corpus_rank_last(*[ctypes.byref(x) for x in ms + n]))
        keys = ("locate_ms", "postings_ms", "score_ms", "select_ms", "rows", "postings", "candidates")
        return dict(zip(keys, [float(x.value) for x in ms] + [int(x.value) for x in n]))

    # ---- passages of ranked hits (fmx_corpus_passages)
    PASSAGE = np.dtype([("raw_off", np.uint64), ("mask", np.uint64), ("value", np.float64), ("raw_len", np.uint32), ("n_occ", np.uint32)])

    def passages_sets_intervals(self, sp, ep, set_off, term_len, q_off, hit_off, hit_doc, window=160, weights=None, max_per=None, cap=None):
        """fmx_corpus_passages: for every hit (hit_off / hit_doc: rank()'s off / doc) the best window of `window` stream bytes
        and the count of every term slot in the hit's file.  Slots as rank_sets_intervals takes them (set_off None: a slot is
        one interval); term_len[t]: the stream length of slot t's strings.  -> (psg, tf): psg a structured array (raw_off, mask,
        value, raw_len, n_occ) per hit, tf[n_hits, stride] with stride = the longest query's slots."""
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        sp, ep, q_off, hit_off = u64(sp), u64(ep), u64(q_off), u64(hit_off)
        term_len = np.ascontiguousarray(term_len, dtype=np.uint32).reshape(-1)
        hit_doc = np.ascontiguousarray(hit_doc, dtype=np.uint32).reshape(-1)
        n_queries, n_terms = q_off.size - 1, term_len.size
        if set_off is not None:
            set_off = u64(set_off)
            if set_off.size != n_terms + 1:
                raise ValueError("set_off has %d entries for %d terms" % (set_off.size, n_terms))
        if sp.size != ep.size or hit_off.size != q_off.size or n_queries < 0:
            raise ValueError("sp and ep, or q_off and hit_off, differ in length")
        n_hits = int(hit_off[-1])
        if hit_doc.size != n_hits:
            raise ValueError("%d hit documents for %d hits" % (hit_doc.size, n_hits))
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if weights.size != n_terms:
                raise ValueError("%d weights for %d terms" % (weights.size, n_terms))
        if cap is None:
            cap = n_hits
        stride_max = int(np.diff(q_off.astype(np.int64)).max()) if n_queries > 0 else 0
        prm = _lib.fmx_passage_params(int(window), int(max_per or 0), 0, 0)
        psg = np.zeros(max(cap, 1), dtype=self.PASSAGE)
        tf = np.zeros(max(cap * max(stride_max, 0), 1), dtype=np.uint32)
        stride = ctypes.c_uint32(0)
        _lib.check(self._L.fmx_corpus_passages(self.corpus.handle, self.searcher.handle, _ptr(sp), _ptr(ep), sp.size,
                                               _ptr(set_off) if set_off is not None else None, n_terms, _ptr(term_len), _ptr(q_off),
                                               n_queries, _ptr(hit_off), _ptr(hit_doc), _ptr(weights) if weights is not None else None,
                                               ctypes.byref(prm), psg.ctypes.data_as(ctypes.c_void_p), _ptr(tf), int(cap),
                                               ctypes.byref(stride)))
        m = min(int(cap), n_hits)
        return psg[:m], tf[:m * stride.value].reshape(m, stride.value)

    def passages(self, queries, hit_off, hit_doc, window=160, weights=None, max_per=None, words=False, ignore_case=False,
                 ignore_marks=False):
        """passages_sets_intervals for `queries` as rank() takes them, searched the same way (one helper: _term_slots).  Under
        ignore_case="unicode" every spelling of a term must have one length: a ValueError names a term of which they differ."""
        q_off, (sp, ep, set_off, term_len) = self._query_slots(queries, words, ignore_case, ignore_marks, same_len=True)
        return self.passages_sets_intervals(sp, ep, set_off, term_len, q_off, hit_off, hit_doc, window=window, weights=weights, max_per=max_per)

    def rank_passages(self, queries, top=10, window=160, k1=1.2, b=0.75, match="any", weights=None, max_per=None, words=False,
                      ignore_case=False, ignore_marks=False):
        """One term search, then the ranking, then the passages of its hits with the ranking's weights.
        -> (off, doc, score, df, weight, psg, tf): rank()'s five, then passages()' two.  ignore_case="unicode": as passages()."""
        if match not in ("any", "all"):
            raise ValueError("match is 'any' or 'all'")
        q_off, (sp, ep, set_off, term_len) = self._query_slots(queries, words, ignore_case, ignore_marks, same_len=True)
        off, doc, score, df, w = self._rank_slots(sp, ep, set_off, q_off, top=top, k1=k1, b=b, match=match, weights=weights, max_per=max_per)
        psg, tf = self.passages_sets_intervals(sp, ep, set_off, term_len, q_off, off, doc, window=window, weights=w, max_per=max_per)
        return off, doc, score, df, w, psg, tf

    def passages_last(self):
        """fmx_corpus_passages_last: {locate_ms, filter_ms, sort_ms, window_ms, rows, occurrences, hits} of this thread's last call."""
        ms = [ctypes.c_double() for _ in range(4)]
        n = [ctypes.c_uint64() for _ in range(3)]
        _lib.check(self._L.fmx_corpus_passages_last(*[ctypes.byref(x) for x in ms + n]))
        keys = ("locate_ms", "filter_ms", "sort_ms", "window_ms", "rows", "occurrences", "hits")
        return dict(zip(keys, [float(x.value) for x in ms] + [int(x.value) for x in n]))
