"""The corpus stream and its position map in plain Python: the checker the corpus tests rest on.

A restatement of DirBWTReader's rules (bwtreader.scala:17-173) as one byte loop -- no numpy tricks, no library call -- with
a PER-POSITION table for the map, so that every stream position has its expected (doc, esc_off, raw_off) written down:

  - a directory's files first (names compared as bytes, ascending), then its subdirectories, recursively;
  - a file is binary (dropped by default) when its first 1024 bytes hold a 0, when it is empty, or when it cannot be opened;
  - raw 0 -> '\\' '0', raw 1 -> '\\' '1', raw 255 -> '\\' 'f'; the backslash is not escaped;
  - one separator byte 1 after every file, the last one included."""
import os

ESCAPES = {0: b"\\0", 1: b"\\1", 255: b"\\f"}


def looks_binary(path):
    try:
        with open(path, "rb") as f:
            head = f.read(1024)
    except OSError:
        return True
    if len(head) == 0:
        return True
    for c in head:
        if c == 0:
            return True
    return False


def walk(root, filter_binary=True):
    """Relative names (bytes, '/'-separated) in stream order."""
    root = os.fsencode(root)
    out = []

    def visit(d, prefix):
        entries = sorted(os.listdir(d))
        for e in entries:
            p = os.path.join(d, e)
            if os.path.isfile(p) and not (filter_binary and looks_binary(p)):
                out.append(prefix + e)
        for e in entries:
            p = os.path.join(d, e)
            if os.path.isdir(p):
                visit(p, prefix + e + b"/")

    visit(root, b"")
    return out


def escape_bytes(raw):
    out = bytearray()
    for c in raw:
        out += ESCAPES.get(c, bytes([c]))
    return bytes(out)


class RefCorpus:
    """stream, doc_start[n_docs + 1], esc_pos[], raw_len[] and table[p] = (doc, esc_off, raw_off) for every stream position."""

    def __init__(self, docs):
        self.docs = [bytes(d) for d in docs]
        stream = bytearray()
        self.doc_start, self.esc_pos, self.raw_len, self.table = [], [], [], []
        for d, raw in enumerate(self.docs):
            start = len(stream)
            self.doc_start.append(start)
            self.raw_len.append(len(raw))
            for i, c in enumerate(raw):
                if c in ESCAPES:
                    self.esc_pos.append(len(stream))
                    for b in ESCAPES[c]:
                        self.table.append((d, len(stream) - start, i))      # both bytes stand for raw byte i
                        stream.append(b)
                else:
                    self.table.append((d, len(stream) - start, i))
                    stream.append(c)
            self.table.append((d, len(stream) - start, len(raw)))          # the separator: (d, raw length of d)
            stream.append(1)
        self.doc_start.append(len(stream))
        self.stream = bytes(stream)

    @classmethod
    def from_dir(cls, root, filter_binary=True):
        names = walk(root, filter_binary)
        docs = []
        for nm in names:
            with open(os.path.join(os.fsencode(root), nm), "rb") as f:
                docs.append(f.read())
        c = cls(docs)
        c.names = names
        return c

    def map(self, p):
        if p >= len(self.stream):
            return (0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF)
        return self.table[p]

    def occurrences(self, q):
        """[(doc, raw offset)] of the raw bytes q in every file, overlapping ones included, sorted: bytes.find per file."""
        out = []
        for d, raw in enumerate(self.docs):
            i = raw.find(q)
            while i >= 0:
                out.append((d, i))
                i = raw.find(q, i + 1)
        return out

    def doc_counts(self, q):
        """[(doc, count)] ascending by doc: in which files the raw bytes q occur, and how often (the document listing)."""
        counts = {}
        for d, _ in self.occurrences(q):
            counts[d] = counts.get(d, 0) + 1
        return sorted(counts.items())

    def list_positions(self, positions):
        """[(doc, count)] ascending by doc of stream positions looked up in the per-position table; None stands for "no
        stream position", and those are counted in a last entry (0xFFFFFFFF, count) when there are any."""
        counts, none = {}, 0
        for p in positions:
            if p is None:
                none += 1
            else:
                d = self.table[p][0]
                counts[d] = counts.get(d, 0) + 1
        out = sorted(counts.items())
        if none:
            out.append((0xFFFFFFFF, none))
        return out
