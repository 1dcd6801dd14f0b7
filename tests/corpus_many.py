"""Corpora of hundreds to tens of thousands of documents, their query set and the interval lists of the key-width cases:
what tests/test_gpu_corpus_many.py runs on the device and tests/test_corpus_cpu.py holds to the shapes they are for.  All of
it is host work with fixed seeds; nothing here touches the library.

The raw bytes are a..d with about 6 % replaced by 0, 1, 255 or a backslash, so the characters '0', '1' and 'f' never occur:
no raw text reads like an escape pair, and a query without a backslash is found in the stream exactly where it stands in
the files (test_the_unescaped_backslash_is_ambiguous... in test_gpu_corpus.py has the other case).  The one query that keeps
the quirk is the lone backslash: every escape pair begins with one, so the stream holds it wherever a file holds a
backslash, a 0, a 1 or a 255 -- `expected_occurrences` states that union."""
import itertools

import numpy as np

ALPHABET = b"abcd"
SPECIALS = (0, 1, 255, 92)
NO_DOC = 0xFFFFFFFF
MAX_ROWS = 8 << 20              # rows of one listing call of the key-width cases (36 bytes of HBM per row)

# name -> (documents, mean length of a non-empty document, share forced empty, seed)
CORPORA = {
    "D255": (255, 29.5, 0.05, 255),
    "D256": (256, 29.5, 0.05, 256),
    "D257": (257, 29.5, 0.05, 257),
    "D5000": (5000, 29.5, 0.05, 5000),
    "D65537": (65537, 4.0, 0.5, 65537),
}


def documents(name):
    """The corpus `name`: geometric lengths, a share of the documents forced empty, and the documents placed by hand."""
    n_docs, mean, empty, seed = CORPORA[name]
    rng = np.random.default_rng(seed)
    lens = rng.geometric(1.0 / mean, n_docs)
    lens[rng.random(n_docs) < empty] = 0
    raw = rng.choice(np.frombuffer(ALPHABET, dtype=np.uint8), int(lens.sum()))
    special = rng.random(raw.size) < 0.06
    raw[special] = rng.choice(np.array(SPECIALS, dtype=np.uint8), int(special.sum()))
    ends = np.cumsum(lens)
    blob = raw.tobytes()
    docs = [blob[int(e - n):int(e)] for n, e in zip(lens, ends)]
    for at, placed in hand_placed(n_docs).items():
        docs[at:at + len(placed)] = placed
    assert len(docs) == n_docs
    return docs


def hand_placed(n_docs):
    """index -> the documents that overwrite the generated ones from there on."""
    a, b, c = n_docs // 3, n_docs // 2, (2 * n_docs) // 3
    return {
        0: [b""],                                   # an empty document first
        a: [b"\x00"],                               # a document that is one escaped byte
        a + 2: [b"\x01", b"\xff"],                  # two such documents next to each other
        b: [b"\xffabca"],                           # begins with an escape
        b + 2: [b"dcb\x00"],                        # ends with an escape
        c: [b"", b"", b""],                         # a run of three empty documents
        n_docs - 1: [b""],                          # an empty document last
    }


def grams(g):
    return [bytes(t) for t in itertools.product(ALPHABET, repeat=g)]


MISSES = [b"azb", b"abzd"]                          # 'z' is not in the alphabet; one shares a call with the 3-grams
QUERIES = grams(1) + grams(2) + grams(3) + [b"\x00", b"\x01", b"\xff", b"\\", b"a\x00", b"\xffb"] + MISSES


def expected_occurrences(ref, q):
    """[(doc, raw offset)] sorted: ref.occurrences(q), and for the lone backslash the union with the three escaped bytes
    (their pairs begin with a backslash; the map gives such a hit the offset of the byte the pair stands for)."""
    if q == b"\\":
        return sorted(ref.occurrences(b"\\") + ref.occurrences(b"\x00") + ref.occurrences(b"\x01") + ref.occurrences(b"\xff"))
    return ref.occurrences(q)


def expected_doc_counts(ref, q):
    """[(doc, count)] ascending: ref.doc_counts(q), and for the lone backslash the union above, counted per document."""
    if q == b"\\":
        counts = {}
        for part in (b"\\", b"\x00", b"\x01", b"\xff"):
            for d, c in ref.doc_counts(part):
                counts[d] = counts.get(d, 0) + c
        return sorted(counts.items())
    return ref.doc_counts(q)


def csr(per_query):
    """[[(doc, count)]] -> (off uint64[k + 1], doc uint32[], cnt uint32[]) as the listing returns them."""
    off = np.zeros(len(per_query) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in per_query])
    flat = [x for p in per_query for x in p]
    doc = np.array([x[0] for x in flat], dtype=np.uint32)
    cnt = np.array([x[1] for x in flat], dtype=np.uint32)
    return off, doc, cnt


def gram_counts(ref, g):
    """{g-gram over a..d: how often it stands in the files}, one pass over the raw documents (for sizing calls only: what a
    test expects comes from doc_counts)."""
    counts = {}
    for raw in ref.docs:
        for i in range(len(raw) - g + 1):
            w = raw[i:i + g]
            counts[w] = counts.get(w, 0) + 1
    return {w: counts.get(w, 0) for w in grams(g)}


def lib_bits(x):
    """The library's rule for doc_bits (x = n_docs) and k_bits (x = k): the smallest b >= 1 with x >> b == 0."""
    b = 1
    while x >> b:
        b += 1
    return b


# (corpus, k, doc_bits + k_bits, radix passes): what each case is for.  k_bits has room for k itself while the interval numbers
# end at k - 1, so at k = 1, 128 and 2048 the key's top bit is never set and the last pass has nothing to order; the cases
# with k = 12, 200 and 3000 have the same number of passes with the top bit in use.
WIDTH_CASES = [
    ("D255", 1, 9, 2),
    ("D255", 12, 12, 2),
    ("D256", 127, 16, 2),           # exactly two full passes
    ("D256", 128, 17, 3),
    ("D256", 200, 17, 3),
    ("D5000", 2047, 24, 3),
    ("D5000", 2048, 25, 4),
    ("D5000", 3000, 25, 4),
    ("D5000", 70000, 30, 4),
    ("D65537", 40000, 33, 5),       # a key above 32 bits
]


def width_case(ref, k, seed=7):
    """The interval list of a key-width case as k tokens: ("hit", gram), ("miss", None) or ("inverted", gram) -- the last is
    the gram's interval with sp and ep swapped (sp > ep: no rows).  A shuffled list of distinct g-grams (at most 256 of
    them) is repeated, every third entry a miss or an inverted interval in turn, with a miss first and a miss last; k = 1 is
    the widest 1-gram alone.  g is the smallest gram length at which the call stays within MAX_ROWS rows, so a call has as
    many rows as the corpus gives below that.  -> (g, tokens, rows of the call)."""
    if k == 1:
        counts = gram_counts(ref, 1)
        w = max(counts, key=lambda x: (counts[x], x))
        return 1, [("hit", w)], counts[w]
    for g in range(1, 9):
        counts = gram_counts(ref, g)
        rng = np.random.default_rng(seed)
        distinct = [w for w in grams(g) if counts[w]]
        distinct = [distinct[i] for i in rng.permutation(len(distinct))[:256]]
        tokens, rows, j = [("miss", None)], 0, 0
        while len(tokens) < k - 1:
            w = distinct[j % len(distinct)]
            if j % 3 == 2:
                tokens.append(("miss", None) if (j // 3) % 2 == 0 else ("inverted", w))
            else:
                tokens.append(("hit", w))
                rows += counts[w]
            j += 1
        tokens.append(("miss", None))
        if rows <= MAX_ROWS:
            return g, tokens, rows
    raise AssertionError("no gram length keeps %d intervals within %d rows" % (k, MAX_ROWS))
