"""Line queries in plain Python / numpy, written from the definitions of include/fmx.h: the key of a record, the
real lines of a text or a corpus stream from lines_ref.Lines, a term as a loop over the candidates with np.searchsorted on the
packed keys of the term's group.  python_query answers the same questions file by file with `in` on split lines."""
import numpy as np

import lines_ref
from lines_ref import LINE_HIT, NO_DOC

ALL_LINES = None
FILE = 0xFFFFFFFF


def keys_of(hits):
    return (hits["doc"].astype(np.uint64) << np.uint64(32)) | hits["line_no"].astype(np.uint64)


def real_lines(lines, docs=None):
    """The LINE_HIT records of the real lines of the text `lines` stands for (a lines_ref.Lines; over a corpus stream, with the
    break set {10, 1}, docs is its corpus_ref.RefCorpus): every global line but the empty piece behind a final break."""
    L = np.arange(lines.n_brk + 1, dtype=np.int64)
    start, end = lines.start(L), lines.end(L)
    if docs is None:
        real = start != lines.len
    else:
        seps = np.array(docs.doc_start[1:], dtype=np.int64) - 1
        real = ~np.isin(start, seps) & (start < lines.len)
    L, start, end = L[real], start[real], end[real]
    rec = np.zeros(L.size, dtype=LINE_HIT)
    rec["doc"], rec["line_no"], rec["start"], rec["len"] = NO_DOC, L + 1, start, end - start
    rec["n_hits"], rec["first"], rec["raw_off"], rec["raw_len"] = 0, 0xFFFFFFFF, start, end - start
    if docs is not None:
        for r, s, e, l_ in zip(rec, start.tolist(), end.tolist(), L.tolist()):
            d, _, ro = docs.table[s]
            assert docs.table[e][0] == d, "a line spans two documents"
            r["doc"], r["raw_off"], r["raw_len"] = d, ro, docs.table[e][2] - ro
            r["line_no"] = l_ - int(lines.line(docs.doc_start[d])) + 1
    return rec


def satisfies(key, term_keys, window):
    """Does the sorted key list hold a record (d, j) with max(1, i - window) <= j <= i + window for key = (d, i)?"""
    d, i = int(key) >> 32, int(key) & 0xFFFFFFFF
    lo = (d << 32) | max(1, i - int(window))
    hi = (d << 32) | min(i + int(window), 0xFFFFFFFF)
    p = int(np.searchsorted(term_keys, np.uint64(lo), side="left"))
    return p < term_keys.size and int(term_keys[p]) <= hi


def line_query(off, hits, queries, lines=None, docs=None):
    """(out_off, records) of queries = [(anchor or None, [(group, window or "file", negate), ..]), ..] over the CSR line-hit
    list (off, hits).  lines / docs: what real_lines takes, needed by a query whose anchor is None."""
    off = np.asarray(off, dtype=np.int64)
    group_keys = [keys_of(hits[off[g]:off[g + 1]]) for g in range(off.size - 1)]
    out, out_off = [], [0]
    every = None
    for q, (anchor, terms) in enumerate(queries):
        if anchor is None:
            if every is None:
                every = real_lines(lines, docs)
            cand = every.copy()
        else:
            cand = hits[off[anchor]:off[anchor + 1]].copy()
        keep = np.ones(cand.size, dtype=bool)
        for g, window, negate in terms:
            w = FILE if window == "file" else int(window)
            for c, k in enumerate(keys_of(cand).tolist()):
                if keep[c]:
                    keep[c] = satisfies(k, group_keys[g], w) != bool(negate)
        cand = cand[keep]
        cand["group"] = q
        out.append(cand)
        out_off.append(out_off[-1] + cand.size)
    return np.array(out_off, dtype=np.uint64), np.concatenate(out) if out else np.zeros(0, dtype=LINE_HIT)


def python_query(docs, anchor, terms):
    """[(doc, 1-based line number, line)] of the query over raw documents, file by file: split on newlines, `in`.  anchor: a
    needle or None for every line; terms: [(needle, window or "file", negate), ..]."""
    out = []
    for d, raw in enumerate(docs):
        pieces = raw.split(b"\n")
        if raw.endswith(b"\n") or not raw:
            pieces = pieces[:-1]
        for i, ln in enumerate(pieces):
            if anchor is not None and anchor not in ln:
                continue
            ok = True
            for needle, window, negate in terms:
                lo, hi = (0, len(pieces)) if window == "file" else (max(0, i - window), min(len(pieces), i + window + 1))
                ok = ok and any(needle in x for x in pieces[lo:hi]) != bool(negate)
            if ok:
                out.append((d, i + 1, ln))
    return out


def hits_of_needles(docs, needles, ref=None):
    """(off, hits) as fmx_occurrence_lines would leave them for the literal needles over the corpus `docs` (raw documents
    without bytes that need an escape when ref is None): from lines_ref.occurrence_lines over the stream."""
    import corpus_ref
    ref = ref or corpus_ref.RefCorpus(docs)
    S = lines_ref.Lines(ref.stream, b"\n\x01")
    T = np.frombuffer(ref.stream, dtype=np.uint8)
    occ_dtype = np.dtype([("group", np.uint32), ("len", np.uint32), ("pos", np.uint64), ("doc", np.uint32), ("raw_len", np.uint32),
                          ("raw_off", np.uint64)])
    off, recs = [0], []
    for g, needle in enumerate(needles):
        pos, i = [], ref.stream.find(needle)
        while i >= 0:
            pos.append(i)
            i = ref.stream.find(needle, i + 1)
        r = np.zeros(len(pos), dtype=occ_dtype)
        r["group"], r["len"], r["pos"] = g, len(needle), pos
        recs.append(r)
        off.append(off[-1] + len(pos))
    assert T.size == S.len
    return lines_ref.occurrence_lines(S, np.array(off, dtype=np.uint64), np.concatenate(recs), docs=ref), S, ref


WORDS = (b"alpha", b"bravo", b"cedar", b"delta", b"ember")


def seeded_corpus(seed=7):
    """37 documents of 0 .. 39 lines over five words (a line holds 0 .. 3 of the words a document draws from), among them an
    empty file, a file that is "\\n" and files without a final newline."""
    rng = np.random.RandomState(seed)
    docs = []
    for d in range(37):
        own = [w for w in WORDS if rng.rand() < 0.7] or [WORDS[0]]
        n_lines = int(rng.randint(0, 40))
        lines = [b" ".join(own[i] for i in rng.randint(0, len(own), size=rng.randint(0, 4))) for _ in range(n_lines)]
        raw = b"\n".join(lines) + (b"\n" if lines and rng.rand() < 0.7 else b"")
        docs.append(raw)
    docs[3], docs[11], docs[20] = b"", b"\n", docs[20].rstrip(b"\n") + b" alpha"
    return docs


def five_queries(A=b"alpha", B=b"bravo", C=b"cedar"):
    """(name, anchor needle or None, [(needle, window, negate)]) of the five questions of the tests."""
    return [("A and B", A, [(B, 0, False)]), ("A not C", A, [(C, 0, True)]), ("-v A", None, [(A, 0, True)]),
            ("A near/2 B", A, [(B, 2, False)]), ("A, B in the file, C nowhere in it", A, [(B, "file", False), (C, "file", True)])]
