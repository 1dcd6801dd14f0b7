"""Ranked retrieval over a corpus index: which files are the best matches for these words?

    python -m findex_amd.rank BASE "words of a query" ["another query" ..] [--top K] [--all] [-w] [-i] [--k1 X] [--b X] [--device D]
                                                                            [--little-endian] [--snippets [W]] [--explain]
                                                                            [--unicode-case [--ignore-marks]]

BASE names BASE.bwt / BASE.aux / BASE.docs as `python -m findex_amd.index --dir D --out BASE` writes them.  Every positional
argument is one query, split on white space into its terms.  Without -w terms are SUBSTRINGS, as everywhere in this index:
`cat` counts in `concatenate` too.  With -w / --words a term counts only where it stands as a whole word: the bytes next to it are
not 0-9 A-Z a-z _ or 0x80 .. 0xFF, or the file ends there (HipFMSearcher.search_words).  A file is scored by BM25 over its terms' occurrence counts
(HipCorpusSearcher.rank, fmx_corpus_rank: scored and cut to the best K on the device).  Output: one line per hit,
`score<TAB>file`, best first; the queries' blocks are separated by a blank line.  --all keeps only files that hold every term of
the query.  -i / --ignore-case counts a term in every ASCII case spelling that occurs (HipFMSearcher.search_fold_batch: `error` finds
Error and ERROR too); it combines with -w.  --unicode-case reads the terms as UTF-8 and counts a term in every case spelling
of its code points that occurs, classes of several bytes included (HipFMSearcher.search_classes_batch: `über` finds Über, `kelvin`
the Kelvin sign, `miss` the long s); --ignore-marks adds the precomposed accented forms of every letter (`cafe` finds café).  It
combines with -w; with --snippets or --explain only where every spelling of a term has one length.  --snippets [W] prints under every hit `<TAB>offset<TAB>text`: the file's window of W
stream bytes (default 160) that holds the most valuable set of the query's terms, by the ranking's weights, read back from the
index (HipCorpusSearcher.rank_passages, fmx_corpus_passages); bytes below 0x20 are shown as a space.  --explain prints under every
hit `<TAB>term=tf ..`: how often each term of the query occurs in the file, the counts the score was computed from.
"""
import argparse
import sys


def parser():
    ap = argparse.ArgumentParser(prog="python -m findex_amd.rank", description=__doc__.split("\n\n")[0],
                                 epilog="Without -w terms are substrings, as everywhere in this index; with -w they are whole words.")
    ap.add_argument("base")
    ap.add_argument("query", nargs="+", help="the words of one query, split on white space; every word is matched as a substring unless -w is given")
    ap.add_argument("--top", type=int, default=10, metavar="K", help="files per query, 1 .. 1024 (default 10)")
    ap.add_argument("--all", dest="all_", action="store_true", help="only files that hold every term of the query")
    ap.add_argument("-w", "--words", action="store_true", help="a term counts only where it stands as a whole word")
    ap.add_argument("-i", "--ignore-case", action="store_true", help="a term counts in every ASCII case spelling")
    ap.add_argument("--unicode-case", action="store_true",
                    help="terms are UTF-8; a term counts in every case spelling of its code points (K / k / the Kelvin sign)")
    ap.add_argument("--ignore-marks", action="store_true", help="with --unicode-case: precomposed accented forms of a letter count too")
    ap.add_argument("--snippets", type=int, nargs="?", const=160, default=None, metavar="W",
                    help="under every hit its best passage of W stream bytes (default 160): <TAB>offset<TAB>text")
    ap.add_argument("--explain", action="store_true", help="under every hit the count of every term in the file: <TAB>term=tf ..")
    ap.add_argument("--k1", type=float, default=1.2)
    ap.add_argument("--b", type=float, default=0.75)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--little-endian", action="store_true")
    return ap


def split_queries(queries, utf8=False):
    """Each query string split on white space into its terms, as bytes (the file system's encoding, like the names; utf8: UTF-8,
    a byte the command line could not decode kept as it is)."""
    import os
    if utf8:
        return [[w.encode("utf-8", "surrogateescape") for w in q.split()] for q in queries]
    return [[os.fsencode(w) for w in q.split()] for q in queries]


def flags_of(a):
    """The keyword arguments of HipCorpusSearcher.rank / rank_passages that the parsed arguments ask for."""
    kw = {"words": True} if a.words else {}
    if a.unicode_case:
        kw["ignore_case"] = "unicode"
        if a.ignore_marks:
            kw["ignore_marks"] = True
    elif a.ignore_case:
        kw["ignore_case"] = True
    return kw


def render(names, off, doc, score):
    """The output lines (bytes, without newlines): `score<TAB>file` per hit, a blank line between two queries."""
    rows = []
    for i in range(len(off) - 1):
        if i:
            rows.append(b"")
        for j in range(int(off[i]), int(off[i + 1])):
            rows.append(repr(float(score[j])).encode() + b"\t" + names[int(doc[j])])
    return rows


_CONTROL = bytes(range(0x20))


def render_passages(names, off, doc, score, queries, raw_off=None, texts=None, tf=None):
    """render()'s lines with, under every hit, `<TAB>raw_off<TAB>text` when raw_off / texts are given (bytes below 0x20 in the
    text shown as a space) and `<TAB>term=tf ..` in query order when the tf rows are given (queries: the terms as bytes)."""
    rows = []
    for i in range(len(off) - 1):
        if i:
            rows.append(b"")
        for j in range(int(off[i]), int(off[i + 1])):
            rows.append(repr(float(score[j])).encode() + b"\t" + names[int(doc[j])])
            if texts is not None:
                rows.append(b"\t" + str(int(raw_off[j])).encode() + b"\t" + bytes(texts[j]).translate(bytes.maketrans(_CONTROL, b" " * 32)))
            if tf is not None:
                rows.append(b"\t" + b" ".join(t + b"=" + str(int(tf[j][s])).encode() for s, t in enumerate(queries[i])))
    return rows


def main(argv=None):
    a = parser().parse_args(argv)
    if not 1 <= a.top <= 1024:
        parser().error("--top is 1 .. 1024")
    if a.snippets is not None and not 1 <= a.snippets < (1 << 32):
        parser().error("--snippets is 1 .. 2^32 - 1")
    if a.ignore_marks and not a.unicode_case:
        parser().error("--ignore-marks goes with --unicode-case")
    queries = split_queries(a.query, utf8=a.unicode_case)
    from .corpus import HipCorpusSearcher
    cs = HipCorpusSearcher.open(a.base, bigEndian=not a.little_endian, device=a.device)
    try:
        kw = flags_of(a)
        out = sys.stdout.buffer
        if a.snippets is not None or a.explain:
            off, doc, score, _, _, psg, tf = cs.rank_passages(queries, top=a.top, window=a.snippets or 160, k1=a.k1, b=a.b,
                                                              match="all" if a.all_ else "any", **kw)
            texts = None
            if a.snippets is not None:
                texts = cs.read(doc, psg["raw_off"], psg["raw_len"]) if doc.size else []
            rows = render_passages(cs.corpus.names, off, doc, score, queries, psg["raw_off"], texts, tf if a.explain else None)
        else:
            off, doc, score, _, _ = cs.rank(queries, top=a.top, k1=a.k1, b=a.b, match="all" if a.all_ else "any", **kw)
            rows = render(cs.corpus.names, off, doc, score)
        for row in rows:
            out.write(row + b"\n")
        out.flush()
    finally:
        cs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
