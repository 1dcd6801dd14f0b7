"""python -m findex_amd.index X.txt [--chunk BYTES] [--little-endian] [--device N] [--fm] [--sa] [--lcp] [--dups L] [--ngrams L[,L..] [--min-count C] [--top K]]
python -m findex_amd.index --dir D --out X [--no-filter-binary] [--data] [--little-endian] [--device N] [--fm] [--sa] [--lcp] [--dups L] [--ngrams L[,L..] [--min-count C] [--top K]]
python -m findex_amd.index --append BASE (FILE | --dir D) [--no-filter-binary] [--little-endian] [--device N] [--fm] [--sa] [--lcp] [--dups L]

Writes X.bwt and X.aux next to the input (BWTTempStorage.genBWTFilename / genAuxFilename, bwtmerger.scala:17-24: the
extension swapped), the files BWTMerger2.merge(FileBWTReader) writes -- the BWT of the reversed file -- big-endian
unless --little-endian.  The suffix sort runs on the device (fmx_bwt_from_text).  A file containing byte 0 is refused:
findex's readers escape it, and this tool does no escaping.

--fm, --sa and --lcp add the sibling files the reference's IndexerApp and SACreator write (genFMFilename / genSAFilename /
genLCPFilename: the extension swapped): X.fm (FMCreator), X.sa (SACreator: n big-endian int32) and X.lcp (LCPCreator:
n - 1 big-endian int32), through the writers of the handle opened on the two files just written.

--dups L (L >= 1) adds X.dups, the stretches of the input whose every window of L bytes occurs more than once
(HipFMSearcher.repeats): one line start<TAB>end per range of the file.  With --dir it lists the passages a reader may delete
and lose nothing -- every copy but the first (HipCorpusSearcher.duplicate_passages) -- as name<TAB>raw_start<TAB>raw_end, by
document and offset; L is then in stream (escaped) bytes and no passage spans two files.

--ngrams L[,L..] adds X.ngrams, the strings of L bytes that occur --min-count times and more (default 2), the --top most
frequent of every length (default 100; 0: all), most frequent first (HipFMSearcher.ngrams): one line
L<TAB>count<TAB>first offset<TAB>bytes per string.  With --dir the lines are the rows of HipCorpusSearcher.frequent_phrases,
L<TAB>count<TAB>files<TAB>name<TAB>raw offset<TAB>bytes -- in how many files the phrase stands, and the file and offset of
its first occurrence; L is then in stream (escaped) bytes and no phrase spans two files.  In the bytes everything outside
0x21 .. 0x7e, and the backslash, is written as a backslash, an x and two hex digits.

--dir D --out X indexes a directory the way the reference's IndexerApp does through DirBWTReader (bwtreader.scala:17-173):
the files of D in a fixed order, binary ones dropped unless --no-filter-binary, bytes 0, 1 and 255 escaped, a separator
byte 1 after every file (findex_amd/corpus.py).  It writes X.bwt and X.aux of that stream, X.docs (this project's own side
file: which stream positions belong to which file), and with --data X.data, the stream itself -- what
DirBWTReader(caching = true) leaves at genDataFilename.  Escaping and the suffix sort run on the device.

--chunk BYTES builds X.bwt / X.aux chunk by chunk: the first BYTES bytes by the suffix sort, the rest appended to that
index on the device (HipFMSearcher.append_text) -- the same files, and the way to a text beyond 2^32 - 2 bytes.

--append BASE merges new text into the index BASE.bwt / BASE.aux without rebuilding it and rewrites both.  With a
BASE.docs beside them the index is a corpus: FILE (named by its base name) or the files of --dir D become further documents
and BASE.docs is rewritten too; without one FILE's bytes are appended to the indexed text.  Side files of the old index
(BASE.fm, .sa, .lcp, .dups) are rewritten when their flags are given and removed otherwise, with a line on stderr: they are
never left stale.  --ngrams is not taken here, and a BASE.ngrams is removed likewise.  --little-endian must be given as it was when BASE was written."""
import argparse
import os
import sys


def output_names(path):
    """(X.bwt, X.aux) for X.txt, as genBWTFilename / genAuxFilename name them."""
    base = os.path.splitext(path)[0]
    return base + ".bwt", base + ".aux"


def sibling_names(path):
    """(X.fm, X.sa, X.lcp) for X.txt, as genFMFilename / genSAFilename / genLCPFilename name them."""
    base = os.path.splitext(path)[0]
    return base + ".fm", base + ".sa", base + ".lcp"


def dups_threshold(text):
    """--dups L: an int >= 1 (below 2^32, a threshold of fmx_repeats)."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("--dups takes an integer, got %r" % text)
    if not 1 <= v < 2 ** 32:
        raise argparse.ArgumentTypeError("--dups takes a length of at least 1")
    return v


def ngram_lengths(text):
    """--ngrams L[,L..]: 1 .. 64 ints >= 1 (below 2^32, the lengths of one fmx_ngrams call)."""
    try:
        v = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("--ngrams takes integers separated by commas, got %r" % text)
    if not 1 <= len(v) <= 64 or any(not 1 <= x < 2 ** 32 for x in v):
        raise argparse.ArgumentTypeError("--ngrams takes 1 to 64 lengths of at least 1")
    return v


def count_arg(least):
    """--min-count C (C >= 1), --top K (K >= 0)"""
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError("an integer is expected, got %r" % text)
        if not least <= v < 2 ** 63:
            raise argparse.ArgumentTypeError("at least %d is expected" % least)
        return v
    return parse


def printable(b):
    """The bytes of an X.ngrams line: 0x21 .. 0x7e as they are, the backslash and everything else as \\xHH."""
    return b"".join(bytes([c]) if 0x21 <= c <= 0x7E and c != 0x5C else b"\\x%02X" % c for c in bytes(b))


def ngrams_name(a):
    """X.ngrams: beside the other outputs."""
    return a.out + ".ngrams" if getattr(a, "dir", None) else os.path.splitext(a.text)[0] + ".ngrams"


def write_ngrams(a, hip, corpus=None):
    """X.ngrams of the parsed arguments `a` from the searcher `hip` (of `corpus`' stream) -> the number of lines."""
    lines = 0
    with open(ngrams_name(a), "wb") as f:
        if corpus is not None:
            from .corpus import HipCorpusSearcher
            cs = HipCorpusSearcher(corpus, hip)
            for L in a.ngrams:
                for text, count, n_docs, doc, raw_off in cs.frequent_phrases(L, min_count=a.min_count, top=a.top):
                    f.write(b"%d\t%d\t%d\t" % (L, count, n_docs) + corpus.names[doc] + b"\t%d\t" % raw_off + printable(text) + b"\n")
                    lines += 1
        else:
            for L, (rec, _) in zip(a.ngrams, hip.ngrams(a.ngrams, min_count=a.min_count, top=a.top, order="count")):
                for r, text in zip(rec, hip.ngram_texts(rec, L)):
                    f.write(b"%d\t%d\t%d\t" % (L, int(r["count"]), int(r["first_pos"])) + printable(text) + b"\n")
                    lines += 1
    return lines


def chunk_bytes(text):
    """--chunk BYTES: an int >= 1."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("--chunk takes a number of bytes, got %r" % text)
    if v < 1:
        raise argparse.ArgumentTypeError("--chunk takes at least 1 byte")
    return v


def append_outputs(a):
    """--append BASE: (BASE.bwt, BASE.aux, BASE.docs) and the side files (BASE.fm, .sa, .lcp, .dups), in that order."""
    b = a.append
    return (b + ".bwt", b + ".aux", b + ".docs"), (b + ".fm", b + ".sa", b + ".lcp", b + ".dups")


def dups_name(a):
    """X.dups: beside the other outputs."""
    if getattr(a, "append", None):
        return a.append + ".dups"
    return a.out + ".dups" if getattr(a, "dir", None) else os.path.splitext(a.text)[0] + ".dups"


def parser():
    ap = argparse.ArgumentParser(prog="python -m findex_amd.index", description=__doc__.split("\n\n")[1])
    ap.add_argument("text", nargs="?", help="the file to index (the single-file form)")
    ap.add_argument("--dir", help="index every file under this directory (needs --out)")
    ap.add_argument("--out", help="with --dir: the outputs are OUT.bwt, OUT.aux, OUT.docs ...")
    ap.add_argument("--no-filter-binary", action="store_true", help="with --dir: keep files that look binary")
    ap.add_argument("--data", action="store_true", help="with --dir: also write OUT.data, the escaped stream")
    ap.add_argument("--little-endian", action="store_true", help="write little-endian headers and counts")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fm", action="store_true", help="also write X.fm (FMCreator)")
    ap.add_argument("--sa", action="store_true", help="also write X.sa (SACreator)")
    ap.add_argument("--lcp", action="store_true", help="also write X.lcp (LCPCreator)")
    ap.add_argument("--chunk", type=chunk_bytes, metavar="BYTES", help="build in chunks of BYTES bytes: the first by the suffix sort, the rest appended")
    ap.add_argument("--append", metavar="BASE", help="append FILE, or the files of --dir D, to the index BASE.bwt / BASE.aux [/ BASE.docs]")
    ap.add_argument("--dups", type=dups_threshold, metavar="L", help="also write X.dups: the passages of L bytes and more that occur more than once")
    ap.add_argument("--ngrams", type=ngram_lengths, metavar="L[,L..]", help="also write X.ngrams: the most frequent strings of L bytes")
    ap.add_argument("--min-count", type=count_arg(1), default=2, metavar="C", help="with --ngrams: strings that occur C times and more (default 2)")
    ap.add_argument("--top", type=count_arg(0), default=100, metavar="K", help="with --ngrams: the K most frequent of every length (default 100; 0: all)")
    return ap


def planned_outputs(a):
    """The files a run with the parsed arguments `a` writes, in the order it writes them."""
    dups = getattr(a, "dups", None)
    if getattr(a, "ngrams", None):
        b = argparse.Namespace(**vars(a))
        b.ngrams = None
        return planned_outputs(b) + [ngrams_name(a)]
    if getattr(a, "dir", None):
        base = a.out + ".x"             # (the name functions swap an extension: OUT itself is the stem)
        fm, sa, lcp = sibling_names(base)
        return list(output_names(base)) + [a.out + ".docs"] + ([a.out + ".data"] if a.data else []) + \
            ([fm] if a.fm else []) + ([sa] if a.sa else []) + ([lcp] if a.lcp else []) + ([dups_name(a)] if dups else [])
    fm, sa, lcp = sibling_names(a.text)
    return list(output_names(a.text)) + ([fm] if a.fm else []) + ([sa] if a.sa else []) + ([lcp] if a.lcp else []) + \
        ([dups_name(a)] if dups else [])


def main_dir(a):
    """The --dir form: X.bwt, X.aux, X.docs, then X.data and the siblings that were asked for."""
    from .corpus import Corpus
    from .construct import bwt_from_text, write_bwt
    try:
        corpus = Corpus.from_dir(a.dir, filter_binary=not a.no_filter_binary, device=a.device)
    except ValueError as e:
        print(str(e), file=sys.stderr)
        return 2
    outs = planned_outputs(a)
    bwt_path, aux_path, docs_path = outs[:3]
    try:
        stream = corpus.stream()
        corpus.drop_stream()            # (the files need the stream on the host anyway; the sort gets the HBM)
        bwt, eof, counts = bwt_from_text(stream, device=a.device)
        write_bwt(bwt_path, aux_path, bwt, eof, counts, bigEndian=not a.little_endian)
        corpus.save(docs_path)
        print("%s: %d files, n = %d, eof = %d -> %s, %s, %s" % (a.dir, corpus.n_docs, bwt.size, eof, bwt_path, aux_path, docs_path))
        if a.data:
            stream.tofile(a.out + ".data")
            print("%s: -> %s" % (a.dir, a.out + ".data"))
        if getattr(a, "dups", None):
            from .corpus import HipCorpusSearcher
            from .searcher import HipFMSearcher
            hip = HipFMSearcher.from_mem(bwt, eof, counts, device=a.device)
            try:
                rows = HipCorpusSearcher(corpus, hip).duplicate_passages(a.dups, keep_first=True)
            finally:
                hip.close()
            with open(dups_name(a), "wb") as f:         # (the names are bytes, as the listing gave them)
                for d, lo, hi in rows:
                    f.write(corpus.names[int(d)] + b"\t%d\t%d\n" % (lo, hi))
            print("%s: %d duplicated passages -> %s" % (a.dir, rows.shape[0], dups_name(a)))
        if getattr(a, "ngrams", None):
            from .searcher import HipFMSearcher
            hip = HipFMSearcher.from_mem(bwt, eof, counts, device=a.device)
            try:
                print("%s: %d frequent phrases -> %s" % (a.dir, write_ngrams(a, hip, corpus), ngrams_name(a)))
            finally:
                hip.close()
    finally:
        corpus.close()
    if a.fm or a.sa or a.lcp:
        from .searcher import HipFMSearcher
        fm_path, sa_path, lcp_path = sibling_names(a.out + ".x")
        hip = HipFMSearcher.from_mem(bwt, eof, counts, device=a.device)
        try:
            for wanted, write, path in ((a.fm, hip.write_fm, fm_path), (a.sa, hip.write_sa, sa_path), (a.lcp, hip.write_lcp, lcp_path)):
                if wanted:
                    write(path)
                    print("%s: -> %s" % (a.dir, path))
        finally:
            hip.close()
    return 0


def main_append(a):
    """The --append form: BASE.bwt / BASE.aux (and BASE.docs) rewritten, the side files rewritten or removed."""
    from .construct import write_bwt
    from .corpus import Corpus, HipCorpusSearcher, list_files
    from .searcher import HipFMSearcher
    (bwt_path, aux_path, docs_path), (fm_path, sa_path, lcp_path, dups_path) = append_outputs(a)
    be = not a.little_endian
    is_corpus = os.path.exists(docs_path)
    if a.dir and not is_corpus:
        print("%s: no %s -- --append --dir needs a corpus index (one written with --dir)" % (a.append, docs_path), file=sys.stderr)
        return 2
    if a.dir:
        names, docs = [], []
        for rel in list_files(a.dir, filter_binary=not a.no_filter_binary):
            try:
                with open(os.path.join(os.fsencode(a.dir), *rel.split(b"/")), "rb") as f:
                    docs.append(f.read())
                names.append(rel)
            except OSError:
                continue
        if not docs:
            print("%s: no files to index" % a.dir, file=sys.stderr)
            return 2
    else:
        with open(a.text, "rb") as f:
            data = f.read()
        if not data and not is_corpus:
            print("%s: empty file, nothing to append" % a.text, file=sys.stderr)
            return 2
        if b"\0" in data and not is_corpus:
            print("%s: contains byte 0 at offset %d; findex's readers escape byte 0 and this tool does not -- refused"
                  % (a.text, data.index(b"\0")), file=sys.stderr)
            return 2
        names, docs = [os.fsencode(os.path.basename(a.text))], [data]
    old = new = corpus = None
    try:
        if is_corpus:
            old = HipCorpusSearcher.open(a.append, bigEndian=be, device=a.device)
            new = old.append_documents(docs, names)
            hip, corpus = new.searcher, new.corpus
        else:
            old = HipFMSearcher(bwt_path, bigEndian=be, device=a.device)
            hip = new = old.append_text(data)
        old.close()
        old = None
        write_bwt(bwt_path, aux_path, hip.bwt_bytes(), hip.eof, hip.counts(), bigEndian=be)
        if corpus is not None:
            corpus.save(docs_path)
        print("%s: n = %d, eof = %d -> %s, %s%s" % (a.append, hip.n, hip.eof, bwt_path, aux_path, ", " + docs_path if corpus is not None else ""))
        for wanted, write, path in ((a.fm, hip.write_fm, fm_path), (a.sa, hip.write_sa, sa_path), (a.lcp, hip.write_lcp, lcp_path)):
            if wanted:
                write(path)
                print("%s: -> %s" % (a.append, path))
        if a.dups and corpus is not None:
            rows = new.duplicate_passages(a.dups, keep_first=True)
            with open(dups_path, "wb") as f:
                for d, lo, hi in rows:
                    f.write(corpus.names[int(d)] + b"\t%d\t%d\n" % (lo, hi))
            print("%s: %d duplicated passages -> %s" % (a.append, rows.shape[0], dups_path))
        elif a.dups:
            ranges, _ = hip.repeats(a.dups)
            with open(dups_path, "w") as f:
                for lo, hi in ranges:
                    f.write("%d\t%d\n" % (lo, hi))
            print("%s: %d repeated ranges -> %s" % (a.append, ranges.shape[0], dups_path))
    finally:
        for h in (old, new):
            if h is not None:
                h.close()
    for wanted, path in ((a.fm, fm_path), (a.sa, sa_path), (a.lcp, lcp_path), (a.dups, dups_path), (False, a.append + ".ngrams")):
        if not wanted and os.path.exists(path):
            os.remove(path)
            print("%s: described the index before the append -- removed" % path, file=sys.stderr)
    return 0


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.append:
        if a.out or a.data or a.chunk or a.ngrams or bool(a.text) == bool(a.dir):
            ap.error("--append BASE takes FILE or --dir D (and no --out, --data, --chunk or --ngrams)")
        return main_append(a)
    if a.chunk and a.dir:
        ap.error("--chunk builds a single text file in chunks")
    if a.dir:
        if a.text or not a.out:
            ap.error("--dir takes --out X and no text file")
        return main_dir(a)
    if a.out or a.data or a.no_filter_binary or not a.text:
        ap.error("a text file, or --dir D --out X")
    with open(a.text, "rb") as f:
        data = f.read()
    if not data:
        print("%s: empty file, nothing to index" % a.text, file=sys.stderr)
        return 2
    if b"\0" in data:
        print("%s: contains byte 0 at offset %d; findex's readers escape byte 0 and this tool does not -- refused"
              % (a.text, data.index(b"\0")), file=sys.stderr)
        return 2
    from .construct import bwt_from_text, bwt_from_text_chunked, write_bwt
    if a.chunk or len(data) > (1 << 32) - 2:        # (beyond one suffix sort: chunks are forced)
        bwt, eof, counts = bwt_from_text_chunked(data, a.chunk or 1 << 30, device=a.device)
    else:
        bwt, eof, counts = bwt_from_text(data, device=a.device)
    bwt_path, aux_path = output_names(a.text)
    write_bwt(bwt_path, aux_path, bwt, eof, counts, bigEndian=not a.little_endian)
    print("%s: n = %d, eof = %d -> %s, %s" % (a.text, bwt.size, eof, bwt_path, aux_path))
    if a.fm or a.sa or a.lcp or a.dups or a.ngrams:
        from .searcher import HipFMSearcher
        fm_path, sa_path, lcp_path = sibling_names(a.text)
        hip = HipFMSearcher.from_mem(bwt, eof, counts, device=a.device)
        try:
            for wanted, write, path in ((a.fm, hip.write_fm, fm_path), (a.sa, hip.write_sa, sa_path), (a.lcp, hip.write_lcp, lcp_path)):
                if wanted:
                    write(path)
                    print("%s: -> %s" % (a.text, path))
            if a.dups:
                ranges, _ = hip.repeats(a.dups)
                with open(dups_name(a), "w") as f:
                    for lo, hi in ranges:
                        f.write("%d\t%d\n" % (lo, hi))
                print("%s: %d repeated ranges -> %s" % (a.text, ranges.shape[0], dups_name(a)))
            if a.ngrams:
                print("%s: %d frequent strings -> %s" % (a.text, write_ngrams(a, hip), ngrams_name(a)))
        finally:
            hip.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
