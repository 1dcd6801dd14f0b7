"""grep over a corpus index: where do these regexes match, in which files?

    python -m findex_amd.grep BASE REGEX [REGEX ..] [--mode all|longest|disjoint] [--max-per N] [--max-steps N] [-C BYTES] [--count]
                                                    [-n] [-A N] [-B N] [--context-lines N] [-c] [-l] [--max-line BYTES]
                                                    [-v] [--and REGEX ..] [--not REGEX ..] [--near N | --same-file] [-w] [-i]
                                                    [--unicode-case]

BASE names BASE.bwt / BASE.aux / BASE.docs as `python -m findex_amd.index --dir D --out BASE` writes them.  One line per
match, `name:raw_off:text`, regex by regex in (file, offset) order; -C BYTES shows that many bytes of the file around the
match, cut at newlines; --count prints one count per regex instead.  The regexes are the reference's (REParser.re2post) and are
matched against the escaped stream (HipCorpusSearcher.grep).  -w keeps only matches that stand as whole words: the bytes next
to a match are not 0-9 A-Z a-z _ or 0x80 .. 0xFF, or the file ends there; it applies to every regex of the call, --and / --not
included.  -i ignores ASCII case: every regex of the call, --and / --not included, is read as Python's re reads it under
re.IGNORECASE | re.ASCII (findex_amd.regex.fold_regex; a construct re reads differently, such as an unquoted ^ or {, is
refused) -- but for \\w, \\d and '.', which keep the meaning they have without -i: the bytes A .. y (and z beside them, the
image of Z), 0 .. 8 and 2 .. 254, not re's classes; it combines with -w.  --unicode-case reads the regexes as UTF-8 and
ignores the case of every code point, as Python's re does on str under re.IGNORECASE (findex_amd.regex.fold_regex_unicode: `über`
finds Über, `k` the Kelvin sign, `σ` the final sigma); a set may hold ASCII only and '.' is one byte; it combines with -w, -n and
--and / --not.

By lines (HipCorpusSearcher.grep_lines; any of the flags below): -n prints `name:line_no:line`, one line of output per matching
line, regex by regex in (file, line) order; -A N / -B N / --context-lines N add that many lines after / before / around, as
`name-line_no-line`, with grep's `--` between groups that do not touch; -c prints `name:count` per file with matching lines,
-l the names of those files.  A line longer than --max-line BYTES is cut to that many bytes around its first match.

Line queries (HipCorpusSearcher.grep_lines_where, evaluated on the device; each implies output by lines and combines with the
flags above): every REGEX is one query's anchor; --and X / --not X (repeatable) keep the anchor's lines that also hold / do not
hold X -- on the same line, within --near N lines, or anywhere in the file with --same-file; -v prints the lines on which no
match of REGEX begins.  A line holds a regex when a match BEGINS on it (use --mode all or longest for grep's strict sense of -v
where matches run over line breaks).
"""
import argparse
import sys

import numpy as np


def line_count(s):
    """argparse type of --near: a number of lines, 0 or more."""
    v = int(s)
    if not 0 <= v < 2 ** 32:
        raise argparse.ArgumentTypeError("a number of lines, 0 .. 2^32 - 1")
    return v


def parser():
    ap = argparse.ArgumentParser(prog="python -m findex_amd.grep", description=__doc__.split("\n\n")[0])
    ap.add_argument("base")
    ap.add_argument("regex", nargs="+")
    ap.add_argument("--mode", choices=("all", "longest", "disjoint"), default="disjoint")
    ap.add_argument("--max-per", type=int, default=None, help="rows taken of every distinct matching string")
    ap.add_argument("--max-steps", type=int, default=0, help="longest match explored (0: the library's default)")
    ap.add_argument("-C", dest="context", type=int, default=0, metavar="BYTES")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("-n", "--line-number", action="store_true", help="whole matching lines with their numbers")
    ap.add_argument("-A", dest="after", type=int, default=None, metavar="N", help="lines of context after a matching line")
    ap.add_argument("-B", dest="before", type=int, default=None, metavar="N", help="lines of context before a matching line")
    ap.add_argument("--context-lines", type=int, default=None, metavar="N", help="lines of context on both sides")
    ap.add_argument("-c", "--count-lines", action="store_true", help="matching lines per file")
    ap.add_argument("-l", "--files-with-matches", action="store_true", help="the files with a matching line")
    ap.add_argument("--max-line", type=int, default=4096, metavar="BYTES", help="longer lines are cut around their first match")
    ap.add_argument("-v", "--invert-match", action="store_true", help="the lines on which no match begins")
    ap.add_argument("--and", dest="and_", action="append", default=[], metavar="REGEX", help="only lines that also hold REGEX (repeatable)")
    ap.add_argument("--not", dest="not_", action="append", default=[], metavar="REGEX", help="only lines that do not hold REGEX (repeatable)")
    near = ap.add_mutually_exclusive_group()
    near.add_argument("--near", type=line_count, default=None, metavar="N", help="--and / --not look N lines to either side (default 0: the same line)")
    near.add_argument("--same-file", action="store_true", help="--and / --not look at the whole file")
    ap.add_argument("-w", "--word-regexp", dest="words", action="store_true", help="only matches that stand as whole words")
    ap.add_argument("-i", "--ignore-case", action="store_true", help="ignore ASCII case in every regex of the call")
    ap.add_argument("--unicode-case", action="store_true", help="ignore the case of every code point (UTF-8) in every regex of the call")
    ap.add_argument("--little-endian", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    return ap


def flags_of(a):
    """The keyword arguments -w and -i add to a grep call; none when neither is given."""
    kw = {"words": True} if getattr(a, "words", False) else {}
    if getattr(a, "unicode_case", False):
        kw["ignore_case"] = "unicode"
    elif getattr(a, "ignore_case", False):
        kw["ignore_case"] = True
    return kw


def with_context(cs, occ, context):
    """Every occurrence with up to `context` raw bytes on either side, cut at the nearest newline towards the match."""
    a = occ["raw_off"] - np.minimum(occ["raw_off"], np.uint64(context))
    lead = (occ["raw_off"] - a).astype(np.int64)
    out = []
    for buf, ld, ln in zip(cs.read(occ["doc"], a, occ["raw_off"] - a + occ["raw_len"] + np.uint64(context)), lead.tolist(),
                           occ["raw_len"].tolist()):
        lo = buf.rfind(b"\n", 0, ld) + 1
        hi = buf.find(b"\n", ld + ln)
        out.append(buf[lo:len(buf) if hi < 0 else hi])
    return out


def by_lines(a):
    """Do the arguments ask for output by lines?"""
    return bool(a.line_number or a.count_lines or a.files_with_matches or a.after is not None or a.before is not None
                or a.context_lines is not None or where(a))


def where(a):
    """Do the arguments ask for a line query (-v, --and, --not, --near, --same-file)?"""
    return bool(a.invert_match or a.and_ or a.not_ or a.near is not None or a.same_file)


def queries_of(a):
    """The line queries of the arguments, as HipCorpusSearcher.grep_lines_where takes them: one per positional regex, which
    is the query's anchor -- or, with -v, a negative term on the same line under the anchor "all lines"; every --and / --not
    adds a positive / negative term with the window of --near N (default 0) or --same-file to every query."""
    window = "file" if a.same_file else (a.near or 0)
    extra = [(r, window, False) for r in a.and_] + [(r, window, True) for r in a.not_]
    if a.invert_match:
        return [(None, [(r, 0, True)] + extra) for r in a.regex]
    return [(r, list(extra)) for r in a.regex]


def context_of(a):
    """(before, after) in lines: -B / -A, each falling back to --context-lines."""
    both = a.context_lines or 0
    return (a.before if a.before is not None else both), (a.after if a.after is not None else both)


def format_lines(names, hits, lines, number=True):
    """`name:line_no:line` (`name:line` without numbers) for every hit, in order."""
    return [names[int(h["doc"])] + (b":%d:" % int(h["line_no"]) if number else b":") + t for h, t in zip(hits, lines)]


def format_context(names, hits, lines, context, number=True):
    """The hits of ONE regex with their context lines (grep_lines' fifth value), as grep -A / -B prints them: a matching
    line as `name:line_no:line`, a context line as `name-line_no-line`, every line once, `--` between two groups that neither
    overlap nor touch."""
    matching = {(int(h["doc"]), int(h["line_no"])): t for h, t in zip(hits, lines)}      # (a hit's text may be cut: --max-line)
    out, last = [], None
    for h, t, (bf, af) in zip(hits, lines, context):
        d, no = int(h["doc"]), int(h["line_no"])
        group = [(no - len(bf) + i, x) for i, x in enumerate(bf)] + [(no, t)] + [(no + 1 + i, x) for i, x in enumerate(af)]
        if last is not None and (last[0] != d or group[0][0] > last[1] + 1):
            out.append(b"--")
        for k, x in group:
            if last is not None and last[0] == d and k <= last[1]:
                continue
            sep = b":" if (d, k) in matching else b"-"
            out.append(names[d] + sep + (b"%d" % k + sep if number else b"") + matching.get((d, k), x))
            last = (d, k)
    return out


def format_counts(names, hits):
    """`name:count` per file with matching lines, in file order."""
    docs, counts = np.unique(hits["doc"], return_counts=True)
    return [names[int(d)] + b":%d" % int(c) for d, c in zip(docs, counts)]


def format_files(names, hits):
    """The names of the files with matching lines, in file order."""
    return [names[int(d)] for d in np.unique(hits["doc"])]


def main_lines(cs, a, out):
    before, after = context_of(a)
    names = cs.corpus.names
    w = flags_of(a)
    if where(a):
        queries = queries_of(a)
        grep_lines = lambda _regexes, **kw: cs.grep_lines_where(queries, **w, **kw)
    else:
        grep_lines = lambda regexes, **kw: cs.grep_lines(regexes, **w, **kw)
    if a.count_lines or a.files_with_matches:
        off, hits, truncated = grep_lines(a.regex, mode=a.mode, max_steps=a.max_steps, max_per=a.max_per)
        fmt = format_counts if a.count_lines else format_files
        for i in range(len(a.regex)):
            for row in fmt(names, hits[int(off[i]):int(off[i + 1])]):
                out.write(row + b"\n")
        return truncated
    res = grep_lines(a.regex, mode=a.mode, max_steps=a.max_steps, max_per=a.max_per, text=True, before=before, after=after,
                     max_line=a.max_line)
    off, hits, truncated, lines = res[:4]
    for i in range(len(a.regex)):
        lo, hi = int(off[i]), int(off[i + 1])
        if before or after:
            rows = format_context(names, hits[lo:hi], lines[lo:hi], res[4][lo:hi], a.line_number)
        else:
            rows = format_lines(names, hits[lo:hi], lines[lo:hi], a.line_number)
        for row in rows:
            out.write(row + b"\n")
    return truncated


def main(argv=None):
    a = parser().parse_args(argv)
    from .corpus import HipCorpusSearcher
    cs = HipCorpusSearcher.open(a.base, bigEndian=not a.little_endian, device=a.device)
    try:
        if by_lines(a):
            out = sys.stdout.buffer
            truncated = main_lines(cs, a, out)
            out.flush()
            if truncated:
                print("matches longer than --max-steps were cut", file=sys.stderr)
            return 0
        off, occ, truncated = cs.grep(a.regex, mode=a.mode, max_steps=a.max_steps, max_per=a.max_per, **flags_of(a))
        out = sys.stdout.buffer
        if a.count:
            for i in range(len(a.regex)):
                out.write(b"%d\n" % (int(off[i + 1]) - int(off[i])))
        elif occ.size:
            texts = with_context(cs, occ, a.context) if a.context else cs.read(occ["doc"], occ["raw_off"], occ["raw_len"])
            for o, t in zip(occ, texts):
                out.write(cs.corpus.names[int(o["doc"])] + b":%d:" % int(o["raw_off"]) + t + b"\n")
        out.flush()
        if truncated:
            print("matches longer than --max-steps were cut", file=sys.stderr)
    finally:
        cs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
