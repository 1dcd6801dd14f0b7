"""grep over a corpus index: where do these regexes match, in which files?

    python -m findex_amd.grep BASE REGEX [REGEX ..] [--mode all|longest|disjoint] [--max-per N] [--max-steps N] [-C BYTES] [--count]

BASE names BASE.bwt / BASE.aux / BASE.docs as `python -m findex_amd.index --dir D --out BASE` writes them.  One line per
match, `name:raw_off:text`, regex by regex in (file, offset) order; -C BYTES shows that many bytes of the file around the
match, cut at newlines; --count prints one count per regex instead.  The regexes are the reference's (REParser.re2post) and are
matched against the escaped stream (HipCorpusSearcher.grep).
"""
import argparse
import sys

import numpy as np


def parser():
    ap = argparse.ArgumentParser(prog="python -m findex_amd.grep", description=__doc__.split("\n\n")[0])
    ap.add_argument("base")
    ap.add_argument("regex", nargs="+")
    ap.add_argument("--mode", choices=("all", "longest", "disjoint"), default="disjoint")
    ap.add_argument("--max-per", type=int, default=None, help="rows taken of every distinct matching string")
    ap.add_argument("--max-steps", type=int, default=0, help="longest match explored (0: the library's default)")
    ap.add_argument("-C", dest="context", type=int, default=0, metavar="BYTES")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--little-endian", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    return ap


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


def main(argv=None):
    a = parser().parse_args(argv)
    from .corpus import HipCorpusSearcher
    cs = HipCorpusSearcher.open(a.base, bigEndian=not a.little_endian, device=a.device)
    try:
        off, occ, truncated = cs.grep(a.regex, mode=a.mode, max_steps=a.max_steps, max_per=a.max_per)
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
