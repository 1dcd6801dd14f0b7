"""python -m findex_amd.index X.txt [--little-endian] [--device N] [--fm] [--sa] [--lcp]

Writes X.bwt and X.aux next to the input (BWTTempStorage.genBWTFilename / genAuxFilename, bwtmerger.scala:17-24: the
extension swapped), the files BWTMerger2.merge(FileBWTReader) writes -- the BWT of the reversed file -- big-endian
unless --little-endian.  The suffix sort runs on the device (fmx_bwt_from_text).  A file containing byte 0 is refused:
findex's readers escape it, and this tool does no escaping.

--fm, --sa and --lcp add the sibling files the reference's IndexerApp and SACreator write (genFMFilename / genSAFilename /
genLCPFilename: the extension swapped): X.fm (FMCreator), X.sa (SACreator: n big-endian int32) and X.lcp (LCPCreator:
n - 1 big-endian int32), through the writers of the handle opened on the two files just written."""
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


def parser():
    ap = argparse.ArgumentParser(prog="python -m findex_amd.index", description=__doc__.split("\n\n")[1])
    ap.add_argument("text")
    ap.add_argument("--little-endian", action="store_true", help="write little-endian headers and counts")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fm", action="store_true", help="also write X.fm (FMCreator)")
    ap.add_argument("--sa", action="store_true", help="also write X.sa (SACreator)")
    ap.add_argument("--lcp", action="store_true", help="also write X.lcp (LCPCreator)")
    return ap


def planned_outputs(a):
    """The files a run with the parsed arguments `a` writes, in the order it writes them."""
    fm, sa, lcp = sibling_names(a.text)
    return list(output_names(a.text)) + ([fm] if a.fm else []) + ([sa] if a.sa else []) + ([lcp] if a.lcp else [])


def main(argv=None):
    a = parser().parse_args(argv)
    with open(a.text, "rb") as f:
        data = f.read()
    if not data:
        print("%s: empty file, nothing to index" % a.text, file=sys.stderr)
        return 2
    if b"\0" in data:
        print("%s: contains byte 0 at offset %d; findex's readers escape byte 0 and this tool does not -- refused"
              % (a.text, data.index(b"\0")), file=sys.stderr)
        return 2
    from .construct import bwt_from_text, write_bwt
    bwt, eof, counts = bwt_from_text(data, device=a.device)
    bwt_path, aux_path = output_names(a.text)
    write_bwt(bwt_path, aux_path, bwt, eof, counts, bigEndian=not a.little_endian)
    print("%s: n = %d, eof = %d -> %s, %s" % (a.text, bwt.size, eof, bwt_path, aux_path))
    if a.fm or a.sa or a.lcp:
        from .searcher import HipFMSearcher
        fm_path, sa_path, lcp_path = sibling_names(a.text)
        hip = HipFMSearcher.from_mem(bwt, eof, counts, device=a.device)
        try:
            for wanted, write, path in ((a.fm, hip.write_fm, fm_path), (a.sa, hip.write_sa, sa_path), (a.lcp, hip.write_lcp, lcp_path)):
                if wanted:
                    write(path)
                    print("%s: -> %s" % (a.text, path))
        finally:
            hip.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
