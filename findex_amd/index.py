"""python -m findex_amd.index X.txt [--little-endian] [--device N]

Writes X.bwt and X.aux next to the input (BWTTempStorage.genBWTFilename / genAuxFilename, bwtmerger.scala:17-24: the
extension swapped), the files BWTMerger2.merge(FileBWTReader) writes -- the BWT of the reversed file -- big-endian
unless --little-endian.  The suffix sort runs on the device (fmx_bwt_from_text).  A file containing byte 0 is refused:
findex's readers escape it, and this tool does no escaping."""
import argparse
import os
import sys


def output_names(path):
    """(X.bwt, X.aux) for X.txt, as genBWTFilename / genAuxFilename name them."""
    base = os.path.splitext(path)[0]
    return base + ".bwt", base + ".aux"


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m findex_amd.index", description=__doc__.split("\n\n")[1])
    ap.add_argument("text")
    ap.add_argument("--little-endian", action="store_true", help="write little-endian headers and counts")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
