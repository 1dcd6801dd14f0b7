"""findex_amd -- MI355X-native FM-index backward search behind findex's SuffixAlgo API.

The compute lives in libfmx.so (hand-written HIP for gfx950, C ABI in include/fmx.h); this
package is the thin host-side mirror of the reference's Scala interface for that path:

    reference (Scala)                              here
    NaiveFMSearcher(filename, bigEndian)           HipFMSearcher(filename, bigEndian=True)
      .n .cf .occ .search .getPrevRange ...          same names, same meaning
    REParser.re2post(str, lineOnly)                REParser.re2post(str, lineOnly=False)
    ReTree(postfix).matchSA(sa)                    ReTree(postfix).matchSA(sa)
    SAResult(sa,len,sp,ep)                         SAResult
    BWTMerger2.merge(FileBWTReader) -> X.bwt/.aux  bwt_from_text(text) + write_bwt(...), python -m findex_amd.index
    BWTMerger2.merge onto an existing index        HipFMSearcher.append_text, .from_text(chunk=), bwt_from_text_chunked,
                                                   HipCorpusSearcher.append_documents, python -m findex_amd.index --append / --chunk
    LCPSuffixWalkingAlgo.getLCP, LCPCreator        HipFMSearcher.getLCP / .lcp / .write_lcp, lcp_from_text(text)
    DirBWTReader(dir) -> one stream, IndexerApp    Corpus.from_dir(dir), HipCorpusSearcher, python -m findex_amd.index --dir
    (beyond the reference)                         HipFMSearcher.match_stats_batch / .mems_batch / .match_stats_text / .mems_text,
                                                   HipCorpusSearcher.shared_passages
                                                   Corpus.to_stream (the inverse of Corpus.map), corpus.unescape_ranges
                                                   HipFMSearcher.extract_text / .extract_text_batch (text by position),
                                                   HipCorpusSearcher.read / .document / .snippets
                                                   HipFMSearcher.occurrences / .finditer (where regexes and hits stand),
                                                   HipCorpusSearcher.grep, python -m findex_amd.grep
                                                   HipFMSearcher.ngrams / .ngram_texts (which strings of L bytes occur, how often),
                                                   HipCorpusSearcher.frequent_phrases, python -m findex_amd.index --ngrams
                                                   HipFMSearcher.line_query (lines with A and B, A not C, A near B, grep -v),
                                                   HipCorpusSearcher.grep_lines_where / .grep_lines_inverted, grep -v / --and / --not
                                                   HipFMSearcher.search_fold / .locate_fold (every case variant that occurs),
                                                   ignore_case= on finditer, grep and rank, grep -i, rank -i
                                                   HipFMSearcher.search_classes_batch / .locate_classes, findex_amd.unicode_fold
                                                   (UTF-8 case folding), ignore_case="unicode" on locate_docs, rank, finditer and grep,
                                                   search_words(classes=..), rank --unicode-case, grep --unicode-case

There is no CPU fallback: importing works anywhere, but every compute call needs the built
library and a HIP device and fails loudly otherwise.
"""
from ._lib import FmxError, MatchError, Re2PostSyntax, LIB_PATH, load  # noqa: F401
from .searcher import ASCII_FOLD, HipFMSearcher, WORD_BYTES, boundary_class, check_fold, class_words, fold_map  # noqa: F401
from .construct import bwt_from_text, bwt_from_text_chunked, bwt_from_text_dev, lcp_from_text, lcp_from_text_dev, write_bwt  # noqa: F401
from .corpus import Corpus, HipCorpusSearcher, escape, is_binary, list_files  # noqa: F401
from .regex import DFA, NFA, REParser, ReTree, SAResult, CompiledRegexes  # noqa: F401



def set_layout(name):
    """fmx_config_set("layout", ...): "auto" | "onehot" | "bytes" for indexes opened afterwards."""
    from . import _lib
    _lib.check(_lib.load().fmx_config_set(b"layout", name.encode()))


def set_checkpoints(name):
    """fmx_config_set("checkpoints", ...): "auto" | "superblock" (bytes layout, indexes opened afterwards)."""
    from . import _lib
    _lib.check(_lib.load().fmx_config_set(b"checkpoints", name.encode()))


def set_ktab(name):
    """fmx_config_set("ktab", ...): "auto" | "off" (handles that have not searched yet)."""
    from . import _lib
    _lib.check(_lib.load().fmx_config_set(b"ktab", name.encode()))


def set_jump(name):
    """fmx_config_set("jump", ...): "auto" | "jumps" | "rows3" | "rows" | "off" -- the row jump table, the three-step row table and
    the row table (handles that have not searched yet)."""
    from . import _lib
    _lib.check(_lib.load().fmx_config_set(b"jump", name.encode()))


def set_pipeline(name):
    """fmx_config_set("pipeline", ...): "off" | "on" -- large host batches in page-locked memory as overlapping chunks."""
    from . import _lib
    _lib.check(_lib.load().fmx_config_set(b"pipeline", name.encode()))


def config_set(key, value):
    """fmx_config_set(key, value): any of the library's process-wide options (include/fmx.h)."""
    from . import _lib
    _lib.check(_lib.load().fmx_config_set(key.encode(), str(value).encode()))


__all__ = ["ASCII_FOLD", "fold_map", "check_fold", "WORD_BYTES", "boundary_class", "class_words", "Corpus", "HipCorpusSearcher", "escape", "is_binary", "list_files", "bwt_from_text", "bwt_from_text_dev", "lcp_from_text", "lcp_from_text_dev", "write_bwt", "config_set", "set_layout", "set_checkpoints", "set_ktab", "set_jump", "set_pipeline", "HipFMSearcher", "REParser", "ReTree", "SAResult", "NFA", "DFA", "CompiledRegexes", "FmxError", "MatchError", "Re2PostSyntax"]
