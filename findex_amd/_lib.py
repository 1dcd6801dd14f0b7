"""ctypes binding of libfmx.so (include/fmx.h).  Fails loudly when the HIP library is missing:
there is no CPU fallback in this package."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB") or os.path.join(_HERE, "lib", "libfmx.so")     # FMX_LIB: A/B runs of two builds

FMX_OK = 0
FMX_ERR_OVERFLOW = 9
ERR_NAMES = {1: "FMX_ERR_IO", 2: "FMX_ERR_FORMAT", 3: "FMX_ERR_ARG", 4: "FMX_ERR_NOMEM", 5: "FMX_ERR_HIP",
             6: "FMX_ERR_UNSUPPORTED", 7: "FMX_ERR_SYNTAX", 8: "FMX_ERR_MATCH", 9: "FMX_ERR_OVERFLOW"}


class FmxError(Exception):
    """A non-zero status from libfmx (the Scala adapter would rethrow it as Exception)."""

    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, code), msg))
        self.code = code


class Re2PostSyntax(FmxError):
    """`throw new Exception("re2post syntax")`, re2/re2.scala"""


class MatchError(FmxError):
    """scala.MatchError from ReTree.apply, re2/retree.scala:235-238,291-294"""


FMX_MATCH_FRONTIER, FMX_MATCH_REFERENCE = 0, 1


class fmx_limits(ctypes.Structure):
    _fields_ = [("max_steps", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("max_frontier", ctypes.c_uint64),
                ("max_branching", ctypes.c_uint32), ("max_iterations", ctypes.c_uint32)]


class fmx_result(ctypes.Structure):
    _fields_ = [("regex", ctypes.c_uint32), ("len", ctypes.c_uint32), ("sp", ctypes.c_uint64),
                ("ep", ctypes.c_uint64)]


class fmx_search_opts(ctypes.Structure):
    _fields_ = [("fixed_len", ctypes.c_uint32), ("packed", ctypes.c_uint32), ("escape_cap", ctypes.c_uint64)]


class fmx_approx_hit(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint32), ("mismatches", ctypes.c_uint32), ("sp", ctypes.c_uint64),
                ("ep", ctypes.c_uint64)]


class fmx_approx_opts(ctypes.Structure):
    _fields_ = [("max_mismatches", ctypes.c_uint32), ("sub_lo", ctypes.c_uint8), ("sub_hi", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16)]


FMX_EDIT_MAX_EDITS = 2
FMX_EDIT_MAX_LEN = 255                # pattern bytes of the edit-distance search (fmx.h)


class fmx_edit_hit(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint32), ("edits", ctypes.c_uint16), ("len", ctypes.c_uint16), ("sp", ctypes.c_uint64),
                ("ep", ctypes.c_uint64)]


class fmx_edit_opts(ctypes.Structure):
    _fields_ = [("max_edits", ctypes.c_uint32), ("sub_lo", ctypes.c_uint8), ("sub_hi", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16)]


FMX_MSTAT_MAX_LEN = 4096
FMX_MSTAT_TILE = 512                  # positions per workgroup tile of the walk kernel (fmx.h)
MSTAT_GROUPS = {"onehot": 16, "bytes": 8}      # lane groups per wave: quads, octets (fmx_device.h, Lay<LAYOUT>::G)


FMX_EXTRACT_TILE = 1024               # output bytes per workgroup tile of the extract kernel (fmx.h)


class fmx_mstat_opts(ctypes.Structure):
    _fields_ = [("max_len", ctypes.c_uint32), ("min_len", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class fmx_mem_hit(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint32), ("len", ctypes.c_uint32), ("end", ctypes.c_uint64), ("sp", ctypes.c_uint64),
                ("ep", ctypes.c_uint64)]


FMX_REPEATS_ALL, FMX_REPEATS_LATER = 0, 1
FMX_REPEATS_MAX_LEVELS = 64
FMX_REPEATS_TILE = 2048               # elements per workgroup of the scans between the repeats passes (fmx.h)


class fmx_repeat_opts(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_uint32), ("stop", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3)]


class fmx_repeat_range(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint64), ("end", ctypes.c_uint64)]


class fmx_repeat_summary(ctypes.Structure):
    _fields_ = [("ranges", ctypes.c_uint64), ("covered_bytes", ctypes.c_uint64), ("classes", ctypes.c_uint64),
                ("windows", ctypes.c_uint64), ("largest_class", ctypes.c_uint64), ("largest_class_pos", ctypes.c_uint64)]


FMX_NGRAMS_BY_ROW, FMX_NGRAMS_BY_COUNT = 0, 1
FMX_NGRAMS_NO_POS = 1
FMX_NGRAMS_MAX_LEVELS = 64
FMX_NGRAMS_MAX_BINS = 65536
FMX_NGRAMS_LDS_BINS = 1024            # counts below it are histogrammed in LDS, the others in global memory (fmx.h)


class fmx_ngram_opts(ctypes.Structure):
    _fields_ = [("order", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("min_count", ctypes.c_uint64), ("top", ctypes.c_uint64),
                ("spectrum_bins", ctypes.c_uint32), ("stop", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3)]


class fmx_ngram(ctypes.Structure):
    _fields_ = [("sp", ctypes.c_uint64), ("count", ctypes.c_uint64), ("first_pos", ctypes.c_uint64)]


class fmx_ngram_summary(ctypes.Structure):
    _fields_ = [("records", ctypes.c_uint64), ("selected", ctypes.c_uint64), ("distinct", ctypes.c_uint64),
                ("windows", ctypes.c_uint64), ("singletons", ctypes.c_uint64), ("largest_count", ctypes.c_uint64),
                ("largest_sp", ctypes.c_uint64), ("largest_pos", ctypes.c_uint64)]


FMX_OCC_ALL, FMX_OCC_LONGEST, FMX_OCC_DISJOINT = 0, 1, 2
FMX_OCC_MAX_LEN = 65535               # bytes of an occurrence (fmx.h)


class fmx_occ_opts(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("max_per", ctypes.c_uint64)]


class fmx_occurrence(ctypes.Structure):
    _fields_ = [("group", ctypes.c_uint32), ("len", ctypes.c_uint32), ("pos", ctypes.c_uint64), ("doc", ctypes.c_uint32),
                ("raw_len", ctypes.c_uint32), ("raw_off", ctypes.c_uint64)]


FMX_PREPARE_LINES = 256               # fmx_prepare / fmx_drop_tables: the line table (fmx.h)


class fmx_line_hit(ctypes.Structure):
    _fields_ = [("group", ctypes.c_uint32), ("doc", ctypes.c_uint32), ("line_no", ctypes.c_uint64), ("start", ctypes.c_uint64),
                ("len", ctypes.c_uint32), ("n_hits", ctypes.c_uint32), ("raw_off", ctypes.c_uint64), ("raw_len", ctypes.c_uint32),
                ("first", ctypes.c_uint32)]


# the same record as a numpy dtype (48 bytes)
LINE_HIT = [("group", "<u4"), ("doc", "<u4"), ("line_no", "<u8"), ("start", "<u8"), ("len", "<u4"), ("n_hits", "<u4"),
            ("raw_off", "<u8"), ("raw_len", "<u4"), ("first", "<u4")]


FMX_LQ_ALL_LINES, FMX_LQ_NOT = 0xFFFFFFFF, 1      # fmx_line_query: the anchor "every real line", a negated term (fmx.h)


class fmx_line_term(ctypes.Structure):
    _fields_ = [("group", ctypes.c_uint32), ("window", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


FMX_MERGE_SEGMENT, FMX_MERGE_WARMUP, FMX_MERGE_TILE, FMX_MERGE_CONTEXT = 256, 32, 4096, 4096      # fmx.h
MAX_TEXT_LEN = (1 << 32) - 2          # bytes one suffix sort takes (u32 suffix indices)


class fmx_merge_opts(ctypes.Structure):
    _fields_ = [("context", ctypes.c_uint64), ("max_context", ctypes.c_uint64), ("segment", ctypes.c_uint32),
                ("warmup", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


class fmx_merge_stats(ctypes.Structure):
    _fields_ = [("piece_ms", ctypes.c_double), ("walk_ms", ctypes.c_double), ("fixup_ms", ctypes.c_double),
                ("emit_ms", ctypes.c_double), ("walk_steps", ctypes.c_uint64), ("fixup_steps", ctypes.c_uint64),
                ("longest_run", ctypes.c_uint64), ("runs", ctypes.c_uint64), ("context", ctypes.c_uint64),
                ("rounds", ctypes.c_uint64), ("need_bytes", ctypes.c_uint64)]


FMX_RANK_ALL = 1
FMX_RANK_MAX_TOP, FMX_RANK_MAX_SLOTS = 1024, 64      # results per query, term slots per query (fmx.h)


class fmx_rank_params(ctypes.Structure):
    _fields_ = [("k1", ctypes.c_double), ("b", ctypes.c_double), ("max_per", ctypes.c_uint64), ("top", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class fmx_passage_params(ctypes.Structure):
    _fields_ = [("window", ctypes.c_uint64), ("max_per", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class fmx_passage(ctypes.Structure):
    _fields_ = [("raw_off", ctypes.c_uint64), ("mask", ctypes.c_uint64), ("value", ctypes.c_double), ("raw_len", ctypes.c_uint32),
                ("n_occ", ctypes.c_uint32)]


class fmx_context_opts(ctypes.Structure):
    _fields_ = [("left", ctypes.c_uint64 * 4), ("right", ctypes.c_uint64 * 4), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


FMX_CTX_START = 0x80


class fmx_fold_opts(ctypes.Structure):
    _fields_ = [("fold", ctypes.c_uint8 * 256), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


FMX_FOLD_MAX_CLASS = 8
FMX_FOLD_MAX_LEN = 255


class fmx_class_table(ctypes.Structure):
    _fields_ = [("cls_off", ctypes.c_void_p), ("mem_off", ctypes.c_void_p), ("mem_bytes", ctypes.c_void_p),
                ("n_classes", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


FMX_CLASS_MAX_MEMBER_LEN = 4
FMX_CLASS_MAX_MEMBERS = 16
FMX_CLASS_MAX_ELEMS = 255
FMX_CLASS_MAX_CLASSES = 65280


class fmx_stats_t(ctypes.Structure):
    _fields_ = [("rank_queries", ctypes.c_uint64), ("backward_steps", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("last_kernel_ms", ctypes.c_double),
                ("index_bytes", ctypes.c_uint64), ("n_blocks", ctypes.c_uint64), ("n_symbols", ctypes.c_uint32),
                ("block_bytes", ctypes.c_uint32), ("build_ms", ctypes.c_double), ("layout", ctypes.c_uint32),
                ("search_residency", ctypes.c_uint32), ("search_requests", ctypes.c_uint64),
                ("frontier_requests", ctypes.c_uint64), ("frontier_elements", ctypes.c_uint64),
                ("frontier_queue_reads", ctypes.c_uint64), ("frontier_queue_writes", ctypes.c_uint64),
                ("frontier_results", ctypes.c_uint64), ("frontier_records", ctypes.c_uint64),
                ("ktab_lookups", ctypes.c_uint64), ("ktab_k", ctypes.c_uint32), ("jump_chars", ctypes.c_uint32),
                ("tables_build_ms", ctypes.c_double), ("jump_lookups", ctypes.c_uint64), ("jump_bytes", ctypes.c_uint64),
                ("row_lookups", ctypes.c_uint64), ("row_bytes", ctypes.c_uint64),
                ("peak_table_build_bytes", ctypes.c_uint64), ("patterns_seen", ctypes.c_uint64),
                ("tables_held_bytes", ctypes.c_uint64), ("table_budget_bytes", ctypes.c_uint64),
                ("hbm_free_after_tables", ctypes.c_uint64), ("tables_alloc_ms", ctypes.c_double)]


# name -> (restype, argtypes); every symbol include/fmx.h declares
_vp, _u64, _i32, _u32, _sz, _cp = (ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t,
                                   ctypes.c_char_p)
_P = ctypes.POINTER
SYMBOLS = {
    "fmx_last_error": (_cp, []),
    "fmx_abi_version": (_i32, []),
    "fmx_config_set": (_i32, [_cp, _cp]),
    "fmx_device_count": (_i32, [_P(_i32)]),
    "fmx_host_alloc": (_i32, [_sz, _P(_vp)]),
    "fmx_host_free": (_i32, [_vp]),
    "fmx_open": (_i32, [_cp, _cp, _i32, _i32, _P(_vp)]),
    "fmx_open_mem": (_i32, [_vp, _u64, _u64, _vp, _i32, _P(_vp)]),
    "fmx_open_dev": (_i32, [_vp, _u64, _u64, _vp, _i32, _vp, _P(_vp)]),
    "fmx_open_block": (_i32, [_vp, _u64, _vp, _u64, _i32, _P(_vp)]),
    "fmx_close": (_i32, [_vp]),
    "fmx_bwt_from_text": (_i32, [_vp, _u64, _vp, _P(_u64), _vp, _i32]),
    "fmx_bwt_from_text_dev": (_i32, [_vp, _u64, _vp, _vp, _P(_u64), _vp, _i32, _vp]),
    "fmx_open_text": (_i32, [_vp, _u64, _i32, _P(_vp)]),
    "fmx_write_bwt": (_i32, [_cp, _cp, _vp, _u64, _u64, _vp, _i32]),
    "fmx_append_text": (_i32, [_vp, _vp, _u64, _P(fmx_merge_opts), _P(_vp)]),
    "fmx_append_text_dev": (_i32, [_vp, _vp, _u64, _P(fmx_merge_opts), _vp, _P(_u64), _vp, _vp]),
    "fmx_merge_last": (_i32, [_P(fmx_merge_stats)]),
    "fmx_index_config_set": (_i32, [_vp, _cp, _cp]),
    "fmx_prepare": (_i32, [_vp, _u32]),
    "fmx_prepare_ex": (_i32, [_vp, _u32, _u64]),
    "fmx_drop_tables": (_i32, [_vp, _u32]),
    "fmx_n": (_i32, [_vp, _P(_u64)]),
    "fmx_eof": (_i32, [_vp, _P(_u64)]),
    "fmx_cf": (_i32, [_vp, _i32, _P(_u64)]),
    "fmx_counts": (_i32, [_vp, _vp]),
    "fmx_device": (_i32, [_vp, _P(_i32)]),
    "fmx_occ_batch": (_i32, [_vp, _vp, _vp, _vp, _sz]),
    "fmx_occ_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "fmx_search_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "fmx_search_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fmx_search_batch_ex": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _P(fmx_search_opts)]),
    "fmx_search_batch_ex_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _P(fmx_search_opts), _vp]),
    "fmx_packed_words": (_sz, [_sz, _sz]),
    "fmx_pack_intervals_dev": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "fmx_unpack_intervals_dev": (_i32, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "fmx_unpack_intervals": (_i32, [_vp, _sz, _sz, _vp, _vp]),
    "fmx_prev_range_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "fmx_prev_range_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fmx_interval_prev_range": (_i32, [_vp, _u64, _u64, _i32, _i32, _vp, _vp, _vp, _P(_sz)]),
    "fmx_lf_walk_batch": (_i32, [_vp, _vp, _sz, _u32, _vp, _vp]),
    "fmx_lf_walk_batch_dev": (_i32, [_vp, _vp, _sz, _u32, _vp, _vp, _vp]),
    "fmx_psi_batch": (_i32, [_vp, _vp, _vp, _sz]),
    "fmx_psi_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _vp]),
    "fmx_next_substr_batch_dev": (_i32, [_vp, _vp, _sz, _u32, _vp, _vp, _vp]),
    "fmx_next_substr": (_i32, [_vp, _u64, _u32, _vp, _P(_u32)]),
    "fmx_prev_substr": (_i32, [_vp, _u64, _u32, _vp]),
    "fmx_next_substr_batch": (_i32, [_vp, _vp, _sz, _u32, _vp, _vp]),
    "fmx_search_batch_multi": (_i32, [_vp, _sz, _vp, _vp, _vp, _vp, _sz]),
    "fmx_extract": (_i32, [_vp, _u64, _u32, _i32, _vp, _P(_u32)]),
    "fmx_write_fm": (_i32, [_vp, _cp]),
    "fmx_locate_batch": (_i32, [_vp, _vp, _sz, _vp]),
    "fmx_locate_batch_dev": (_i32, [_vp, _vp, _sz, _vp, _vp]),
    "fmx_locate_intervals": (_i32, [_vp, _vp, _vp, _sz, _u64, _vp, _vp, _sz]),
    "fmx_locate_intervals_dev": (_i32, [_vp, _vp, _vp, _sz, _u64, _vp, _vp, _sz, _vp]),
    "fmx_locate_info": (_i32, [_vp, _P(_u32), _P(_u64), _P(ctypes.c_double)]),
    "fmx_write_sa": (_i32, [_vp, _cp]),
    "fmx_lcp_from_text_dev": (_i32, [_vp, _u64, _vp, _vp, _i32, _vp]),
    "fmx_lcp_from_text": (_i32, [_vp, _u64, _vp, _i32]),
    "fmx_lcp_batch": (_i32, [_vp, _vp, _sz, _vp]),
    "fmx_lcp_batch_dev": (_i32, [_vp, _vp, _sz, _vp, _vp]),
    "fmx_lcp_range": (_i32, [_vp, _u64, _u64, _vp]),
    "fmx_lcp_range_dev": (_i32, [_vp, _u64, _u64, _vp, _vp]),
    "fmx_lcp_info": (_i32, [_vp, _P(_u64), _P(ctypes.c_double), _P(_u32), _P(_u64), _P(_u64)]),
    "fmx_write_lcp": (_i32, [_vp, _cp]),
    "fmx_lcp_last_phases": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)]),
    "fmx_search_approx_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_approx_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_approx_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_approx_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_approx_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_search_edit_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_edit_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_edit_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_edit_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_edit_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_match_stats_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_mstat_opts), _vp, _vp, _vp]),
    "fmx_match_stats_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _u64, _P(fmx_mstat_opts), _vp, _vp, _vp, _vp]),
    "fmx_mems_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_mstat_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_mems_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _u64, _P(fmx_mstat_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_mstat_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_repeats": (_i32, [_vp, _vp, _sz, _P(fmx_repeat_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_repeats_dev": (_i32, [_vp, _vp, _sz, _P(fmx_repeat_opts), _vp, _vp, _sz, _P(_sz), _vp, _vp]),
    "fmx_repeats_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)]),
    "fmx_ngrams": (_i32, [_vp, _vp, _sz, _P(fmx_ngram_opts), _vp, _vp, _sz, _P(_sz), _vp, _vp]),
    "fmx_ngrams_dev": (_i32, [_vp, _vp, _sz, _P(fmx_ngram_opts), _vp, _vp, _sz, _P(_sz), _vp, _vp, _vp]),
    "fmx_ngrams_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)]),
    "fmx_extract_text_batch": (_i32, [_vp, _vp, _vp, _sz, _vp]),
    "fmx_extract_text_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _u64, _vp, _vp]),
    "fmx_extract_info": (_i32, [_vp, _P(_u32), _P(_u64), _P(ctypes.c_double)]),
    "fmx_extract_last": (_i32, [_P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_corpus_build": (_i32, [_vp, _u64, _vp, _u64, _i32, _P(_vp)]),
    "fmx_corpus_build_dev": (_i32, [_vp, _u64, _vp, _u64, _i32, _vp, _P(_vp)]),
    "fmx_corpus_free": (_i32, [_vp]),
    "fmx_corpus_info": (_i32, [_vp, _P(_u64), _P(_u64), _P(_u64), _P(_u64), _P(ctypes.c_double), _P(_u32)]),
    "fmx_corpus_stream": (_i32, [_vp, _vp, _u64]),
    "fmx_corpus_stream_dev": (_i32, [_vp, _P(_vp), _P(_u64)]),
    "fmx_corpus_drop_stream": (_i32, [_vp]),
    "fmx_corpus_open_index": (_i32, [_vp, _vp, _P(_vp)]),
    "fmx_corpus_tables": (_i32, [_vp, _vp, _vp, _vp]),
    "fmx_corpus_from_tables": (_i32, [_vp, _vp, _vp, _u64, _u64, _i32, _P(_vp)]),
    "fmx_corpus_map": (_i32, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "fmx_corpus_map_dev": (_i32, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "fmx_corpus_doc_list": (_i32, [_vp, _vp, _vp, _vp, _sz, _u64, _u64, _vp, _vp, _vp, _sz]),
    "fmx_corpus_doc_list_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "fmx_corpus_doc_list_phases": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)]),
    "fmx_corpus_escape": (_i32, [_vp, _sz, _vp, _sz, _P(_sz)]),
    "fmx_corpus_rank": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _P(fmx_rank_params), _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "fmx_corpus_rank_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _P(fmx_rank_params), _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "fmx_corpus_rank_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(_u64),
                                    _P(_u64), _P(_u64)]),
    "fmx_corpus_rank_sets": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _P(fmx_rank_params), _vp, _vp, _vp, _vp, _sz, _vp,
                                    _vp]),
    "fmx_corpus_rank_sets_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _P(fmx_rank_params), _vp, _vp, _vp, _vp, _sz,
                                        _vp, _vp, _vp]),
    "fmx_corpus_passages": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _P(fmx_passage_params), _vp, _vp,
                                   _sz, _P(_u32)]),
    "fmx_corpus_passages_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _P(fmx_passage_params), _vp,
                                       _vp, _sz, _P(_u32), _vp]),
    "fmx_corpus_passages_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(_u64),
                                        _P(_u64), _P(_u64)]),
    "fmx_occ_host": (_i32, [_vp, _i32, ctypes.c_int64, _P(_u64)]),
    "fmx_calc_gaps_chain": (_i32, [_vp, _vp, _sz, _u64, _i32, _u64, _vp, _P(_sz)]),
    "fmx_regex_compile": (_i32, [_cp, _i32, _P(_vp)]),
    "fmx_regex_compile_batch": (_i32, [_vp, _sz, _i32, _vp, _vp]),
    "fmx_regex_free_batch": (_i32, [_vp, _sz]),
    "fmx_nfa_compile": (_i32, [_cp, _i32, _i32, _P(_vp)]),
    "fmx_dfa_compile": (_i32, [_vp, _u32, _u32, _vp, _P(_vp)]),
    "fmx_regex_free": (_i32, [_vp]),
    "fmx_regex_tables": (_i32, [_vp, _P(_u32), _vp, _vp, _vp, _vp, _P(_u32), _vp, _P(_u32), _vp]),
    "fmx_regex_post_string": (_i32, [_cp, _i32, _vp, _sz]),
    "fmx_regex_match_batch": (_i32, [_vp, _vp, _sz, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_regex_batch_create": (_i32, [_vp, _vp, _sz, _P(_vp)]),
    "fmx_regex_batch_free": (_i32, [_vp]),
    "fmx_regex_batch_info": (_i32, [_vp, _P(_u64), _P(_u64), _P(_u64), _P(_u64)]),
    "fmx_regex_batch_match": (_i32, [_vp, _vp, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_regex_batch_match_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_occurrences": (_i32, [_vp, _vp, _vp, _sz, _sz, _P(fmx_occ_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_occurrences_dev": (_i32, [_vp, _vp, _vp, _sz, _sz, _P(fmx_occ_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_occurrences_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(_u64)]),
    "fmx_context_filter": (_i32, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _P(_sz)]),
    "fmx_context_filter_dev": (_i32, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_context_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_search_context_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_context_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_context_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_context_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_search_fold_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_fold_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_fold_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_fold_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_search_context_fold_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_context_opts), _P(fmx_fold_opts), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_context_fold_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_context_opts), _P(fmx_fold_opts), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_fold_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_search_classes_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_class_table), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_classes_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_class_table), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_search_context_classes_batch": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_context_opts), _P(fmx_class_table), _vp, _vp, _sz, _P(_sz)]),
    "fmx_search_context_classes_batch_dev": (_i32, [_vp, _vp, _vp, _sz, _P(fmx_context_opts), _P(fmx_class_table), _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_classes_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(_u64), _P(_u64)]),
    "fmx_lines_prepare": (_i32, [_vp, _vp, _sz]),
    "fmx_lines_info": (_i32, [_vp, _P(_u64), _vp, _P(_u32), _P(_u32), _P(_u64), _P(ctypes.c_double)]),
    "fmx_lines_batch": (_i32, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "fmx_lines_batch_dev": (_i32, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "fmx_line_spans": (_i32, [_vp, _vp, _sz, _vp, _vp]),
    "fmx_line_spans_dev": (_i32, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "fmx_occurrence_lines": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _P(_sz)]),
    "fmx_occurrence_lines_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_lines_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)]),
    "fmx_line_query": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _P(_sz)]),
    "fmx_line_query_dev": (_i32, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_line_query_last": (_i32, [_P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_uint64),
                                   _P(ctypes.c_uint64)]),
    "fmx_regex_batch_create_multi": (_i32, [_vp, _sz, _vp, _sz, _P(_vp)]),
    "fmx_regex_batch_free_multi": (_i32, [_vp]),
    "fmx_regex_batch_match_multi": (_i32, [_vp, _vp, _vp, _sz, _P(_sz), _vp]),
    "fmx_gather": (_i32, [_vp, _sz, _vp, _vp, _sz, _vp]),
    "fmx_comm_unique_id": (_i32, [_vp]),
    "fmx_comm_create_rank": (_i32, [_vp, _i32, _i32, _vp, _P(_vp)]),
    "fmx_comm_create_all": (_i32, [_vp, _sz, _P(_vp)]),
    "fmx_comm_info": (_i32, [_vp, _P(_i32), _P(_i32)]),
    "fmx_comm_free": (_i32, [_vp]),
    "fmx_allgather_dev": (_i32, [_vp, _vp, _vp, _sz, _vp]),
    "fmx_gather_dev": (_i32, [_vp, _vp, _vp, _sz, _i32, _vp]),
    "fmx_stats": (_i32, [_vp, _P(fmx_stats_t)]),
    "fmx_stats_reset": (_i32, [_vp]),
    "fmx_last_kernel_ms": (_i32, [_vp, _P(ctypes.c_double)]),
}

_lib = None


def load():
    """Loads libfmx.so once.  torch (if installed) is imported first so that both share the one
    HIP runtime torch ships; raises ImportError when the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("findex_amd: %s is missing -- run `python -m findex_amd.build` "
                          "(there is no CPU fallback)" % LIB_PATH)
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


FMX_TRUNCATED = 10


def check(rc):
    """Raises for error statuses; returns the status otherwise (FMX_OK or FMX_TRUNCATED)."""
    if rc == FMX_TRUNCATED:
        return rc
    if rc != FMX_OK:
        msg = (load().fmx_last_error() or b"").decode("utf-8", "replace")
        if rc == 7:
            raise Re2PostSyntax(rc, msg)
        if rc == 8:
            raise MatchError(rc, msg)
        raise FmxError(rc, msg)
    return rc
