/*
 * fmx.h -- C ABI of libfmx.so, the MI355X-native FM-index backward-search engine.
 *
 * This is the drop-in boundary for findex's search hot path.  The reference
 * (martende/findex, Scala) has no FFI layer; its seam is the Scala trait
 * SuffixAlgo / SuffixWalkingAlgo (src/main/scala/org/fmindex/findex.scala:9-57)
 * that every search engine is written against.  Each entry point below names the
 * reference member it replaces; INTEGRATION.md shows the JNI stub and the Scala
 * adapter class (`HipFMSearcher extends SuffixWalkingAlgo`) a maintainer would
 * add on the reference side.
 *
 * Conventions
 *  - Every function returns an int status (FMX_OK == 0).  No exception crosses the
 *    ABI; fmx_last_error() gives a thread-local message for the last failure.
 *  - "No match" is a value, not an error: a miss is reported as sp == ep
 *    (the Scala adapter maps that to None, findex.scala:30,35).
 *  - Positions are uint64 (the reference's Int widened; identical for n < 2^31).
 *  - Symbols are unsigned bytes.  The reference indexes with a signed Byte and
 *    throws on bytes >= 0x80 (findex.scala:21,26); accepting them is a documented
 *    superset.
 *  - The caller owns every buffer it passes; the library keeps no caller pointer
 *    after a call returns (fmx_open_dev copies the BWT).  Handles own their device
 *    memory.  An index handle is immutable after open: concurrent calls on one
 *    handle are allowed from different host threads.
 *  - Plain entry points take HOST pointers and move data themselves.  The `_dev`
 *    twins take DEVICE pointers plus a hipStream_t (as void*) and only enqueue
 *    work: inputs already resident in HBM, outputs left in HBM.  (One exception, stated at
 *    fmx_prepare: the single search that builds a handle's derived tables at its threshold when the
 *    caller never called fmx_prepare; fmx_regex_batch_match_dev is synchronous by design.)
 *  - There is no CPU fallback anywhere: without a usable HIP device every compute
 *    entry point fails with FMX_ERR_HIP.
 */
#ifndef FMX_H
#define FMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMX_ABI_VERSION 5

enum {
  FMX_OK = 0,
  FMX_ERR_IO = 1,          /* cannot open/read a file (reference: java.io exceptions) */
  FMX_ERR_FORMAT = 2,      /* bad size/header ("File %s bad size", bwtmerger.scala:153,261-262) */
  FMX_ERR_ARG = 3,         /* null handle / out-of-range argument (reference: ArrayIndexOutOfBounds) */
  FMX_ERR_NOMEM = 4,       /* host or device allocation failed */
  FMX_ERR_HIP = 5,         /* HIP runtime error / no device */
  FMX_ERR_UNSUPPORTED = 6, /* valid input this build cannot serve */
  FMX_ERR_SYNTAX = 7,      /* "re2post syntax" (re2/re2.scala:84,87,109,133,141,159,174) */
  FMX_ERR_MATCH = 8,       /* scala.MatchError from ReTree.apply (re2/retree.scala:235-238,291-294) */
  FMX_ERR_OVERFLOW = 9,    /* a caller-sized output or a device work queue was too small */
  FMX_TRUNCATED = 10       /* not an error: outputs are valid but a search was cut at a limit (regex max_steps) */
};

typedef struct fmx_index fmx_index;   /* replaces class NaiveFMSearcher, bwtmerger.scala:335-421 */
typedef struct fmx_regex fmx_regex;   /* replaces class ReTree, re2/retree.scala:485 */
typedef struct fmx_regex_batch fmx_regex_batch;   /* a set of compiled regexes made resident on a device */

const char *fmx_last_error(void);
int fmx_abi_version(void);
/* Process-wide options.  The table keys ("ktab", "jump", "jump_pairs", "search_lanes", "jump_chars", "tables_after", "table_budget",
 * "locate_sample": the locate samples' rate, fmx_locate_batch; "extract_sample": the inverse-SA samples' rate,
 * fmx_extract_text_batch; "lines_shift": the line table's directory step 2^S, 4 .. 16, fmx_lines_batch) are the
 * DEFAULTS a handle copies when it is opened; fmx_index_config_set changes one handle's own copy afterwards, so two handles
 * in one process (one JVM) can differ.  key "layout": "auto" (default: one-hot bit-vectors, one 64-byte block per
 * rank query, when sigma*n/7 bytes fit in free HBM and n < 2^37; else BWT bytes + checkpoints, two
 * lines per rank query), "onehot", "bytes".  key "ktab": "auto" (default) / "off": the k-mer jump table that
 * answers a search's first K backward steps with one lookup (built on a handle's first search; K is chosen from n
 * and the alphabet: fmx_stats_t.ktab_k).  key "validate": "0" (default) / "1": the device-pointer search entry
 * point then checks on the device that d_off is non-decreasing and fails with FMX_ERR_ARG otherwise (one more small
 * kernel and a synchronisation per call: a debugging aid; the host-pointer form always checks).  key "checkpoints": "auto" (default: the bytes layout keeps absolute
 * 32-bit checkpoints whenever every symbol occurs fewer than 2^32 times) or "superblock" (always the relative
 * checkpoints + 64-bit superblock counts that larger counts need; for tests).  Affects indexes opened afterwards.
 * key "jump": "auto" (default) / "jumps" / "rows3" / "rows" / "off": the derived tables that serve searches whose
 * interval has narrowed to ONE ROW, where a backward step is a comparison with the text in front of that row's suffix:
 *   - the row jump table: per row the nine BWT characters an LF walk from it reads and the row it ends on, 16 n
 *     bytes -- nine steps of a literal search with one 16-byte lookup when the pattern's next nine characters match
 *     (key "jump_chars": "8" .. "11" characters per entry for tables built afterwards; 9 is the default)
 *     (built when 16 n bytes + 8 GiB of HBM are free -- one allocation: key "tables_after" says when).
 *     Key "jump_pairs": "auto" (default) / "on" / "off": the table holds PAIRS of entries, a row's own and that of the
 *     row it lands on, side by side in 32 bytes -- one memory request (a 64-byte sector either way) then serves up to
 *     2 x jump_chars steps.  32 n bytes; "auto" builds pairs for the one-hot layout when the index has 2^30 rows or more
 *     and 32 n bytes + 8 GiB are free ("on": whenever they are free);
 *     Key "search_lanes": "auto" (default) / "quads" / "pairs", a test and diagnosis key: with a row jump table and the
 *     three-step row table on the one-hot layout, a search may serve each pattern by a pair of lanes instead of four (32
 *     patterns per wave instead of 16).  "auto" does so for batches of at least 512 patterns per compute unit (131 072 on
 *     an MI355X), "quads" never, "pairs" whenever those tables are there.  Results are the same either way;
 *   - the three-step row table: the same with three characters, 8 n bytes -- built instead where the jump table does
 *     not fit; the one-row part of every pattern is then walked by one lane per pattern;
 *   - the row table: BWT'[r] and LF r in 8 bytes per row -- the regex frontier steps its one-row elements with it
 *     (built at a handle's first regex match when 8 n bytes + 4 GiB are free); a literal search on a handle that has
 *     it, and no jump table, uses it like the three-step table.
 * "auto" builds what fits, at first use or in fmx_prepare; "jumps" / "rows3" / "rows" allow only the one; "off" none.
 * fmx_stats_t.jump_bytes, .row_bytes.  Results and executed-step counts are the same with and without them.
 * key "tables_after": "auto" (default) / N: WHEN a handle's derived tables are built.  A table pays only for a caller that
 * searches much: at C3 (n = 2^32) the row tables take ~1.5 s and 96 GiB and save 0.4 ms per million patterns.  So they are
 * built by fmx_prepare, or by the search that brings the patterns the handle has been asked for to the threshold -- auto:
 * n / 64 patterns (at least 65536) for the row tables, 1024 patterns for the k-mer table; N: that many for both (0: at the
 * first search).  A per-call adapter's single queries never build one.  (The regex frontier builds the k-mer table and its
 * row table at a handle's first match: a frontier is thousands of steps.)  fmx_stats_t.patterns_seen,
 * .peak_table_build_bytes; fmx_drop_tables frees them again.
 * key "table_budget": "auto" (default) / N / F: the most device memory ALL derived tables of a handle (k-mer table, row
 * tables, row jump table, select directory) may hold together -- N bytes, or a fraction F written with a point ("0.5": that
 * share of the HBM that is free when a table is decided, the handle's own tables counted as free); "auto": whatever fits
 * beside the built-in margins (8 GiB for the row jump table, 4-8 GiB for the others).  Under a budget the k-mer table takes
 * at most a quarter of it, then the three-step row table (8 n), then the row jump table as pairs (32 n) if that still fits,
 * else as single entries (16 n), else not at all -- searches give the same answers with any subset.  At C3 (n = 2^32) "auto"
 * ends up holding 4 + 32 + 128 GiB beside the 81 GiB index; "100000000000" keeps it to 4 + 32 + 64 GiB.
 * fmx_stats_t.tables_held_bytes, .table_budget_bytes, .hbm_free_after_tables; fmx_prepare_ex sets it with the build.
 * key "pipeline": "off" (default) / "on": fmx_search_batch with 128 k patterns or more in page-locked buffers cut into
 * chunks whose uploads, searches and downloads overlap on three streams, instead of whole arrays up, one search, whole
 * arrays down.  Same results; which is faster depends on how the platform's asynchronous copies compare with its
 * synchronous ones (here: the synchronous form, hence the default).
 * key "threads": host threads the library's own parallel parts use (fmx_regex_compile_batch, making a regex batch
 * resident); "0" = detect (default). */
int fmx_config_set(const char *key, const char *value);
/* Page-locked host memory for batch buffers (hipHostMalloc): the host-pointer entry points move such buffers
 * by DMA at link speed; pageable memory works everywhere too, through the runtime's staging copies.  A JNI adapter
 * wraps these in direct ByteBuffers. */
int fmx_host_alloc(size_t bytes, void **out);
int fmx_host_free(void *p);
/* Number of HIP devices visible (0 and FMX_OK when there is none). */
int fmx_device_count(int *count);

/* ---- open / close ------------------------------------------------------------
 * fmx_open      : NaiveFMSearcher(filename, bigEndian) constructor, bwtmerger.scala:335-353,
 *                 reading X.bwt (BWTLoader :144-174) and X.aux (AUXLoader :130-142).  The
 *                 reference's third file, X.fm (FMLoader :252-290), is not needed: its content
 *                 is a function of the other two (FMCreator :424-533) and the device rank
 *                 dictionary is built from them directly.  An X.fm that IS there (the .bwt's name
 *                 with the extension swapped, :33-36) is held to FMLoader's checks -- element size
 *                 4, size * 4 + 9 == file length (:259-262) -- and to n = fm.size (:339) being the
 *                 .bwt's n: FMX_ERR_FORMAT otherwise, as the reference throws.
 * fmx_open_mem  : the same from host memory (bwt[n] raw bytes incl. the filler at slot eof,
 *                 counts[256] = the .aux array).
 * fmx_open_dev  : the same with the BWT bytes already in device memory; counts may be NULL
 *                 (then they are computed on the device).
 * counts[0] must be 0 (the reference's readers escape byte 0, bwtreader.scala:136-155, and its
 * FMCreator gives symbol 0 exactly the one EOF slot, bwtmerger.scala:440-450).  Unlike the
 * reference, open verifies counts against the BWT and fails with FMX_ERR_FORMAT on mismatch. */
int fmx_open(const char *bwt_path, const char *aux_path, int big_endian, int device, fmx_index **out);
int fmx_open_mem(const uint8_t *bwt, uint64_t n, uint64_t eof, const int64_t counts[256], int device,
                 fmx_index **out);
int fmx_open_dev(const void *d_bwt, uint64_t n, uint64_t eof, const int64_t *counts_or_null, int device,
                 void *stream, fmx_index **out);
/* fmx_open_block : class NaiveBWTSearcher(bwt, bucketStarts, rk0), findex.scala:459-506 -- the searcher
 *                  BWTMerger2.calcGaps (bwtmerger.scala:981-1023) uses over one block's raw BWT.  cf(c) is the
 *                  caller's bucket_starts[c]; occ(c, key) = occurrences of byte c in bwt[0..key] without row rk0
 *                  (c is taken & 0xff by the byte-typed batch entry points, like :480), including the reference's
 *                  last-slot rule (:500-502): a symbol whose only occurrence is position 0 answers 0.  The block
 *                  must not contain byte 0 (FMX_ERR_UNSUPPORTED; the merger's input is 0-free).  The handle
 *                  serves every entry point (search, getPrevRange ... are inherited from SuffixAlgo there too). */
int fmx_open_block(const uint8_t *bwt, uint64_t n, const int64_t bucket_starts[256], uint64_t rk0, int device,
                   fmx_index **out);
int fmx_close(fmx_index *idx);          /* NULL: nothing to close, FMX_OK */

/* ---- construction from text: BWTMerger2.merge(FileBWTReader), bwtmerger.scala:654-1261 --------------
 * text -> BWT of reverse(text) + EOF, as the merger writes it (copyReverse :1106-1108, sa2BWT :782-810, aux
 * :841-856): bwt[i] is the byte before suffix SA[i] of s = reverse(text) + sentinel, *eof the row whose suffix is
 * all of s, filled with the byte of the row above (of the row below when eof == 0); counts[c] = occurrences of c
 * in the text.  A hand-written suffix sort on the device (prefix doubling over LSD radix sorts).
 *  - 1 <= len <= 2^32 - 2 (n = len + 1 suffixes, u32 indices); len > 2^32 - 2 -> FMX_ERR_UNSUPPORTED.
 *  - NULL pointer or len == 0 -> FMX_ERR_ARG; a 0 byte in the text -> FMX_ERR_UNSUPPORTED (the reference's readers
 *    escape byte 0 and counts[0] must be 0, as for fmx_open_block).  These are checked before the device is touched
 *    (the 0 byte of a device-resident text is found by the first kernel: FMX_ERR_UNSUPPORTED then too).  A valid text
 *    without a device: FMX_ERR_HIP, no CPU fallback.
 *  - Construction ALLOCATES AND SYNCHRONISES: it is not a _dev call in the sense of the fmx_prepare contract, and it
 *    returns FMX_ERR_HIP under a stream capture.  Peak device memory: ~37.3 bytes per text byte of temporaries (4 of
 *    them the suffix array, which a given d_sa_or_null replaces; the host-pointer forms add 2 for the text and the BWT
 *    in HBM), checked against the free HBM before anything is allocated: FMX_ERR_NOMEM, with the need in the message.  Every temporary is freed
 *    before the call returns; the same text gives the same bytes on every run.
 * fmx_bwt_from_text     : host text in, host bwt[len + 1] out.
 * fmx_bwt_from_text_dev : device text in, device bwt[len + 1] out, enqueued on `stream` (a hipStream_t, NULL: the
 *                         null stream) and synchronised; d_sa_or_null, when given, receives the suffix array of s
 *                         (u32[len + 1]).  eof and counts are host pointers.
 * fmx_open_text         : the index of the text, as fmx_open of the files fmx_bwt_from_text would give (the BWT
 *                         never leaves the device).
 * fmx_write_bwt         : X.bwt (BWTLoader, :144-174: int64 size, int64 eof, then the n bytes) and X.aux (AUXLoader,
 *                         :130-142: 256 int64 counts), big- or little-endian; host only. */
int fmx_bwt_from_text(const uint8_t *text, uint64_t len, uint8_t *bwt, uint64_t *eof, int64_t counts[256], int device);
int fmx_bwt_from_text_dev(const void *d_text, uint64_t len, void *d_bwt, void *d_sa_or_null, uint64_t *eof,
                          int64_t counts[256], int device, void *stream);
int fmx_open_text(const uint8_t *text, uint64_t len, int device, fmx_index **out);
int fmx_write_bwt(const char *bwt_path, const char *aux_path, const uint8_t *bwt, uint64_t n, uint64_t eof,
                  const int64_t counts[256], int big_endian);

/* ---- append: new text merged into an index without rebuilding it (BWTMerger2's way to a large index) ----
 * A = the indexed text (a bytes, n = a + 1 rows), B = the new text (len bytes, no 0 byte).  The result is byte for byte what
 * fmx_bwt_from_text(A + B) gives: eof, counts and the filler at the eof slot included.  With R = reverse(B) the new string
 * is R . s_A: the rows of A keep their order and their bytes (A's eof row takes R's last byte), and the len new suffixes
 * are placed among them --
 *   gap ranks : how many rows of A lie before each new suffix.  One chain of len dependent rank steps, cut into segments
 *               of `segment` positions: a lane group starts `warmup` positions to the right of its segment with the full
 *               row range and walks left; once its interval is empty the rank is exact.  Positions whose interval is
 *               still not empty inside the segment (B shares a stretch with A there) are walked again as the plain chain,
 *               one walker per maximal run: correct for every B, slow where B repeats A (B == A is one run of len steps).
 *   order     : the new suffixes among themselves, from the suffix sort of tail(A, M) + B with M = min(a, context); the
 *               piece's LCP array tells whether a comparison reached the piece's end, and then context doubles and the
 *               piece is rebuilt, until M == a or context passes max_context (FMX_ERR_UNSUPPORTED, the context that
 *               would be tried next in the message).  tail(A, M) comes from the handle by one Psi walk from the eof row
 *               (it builds the handle's select directory, as fmx_next_substr does).
 *   emit      : per tile of FMX_MERGE_TILE output rows, the new bytes and the next rows of A, 16 bytes per store.
 * Rows and ranks are 64-bit: n + len may exceed 2^32 (len itself, with the context, stays within the suffix sort's limit).
 * fmx_merge_opts: NULL = all defaults.  context 0 = FMX_MERGE_CONTEXT; max_context 0 = no limit; segment 0 = the header's
 *   FMX_MERGE_SEGMENT and FMX_MERGE_WARMUP, segment != 0 = segment and warmup both as given (warmup 0 is a valid choice);
 *   reserved must be 0.
 * fmx_append_text     : host text in, a NEW handle out; idx is untouched, stays valid, and the caller closes both.
 * fmx_append_text_dev : device text in, the merged BWT (n + len bytes) into the caller's device buffer, eof and counts to
 *                       host pointers: ready for fmx_open_dev.  Enqueued on `stream` and synchronised.
 * fmx_merge_last      : the calling thread's last append: device-event times (ms) of its phases, the backward steps of the
 *                       segment walk, the steps, number and longest of the fix-up runs, the context used and the number of
 *                       pieces built.
 * Like construction these calls ALLOCATE AND SYNCHRONISE: FMX_ERR_HIP under a stream capture, decided before anything is
 * allocated, the capture left valid.  The need in device memory -- the piece's temporaries (~47 bytes per piece byte), 17
 * bytes per new byte for ranks, rows and bytes, and in the host form the text, the n + len output bytes and the new
 * handle's rank dictionary -- is checked against the free HBM before each piece: FMX_ERR_NOMEM with the need in the
 * message.  Every temporary is freed on every path; the same inputs give the same bytes on every run.
 * Refusals, decided before the device is touched, in this order: a NULL text or output, len == 0, a non-zero reserved
 * word: FMX_ERR_ARG; len + context > 2^32 - 2, a 0 byte in a host text: FMX_ERR_UNSUPPORTED; a NULL handle: FMX_ERR_ARG; an
 * fmx_open_block handle, n + len >= 2^38: FMX_ERR_UNSUPPORTED.  (A 0 byte in a device text is found by the piece's first
 * kernel: FMX_ERR_UNSUPPORTED then too.) */
#define FMX_MERGE_SEGMENT 256      /* positions of B per lane group of the rank walk */
#define FMX_MERGE_WARMUP 32        /* positions a group starts to the right of its segment */
#define FMX_MERGE_TILE 4096        /* output rows per workgroup tile of the emit kernel */
#define FMX_MERGE_CONTEXT 4096     /* bytes of A's tail in the first piece */
typedef struct fmx_merge_opts {
  uint64_t context;
  uint64_t max_context;
  uint32_t segment;
  uint32_t warmup;
  uint32_t reserved[4];
} fmx_merge_opts;
typedef struct fmx_merge_stats {
  double piece_ms, walk_ms, fixup_ms, emit_ms;
  uint64_t walk_steps, fixup_steps, longest_run, runs;
  uint64_t context;                /* M of the piece that passed: min(a, context after the retries) */
  uint64_t rounds;                 /* pieces built */
  uint64_t need_bytes;             /* the device memory need that was checked before the last piece */
} fmx_merge_stats;
int fmx_append_text(const fmx_index *idx, const uint8_t *text, uint64_t len, const fmx_merge_opts *opts, fmx_index **out);
int fmx_append_text_dev(const fmx_index *idx, const void *d_text, uint64_t len, const fmx_merge_opts *opts, void *d_bwt_out,
                        uint64_t *eof, int64_t counts[256], void *stream);
int fmx_merge_last(fmx_merge_stats *out);
/* One handle's own table policy (the keys fmx_config_set lists as table keys; FMX_ERR_ARG for any other key or a bad value).
 * Tables that exist are not touched: fmx_drop_tables + fmx_prepare rebuild under the new policy. */
int fmx_index_config_set(fmx_index *idx, const char *key, const char *value);
/* Builds now what a handle otherwise builds when its searches reach the "tables_after" threshold (literal search) or
 * at first use (Psi, regex match) -- FMX_PREPARE_KTAB: the k-mer jump table (up to min(16 GiB, a quarter of the free
 * HBM, a quarter of the budget)); FMX_PREPARE_SELECT: the select directory (first Psi / nextSubstr; at most ~n bytes);
 * FMX_PREPARE_JUMP: the tables of the literal search's one-row part -- the three-step row table and the row jump table
 * (8 n + 16 n or 32 n bytes, one allocation each; each skipped when that much HBM is not free or not in the handle's
 * budget); FMX_PREPARE_FRONTIER: the regex frontier's row table (8 n bytes, otherwise built at the first regex match);
 * FMX_PREPARE_SEARCH (implied by KTAB and JUMP): calibrates the literal search kernel the handle's tables select -- a few
 * 60-us launches on the library's own stream that count how many of its workgroups a CU really holds
 * (fmx_stats_t.search_residency).  Each flag stands for its own table only: FMX_PREPARE_KTAB alone leaves the row tables to
 * their threshold.
 * THE CONTRACT: after fmx_prepare has built a table, no later call builds, allocates for, or synchronises a stream for
 * THAT table; with KTAB | JUMP (| FRONTIER | SELECT for regex / Psi callers) prepared, every _dev entry point only
 * enqueues work -- safe inside a stream capture, and a caller that times its first search times a search.  Without
 * fmx_prepare, the ONE search that brings a handle to its "tables_after" threshold builds the tables inside the call
 * (it allocates and synchronises `stream`; FMX_ERR_HIP under a stream capture), and calibrates; every other _dev
 * call only enqueues.  A table that cannot be built (no memory, no budget) is left out: searches then walk every step on
 * the rank dictionary, with the same results.  The time spent is reported as fmx_stats_t.tables_build_ms.
 * fmx_prepare_ex: the same under a budget -- budget_bytes != 0 becomes the handle's "table_budget" first. */
enum { FMX_PREPARE_KTAB = 1, FMX_PREPARE_SELECT = 2, FMX_PREPARE_JUMP = 4, FMX_PREPARE_FRONTIER = 8, FMX_PREPARE_SEARCH = 16,
       FMX_PREPARE_LOCATE = 32 /* the locate samples (fmx_locate_batch below); fmx_drop_tables frees them */,
       FMX_PREPARE_LCP = 64 /* the LCP array (fmx_lcp_batch below); fmx_drop_tables frees it */,
       FMX_PREPARE_EXTRACT = 128 /* the inverse-SA samples (fmx_extract_text_batch below); fmx_drop_tables frees them */,
       FMX_PREPARE_LINES = 256 /* the line table (fmx_lines_batch below), with the default break set {10} unless the handle has
                                  one already, whatever its set; fmx_drop_tables frees it */ };
int fmx_prepare(const fmx_index *idx, unsigned what);
int fmx_prepare_ex(fmx_index *idx, unsigned what, uint64_t budget_bytes);
/* Frees derived tables again (what = FMX_PREPARE_KTAB | FMX_PREPARE_JUMP | FMX_PREPARE_FRONTIER | FMX_PREPARE_LOCATE |
 * FMX_PREPARE_LCP | FMX_PREPARE_EXTRACT (the inverse-SA samples) | FMX_PREPARE_LINES (the line table) in any combination: the k-mer table / the row jump table and the three-step row table, 16-32 n + 8 n bytes /
 * the frontier's row table, 8 n bytes / the locate samples / the LCP array, 4 n bytes) and forgets the handle's pattern count, so that they come back only by fmx_prepare or when the threshold is met
 * anew (under the handle's policy as it is then).  No other call may be using the handle. */
int fmx_drop_tables(fmx_index *idx, unsigned what);

/* ---- scalars: SuffixAlgo.n / cf, findex.scala:10-12; NaiveFMSearcher.cf bwtmerger.scala:346-352 */
int fmx_n(const fmx_index *idx, uint64_t *n);
int fmx_eof(const fmx_index *idx, uint64_t *eof);
int fmx_cf(const fmx_index *idx, int c, uint64_t *out);
int fmx_counts(const fmx_index *idx, int64_t out[256]);
int fmx_device(const fmx_index *idx, int *device);

/* ---- batched rank: SuffixAlgo.occ(c,i), findex.scala:13; NaiveFMSearcher.occ bwtmerger.scala:354-375.
 * out[q] = #{p <= i[q] : BWT'[p] == c[q]}, BWT' = BWT with slot eof read as symbol 0; i = -1 gives 0;
 * i >= n is clamped to n-1 (what the binary search returns for any key past the last entry).
 * THE DEVICE FORMS BELOW CANNOT VALIDATE THEIR OPERANDS (the host forms reject them with FMX_ERR_ARG); their kernels
 * clamp them instead, before any address is formed, so that no operand value leads outside the index:
 *   fmx_occ_batch_dev                              : i as above;
 *   fmx_prev_range_batch_dev                       : sp > n and ep > n are read as n (sp > ep is not an error there: the
 *                                                    two ranks are computed independently);
 *   fmx_lf_walk_batch_dev, fmx_psi_batch_dev,
 *   fmx_next_substr_batch_dev                      : a row >= n is read as n-1.
 * The answer is that of the clamped operand. */
int fmx_occ_batch(const fmx_index *idx, const uint8_t *c, const int64_t *i, uint64_t *out, size_t k);
int fmx_occ_batch_dev(const fmx_index *idx, const void *d_c, const void *d_i, void *d_out, size_t k, void *stream);

/* ---- batched literal backward search: SuffixAlgo.search, findex.scala:15-31.
 * Pattern q is pat[off[q] .. off[q+1]) (off has k+1 entries), matched last byte first from (0, n);
 * sp[q], ep[q] receive the loop's final values: a hit iff sp < ep, a miss has sp == ep.
 * An empty pattern yields (0, n).  The host form validates the offsets (non-decreasing); the device form
 * cannot look at them: d_off must hold k+1 non-decreasing offsets into the d_pat buffer, or the kernel reads
 * outside it.  A host-pointer batch of 128k patterns or more whose four buffers are page-locked (fmx_host_alloc) is
 * pipelined in chunks over two streams (copies of one chunk beside the kernel of another);
 * fmx_stats_t.last_kernel_ms is then the whole device side of the call. */
int fmx_search_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, uint64_t *sp, uint64_t *ep,
                     size_t k);
int fmx_search_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, void *d_sp, void *d_ep,
                         size_t k, void *stream);
/* The lean forms of the same search (round 4; what the host link and the multi-GPU exchange carry):
 *   fixed_len > 0 : every pattern has this many bytes and pattern q is pat[q * fixed_len ..): `off` is not read and may be
 *                   NULL -- 8 bytes per pattern less up the link, and the kernels compute the offsets instead of loading them;
 *   packed & FMX_SEARCH_PACKED : the intervals come back in the 8-BYTE FORM, into `sp` (fmx_packed_words(k, escape_cap) words; `ep` is
 *                   not written and may be NULL in the host form; in the device form d_ep is k words of scratch and d_sp's
 *                   first k words are overwritten in place).
 * The 8-byte form: word q = sp[q] | w << 40 with w = min(ep[q] - sp[q], 0xFFFFFF) -- rows are < 2^38, and a miss (sp == ep:
 * None in the reference, findex.scala:30) keeps the loop's sp at its failing step with w = 0.  An interval of 2^24 - 1 rows
 * or more (patterns of a character or two) has w = 0xFFFFFF and its ep in the ESCAPE LIST behind the k words: word k = the
 * number of such intervals, then pairs (q, ep[q]) in no particular order, room for escape_cap of them.  When more than
 * escape_cap intervals are that wide, word k still counts them all, fmx_unpack_intervals returns FMX_ERR_OVERFLOW and the
 * caller asks for the 16-byte form instead (device side: compare word k with escape_cap).
 *   packed & FMX_SEARCH_MISS_NONE : a pattern that does not occur MAY come back as (0, 0) instead of the loop's values at its
 *                   failing step.  SuffixAlgo.search returns None for it either way (findex.scala:30: `if (sp < ep) Some((sp, ep))
 *                   else None`) -- the values a miss ends with are not observable through the reference's API, and finding them
 *                   costs a walk of up to five dependent memory round trips per miss where a row-table lookup has already shown
 *                   that the pattern's text differs from its row's.  Hits are unchanged; fmx_stats' rank_queries counts the
 *                   reference loop's steps on every pattern as before (they are known from where the texts differ).  Which
 *                   misses are canonicalised is the kernels' business (those found by a table lookup; a miss found by a rank
 *                   query keeps its values): test sp < ep, nothing else.  The JVM adapter, which returns Option, always asks.
 * opts == NULL is fmx_search_batch[_dev] exactly. */
#define FMX_SEARCH_PACKED 1u
#define FMX_SEARCH_MISS_NONE 2u
typedef struct fmx_search_opts {
  uint32_t fixed_len;
  uint32_t packed;       /* bit set: FMX_SEARCH_PACKED | FMX_SEARCH_MISS_NONE (1 = the packed form, as until ABI 5) */
  uint64_t escape_cap;
} fmx_search_opts;
int fmx_search_batch_ex(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, uint64_t *sp, uint64_t *ep,
                        size_t k, const fmx_search_opts *opts);
int fmx_search_batch_ex_dev(const fmx_index *idx, const void *d_pat, const void *d_off, void *d_sp, void *d_ep,
                            size_t k, const fmx_search_opts *opts, void *stream);
/* The 8-byte form on its own: pack device-resident (sp, ep) arrays (d_packed may be d_sp: in place), unpack them on the
 * device (the first min(word k, escape_cap) escape entries are applied) or on the host (a decode of the caller's own
 * buffer: FMX_ERR_OVERFLOW as above, FMX_ERR_FORMAT when an escape entry names a pattern >= k). */
size_t fmx_packed_words(size_t k, size_t escape_cap);
int fmx_pack_intervals_dev(const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, size_t escape_cap,
                           void *d_packed, void *stream);
int fmx_unpack_intervals_dev(const fmx_index *idx, const void *d_packed, size_t k, size_t escape_cap, void *d_sp,
                             void *d_ep, void *stream);
int fmx_unpack_intervals(const uint64_t *packed, size_t k, size_t escape_cap, uint64_t *sp, uint64_t *ep);

/* One process, several GPUs: the batch is cut into contiguous slices balanced by pattern bytes, slice r is
 * searched on idxs[r] (one handle per device, every handle a replica of the same index) from its own host
 * thread, and each slice's intervals land in their range of sp / ep -- the single-process form of SURVEY.md 8e
 * (no collective; the one-process-per-GPU form with an RCCL all-gather is findex_amd/distributed.py). */
int fmx_search_batch_multi(fmx_index *const *idxs, size_t n_idx, const uint8_t *pat, const uint64_t *off,
                           uint64_t *sp, uint64_t *ep, size_t k);

/* ---- batched single step: SuffixAlgo.getPrevRange(sp,ep,c), findex.scala:32-36.
 * sp1 = cf(c)+occ(c,sp-1), ep1 = cf(c)+occ(c,ep-1); empty iff sp1 >= ep1.  Needs sp <= ep <= n. */
int fmx_prev_range_batch(const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, const uint8_t *c,
                         uint64_t *sp1, uint64_t *ep1, size_t k);
int fmx_prev_range_batch_dev(const fmx_index *idx, const void *d_sp, const void *d_ep, const void *d_c,
                             void *d_sp1, void *d_ep1, size_t k, void *stream);

/* ---- character-class step: SuffixAlgo.getIntervalPrevRange(sp,ep,cstart,cend), findex.scala:37-51.
 * All c in [cstart, cend] (inclusive, 0 <= cstart, cend <= 255); only non-empty ranges are
 * returned, in DESCENDING c like the reference's prepended list.  out arrays need cend-cstart+1
 * slots; *n_out = number written. */
int fmx_interval_prev_range(const fmx_index *idx, uint64_t sp, uint64_t ep, int cstart, int cend,
                            uint64_t *out_sp, uint64_t *out_ep, uint8_t *out_c, size_t *n_out);

/* ---- LF walks: NaiveFMSearcher.getPrevI / prevSubstr, bwtmerger.scala:386-389,409-419.
 * For each start row: `len` times emit BWT'[row] (0 at the EOF row) and step row = LF(row).
 * out_bytes is k*len bytes (walk q at q*len, in emission order = prevSubstr's string);
 * end_rows (optional) receives the row after the last step. */
int fmx_lf_walk_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint32_t len, uint8_t *out_bytes,
                      uint64_t *end_rows);
int fmx_lf_walk_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, uint32_t len, void *d_out_bytes,
                          void *d_end_rows, void *stream);

/* ---- Psi walks: NaiveFMSearcher.getNextI / nextSubstr, bwtmerger.scala:390-405.
 * fmx_psi_batch: out[q] = fm[rows[q]] (the inverted-list entry = select on the rank dictionary).
 * fmx_next_substr: the reference's nextSubstr(sp,len): walk Psi, stop after a 0 byte, reversed;
 * out needs len bytes, *out_len = bytes written. */
int fmx_psi_batch(const fmx_index *idx, const uint64_t *rows, uint64_t *out, size_t k);
int fmx_psi_batch_dev(const fmx_index *idx, const void *d_rows, void *d_out, size_t k, void *stream);
/* Device form of the batched nextSubstr: d_out is k*len bytes in WALK order (the reference's `ret` before its
 * final .reverse, bwtmerger.scala:404), d_out_len[q] (uint32) = bytes of walk q written. */
int fmx_next_substr_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, uint32_t len, void *d_out,
                              void *d_out_len, void *stream);
/* The first Psi / nextSubstr call on a handle builds a select directory on the device (at most ~n bytes; it is
 * counted in fmx_stats_t.index_bytes from then on).  The build allocates and synchronises the stream, so like the
 * locate samples and the LCP array it happens in fmx_prepare(FMX_PREPARE_SELECT) or in a first call OUTSIDE a stream
 * capture: without the directory, fmx_psi_batch_dev / fmx_next_substr_batch_dev on a capturing stream return
 * FMX_ERR_HIP ("... outside a stream capture"), allocate nothing and leave the capture valid.  A build that fails
 * frees what it had allocated. */
int fmx_next_substr(const fmx_index *idx, uint64_t sp, uint32_t len, uint8_t *out, uint32_t *out_len);
/* the same for k rows at once (rendering a result list): out is k*len bytes, row q's string at q*len, out_len[q]
 * bytes of it written. */
int fmx_next_substr_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint32_t len, uint8_t *out,
                          uint32_t *out_len);
int fmx_prev_substr(const fmx_index *idx, uint64_t sp, uint32_t len, uint8_t *out);
/* Both directions behind one entry point (the name SURVEY.md 8b lists): direction > 0 = nextSubstr (the text
 * that starts at row's suffix, what SAResult.toString prints, re2.scala:11-15), direction < 0 = prevSubstr
 * (len bytes, *out_len = len).  out needs len bytes. */
int fmx_extract(const fmx_index *idx, uint64_t row, uint32_t len, int direction, uint8_t *out, uint32_t *out_len);

/* ---- BWTMerger2.calcGaps' rank loop, bwtmerger.scala:981-1023.  calcGaps keeps ONE running rank over
 * the bytes of the older text -- curRank = bucketStarts(c) + searcher.occ(c, curRank - 1): each rank query needs the
 * one before, so the loop cannot be batched, and one such chain runs slower on the GPU than on a host core
 * (profiles/r02_calcgaps_chain.txt).  These two entry points therefore answer on the HOST, from a host copy of the
 * handle's BWT' with symbol counts every 256 positions (built at first use; n <= 2^31: a merge block) -- one
 * count + a scan of < 256 bytes per query where NaiveBWTSearcher.occ (findex.scala:479-505) binary-searches an
 * inverted list.  Same answers as fmx_occ_batch on the handle (fmx_open_block quirks included).  Not a fallback:
 * every batch entry point stays on the device.
 * fmx_occ_host        : one occ(c, i) -- what a `searcher: SuffixAlgo` adapter hands calcGaps unchanged.
 * fmx_calc_gaps_chain : the loop's rank chain itself over k bytes from curRank = rank0: ranks[j] = the rank after byte
 *                       j, with the loop's own correction for c == last_char (last_char < 0: none): a rank above
 *                       rklst is bumped by one (:1011-1012); a rank EQUAL to rklst needs the caller's KMP buffer /
 *                       longSuffixCmp (:1004-1010), so the chain stops there: *done = j < k, ranks[j] = the
 *                       uncorrected rank; the caller fixes ranks[j] and calls again from byte j + 1 with rank0 =
 *                       the fixed value.  *done == k: all bytes processed. */
int fmx_occ_host(const fmx_index *idx, int c, int64_t i, uint64_t *out);
int fmx_calc_gaps_chain(const fmx_index *idx, const uint8_t *c, size_t k, uint64_t rank0, int last_char, uint64_t rklst,
                        uint64_t *ranks, size_t *done);

/* ---- FMCreator.create, bwtmerger.scala:424-533: writes the reference's .fm file (inverted position
 * lists, 4-byte big-endian entries) from the device structure, so that findex's own NaiveFMSearcher
 * and tests can consume an index this engine prepared.  n must be < 0xffffffff (the reference has
 * no 8-byte entry format, :465-469). */
int fmx_write_fm(const fmx_index *idx, const char *path);

/* ---- locate: the text position of a suffix-array row -- SALoader (bwtmerger.scala:214-249) reading the X.sa that
 * SACreator (:535-556) writes, and Util.bwtFm2sa (util.scala:213-224), the same walk over in-memory arrays.
 * Definitions: s = reverse(text) + sentinel, n = len + 1 rows; SA[row] = position in s of the row's suffix, so
 * SA[eof] = 0, SA[0] = n - 1 and SA[LF(r)] = SA[r] - 1 for every r != eof.  A search for reverse(q), q a text string of
 * length m, has rows r; q begins at text offset n - 1 - SA[r] - m (LCPSearcher.getStringOn, :322-333, reads the text there).
 * The handle keeps a SAMPLED suffix array: the rows with SA % s == 0 (s = the key "locate_sample", 1 .. 4096, default 32;
 * fmx_config_set: the default, fmx_index_config_set: one handle's own), as a bit-vector over the rows in the one-hot
 * rank-block format (~n / 7 bytes) and their SA values in row order (4 n / s bytes; 8 n / s above 2^32 rows).  It is
 * built from the BWT alone by inverting it on the device (fmx_open of .bwt/.aux has no suffix array), by
 * fmx_prepare(FMX_PREPARE_LOCATE) or else by the first locate call -- which then allocates and synchronises, like the
 * select directory at the first Psi call.  It is outside the table budget and changes no other table.  An index that is
 * not the BWT of one text (its LF cycle through row 0 is shorter than n) gets FMX_ERR_FORMAT; fmx_open_block handles
 * get FMX_ERR_UNSUPPORTED.  A locate walks LF from the row to the next sampled row: (s - 1) / 2 steps on average.
 * fmx_locate_batch     : out_pos[q] = SA[rows[q]]; FMX_ERR_ARG for a row >= n.
 * fmx_locate_batch_dev : the same on device pointers; a row >= n gets UINT64_MAX.  With the samples prepared it only
 *                        enqueues (safe inside a stream capture).
 * fmx_locate_intervals : interval i gets the SA of rows sp[i] .. sp[i] + min(ep[i] - sp[i], max_per) - 1 (max_per 0: no
 *                        limit; an interval with ep <= sp: none), in row order; out_off (k + 1 entries) = the exclusive scan
 *                        of those counts, out_off[k] = the total.  Nothing is written past out_pos[cap - 1]; the host form
 *                        returns FMX_ERR_OVERFLOW when the total exceeds cap (out_off complete, the first cap positions
 *                        written); the _dev form leaves the total in d_out_off[k] for the caller to check.
 * fmx_locate_info      : the rate, device bytes and build time (ms) of the samples; 0 bytes when they are not built.
 * fmx_write_sa         : SACreator's X.sa: n big-endian int32 values, SA[row] at byte 4 row.  n must be < 2^32
 *                        (FMX_ERR_UNSUPPORTED otherwise, as fmx_write_fm); uses the inversion at s = 1 into a temporary of
 *                        4 n bytes, the handle's own samples untouched. */
int fmx_locate_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint64_t *out_pos);
int fmx_locate_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, void *d_out_pos, void *stream);
int fmx_locate_intervals(const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t k, uint64_t max_per,
                         uint64_t *out_off, uint64_t *out_pos, size_t cap);
int fmx_locate_intervals_dev(const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, uint64_t max_per,
                             void *d_out_off, void *d_out_pos, size_t cap, void *stream);
int fmx_locate_info(const fmx_index *idx, uint32_t *rate, uint64_t *bytes, double *build_ms);
int fmx_write_sa(const fmx_index *idx, const char *path);

/* ---- LCP: LCPSuffixWalkingAlgo.getLCP (findex.scala:59-62) over the X.lcp that LCPCreator.create (bwtmerger.scala:558-652)
 * writes and LCPLoader (:176-211) reads; Util.bwtFm2LCP (util.scala:153-212) is the same over in-memory arrays.
 * Definitions: s, n and SA as for locate.  LCP[r] = length of the longest common prefix of the suffixes of rows r and r + 1
 * for r < n - 1, LCP[n - 1] = 0: a row is paired with the row BELOW it (the reference's convention, not the textbooks').
 * The sentinel is unique, so LCP[0] = 0 and no comparison runs past the end of s.
 * The array is built on the device from s and its suffix array (successor array, a pass in text order that
 * carries the match length from one position to the next, a gather back into row order).  Like construction the builds
 * ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture), check their need against the free HBM first
 * (FMX_ERR_NOMEM with the need in the message) and free every temporary on every path.  Inputs with long repeats (a run of
 * one letter) are correct and terminate; they are not fast.
 * fmx_lcp_from_text_dev : no handle.  d_text = the text (len bytes), d_sa = the suffix array of s as fmx_bwt_from_text_dev
 *                         leaves it in d_sa_or_null (u32[len + 1]), d_lcp = u32[len + 1] out.  1 <= len <= 2^32 - 2.  Peak
 *                         device memory 5 (len + 1) bytes beside the caller's three arrays.  Every index read from d_sa is
 *                         clamped below n: a d_sa that is no suffix array gives unspecified values, never a wild access.
 * fmx_lcp_from_text     : host text in, host lcp[len + 1] out: the suffix sort of fmx_bwt_from_text_dev, then the above.
 * A handle (fmx_open of .bwt/.aux has neither text nor suffix array) gets both from the inversion that builds the locate
 * samples, then runs the same core.  It keeps u32 LCP[n], 4 n bytes, outside the table budget: built by
 * fmx_prepare(FMX_PREPARE_LCP) or else by the first call below that needs it, freed by fmx_drop_tables(FMX_PREPARE_LCP) and
 * fmx_close.  fmx_open_block handles and n >= 2^32 get FMX_ERR_UNSUPPORTED; an index that is not the BWT of one text
 * FMX_ERR_FORMAT (as locate).
 * fmx_lcp_batch     : getLCP(i) / LCPLoader.read(i) for k rows: out[q] = LCP[rows[q]]; FMX_ERR_ARG for a row >= n.
 * fmx_lcp_batch_dev : the same on device pointers (u64 rows, u32 out); a row >= n gets UINT32_MAX.  With the array prepared
 *                     it only enqueues (safe inside a stream capture).
 * fmx_lcp_range[_dev] : LCPLoader.readAll's slice: out[t] = LCP[first + t], first + count <= n (FMX_ERR_ARG otherwise); the
 *                     device form is one device-to-device copy and, with the array prepared, only enqueues.
 * fmx_lcp_info      : device bytes of the array (0: not built), its build time (ms), the largest entry, the FIRST row that
 *                     holds it and the sum of all entries; any pointer may be NULL.
 * fmx_write_lcp     : LCPCreator's X.lcp: no header, big-endian int32, LCP[r] at byte 4 r for r = 0 .. n - 2 -- n - 1
 *                     entries, 4 (n - 1) bytes, as the reference's loop writes it (it never writes slot n - 1).
 * fmx_lcp_last_phases : device time (ms) the calling thread's last array build spent in its three phases (successor array,
 *                     text-order pass, gather): what tools/lcp_bench.py reports. */
int fmx_lcp_from_text_dev(const void *d_text, uint64_t len, const void *d_sa, void *d_lcp, int device, void *stream);
int fmx_lcp_from_text(const uint8_t *text, uint64_t len, uint32_t *lcp, int device);
int fmx_lcp_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint32_t *out);
int fmx_lcp_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, void *d_out, void *stream);
int fmx_lcp_range(const fmx_index *idx, uint64_t first, uint64_t count, uint32_t *out);
int fmx_lcp_range_dev(const fmx_index *idx, uint64_t first, uint64_t count, void *d_out, void *stream);
int fmx_lcp_info(const fmx_index *idx, uint64_t *bytes, double *build_ms, uint32_t *max_lcp, uint64_t *max_row,
                 uint64_t *sum_lcp);
int fmx_write_lcp(const fmx_index *idx, const char *path);
int fmx_lcp_last_phases(double *phi_ms, double *plcp_ms, double *gather_ms);

/* ---- extract: the text itself, by text position.  Beyond the reference, whose nextSubstr / prevSubstr start from a row.
 * DESIGN.md 17.  Definitions: s, n and SA as for locate; the row with SA == v (v >= 1) holds the BWT byte s[v - 1] =
 * text[n - 1 - v], so an LF walk from it reads the text forwards.  The handle keeps INVERSE-SA SAMPLES: isa[j] = the row with
 * SA == j * s for j = 0 .. (n - 1) / s (s = the key "extract_sample", 1 .. 4096, default 32; fmx_config_set: the default,
 * fmx_index_config_set: one handle's own), 4 bytes each, 8 above 2^32 rows.  They are built by
 * fmx_prepare(FMX_PREPARE_EXTRACT) or else by the first extract call -- which then allocates and synchronises (FMX_ERR_HIP
 * "... outside a stream capture" under a capture, nothing allocated, the capture left valid): from the handle's locate
 * samples by one scatter pass when those exist at the same rate, otherwise by the inversion that builds the locate samples
 * (same array either way).  The need, temporaries included, is checked against the free HBM first (FMX_ERR_NOMEM with the
 * need in the message); every temporary is freed on every path.  Outside the table budget; no other table changes.
 * Refusals as locate: fmx_open_block handles and n >= 2^37 FMX_ERR_UNSUPPORTED, an index that is not the BWT of one text
 * FMX_ERR_FORMAT.  A range is cut at every text offset t with (n - 1 - t) % s == 0 and each piece is a walk of its own from
 * the next sample (or from row 0): at most s - 1 skipped and s emitted LF steps, about 1.5 steps per byte for ranges shorter
 * than s and 1 for long ones.  Every step counts as one rank query in fmx_stats_t.rank_queries.
 * The batch is k ranges: range q is the off[q + 1] - off[q] text bytes from text offset pos[q], written at
 * out[off[q] .. off[q + 1]); off has k + 1 entries, off[0] == 0.
 * fmx_extract_text_batch     : host pointers.  FMX_ERR_ARG, decided before the device is touched: a null handle or pointer,
 *                              off[0] != 0, decreasing offsets, pos[q] + length > n - 1 (the text's length), k > 2^26,
 *                              off[k] >= 2^32.  k == 0 or only empty ranges: FMX_OK, nothing written.
 * fmx_extract_text_batch_dev : device pointers, n_bytes = off[k] given by the host.  With the samples prepared it only
 *                              enqueues (safe inside a stream capture).  IT CANNOT VALIDATE ITS OPERANDS; its kernel clamps
 *                              them before any address is formed: the range that owns an output byte is searched in
 *                              d_off[0 .. k] only, a byte that no range covers (offsets that decrease, n_bytes beyond
 *                              d_off[k]) is written as 0, a byte whose text offset is n - 1 or more is written as 0, rows read
 *                              from the samples are read as at most n - 1.  Nothing is written outside d_out[0 .. n_bytes).
 * fmx_extract_info           : the rate, device bytes and build time (ms) of the samples; 0 bytes when they are not built.
 * fmx_extract_last           : the calling thread's last host-pointer call: device time (ms) of the kernel, LF steps made,
 *                              memory requests (BWT bytes and rank-dictionary lines); any pointer may be NULL.
 * FMX_EXTRACT_TILE: the output bytes a workgroup of the kernel takes at a time (what tests aim at). */
#define FMX_EXTRACT_TILE 1024
int fmx_extract_text_batch(const fmx_index *idx, const uint64_t *pos, const uint64_t *off, size_t k, uint8_t *out);
int fmx_extract_text_batch_dev(const fmx_index *idx, const void *d_pos, const void *d_off, size_t k, uint64_t n_bytes,
                               void *d_out, void *stream);
int fmx_extract_info(const fmx_index *idx, uint32_t *rate, uint64_t *bytes, double *build_ms);
int fmx_extract_last(double *ms, uint64_t *steps, uint64_t *requests);

/* ---- approximate search: literal patterns with up to FMX_APPROX_MAX_MISMATCHES substituted bytes (Hamming distance; no
 * insertions or deletions: those are fmx_search_edit_batch, below).  Beyond the reference.  DESIGN.md 15.
 * For pattern P of m bytes (matched last byte first, as fmx_search_batch takes it), a budget e = max_mismatches and a
 * substitution range [sub_lo, sub_hi], a HIT is a byte string Q of m bytes that differs from P in d <= e positions, holds a
 * byte of the range at every differing position, and for which the reference's search(Q) loop (findex.scala:15-31) ends with
 * sp < ep.  It is reported as (pattern, d, sp, ep) with (sp, ep) exactly what fmx_search_batch returns for Q.  The definition
 * rests on cf / occ alone, so it holds for any handle (distinct Q of one length have disjoint intervals: LF is a permutation).
 * Symbol 0, the EOF slot, is never substituted (sub_lo >= 1); where Q agrees with P it holds whatever byte P holds.  An empty
 * pattern has the one hit (0, n) with d = 0; with e = 0 the hits are the patterns fmx_search_batch finds, with its intervals.
 * Results are in CSR form: pattern q's hits are out[out_off[q] .. out_off[q + 1]), by ascending sp (unique within a pattern),
 * out_off[k] == *n_out: the same input gives the same bytes on every run.
 * opts == NULL: e = 0 and the default range 1 .. 255 (sub_lo = sub_hi = 0 asks for the default range too).
 * Capacity: when the batch has more than cap hits nothing is written past out[cap - 1] and the call returns FMX_ERR_OVERFLOW
 * with *n_out = the EXACT total (out and out_off are then unspecified: call again with cap >= *n_out); cap == 0 with
 * out == NULL is the counting call.
 * FMX_ERR_ARG, decided before the device is touched: a null handle, n_out or out_off; max_mismatches above the maximum;
 * sub_lo > sub_hi, or exactly one of them 0; reserved != 0; decreasing offsets (host form); k > 2^26; cap >= 2^32.
 * FMX_ERR_UNSUPPORTED: fmx_open_block handles (and indexes of 2^38 rows or more).
 * fmx_search_approx_batch_dev: device pointers for patterns, offsets and outputs, n_out a host pointer.  Both forms ALLOCATE
 * AND SYNCHRONISE (FMX_ERR_HIP under a stream capture) and free every temporary on every path: 24 cap bytes of staging, and
 * 24 bytes per hit of sort keys and values, beside a quarter megabyte of counters.  They use the rank dictionary only, build no derived
 * table and do not count as patterns seen; their steps are added to the handle's counters (rank_queries, backward_steps,
 * search_requests) and the call to launches.
 * fmx_approx_last: the calling thread's last call: device time (ms) of the search kernel and of the ordering step, backward
 * steps executed, rank-dictionary requests issued; any pointer may be NULL. */
#define FMX_APPROX_MAX_MISMATCHES 3
typedef struct fmx_approx_hit {
  uint32_t pattern;
  uint32_t mismatches;
  uint64_t sp;
  uint64_t ep;
} fmx_approx_hit; /* 24 bytes */
typedef struct fmx_approx_opts {
  uint32_t max_mismatches; /* 0 .. FMX_APPROX_MAX_MISMATCHES */
  uint8_t sub_lo, sub_hi;  /* substitution symbols, inclusive; 0,0 = the default 1 .. 255 */
  uint16_t reserved;       /* must be 0 */
} fmx_approx_opts;
int fmx_search_approx_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k,
                            const fmx_approx_opts *opts, uint64_t *out_off /* k + 1 */, fmx_approx_hit *out, size_t cap,
                            size_t *n_out);
int fmx_search_approx_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k,
                                const fmx_approx_opts *opts, void *d_out_off, void *d_out, size_t cap, size_t *n_out,
                                void *stream);
int fmx_approx_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests);

/* ---- approximate search with insertions and deletions: edit distance up to FMX_EDIT_MAX_EDITS.  Beyond the reference.
 * DESIGN.md 19.
 * P is a pattern of m bytes (matched last byte first, as everywhere), e = max_edits the budget, A = [sub_lo, sub_hi] the
 * symbol range (sub_lo >= 1; 0, 0 = the default 1 .. 255).  d_A(Q, P) is the smallest cost of an alignment of Q with P in which
 *   - equal bytes cost 0, whatever the byte (0 included);
 *   - a Q byte of A standing for a different P byte costs 1 (substitution);
 *   - a Q byte of A standing for nothing costs 1 (insertion);
 *   - a P byte standing for nothing costs 1, whatever the byte (deletion);
 *   - a Q byte outside A may only stand for an equal P byte.
 * With the default range and no byte 0 in the text d_A is the Levenshtein distance.
 * A HIT is a byte string Q of any length (necessarily m - e .. m + e) with d = d_A(Q, P) <= e for which the reference's
 * search(Q) loop (findex.scala:15-31) ends with sp < ep.  It is reported as (pattern, d, len = |Q|, sp, ep) with (sp, ep)
 * exactly what fmx_search_batch returns for Q.  The empty Q is a hit when m <= e (d = m, the interval (0, n), len 0); an empty
 * P therefore has the hit (0, n) with d = 0 and every occurring string over A of 1 .. e bytes.  With e = 0 the hits are those
 * of the exact search, with len = m.  The definition rests on cf / occ alone, so it holds for any handle.  Distinct Q of one
 * length have disjoint intervals; Q of different lengths may share sp.
 * Results are in CSR form: pattern q's hits are out[out_off[q] .. out_off[q + 1]), by ascending (sp, len) (unique within a
 * pattern), out_off[k] == *n_out: the same input gives the same bytes on every run.
 * opts == NULL: e = 0 and the default range.
 * Capacity, the counting call and the refusals are those of fmx_search_approx_batch: more than cap hits -> nothing is written
 * past out[cap - 1], FMX_ERR_OVERFLOW with *n_out = the EXACT total (out and out_off then unspecified); cap == 0 with
 * out == NULL is the counting call.
 * FMX_ERR_ARG, decided before the device is touched: a null handle, n_out or out_off; max_edits above the maximum;
 * sub_lo > sub_hi, or exactly one of them 0; reserved != 0; decreasing offsets (host form); k > 2^23; cap >= 2^32; a pattern
 * of more than FMX_EDIT_MAX_LEN bytes (host form).  The device form cannot see the lengths: its kernel skips such a pattern
 * and raises a flag, and the call returns FMX_ERR_ARG after the launch with no hits written and *n_out untouched.
 * FMX_ERR_UNSUPPORTED: fmx_open_block handles (and indexes of 2^38 rows or more).
 * Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture) and free every temporary on every path.  The
 * working set: 24 cap bytes of staging; the walk's stacks, 258 frames of 320 bytes (82 560 bytes) for every wave of the launch,
 * four waves per workgroup and at most the workgroups the device holds at once (one per four patterns for a small batch; about
 * 0.6 GB at 1792 workgroups); 24 bytes per hit of sort keys and values; a quarter megabyte of counters.  Staging, stacks and
 * counters are checked against the free device memory first: FMX_ERR_NOMEM with the need in the message.
 * The calls use the rank dictionary only, build no derived table and do not count as patterns seen; their steps are added to
 * the handle's counters (rank_queries, backward_steps, search_requests) and the call to launches.
 * fmx_edit_last: the calling thread's last call: device time (ms) of the search kernel and of the ordering step, backward
 * steps executed, rank-dictionary requests issued; any pointer may be NULL. */
#define FMX_EDIT_MAX_EDITS 2
#define FMX_EDIT_MAX_LEN 255 /* pattern bytes */
typedef struct fmx_edit_hit {
  uint32_t pattern;
  uint16_t edits;
  uint16_t len; /* bytes of the string that occurs */
  uint64_t sp;
  uint64_t ep;
} fmx_edit_hit; /* 24 bytes */
typedef struct fmx_edit_opts {
  uint32_t max_edits;     /* 0 .. FMX_EDIT_MAX_EDITS */
  uint8_t sub_lo, sub_hi; /* symbols that may be inserted or substituted, inclusive; 0,0 = the default 1 .. 255 */
  uint16_t reserved;      /* must be 0 */
} fmx_edit_opts;
int fmx_search_edit_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_edit_opts *opts,
                          uint64_t *out_off /* k + 1 */, fmx_edit_hit *out, size_t cap, size_t *n_out);
int fmx_search_edit_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_edit_opts *opts,
                              void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream);
int fmx_edit_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests);

/* ---- matching statistics and maximal exact matches (MEMs) of long queries.  Beyond the reference.  DESIGN.md 16.
 * The batch is k patterns, contiguous in pat: pattern q is pat[off[q] .. off[q + 1]), off[0] == 0, off[k] == n_bytes.  The
 * statistics are PARALLEL TO pat: entry j belongs to byte j.  For byte j of pattern q let e = j - off[q] + 1 and
 * L = min(e, max_len): the reference's loop (findex.scala:15-31) runs from (0, n) over pat[j], pat[j - 1], .., stops before
 * the first step whose result is empty and after L steps at the latest.  len[j] = the steps completed, (sp[j], ep[j]) = the
 * interval after the last of them, (0, n) when len[j] == 0.  A walk never crosses into pattern q - 1.  On the BWT of a text
 * len[j] is the length of the longest suffix of pat[off[q] .. j], capped at max_len, that occurs, and (sp, ep) what
 * fmx_search_batch returns for that suffix; byte 0 in a pattern is treated as the exact search treats it.
 * MEMs: with min_len >= 1, byte j ends a reported match iff len[j] >= min_len and (j is the last byte of its pattern or
 * len[j + 1] <= len[j]); the hit is (pattern q, len, end = e, sp, ep), the match P[end - len .. end), left-maximal by
 * construction.  A hit with len == max_len is SATURATED: it may be a piece of a longer match, and a run of saturated
 * positions is reported position by position (raise max_len).  Output is CSR: out_off[k + 1], a pattern's hits by ascending
 * end -- the same input gives the same bytes on every run.
 * fmx_match_stats_batch_dev ONLY ENQUEUES (no allocation, copy or synchronisation: safe inside a stream capture) and cannot
 * validate its operands: a position that no pattern covers gets len 0, (0, n), and no operand value leads outside pat or the
 * index.  The host form and both MEM forms ALLOCATE AND SYNCHRONISE (the _dev MEM form: FMX_ERR_HIP under a stream capture,
 * decided before anything is allocated); their need -- for the MEM calls 20 bytes per pattern byte of statistics plus 4 for
 * the scan -- is checked against the free HBM first (FMX_ERR_NOMEM with the need in the message), and every temporary is
 * freed on every path.  fmx_mems_batch: FMX_ERR_OVERFLOW with the exact *n_out when the hits exceed cap (records past cap
 * are not written); cap == 0 with out == NULL is the counting call.
 * FMX_ERR_ARG, decided before the device is touched: a null handle or output; max_len > FMX_MSTAT_MAX_LEN; min_len >
 * max_len; reserved != 0; off[0] != 0 or decreasing offsets (host forms); k > 2^26; n_bytes >= 2^32; cap >= 2^32.
 * FMX_ERR_UNSUPPORTED: fmx_open_block handles.
 * All forms use the rank dictionary only, build no derived table and do not count as patterns seen; every executed step,
 * the one that empties an interval included, is added to the handle's counters (rank_queries, backward_steps,
 * search_requests).  fmx_mstat_last: the calling thread's last host or MEM call (the enqueue-only form does not update it):
 * device time (ms) of the walk kernel and of the compaction, steps executed, rank-dictionary requests; any pointer may be NULL.
 * FMX_MSTAT_TILE: the positions a workgroup of the walk kernel takes at a time (what tests aim at). */
#define FMX_MSTAT_MAX_LEN 4096
#define FMX_MSTAT_TILE 512
typedef struct fmx_mstat_opts {
  uint32_t max_len;     /* 1 .. FMX_MSTAT_MAX_LEN; 0 = the maximum */
  uint32_t min_len;     /* MEMs only; 0 = 1 */
  uint32_t reserved[2]; /* must be 0 */
} fmx_mstat_opts;
typedef struct fmx_mem_hit {
  uint32_t pattern;
  uint32_t len;
  uint64_t end;
  uint64_t sp;
  uint64_t ep;
} fmx_mem_hit; /* 32 bytes */
int fmx_match_stats_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_mstat_opts *opts,
                          uint32_t *out_len, uint64_t *out_sp_or_null, uint64_t *out_ep_or_null);
int fmx_match_stats_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, uint64_t n_bytes,
                              const fmx_mstat_opts *opts, void *d_len, void *d_sp_or_null, void *d_ep_or_null, void *stream);
int fmx_mems_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_mstat_opts *opts,
                   uint64_t *out_off /* k + 1 */, fmx_mem_hit *out, size_t cap, size_t *n_out);
int fmx_mems_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, uint64_t n_bytes,
                       const fmx_mstat_opts *opts, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream);
int fmx_mstat_last(double *walk_ms, double *compact_ms, uint64_t *steps, uint64_t *requests);

/* ---- repeats: the stretches of the indexed text that occur more than once, from the LCP array.  Beyond the reference, whose
 * one consumer of the array is an unfinished experiment.  DESIGN.md 18.
 * Definitions.  T is the text of m = n - 1 bytes, L >= 1 a threshold.  The WINDOW at t (0 <= t <= m - L) is T[t .. t + L).
 * With a stop byte c != 0 a window that contains c is not ELIGIBLE; with c == 0 every window is (byte 0 never occurs in a
 * text).  A CLASS is the set of all eligible windows with the same L bytes -- occurrences may overlap: "aaaa" at L = 2 has
 * one class of three windows -- and it is REPEATED when it has at least two windows.  The MODE decides which windows of a
 * repeated class are FLAGGED: FMX_REPEATS_ALL every one of them, FMX_REPEATS_LATER every one but the one with the smallest t
 * ("keep the first copy").  The RESULT is the union of [t, t + L) over the flagged windows, reported as its maximal ranges
 * [start, end) in text offsets, ascending; two ranges that abut are one range.  A stop byte is never covered, so with a
 * corpus' separator as the stop byte no range spans two documents.  The SUMMARY of a threshold: the number of ranges, the
 * covered bytes, the repeated classes, the flagged windows, the size of the largest repeated class and the smallest text
 * offset of a window of that class (among classes of that size: the smallest such offset); all 0 when nothing repeats.
 * The same input gives the same bytes on every run.
 * In the index's terms (s = reverse(T) + sentinel, SA and LCP as for locate and the LCP array): window t is s[p .. p + L)
 * with p = m - t - L; the windows of one class are a maximal run of rows whose consecutive LCP[r] >= L; a row belongs to a
 * repeated class iff LCP[r - 1] >= L or LCP[r] >= L; the smallest t is the largest SA value of the run.
 * One call takes k thresholds (1 .. FMX_REPEATS_MAX_LEVELS) and pays for the suffix array once: one inversion, then one set
 * of streaming passes per threshold.  Output is CSR: threshold j's ranges are out[out_off[j] .. out_off[j + 1]),
 * out_off[k] == *n_out.  Capacity: with more than cap ranges the call returns FMX_ERR_OVERFLOW with the exact total in
 * *n_out, out_off complete and the summaries valid; nothing is written past out[cap - 1]; cap == 0 with out == NULL is the
 * counting call.  opts == NULL: FMX_REPEATS_ALL and no stop byte.  A threshold above m is valid and has no ranges.
 * FMX_ERR_ARG, decided before the device is touched: a null handle, min_len, out_off or n_out; k == 0 or k >
 * FMX_REPEATS_MAX_LEVELS; a threshold of 0; a mode above 1; a reserved byte that is not 0; cap >= 2^32.
 * The call needs the handle's LCP array and builds it when absent, with its refusals: fmx_open_block handles and n >= 2^32
 * FMX_ERR_UNSUPPORTED, an index that is not the BWT of one text FMX_ERR_FORMAT.  Both forms ALLOCATE AND SYNCHRONISE (the
 * _dev form: FMX_ERR_HIP under a stream capture, decided before anything is allocated, the capture left valid).  The need --
 * about 18 bytes per row beside the LCP array: the suffix array, s, two u32 work arrays, the stop scan and the flags, plus
 * the inversion's temporaries and the LCP build's when that is still to come -- is checked against the free HBM first
 * (FMX_ERR_NOMEM with the need in the message); every temporary is freed on every path.  No table and no counter of patterns
 * seen changes; the launches are added to the handle's.
 * fmx_repeats_dev : d_out_off (u64[k + 1]) and d_out (16-byte records) in device memory; min_len, n_out and the summaries
 *                   stay host pointers.
 * fmx_repeats_last: device time (ms) of the calling thread's last call by phase -- the inversion (with the stop scan), the
 *                   class passes, the coverage passes, the compaction -- summed over the thresholds; any pointer may be NULL.
 * FMX_REPEATS_TILE: the elements one workgroup of the scans takes -- where a carry crosses from one workgroup's stretch of
 * rows or text bytes to the next (what tests aim at). */
#define FMX_REPEATS_ALL 0u
#define FMX_REPEATS_LATER 1u
#define FMX_REPEATS_MAX_LEVELS 64
#define FMX_REPEATS_TILE 2048
typedef struct fmx_repeat_opts {
  uint32_t mode;       /* FMX_REPEATS_ALL | FMX_REPEATS_LATER */
  uint8_t stop;        /* the stop byte; 0 = none */
  uint8_t reserved[3]; /* must be 0 */
} fmx_repeat_opts;
typedef struct fmx_repeat_range {
  uint64_t start, end;
} fmx_repeat_range; /* 16 bytes */
typedef struct fmx_repeat_summary {
  uint64_t ranges, covered_bytes, classes, windows, largest_class, largest_class_pos;
} fmx_repeat_summary; /* 48 bytes */
int fmx_repeats(const fmx_index *idx, const uint32_t *min_len, size_t k, const fmx_repeat_opts *opts,
                uint64_t *out_off /* k + 1 */, fmx_repeat_range *out, size_t cap, size_t *n_out,
                fmx_repeat_summary *summary_or_null /* k */);
int fmx_repeats_dev(const fmx_index *idx, const uint32_t *min_len, size_t k, const fmx_repeat_opts *opts, void *d_out_off,
                    void *d_out, size_t cap, size_t *n_out, fmx_repeat_summary *summary_or_null /* k */, void *stream);
int fmx_repeats_last(double *invert_ms, double *class_ms, double *cover_ms, double *compact_ms);

/* ---- n-grams: which strings of L bytes occur in the indexed text, and how often -- the k-mer table, its multiplicity
 * spectrum and the most frequent phrases, from the LCP array.  Beyond the reference.  DESIGN.md 22.
 * Definitions.  WINDOW, ELIGIBLE (a stop byte c != 0: a window that contains c is not) and CLASS are those of the repeats
 * section: a class is the set of all eligible windows with the same L bytes.  The COUNT of a class is its number of windows
 * (overlapping windows count: "aaaa" at L = 2 is one class of count 3), its FIRST position the smallest t.
 * In the index's terms: a class is a maximal run of rows whose consecutive LCP[r] >= L; its interval [sp, sp + count) is the
 * one search(reverse(window)) returns, its first position m - L - (the largest SA value of the run).  Exactly min(L, n)
 * rows have fewer than L bytes in front of the sentinel; each is a run of one row and no window.
 * One call takes k lengths (1 .. FMX_NGRAMS_MAX_LEVELS) and returns per length
 *   RECORDS  fmx_ngram (sp, count, first_pos), one per eligible class with count >= min_count.  FMX_NGRAMS_BY_ROW: ascending
 *            by sp (the lexicographic order of reverse(window)); FMX_NGRAMS_BY_COUNT: descending by count, ties ascending by
 *            sp -- a total order.  top != 0 keeps the first `top` records of that order.  CSR as in repeats: length j's
 *            records are out[out_off[j] .. out_off[j + 1]), out_off[k] == *n_out.
 *   SUMMARY  fmx_ngram_summary: records (after top), selected (classes with count >= min_count, before top), distinct
 *            (eligible classes of every count), windows (eligible windows), singletons, largest_count, largest_sp (the
 *            smallest sp among the classes of that count) and largest_pos (its first position); all 0 without a class.
 *   SPECTRUM (spectrum_bins = B in 1 .. FMX_NGRAMS_MAX_BINS; 0: none) uint64 spectrum[k * B]: entry c (1 <= c < B) of a length
 *            is the number of eligible classes of count c, entry 0 the number with count >= B.
 * opts == NULL: BY_ROW, min_count 2, no top, no spectrum, no stop byte.
 * FMX_NGRAMS_NO_POS (a flag): first_pos and largest_pos come back as UINT64_MAX and NO INVERSION IS RUN -- counts, intervals,
 * order, summary and spectrum come from the LCP array alone, the rows that are no windows by the closed form above.  Valid
 * only with stop == 0 and min_count >= 2 (eligibility needs text positions, and a listed singleton has to be told from a short
 * row); every other field equals the call with positions bit for bit.
 * Capacity, the counting call (cap == 0, out == NULL), FMX_ERR_OVERFLOW with the exact total and out_off and the summaries
 * complete, "nothing written past out[cap - 1]" and determinism: as in repeats.  A length above m is valid, has no records
 * and runs no pass.
 * FMX_ERR_ARG, decided before the device is touched: a null handle, lengths, out_off or n_out; k == 0 or k >
 * FMX_NGRAMS_MAX_LEVELS; a length of 0; order > 1; an unknown flag; min_count == 0; FMX_NGRAMS_NO_POS with a stop byte or with
 * min_count == 1; spectrum_bins > FMX_NGRAMS_MAX_BINS; spectrum_bins != 0 with a null spectrum; a reserved byte that is not 0;
 * cap >= 2^32.
 * The call needs the handle's LCP array and builds it when absent, with its refusals: fmx_open_block handles and n >= 2^32
 * FMX_ERR_UNSUPPORTED before the device is touched, an index that is not the BWT of one text FMX_ERR_FORMAT.  Both forms
 * ALLOCATE AND SYNCHRONISE (the _dev form: FMX_ERR_HIP under a stream capture, decided before anything is allocated, the
 * capture left valid).  The need -- with positions about 17 bytes per row beside the LCP array (the suffix array, s, three u32
 * work arrays) and 4 more with a stop byte, plus the inversion's temporaries; without positions 8 bytes per row; the LCP
 * build's when that is still to come -- is checked against the free HBM first, the sort's buffers (28 bytes per selected class)
 * once a length's selected classes are counted (FMX_ERR_NOMEM with the need in the message); every temporary is freed on every
 * path.  No table and no counter of patterns seen changes; the launches are added to the handle's.
 * fmx_ngrams_dev : d_out_off (u64[k + 1]) and d_out (24-byte records) in device memory; lengths, n_out, the summaries and
 *                  the spectrum stay host pointers.
 * fmx_ngrams_last: device time (ms) of the calling thread's last call by phase -- the inversion (with the stop scan; 0 for a
 *                  FMX_NGRAMS_NO_POS call), the class passes, the selection (slot scan, keys, records), the sort -- summed over
 *                  the lengths; any pointer may be NULL.
 * FMX_NGRAMS_LDS_BINS: counts below it are histogrammed in LDS, counts at or above it go to global memory one by one (what
 * tests stand on both sides of). */
#define FMX_NGRAMS_BY_ROW 0u
#define FMX_NGRAMS_BY_COUNT 1u
#define FMX_NGRAMS_NO_POS 1u
#define FMX_NGRAMS_MAX_LEVELS 64
#define FMX_NGRAMS_MAX_BINS 65536u
#define FMX_NGRAMS_LDS_BINS 1024
typedef struct fmx_ngram_opts {
  uint32_t order;         /* FMX_NGRAMS_BY_ROW | FMX_NGRAMS_BY_COUNT */
  uint32_t flags;         /* FMX_NGRAMS_NO_POS or 0 */
  uint64_t min_count;     /* >= 1 */
  uint64_t top;           /* 0 = all */
  uint32_t spectrum_bins; /* 0 .. FMX_NGRAMS_MAX_BINS */
  uint8_t stop;           /* the stop byte; 0 = none */
  uint8_t reserved[3];    /* must be 0 */
} fmx_ngram_opts; /* 32 bytes */
typedef struct fmx_ngram {
  uint64_t sp, count, first_pos;
} fmx_ngram; /* 24 bytes */
typedef struct fmx_ngram_summary {
  uint64_t records, selected, distinct, windows, singletons, largest_count, largest_sp, largest_pos;
} fmx_ngram_summary; /* 64 bytes */
int fmx_ngrams(const fmx_index *idx, const uint32_t *lengths, size_t k, const fmx_ngram_opts *opts,
               uint64_t *out_off /* k + 1 */, fmx_ngram *out, size_t cap, size_t *n_out,
               fmx_ngram_summary *summary_or_null /* k */, uint64_t *spectrum_or_null /* k * spectrum_bins */);
int fmx_ngrams_dev(const fmx_index *idx, const uint32_t *lengths, size_t k, const fmx_ngram_opts *opts, void *d_out_off,
                   void *d_out, size_t cap, size_t *n_out, fmx_ngram_summary *summary_or_null /* k */,
                   uint64_t *spectrum_or_null /* k * spectrum_bins */, void *stream);
int fmx_ngrams_last(double *invert_ms, double *class_ms, double *select_ms, double *sort_ms);

/* ---- corpus: a directory of files as ONE index -- DirBWTReader (bwtreader.scala:17-173), the input side of the reference's
 * IndexerApp -- and, beyond the reference, the way back from a stream position to (document, offset).
 * The STREAM: the documents in the caller's order; in each, raw byte 0 becomes '\' '0', raw 1 becomes '\' '1' and raw 255
 * becomes '\' 'f' (:144-155; the backslash itself is not escaped, the reference's quirk), and after every document, the last
 * one included, comes one separator byte 1 (:133-137).  Byte 1 therefore occurs only between documents: no match of an
 * escaped pattern spans two of them.  Which files make up the documents, and in which order, is the host's business
 * (findex_amd/corpus.py: list_files); this ABI takes their raw bytes back to back and their end offsets.
 * An fmx_corpus is bound to one device.  It owns the MAP -- doc_start[n_docs + 1] (each document's first stream position,
 * the last entry the stream length; strictly increasing), esc_pos[n_esc] (the stream position of each escape's backslash,
 * ascending) and the escapes in front of each document -- and, until fmx_corpus_drop_stream, the stream itself in HBM.
 * Limits: 1 <= n_docs < 2^32 - 1, 1 <= stream length <= 2^32 - 2 (the suffix sort's): FMX_ERR_UNSUPPORTED beyond.
 * fmx_corpus_build     : raw[raw_len] on the host, doc_ends[n_docs] (non-decreasing, repeated for empty documents, the last
 *                        == raw_len; FMX_ERR_ARG otherwise) -> a corpus.  The stream is built on the device (a count pass per
 *                        tile of raw bytes, a scan, an emit pass through LDS; no atomics: the same input gives the same bytes
 *                        on every run).  Like index construction it ALLOCATES AND SYNCHRONISES: FMX_ERR_HIP under a stream
 *                        capture; what it needs is checked against the free HBM first -- before the first allocation the part
 *                        known without the escape count, after the count pass the exact rest (FMX_ERR_NOMEM with the need in
 *                        the message); every temporary is freed on every path.
 * fmx_corpus_build_dev : the same with the raw bytes already in HBM (doc_ends stays a host pointer), on `stream`.
 * fmx_corpus_info      : documents, stream length, escapes, device bytes held, build time (ms), and the build's tile size in
 *                        raw bytes (what tests aim at); any pointer may be NULL, and so may the corpus (then only the tile
 *                        size is meaningful).
 * fmx_corpus_stream    : the stream copied to the host (cap >= stream length, FMX_ERR_OVERFLOW otherwise): what
 *                        DirBWTReader(caching = true) leaves at genDataFilename, X.data.
 * fmx_corpus_stream_dev: the stream's device pointer (valid until the stream is dropped or the corpus freed).
 * fmx_corpus_drop_stream: frees the stream in HBM; the map stays.
 * fmx_corpus_open_index: fmx_bwt_from_text_dev over the stream, then fmx_open_dev on its output -- no host round trip of the
 *                        text; an ordinary fmx_index (close it with fmx_close; it does not depend on the corpus).
 * fmx_corpus_tables    : host copies of doc_start[n_docs + 1], raw_len[n_docs] (each document's length on disk) and
 *                        esc_pos[n_esc]; any pointer may be NULL.
 * fmx_corpus_from_tables: a corpus (map only, no stream) from such copies; tables that contradict each other: FMX_ERR_FORMAT.
 * fmx_corpus_map       : for k stream positions p: doc = the largest d with doc_start[d] <= p, esc_off = p - doc_start[d]
 *                        (the offset in the escaped document), raw_off = esc_off - #{e in esc_pos : doc_start[d] <= e < p}
 *                        (the offset in the file on disk).  The second byte of an escape maps to the raw offset of the byte it
 *                        stands for; a separator maps to (d, the raw length of d); p >= stream length gives doc = UINT32_MAX
 *                        (and UINT64_MAX offsets).  Two binary searches per position.
 * fmx_corpus_map_dev   : the same on device pointers (u64 pos, u32 doc, u64 offsets); it only enqueues (safe inside a stream
 *                        capture).
 * fmx_corpus_doc_list  : for k row intervals (sp, ep) of `idx` -- the index of this corpus' stream -- found by searching the
 *                        reverse of an escaped pattern of pat_len stream bytes: the distinct documents of each interval's
 *                        first min(ep - sp, max_per) rows (max_per 0: all) with their hit counts, in CSR form: out_off[k + 1],
 *                        out_doc[], out_cnt[]; within an interval the documents ascend.  A row whose position
 *                        stream_len - pat_len - SA is not a stream position (an interval that no such search found, a
 *                        wrong pat_len) is listed as document UINT32_MAX, after the interval's real documents.  Nothing is written past entry
 *                        cap - 1; the host form returns FMX_ERR_OVERFLOW when out_off[k] > cap (out_off complete, the first
 *                        cap entries written), the _dev form leaves the total in d_out_off[k] for the caller to check.  Locate,
 *                        map, a radix sort of (interval, document) keys, heads and compaction, all on the device.  Both forms
 *                        allocate and synchronise (FMX_ERR_HIP under a stream capture).
 * fmx_corpus_doc_list_phases: device time (ms) of the calling thread's last listing in its four phases.
 * fmx_corpus_free      : NULL is FMX_OK.
 * fmx_corpus_escape    : host helper: a query escaped the way the stream is (at most 2 len bytes; *out_len = the bytes
 *                        needed, FMX_ERR_OVERFLOW when cap is smaller). */
typedef struct fmx_corpus fmx_corpus;
int fmx_corpus_build(const uint8_t *raw, uint64_t raw_len, const uint64_t *doc_ends, uint64_t n_docs, int device,
                     fmx_corpus **out);
int fmx_corpus_build_dev(const void *d_raw, uint64_t raw_len, const uint64_t *doc_ends, uint64_t n_docs, int device,
                         void *stream, fmx_corpus **out);
int fmx_corpus_free(fmx_corpus *corpus);
int fmx_corpus_info(const fmx_corpus *corpus, uint64_t *n_docs, uint64_t *stream_len, uint64_t *n_esc, uint64_t *bytes,
                    double *build_ms, uint32_t *tile_bytes);
int fmx_corpus_stream(const fmx_corpus *corpus, uint8_t *out, uint64_t cap);
int fmx_corpus_stream_dev(const fmx_corpus *corpus, const void **d_stream, uint64_t *stream_len);
int fmx_corpus_drop_stream(fmx_corpus *corpus);
int fmx_corpus_open_index(const fmx_corpus *corpus, void *stream, fmx_index **out);
int fmx_corpus_tables(const fmx_corpus *corpus, uint64_t *doc_start, uint64_t *raw_len, uint64_t *esc_pos);
int fmx_corpus_from_tables(const uint64_t *doc_start, const uint64_t *raw_len, const uint64_t *esc_pos, uint64_t n_docs,
                           uint64_t n_esc, int device, fmx_corpus **out);
int fmx_corpus_map(const fmx_corpus *corpus, const uint64_t *pos, size_t k, uint32_t *doc, uint64_t *esc_off,
                   uint64_t *raw_off);
int fmx_corpus_map_dev(const fmx_corpus *corpus, const void *d_pos, size_t k, void *d_doc, void *d_esc_off,
                       void *d_raw_off, void *stream);
int fmx_corpus_doc_list(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t k,
                        uint64_t pat_len, uint64_t max_per, uint64_t *out_off, uint32_t *out_doc, uint32_t *out_cnt,
                        size_t cap);
int fmx_corpus_doc_list_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k,
                            uint64_t pat_len, uint64_t max_per, void *d_out_off, void *d_out_doc, void *d_out_cnt,
                            size_t cap, void *stream);
int fmx_corpus_doc_list_phases(double *locate_ms, double *map_ms, double *sort_ms, double *compact_ms);
int fmx_corpus_escape(const uint8_t *in, size_t len, uint8_t *out, size_t cap, size_t *out_len);

/* ---- ranked retrieval: the top-K documents of multi-term queries by BM25.  Beyond the reference.  DESIGN.md 26.
 * The definition is exact, not "BM25 up to rounding": a result can be compared bit for bit.
 * INPUTS.  A call takes n_terms term slots.  Slot t is a row interval (sp[t], ep[t]) of `idx`, the index of this corpus'
 * stream, as a search for the reverse of the escaped term finds it.  q_off[n_queries + 1] cuts the slots into queries
 * (q_off[0] == 0, non-decreasing, q_off[n_queries] == n_terms): slots are never shared between queries, and a term given
 * twice in a query is two slots and counts twice.
 * DOCUMENT OF A ROW.  The document that holds stream position stream_len - 1 - SA, the LAST byte of the occurrence.  It does
 * not depend on the term's length, so terms of any lengths share one call (fmx_corpus_doc_list needs one call per length);
 * an escaped term never holds the separator byte 1, so its first and last byte lie in one document.  A row with
 * SA > stream_len - 1 belongs to no document and is dropped.
 * TERM FREQUENCY.  tf(t, d) = the rows of slot t in document d; overlapping occurrences count.  With max_per != 0 only the
 * first min(ep - sp, max_per) rows of every slot are taken, as fmx_locate_intervals takes them.  df(t) = the documents with
 * tf(t, d) > 0.
 * CORPUS CONSTANTS.  N = n_docs (empty documents count); len(d) = the RAW length of d = doc_start[d + 1] - doc_start[d] - 1
 * - (the escapes of d); avglen = (double)(stream_len - n_docs - n_esc) / (double)n_docs.
 * WEIGHTS.  `weights` (n_terms doubles, all finite, else FMX_ERR_ARG; negative ones allowed) are used as they are; NULL:
 * w(t) = log(1.0 + ((double)(N - df) + 0.5) / ((double)df + 0.5)), computed on the HOST in double (std::log) from the df the
 * call reads back.  The weights used and the df come back through out_weight and out_df; either may be NULL.
 * SCORE.  IEEE double on the device, every operation rounded once and none contracted into an FMA, in this order:
 *   r     = avglen == 0 ? 0.0 : (double)len(d) / avglen
 *   nd    = k1 * ((1.0 - b) + b * r)
 *   c(t)  = w(t) * (((double)tf * (k1 + 1.0)) / ((double)tf + nd))
 *   score = (((0.0 + c(t0)) + c(t1)) + ..) over the query's slots with tf > 0, in ascending slot order
 * with k1 >= 0 and 0 <= b <= 1, both finite (FMX_ERR_ARG otherwise).
 * CANDIDATES of a query: the documents with tf > 0 for at least one of its slots; with FMX_RANK_ALL only those with
 * tf > 0 for every one of its slots.
 * OUTPUT.  CSR over the queries: out_off[n_queries + 1], out_doc[], out_score[].  Query i gets its min(top, candidates) best
 * by score descending, equal scores (plain == on the doubles; a score is never -0.0) by document ascending.  A query with no
 * slots or no candidates gets nothing.  Nothing is written past entry cap - 1; the host form returns FMX_ERR_OVERFLOW when
 * out_off[n_queries] > cap (out_off complete, the first cap entries written), the _dev form leaves the total in
 * d_out_off[n_queries] for the caller to check.
 * LIMITS, each refused with a message that names it: 1 <= top <= 1024 and at most 64 slots per query (FMX_ERR_ARG); fewer
 * than 2^32 - 1 located rows per call, and bits_for(n_queries) + bits_for(n_docs) + bits_for(slots of the longest query) <=
 * 64, bits_for(v) being the bits that hold 0 .. v (FMX_ERR_UNSUPPORTED); the handles locate refuses.
 * The host form decides every FMX_ERR_ARG above before a handle or the device is touched.  fmx_corpus_rank_dev: the same with
 * every array a device pointer (u64 sp / ep / q_off / out_off, f64 weights / out_score / out_weight, u32 out_doc / out_df).
 * Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture, decided before anything is allocated); the need is
 * checked against the free HBM before every allocation (FMX_ERR_NOMEM with the need in the message) and every temporary is
 * freed on every path.  Locate, the listing's key sort, a second sort over the postings, one lane per candidate for the
 * score and one workgroup per query for the selection (a radix select above 1024 candidates, a bitonic sort in LDS); no
 * atomic decides an order: the same input gives the same bytes.
 * fmx_corpus_rank_last: device time (ms) of the calling thread's last ranking in its four phases, and the rows located,
 * the (slot, document) postings and the (query, document) candidates it went through. */
#define FMX_RANK_ALL 1u
typedef struct fmx_rank_params {
  double k1, b;
  uint64_t max_per; /* rows taken of every slot; 0 = all */
  uint32_t top;     /* results per query, 1 .. 1024 */
  uint32_t flags;   /* FMX_RANK_ALL or 0 */
} fmx_rank_params;  /* 32 bytes */
int fmx_corpus_rank(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_terms,
                    const uint64_t *q_off, size_t n_queries, const fmx_rank_params *params, const double *weights,
                    uint64_t *out_off, uint32_t *out_doc, double *out_score, size_t cap, uint32_t *out_df,
                    double *out_weight);
int fmx_corpus_rank_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_terms,
                        const void *d_q_off, size_t n_queries, const fmx_rank_params *params, const void *d_weights,
                        void *d_out_off, void *d_out_doc, void *d_out_score, size_t cap, void *d_out_df,
                        void *d_out_weight, void *stream);
int fmx_corpus_rank_last(double *locate_ms, double *postings_ms, double *score_ms, double *select_ms, uint64_t *rows,
                         uint64_t *postings, uint64_t *candidates);
/* fmx_corpus_rank_sets: the same ranking where a term slot is a SET of intervals: n_iv intervals sp[] / ep[],
 * and set_off[n_terms + 1] (starting at 0, never decreasing, ending at n_iv; FMX_ERR_ARG otherwise) cuts them into the
 * n_terms slots q_off speaks of.  tf(t, d) = the rows of ALL of slot t's intervals in document d: the caller promises
 * intervals that are disjoint inside a slot, and a row given twice counts twice.  max_per applies per interval.  A slot
 * without intervals has df = 0.  weights, out_df and out_weight are per slot.  Everything else -- the score, the tie order,
 * the limits (with n_iv < 2^32 - 1 in the place of the interval count), the outputs, fmx_corpus_rank_last -- is
 * fmx_corpus_rank's, and with set_off = 0, 1, .., n_terms the outputs are fmx_corpus_rank's byte for byte.  What the
 * whole-word ranking runs on: the row ranges fmx_search_context_batch leaves are rows of the plain term.
 * fmx_corpus_rank_sets_dev: every array a device pointer (d_set_off: u64[n_terms + 1]). */
int fmx_corpus_rank_sets(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_iv,
                         const uint64_t *set_off, size_t n_terms, const uint64_t *q_off, size_t n_queries,
                         const fmx_rank_params *params, const double *weights, uint64_t *out_off, uint32_t *out_doc,
                         double *out_score, size_t cap, uint32_t *out_df, double *out_weight);
int fmx_corpus_rank_sets_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
                             const void *d_set_off, size_t n_terms, const void *d_q_off, size_t n_queries,
                             const fmx_rank_params *params, const void *d_weights, void *d_out_off, void *d_out_doc,
                             void *d_out_score, size_t cap, void *d_out_df, void *d_out_weight, void *stream);

/* ---- passages: for every ranked hit the window of W stream bytes that holds the most valuable set of the query's terms,
 * and the count of every term in the hit's file.  Beyond the reference.  DESIGN.md 29.  Exact, like the ranking: a result
 * can be compared bit for bit.
 * INPUTS.  corpus, idx and the term slots exactly as fmx_corpus_rank_sets takes them: n_iv intervals sp[] / ep[],
 * set_off[n_terms + 1] cuts them into slots (NULL: one interval per slot, n_iv == n_terms, else FMX_ERR_ARG),
 * q_off[n_queries + 1] cuts the slots into queries of at most 64 slots.  term_len[n_terms] (u32, >= 1, else FMX_ERR_ARG):
 * the length in STREAM bytes of the strings of slot t; all intervals of a slot share it (an exact term, its case spellings
 * and its whole-word runs do).  The hits: hit_off[n_queries + 1] (from 0, never decreasing) and hit_doc[n_hits], n_hits =
 * hit_off[n_queries], are fmx_corpus_rank's out_off / out_doc as they come, in any order inside a query; every hit_doc <
 * n_docs and no (query, document) pair twice, else FMX_ERR_ARG with the pair in the message; a document may be a hit of
 * several queries.  weights[n_terms]: doubles, all finite, else FMX_ERR_ARG; negative ones allowed; NULL: 1.0 each.
 * params: 1 <= window < 2^32; flags and reserved 0 (FMX_ERR_ARG otherwise); max_per rows of every INTERVAL, 0 = all, as the
 * ranking takes them.
 * DEFINITIONS, for hit h = (query i, document d).  A located row with suffix-array value SA of slot s has its last byte at
 * stream position e = stream_len - 1 - SA (the ranking's rule: a row belongs to the same document in both calls) and its
 * first at f = e - term_len[s] + 1.  It is an OCCURRENCE of (h, s) when s is a slot of query i, e lies in document d and
 * f >= doc_start[d]; a row that fails the last condition is dropped from everything, the counts included (it cannot happen
 * with honest term_len).  tf(h, s) = the occurrences of (h, s): for honest inputs the ranking's tf.  The window STARTS of h
 * are the f of all its occurrences; the window of a start a is [a, a + window).  cover(a) = the slots s of the query that
 * have an occurrence with f >= a and e < a + window.  value(a) = ((0.0 + w(s0)) + w(s1)) + .. over the slots of cover(a) in
 * ascending slot order, IEEE double, one rounding per addition.  The BEST window is the start with the largest value (plain
 * > on doubles), equal values to the smallest a.  It is clipped at b = min(a + window, doc_start[d + 1] - 1): the separator
 * is never part of a passage and no passage reaches into the next document.
 * OUTPUT.  One fmx_passage per hit in the order of hit_doc: raw_off = the raw offset of a in the document; raw_len =
 * raw_off(b - 1) + 1 - raw_off(a), both from the corpus map, where both bytes of an escape pair stand for their raw byte;
 * mask bit j set when the query's j-th slot is in the cover; value; n_occ = the occurrences of the hit.  A hit without
 * occurrences gets all zeros.  out_tf: u32[n_hits * stride], stride = the slot count of the call's longest query, returned
 * through *out_stride; entry h * stride + j = tf of the j-th slot of h's query, the padding 0.  cap counts hits: nothing is
 * written past record cap - 1 or past cap * stride counts; FMX_ERR_OVERFLOW when n_hits > cap (the first cap hits written).
 * LIMITS, each refused with a message that names it: fewer than 2^32 - 1 located rows per call, and bits_for(n_hits) +
 * bits_for(slots of the longest query) + bits_for(stream_len - 1) <= 64 (FMX_ERR_UNSUPPORTED); the handles locate refuses;
 * the shape errors of q_off / set_off / hit_off (FMX_ERR_ARG).  The host form decides every FMX_ERR_ARG that needs no
 * handle before a handle or the device is touched.  fmx_corpus_passages_dev: every array a device pointer (u64 sp / ep /
 * set_off / q_off / hit_off, u32 term_len / hit_doc / out_tf, f64 weights); params and out_stride stay host pointers; it
 * reads d_hit_off[n_queries] back with its first synchronisation and returns FMX_ERR_OVERFLOW the same way.  Both forms
 * ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture, decided before anything is allocated); the need is checked
 * against the free HBM before every allocation and every temporary is freed on every path.  A sort of the hits, locate, one
 * lane per located row to keep those of hit documents, a sort of the kept ones, one wave per hit for the windows; no atomic
 * decides an order or a value: the same input gives the same bytes.
 * fmx_corpus_passages_last: device time (ms) of the calling thread's last call in its four phases, the rows located, the
 * occurrences kept and the hits. */
typedef struct fmx_passage_params {
  uint64_t window;  /* stream bytes, 1 .. 2^32 - 1 */
  uint64_t max_per; /* rows taken of every interval; 0 = all */
  uint32_t flags;   /* 0 */
  uint32_t reserved;
} fmx_passage_params; /* 24 bytes */
typedef struct fmx_passage {
  uint64_t raw_off; /* of the window's first byte in its document */
  uint64_t mask;    /* bit j: the query's j-th slot is covered */
  double value;
  uint32_t raw_len; /* raw bytes of the clipped window */
  uint32_t n_occ;   /* occurrences of the hit */
} fmx_passage;      /* 32 bytes */
int fmx_corpus_passages(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_iv,
                        const uint64_t *set_off, size_t n_terms, const uint32_t *term_len, const uint64_t *q_off,
                        size_t n_queries, const uint64_t *hit_off, const uint32_t *hit_doc, const double *weights,
                        const fmx_passage_params *params, fmx_passage *out, uint32_t *out_tf, size_t cap,
                        uint32_t *out_stride);
int fmx_corpus_passages_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
                            const void *d_set_off, size_t n_terms, const void *d_term_len, const void *d_q_off,
                            size_t n_queries, const void *d_hit_off, const void *d_hit_doc, const void *d_weights,
                            const fmx_passage_params *params, void *d_out, void *d_out_tf, size_t cap,
                            uint32_t *out_stride, void *stream);
int fmx_corpus_passages_last(double *locate_ms, double *filter_ms, double *sort_ms, double *window_ms, uint64_t *rows,
                             uint64_t *occurrences, uint64_t *hits);

/* ---- regex: REParser.re2post (re2/re2.scala:50-185) + ReTree.apply (re2/retree.scala:156-370).
 * Bytes of `re` are Latin-1 characters.  FMX_ERR_SYNTAX / FMX_ERR_MATCH mirror the reference's
 * "re2post syntax" exception and scala.MatchError. */
int fmx_regex_compile(const char *re, int line_only, fmx_regex **out);
int fmx_regex_free(fmx_regex *re);
/* The same for k regexes at once, compiled on all the host cores the process may use (its affinity mask capped by the
 * cgroup CPU quota; fmx_config_set("threads", "N") overrides): out[i] = the handle of res[i] or NULL, status[i]
 * (optional) = FMX_OK / FMX_ERR_SYNTAX / FMX_ERR_MATCH exactly as fmx_regex_compile(res[i]) returns.  The call itself
 * returns FMX_OK when it ran (whatever the regexes' own statuses; fmx_last_error() then describes the first one that
 * failed), FMX_ERR_ARG / FMX_ERR_NOMEM otherwise.  The reference compiles one regex per REParser.re2post + ReTree
 * call (re2/re2.scala:50-185, re2/retree.scala:156-423); a batch of 100 k is what config C4 hands over at once.
 * fmx_regex_free_batch frees k handles (NULL entries allowed). */
int fmx_regex_compile_batch(const char *const *res, size_t k, int line_only, fmx_regex **out, int *status);
int fmx_regex_free_batch(fmx_regex *const *res, size_t k);
/* Flat Glushkov tables (what ReTree._matchSA touches): per CharNode its byte, `num`
 * (retree.scala:393-423), isLast (:40-50), and `follows` (:14-38) as a CSR list that keeps the
 * reference's order and multiplicity; `firsts` = root.firsts.  Any output pointer may be NULL;
 * sizes come back through the n_* pointers. */
int fmx_regex_tables(const fmx_regex *re, uint32_t *n_states, uint8_t *st_c, int32_t *st_num, uint8_t *st_last,
                     int32_t *fol_off /* n_states+1 */, uint32_t *n_follows, int32_t *fol, uint32_t *n_firsts,
                     int32_t *firsts);
/* re2poststr, re2/re2.scala:187 (UTF-8). */
int fmx_regex_post_string(const char *re, int line_only, char *out, size_t cap);

enum {
  FMX_MATCH_FRONTIER = 0,   /* breadth-first over the whole batch: every match, the throughput path */
  FMX_MATCH_REFERENCE = 1   /* the reference's own pop order and limits, one regex per lane group */
};

/* ---- the reference's two other SA-interval engines, served by the same frontier kernel:
 * fmx_nfa_compile : REParser.createNFA (re2/re2.scala:264-334) for REParser.matchSA (:568-693): Thompson
 *                   NFA, epsilon closures folded into the tables.  `src` is a regex for re2post or, with
 *                   src_is_postfix, a postfix string for post2re (:188-205) as the reference's tests use.
 *                   FMX_ERR_MATCH where the reference throws scala.MatchError ([..] sets; a regex that
 *                   matches the empty string).  matchSA's maxLength is fmx_limits.max_steps.
 * fmx_dfa_compile : DFA.compileBuckets + DFA.matchSA (dfa.scala:190-213,231-289) over a caller-built
 *                   transition table moves[nstates][nchars] (-1 = none), finish[nstates]: as in the
 *                   reference only single-character actions expand (runs of equal targets are "buckets",
 *                   which StatePoint.expand ignores, :247-251).
 * Both return an fmx_regex handle for fmx_regex_match_batch / fmx_regex_batch_* in frontier mode: every match.
 * The reference's cuts for these two engines -- REParser.matchSA's maxIterations (re2.scala:612) and DFA.matchSA's
 * 500 iterations (dfa.scala:268) -- stop the search after a number of POPS, and the pop order is not defined by the
 * reference's source: the NFA engine seeds its queue from an immutable Set of state objects hashed by identity and
 * takes equal-length elements in heap-layout order, the DFA engine takes `head` of an immutable HashSet.  Two
 * orders the source allows return different results once a cut binds (and the same multiset while it does not):
 * tests/test_oracle_engines.py::test_order_dependent_cuts_are_not_reproducible_without_the_jvm.  So there is no
 * reference-order mode for them; FMX_MATCH_REFERENCE exists for ReTree, whose order IS defined by its source
 * (CharNode.num and Scala's binary heap). */
int fmx_nfa_compile(const char *src, int line_only, int src_is_postfix, fmx_regex **out);
int fmx_dfa_compile(const int32_t *moves, uint32_t nstates, uint32_t nchars, const uint8_t *finish,
                    fmx_regex **out);

typedef struct fmx_limits {
  /* mode = FMX_MATCH_FRONTIER.  The frontier kernel steps every element of every regex's frontier (in the order
   * that suits the device: elements are independent), so its results equal the reference's (as a multiset) whenever
   * the reference's limits do not bind:
   * max_steps   = longest match explored (levels); 0 = default 4096.  When the frontier is still alive
   *               there, the call returns FMX_TRUNCATED with every match of length <= max_steps.  (On
   *               the BWT of a real text a frontier always dies -- no match is longer than the text --
   *               but on a synthetic "BWT" that is just a random string, LF has short cycles and x* can
   *               run forever.)
   * max_frontier= capacity of the device work queue in elements, 0 = default (1<<22): what the waves cannot
   *               hold in their own pools is queued in HBM (64 slices of two buffers each, about
   *               max_frontier / 50 entries per buffer); FMX_ERR_OVERFLOW when a buffer fills up.
   * Results and per-regex counts are written by the device itself when `out` / `per_regex_count` are
   * page-locked memory (fmx_host_alloc); pageable buffers are filled by a copy after the search.
   * mode = FMX_MATCH_REFERENCE.  ReTree._matchSA exactly (re2/retree.scala:618-653): the priority queue
   * of Scala 2.10 replayed per regex, loop while queue non-empty && queue.length < max_branching &&
   * (max_iterations == 0 || i < max_iterations), i from 1.  Results come back per regex in the
   * reference's list order (newest first).  ReTree.matchSA's defaults are 1024 / 1000 (:570). */
  uint32_t max_steps;
  uint32_t mode;
  uint64_t max_frontier;
  uint32_t max_branching;
  uint32_t max_iterations;
} fmx_limits;

typedef struct fmx_result {   /* SAResult(sa,len,sp,ep), re2/re2.scala:9-19, + which regex */
  uint32_t regex;
  uint32_t len;
  uint64_t sp;
  uint64_t ep;
} fmx_result;

/* ReTree.matchSA over a batch of compiled regexes (re2/retree.scala:570-653): frontier items
 * (regex, CharNode, len, sp, ep) start at root.firsts x (0, 0, n); each is stepped with
 * getPrevRange; isLast states emit a result, the others push their follows.  In frontier mode results
 * are written sorted by (regex, len, sp, ep); in reference mode per regex in the reference's own
 * list order.  per_regex_count (optional, k entries) = results per
 * regex.  FMX_ERR_OVERFLOW if out (cap entries) or the work queue was too small: *n_out then
 * holds the number of results found so far / needed.  FMX_TRUNCATED: see fmx_limits.max_steps. */
int fmx_regex_match_batch(const fmx_index *idx, fmx_regex *const *res, size_t k, const fmx_limits *lim,
                          fmx_result *out, size_t cap, size_t *n_out, uint32_t *per_regex_count);

/* The same in two stages for serving: make a batch of compiled regexes resident on idx's device
 * once (concatenated tables + the level-0 frontier), then match it any number of times, in either mode
 * (FMX_MATCH_REFERENCE needs a batch of fmx_regex_compile handles only).  One match at a time per batch. */
int fmx_regex_batch_create(const fmx_index *idx, fmx_regex *const *res, size_t k, fmx_regex_batch **out);
int fmx_regex_batch_free(fmx_regex_batch *batch);
/* Sizes of a resident batch: regexes, CharNode states, follow entries, start elements (any pointer may be NULL). */
int fmx_regex_batch_info(const fmx_regex_batch *batch, uint64_t *n_regexes, uint64_t *n_states, uint64_t *n_follows,
                         uint64_t *n_firsts);
int fmx_regex_batch_match(const fmx_index *idx, fmx_regex_batch *batch, const fmx_limits *lim, fmx_result *out,
                          size_t cap, size_t *n_out, uint32_t *per_regex_count);
/* The same with the results left in HBM (frontier mode): d_out = device memory for cap fmx_result records,
 * d_per_regex_count = device memory for k counts or NULL; *n_out = the number of results.  The device-pointer
 * form of the regex path, like fmx_search_batch_dev for literals: what a caller that post-processes on the device
 * (or gathers over RCCL, findex_amd/distributed.py) uses -- nothing crosses the host link but the count.  The call
 * is synchronous (the search needs the host between launch chains). */
int fmx_regex_batch_match_dev(const fmx_index *idx, fmx_regex_batch *batch, const fmx_limits *lim, void *d_out,
                              size_t cap, size_t *n_out, void *d_per_regex_count);

/* ---- occurrences: where the strings of (group, len, sp, ep) intervals stand in the text, reduced and in CSR order.  Beyond
 * the reference, whose SAResult can only print one row's string.  DESIGN.md 20.
 * s, n and SA are as for locate; the text has n - 1 bytes.  The input is k records fmx_result {regex, len, sp, ep} with
 * `regex` read as a GROUP number < n_groups: the results a regex batch leaves in HBM (fmx_regex_batch_match_dev) have that form
 * already, edit, mismatch and exact hits after a repack.
 * The OCCURRENCES OF ONE RECORD: its first min(ep - sp, max_per) rows r (max_per == 0: all) give (group, pos, len) with
 * pos = n - 1 - len - SA[r] -- the string begins at text offset pos and is len bytes long (locate_text's arithmetic with the
 * record's own length).  A record with ep <= sp or len == 0 has none; a row with SA[r] + len > n - 1 is dropped (no real
 * result has one).
 * WITH A CORPUS (corpus != NULL, idx the index of its stream; n - 1 != stream length is FMX_ERR_ARG) the document is d =
 * doc(pos) and an occurrence is kept only if pos + len <= doc_start[d + 1] - 1: it lies inside one document and does not touch
 * its separator.  That happens BEFORE the reduction, so a shorter match at the same start that fits its file can still win.  A
 * kept occurrence carries doc, raw_off = the raw offset of pos and raw_len = the raw offset of (pos + len - 1) + 1 - raw_off,
 * both by fmx_corpus_map's rules.  Without a corpus doc = UINT32_MAX, raw_off = pos, raw_len = len.  One known limit, as
 * elsewhere in the corpus code: the stream is compared in its escaped form, so an end may fall inside an escape pair; its raw
 * offset is then that of the byte the pair stands for.
 * MODES (fmx_occ_opts.mode), per group:
 *   FMX_OCC_ALL      every distinct (pos, len): records that repeat give occurrences that repeat, and those are merged (the
 *                    frontier keeps multiplicity);
 *   FMX_OCC_LONGEST  for every pos the occurrence with the largest len;
 *   FMX_OCC_DISJOINT the LONGEST set by ascending pos: its first element, and after an element (pos, len) the first one with
 *                    pos' >= pos + len -- the leftmost non-overlapping reading, what finditer or grep -o show.
 * OUTPUT is CSR over groups: group g's records are out[out_off[g] .. out_off[g + 1]), ascending by (pos, len), and
 * out_off[n_groups] == *n_out.  The same input gives the same bytes on every run.  opts == NULL: FMX_OCC_ALL, no limit.
 * Capacity: more than cap occurrences -> FMX_ERR_OVERFLOW with the EXACT total in *n_out (out and, in the host form, out_off
 * then unspecified); nothing is written past out[cap - 1]; cap == 0 with out == NULL is the counting call.
 * FMX_ERR_ARG, decided before the device is touched: a null handle, out_off or n_out; mode > 2; reserved != 0; k > 2^26;
 * n_groups == 0 or > 2^26; cap >= 2^32; a record with group >= n_groups, len > FMX_OCC_MAX_LEN or sp > ep (host form).  The
 * device form cannot see the records: its kernels read ep > n as n, skip a bad record and raise a flag, and the call returns
 * FMX_ERR_ARG after the launch with nothing reported (outputs and *n_out untouched).  No record value leads outside the index
 * or the outputs.
 * Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture, decided before anything is allocated, the capture
 * left valid) and free every temporary on every path.  They need the locate samples and build them when absent, with locate's
 * refusals: fmx_open_block handles FMX_ERR_UNSUPPORTED, an index that is not the BWT of one text FMX_ERR_FORMAT.  Limit:
 * n >= 2^32 is FMX_ERR_UNSUPPORTED (positions are 32 bits in the sort key; a corpus stream has that limit anyway).  The rows to
 * locate, R = the sum of min(ep - sp, max_per), must be < 2^32: FMX_ERR_OVERFLOW otherwise, with a message that says to lower
 * max_per -- known after the scan and before anything row-sized is allocated.  The need -- 36 bytes per row (the SA values, two
 * key and two value buffers of the radix sort, the flags), 24 more with FMX_OCC_DISJOINT (the compacted set, two jump buffers,
 * the marks), 4 more when group, pos and len do not fit one 64-bit key, plus 24 bytes per record, the sort's histograms and
 * the scans' block totals -- is checked against the free HBM first: FMX_ERR_NOMEM with the need in the message.
 * No derived search table and no count of patterns seen changes; the launches are added to the handle's.
 * fmx_occurrences_dev : d_rec (24-byte records), d_out_off (u64[n_groups + 1]) and d_out (32-byte records) in device memory;
 *                       n_out stays a host pointer.
 * fmx_occurrences_last: the calling thread's last call: device time (ms) of the locate walks, of the keys and the sort, of the
 *                       selection, of the compaction, and the rows located; any pointer may be NULL. */
#define FMX_OCC_ALL 0u
#define FMX_OCC_LONGEST 1u
#define FMX_OCC_DISJOINT 2u
#define FMX_OCC_MAX_LEN 65535
typedef struct fmx_occ_opts {
  uint32_t mode;     /* FMX_OCC_ALL | FMX_OCC_LONGEST | FMX_OCC_DISJOINT */
  uint32_t reserved; /* must be 0 */
  uint64_t max_per;  /* rows taken of every record; 0 = all */
} fmx_occ_opts;      /* 16 bytes */
typedef struct fmx_occurrence {
  uint32_t group;
  uint32_t len;
  uint64_t pos;
  uint32_t doc;     /* UINT32_MAX without a corpus */
  uint32_t raw_len;
  uint64_t raw_off;
} fmx_occurrence; /* 32 bytes */
int fmx_occurrences(const fmx_index *idx, const fmx_corpus *corpus_or_null, const fmx_result *rec, size_t k, size_t n_groups,
                    const fmx_occ_opts *opts, uint64_t *out_off /* n_groups + 1 */, fmx_occurrence *out, size_t cap,
                    size_t *n_out);
int fmx_occurrences_dev(const fmx_index *idx, const fmx_corpus *corpus_or_null, const void *d_rec, size_t k, size_t n_groups,
                        const fmx_occ_opts *opts, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream);
int fmx_occurrences_last(double *locate_ms, double *sort_ms, double *select_ms, double *compact_ms, uint64_t *rows);

/* ---- context: the rows of intervals whose NEIGHBOURING TEXT BYTES are in a class -- whole-word matching.  Beyond the
 * reference.  DESIGN.md 27.
 * s = reverse(text) + sentinel, n and SA as for locate.  A row r of the interval of a string of s of length len is the
 * occurrence of the (reversed) string at text offset pos = n - 1 - len - SA[r].  THE BYTE BEHIND that occurrence, text[pos +
 * len], is the BWT byte of row r; the occurrence that ends where the text ends is row eof, whose byte reads as 0 (no real
 * symbol is 0).  THE BYTE IN FRONT is matched by a search: the rows of a.X (a in front of X in the text) are rows of X.
 * The occurrence at text offset 0, if there is one, is the first row of X's interval, and it is there iff that row is
 * LF^len(0).  The text is not needed and is not in HBM.
 *
 * fmx_context_filter: a per-record map.  INPUT: k records fmx_result {group, len, sp, ep}; mode, k bytes or NULL (all 0):
 * bits 0..6 = lead, the bytes of the record's string that are left context (the front bytes of the text string), already
 * matched by whoever made the record; bit 7 = FMX_CTX_START; right[4], a 256-bit set: bit c (word c / 64, bit c % 64) set <=>
 * byte c may follow the occurrence, bit 0 <=> the text may end there.
 * CANDIDATE ROWS of record j: without FMX_CTX_START every r in [sp, min(ep, n)); with it (lead must be 0, FMX_ERR_ARG
 * otherwise) only r = sp, and only if sp < ep and sp == LF^len(0): the occurrence that begins at text offset 0.
 * A candidate PASSES iff bit BWT[r] of right is set (BWT[eof] read as 0).  OUTPUT for record j: the maximal runs of passing
 * rows inside the record as fmx_result {group, len - lead, run_sp, run_ep}, ascending; a record with len <= lead or sp >= ep
 * yields nothing.  out_off[k + 1] is CSR over the INPUT RECORDS, out_off[k] == *n_out.  The runs are rows of the input
 * record: fmx_locate_intervals, fmx_occurrences and the ranking work on them unchanged.  The same input gives the same bytes;
 * no atomic decides an order.
 * Capacity as fmx_occurrences: more than cap runs -> FMX_ERR_OVERFLOW with the EXACT total in *n_out (out and, in the host
 * form, out_off then unspecified); nothing is written past out[cap - 1]; cap == 0 with out == NULL is the counting call.
 * FMX_ERR_ARG, decided before the device is touched: a null handle, right, out_off or n_out; k > 2^26; a record with len >
 * FMX_OCC_MAX_LEN or sp > ep, FMX_CTX_START with lead != 0 (host form).  The device form cannot see the records: its kernels
 * skip a bad record and raise a flag, and the call returns FMX_ERR_ARG after the launch with nothing reported.  No record
 * value leads outside the index or the outputs.  fmx_open_block handles: FMX_ERR_UNSUPPORTED.
 * Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture, decided before anything is allocated, the capture
 * left valid), check the need against the free HBM before every allocation (FMX_ERR_NOMEM) and free every temporary on every
 * path.  Rows are 64-bit and the call sets no limit on n; the rows are cut into chunks of 1024 and the run slots numbered in 32
 * bits: 2^32 - 1 chunks or runs and more in ONE call are FMX_ERR_OVERFLOW (the runs with their exact total).  The chain LF^j(0)
 * is walked by one lane group, as far as the longest FMX_CTX_START record of the call and never past j = n - 1; it is not kept.
 * No derived table and no count of patterns changes; the launches are added to the handle's.
 * fmx_context_filter_dev: d_rec (24-byte records), d_mode (bytes or NULL), d_out_off (u64[k + 1]), d_out (24-byte records) in
 *                       device memory; right and n_out stay host pointers.
 * fmx_context_last    : the calling thread's last call: device time (ms) of the search (fmx_search_context_batch only), of the
 *                       chain, and of ranges + count + scans + emit; the rows tested and the runs found.
 *
 * fmx_search_context_batch: k literal patterns (given as fmx_search_batch takes them: strings of s, the text string reversed;
 * non-empty, at most FMX_OCC_MAX_LEN - 1 bytes, no byte 0, FMX_ERR_ARG otherwise) with a class on each side.  opts->left /
 * ->right are 256-bit sets as above, in TEXT terms: left bit a <=> byte a may stand in front of the occurrence, bit 0 <=> the
 * text may begin there; flags and reserved must be 0.  RESULT for pattern i of m_i bytes: the rows of its interval whose left
 * and right neighbours are in the classes, as disjoint ranges {i, m_i, sp, ep} in ascending sp (two ranges may be adjacent);
 * out_off[k + 1] is CSR over the PATTERNS.  Capacity, errors and the device form's flag are the filter's.
 * How: pattern i is expanded on the device into itself and a.P_i for every a >= 1 of left whose count in the index is not 0;
 * ONE fmx_search_batch_dev over the expansion -- the derived search tables and the handle's pattern counters behave as for
 * any search of that many patterns, k * (1 + such bytes), which must not exceed 2^26 --; per pattern the plain interval with
 * FMX_CTX_START (only if bit 0 of left is set), then the a intervals with lead = 1 in ascending a, which is ascending sp; then
 * the filter above. */
#define FMX_CTX_START 0x80u
typedef struct fmx_context_opts {
  uint64_t left[4];
  uint64_t right[4];
  uint32_t flags;    /* must be 0 */
  uint32_t reserved; /* must be 0 */
} fmx_context_opts;  /* 72 bytes */
int fmx_context_filter(const fmx_index *idx, const fmx_result *rec, const uint8_t *mode_or_null, size_t k, const uint64_t *right,
                       uint64_t *out_off /* k + 1 */, fmx_result *out, size_t cap, size_t *n_out);
int fmx_context_filter_dev(const fmx_index *idx, const void *d_rec, const void *d_mode_or_null, size_t k, const uint64_t *right,
                           void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream);
int fmx_context_last(double *search_ms, double *chain_ms, double *filter_ms, uint64_t *rows, uint64_t *runs);
int fmx_search_context_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k,
                             const fmx_context_opts *opts, uint64_t *out_off /* k + 1 */, fmx_result *out, size_t cap,
                             size_t *n_out);
int fmx_search_context_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k,
                                 const fmx_context_opts *opts, void *d_out_off, void *d_out, size_t cap, size_t *n_out,
                                 void *stream);

/* ---- case folding: literal search under a byte map.  Beyond the reference.  DESIGN.md 28.
 * A FOLD MAP is uint8_t fold[256]: fold[c] is the representative of c's class, and two bytes are equivalent iff their fold
 * values are equal.  A map is VALID when fold[fold[c]] == fold[c] for every c, fold[0] == 0 and no other byte folds to 0, and
 * no class has more than FMX_FOLD_MAX_CLASS members; flags and reserved must be 0.  Anything else is FMX_ERR_ARG before the
 * device is touched.  opts == NULL means ASCII case folding: A..Z fold to a..z, every other byte to itself.
 * For a pattern P of m bytes (given as fmx_search_batch takes it: a string of s, matched last byte first) a HIT is a byte
 * string Q of m bytes with fold[Q[j]] == fold[P[j]] at every j for which the reference's search(Q) loop (findex.scala:15-31)
 * ends with sp < ep.  It is reported as fmx_result {group = pattern, len = m, sp, ep} with (sp, ep) exactly what
 * fmx_search_batch returns for Q.
 *  - The definition rests on cf / occ alone, so it holds for any handle, synthetic BWTs included.
 *  - Distinct Q of one length have disjoint intervals (LF is a permutation).
 *  - A position whose class is a singleton in the map is a plain step of the exact search with all its quirks, byte 0
 *    included (a class of two or more never holds byte 0, so the EOF row is never reached by folding).
 *  - With the identity map the hits are those of fmx_search_batch -- one for a pattern it finds, none for one it does not --
 *    and the backward steps made are its steps.
 *  - An empty pattern has the one hit (0, n).
 * Only variants that occur are followed: the search branches on the index and dies where the text does; a class member that
 * is absent from the index costs nothing.
 * Results are in CSR form over the patterns: out_off[k + 1], 24-byte records, ascending sp within a pattern, out_off[k] ==
 * *n_out.  The same input gives the same bytes on every run; no atomic decides an order.
 * Capacity, the counting call (cap == 0, out == NULL), FMX_ERR_OVERFLOW with the EXACT total in *n_out, k <= 2^26 and cap <
 * 2^32 are those of fmx_search_approx_batch, as is the order of the refusals (the null handle last).
 * FMX_ERR_UNSUPPORTED: fmx_open_block handles and indexes of 2^38 rows or more.
 * A pattern has at most FMX_FOLD_MAX_LEN bytes: the host form refuses a longer one (FMX_ERR_ARG, before the device is
 * touched); the device form's kernel skips it and raises a flag, and the call returns FMX_ERR_ARG after the launch with no
 * hits written and *n_out untouched.
 * Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture, decided first, the capture left valid) and free
 * every temporary on every path: 24 cap bytes of staging, 24 bytes per hit of sort keys and values, the counters, and a stack
 * of (FMX_FOLD_MAX_CLASS - 1) entries of 24 bytes per byte of the longest pattern -- the device form, which does not know
 * the lengths, takes FMX_FOLD_MAX_LEN -- per resident wave, checked against the free device memory first (FMX_ERR_NOMEM with the need in the message).  They use the rank dictionary only, build no derived table and do
 * not count as patterns seen; their steps are added to the handle's counters (rank_queries, backward_steps, search_requests)
 * and the call to launches.
 * fmx_search_context_fold_batch[_dev]: fmx_search_context_batch with this search in the place of fmx_search_batch_dev.  The
 * expansion is the same (P_i, and a.P_i for every occurring a >= 1 of left); the step with a is EXACT even if the map folds
 * a; every hit is a record of the ORIGINAL pattern, plain variants under FMX_CTX_START (dropped unless bit 0 of left is set),
 * a variants with lead = 1, ascending sp and on equal sp the FMX_CTX_START record first; then the filter, unchanged, and its
 * output re-cut to CSR over the patterns.  Patterns are non-empty, at most FMX_FOLD_MAX_LEN - 1 bytes, without byte 0.  The
 * variants that occur are the filter's records and its limit is theirs: more than 2^26 in one call are FMX_ERR_ARG.
 * fmx_fold_last: the calling thread's last call: device time (ms) of the search kernel and of the ordering step, backward
 * steps executed (the ones that come back empty included), rank-dictionary requests issued; any pointer may be NULL. */
#define FMX_FOLD_MAX_CLASS 8
#define FMX_FOLD_MAX_LEN 255
typedef struct fmx_fold_opts {
  uint8_t fold[256];
  uint32_t flags;    /* must be 0 */
  uint32_t reserved; /* must be 0 */
} fmx_fold_opts;     /* 264 bytes */
int fmx_search_fold_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_fold_opts *opts,
                          uint64_t *out_off /* k + 1 */, fmx_result *out, size_t cap, size_t *n_out);
int fmx_search_fold_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_fold_opts *opts,
                              void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream);
int fmx_search_context_fold_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k,
                                  const fmx_context_opts *ctx, const fmx_fold_opts *fold, uint64_t *out_off /* k + 1 */,
                                  fmx_result *out, size_t cap, size_t *n_out);
int fmx_search_context_fold_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k,
                                      const fmx_context_opts *ctx, const fmx_fold_opts *fold, void *d_out_off, void *d_out,
                                      size_t cap, size_t *n_out, void *stream);
int fmx_fold_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests);

/* ---- string classes: literal search where a pattern position stands for a set of byte strings of different lengths (UTF-8
 * case folding: {K, k, U+212A}, {S, s, U+017F}).  Beyond the reference.  DESIGN.md 30.
 * A CLASS TABLE (fmx_class_table, host memory in both forms of the call) holds n_classes classes: the members of class c are
 * members cls_off[c] .. cls_off[c + 1] - 1, and member j is the bytes mem_bytes[mem_off[j] .. mem_off[j + 1]).  cls_off[0] ==
 * mem_off[0] == 0.  The table is VALID when every member has 1 .. FMX_CLASS_MAX_MEMBER_LEN bytes and no byte 0, a class has
 * 1 .. FMX_CLASS_MAX_MEMBERS members, the members of a class are distinct and none is a prefix of another, n_classes <=
 * FMX_CLASS_MAX_CLASSES, and flags and reserved are 0.  Anything else is FMX_ERR_ARG before the device is touched, with the
 * offending class in the message.  tab == NULL is the empty table (every element must be a literal then).
 * A PATTERN is a sequence of uint16_t ELEMENTS, pattern i being el[el_off[i] .. el_off[i + 1]): an element < 256 is that
 * literal byte, an element >= 256 is class (element - 256), which must be in the table (the host form refuses another one
 * before the device is touched; the device form's kernel skips the pattern and the call returns FMX_ERR_ARG after the launch).
 * Patterns and members are strings of s, as fmx_search_batch takes them: elements are matched last first, and a member's
 * bytes last first.
 * A HIT of pattern P of e elements is a byte string Q = m_1 m_2 .. m_e, m_j being P's j-th literal byte or a member of P's j-th
 * class, for which the reference's search(Q) loop (findex.scala:15-31) ends with sp < ep.  It is reported as fmx_result
 * {group = pattern, len = the bytes of Q, sp, ep} with (sp, ep) exactly what fmx_search_batch returns for Q.
 *  - Distinct hits of one pattern have disjoint intervals: two spellings first differ inside two members of which neither is
 *    a prefix of the other, so neither spelling is a prefix of the other and no suffix of s begins with both.  Hence
 *    "ascending sp" is a total order and the same input gives the same bytes on every run.  (Members are strings of s: for
 *    strings of the text, which a caller reverses, the rule reads "none is a suffix of another".  The UTF-8 encodings of
 *    distinct code points satisfy both.)
 *  - A literal element is a plain step of the exact search with all its quirks, byte 0 included.
 *  - A pattern of literals only has fmx_search_batch's hit, and the call makes exactly its steps.
 *  - A table made of a valid fold map (every class its single-byte members) gives fmx_search_fold_batch's offsets and records.
 *  - An empty pattern has the one hit (0, n) with len 0.
 * Only spellings that occur are followed; a member's bytes are stepped one after the other and the member dies at its first
 * empty interval.  On a node of one row only members whose LAST byte (the first one stepped) equals BWT'[sp] are stepped (none
 * on the EOF row).
 * A pattern has at most FMX_CLASS_MAX_ELEMS elements: the host form refuses a longer one, the device form's kernel skips it
 * and raises a flag, and the call returns FMX_ERR_ARG after the launch with no hits written and *n_out untouched.
 * Results, capacity, the counting call, FMX_ERR_OVERFLOW with the EXACT total, k <= 2^26, cap < 2^32, FMX_ERR_UNSUPPORTED for
 * fmx_open_block handles and n >= 2^38, the refusal under a stream capture (decided first), the order of the refusals and the
 * counters are fmx_search_fold_batch's.  Temporaries: 24 cap bytes of staging, 24 bytes per hit of sort keys and values, the
 * counters, 128 bytes per class, and per resident wave a stack of (largest class of the table - 1) entries of 24 bytes per
 * element of the longest pattern (the device form: FMX_CLASS_MAX_ELEMS), checked against the free device memory first
 * (FMX_ERR_NOMEM with the need in the message).  The rank dictionary only; no derived table is built or used.
 * Of cls_off only [cls_off[c], cls_off[c + 1]) is read per class and of mem_off the entries those name: the arrays' real sizes
 * are the caller's word, and a gap or an overlap between two classes is taken as it stands.  The sort space of the ordering
 * step is allocated once the hits are counted (FMX_ERR_NOMEM from that allocation).
 * fmx_search_context_classes_batch[_dev]: fmx_search_context_fold_batch with this search in the place of the fold search.  The
 * expansion P_i, a.P_i appends a as a LITERAL element; the lead bit, the filter and the re-cut to CSR are the same code.
 * Patterns are non-empty, at most FMX_CLASS_MAX_ELEMS - 1 elements, without the literal 0; a hit's len is the bytes of its
 * spelling, so a term's runs may differ in len.
 * fmx_classes_last: as fmx_fold_last, of the calling thread's last class search. */
#define FMX_CLASS_MAX_MEMBER_LEN 4
#define FMX_CLASS_MAX_MEMBERS 16
#define FMX_CLASS_MAX_ELEMS 255
#define FMX_CLASS_MAX_CLASSES 65280
typedef struct fmx_class_table {
  const uint64_t *cls_off;  /* n_classes + 1 */
  const uint64_t *mem_off;  /* cls_off[n_classes] + 1 */
  const uint8_t *mem_bytes; /* mem_off[cls_off[n_classes]] */
  uint64_t n_classes;
  uint32_t flags;    /* must be 0 */
  uint32_t reserved; /* must be 0 */
} fmx_class_table;   /* 40 bytes */
int fmx_search_classes_batch(const fmx_index *idx, const uint16_t *el, const uint64_t *el_off, size_t k,
                             const fmx_class_table *tab, uint64_t *out_off /* k + 1 */, fmx_result *out, size_t cap,
                             size_t *n_out);
int fmx_search_classes_batch_dev(const fmx_index *idx, const void *d_el, const void *d_el_off, size_t k,
                                 const fmx_class_table *tab, void *d_out_off, void *d_out, size_t cap, size_t *n_out,
                                 void *stream);
int fmx_search_context_classes_batch(const fmx_index *idx, const uint16_t *el, const uint64_t *el_off, size_t k,
                                     const fmx_context_opts *ctx, const fmx_class_table *tab, uint64_t *out_off /* k + 1 */,
                                     fmx_result *out, size_t cap, size_t *n_out);
int fmx_search_context_classes_batch_dev(const fmx_index *idx, const void *d_el, const void *d_el_off, size_t k,
                                         const fmx_context_opts *ctx, const fmx_class_table *tab, void *d_out_off, void *d_out,
                                         size_t cap, size_t *n_out, void *stream);
int fmx_classes_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests);

/* ---- lines: the map from a text position to its line, and occurrences reduced to the distinct lines that hold them (grep -n
 * over an index).  Beyond the reference.  DESIGN.md 23.
 * t is the indexed text of n - 1 bytes; positions are the `pos` of fmx_occurrence, so the occurrence of a one-byte string at
 * row r stands at n - 2 - SA[r].  A BREAK SET B holds 1 .. 4 distinct byte values (none of them 0); brk[0 .. n_brk) are the
 * positions p with t[p] in B, ascending.
 *   line(p)  = #{ j : brk[j] < p }: a 0-based GLOBAL line index; a break byte belongs to the line it ends.
 *   start(L) = 0 for L == 0, else brk[L - 1] + 1.
 *   end(L)   = brk[L] for L < n_brk, else n - 1: exclusive, the break byte is not part of the line.
 * There are n_brk + 1 lines; the last may be empty.  B is {10} for a plain text and {10, 1} for a corpus stream: byte 1 is the
 * separator behind every document (the corpus section above), so no line spans two files, and the 1-based line number of p in
 * its document d is line(p) - line(doc_start[d]) + 1.  Escape pairs never contain a break byte, so the raw offsets of starts
 * and ends follow fmx_corpus_map's rules unchanged.
 * THE TABLE is derived from the index alone, like the locate samples: the breaks are the rows of the buckets [cf(c), cf(c + 1))
 * of the c in B, located, turned into positions and sorted (no atomics: the same input gives the same bytes on every run).  It
 * holds brk[] as u32 and a directory dir[i] = #{ j : brk[j] < i 2^S }, i = 0 .. ((n - 1) >> S) + 1, as u32; S is the key
 * "lines_shift", 4 .. 16, default 6 (fmx_config_set: the default; fmx_index_config_set: one handle's).  A lookup reads
 * dir[p >> S] and dir[(p >> S) + 1] and takes a lower bound among at most 2^S consecutive entries of brk.  Size: 4 n_brk +
 * 4 (n >> S) bytes, outside the table budget.  The build needs the locate samples and builds them when absent, with locate's
 * refusals (fmx_open_block handles FMX_ERR_UNSUPPORTED, an index that is not the BWT of one text FMX_ERR_FORMAT); it allocates
 * and synchronises (FMX_ERR_HIP under a stream capture, decided before anything is allocated, the capture left valid), checks
 * its need -- the SA values, two key and two value buffers, the histograms and the table itself -- against the free HBM first
 * (FMX_ERR_NOMEM with the need in the message) and frees every temporary on every path.  Limit: n >= 2^32 is
 * FMX_ERR_UNSUPPORTED (fmx_occurrences and the corpus stream have that limit anyway); positions and line indices are uint64_t
 * in every signature so that lifting it changes no ABI.
 * A call that finds no table builds one: with the set {10} without a corpus and {10, 1} with one.  A table whose set lacks
 * byte 1, combined with a corpus, is FMX_ERR_ARG.
 * fmx_lines_prepare   : builds the table for `breaks` (NULL / 0: {10}); an equal set (in any order): nothing to do; another
 *                       set: the table is rebuilt.  FMX_ERR_ARG before the device is touched: a null handle, n_breaks > 4, a
 *                       repeated break byte, break byte 0.
 * fmx_lines_info      : the breaks found, the set, S, the table's bytes and its build time (0 breaks / bytes / ms and the
 *                       default set while there is none); any pointer may be NULL.
 * fmx_lines_batch     : for k positions line, start(line) and end(line); any output may be NULL; a position p >= n - 1 gives
 *                       UINT64_MAX in all three.
 * fmx_line_spans      : for k global line indices start and end; an index L > n_brk gives UINT64_MAX in both.
 * The _dev forms of both take device pointers (u64 throughout) and, with a table present, ONLY ENQUEUE on `stream`; without
 * one they build it first, and under a stream capture return FMX_ERR_HIP before anything is allocated.  k == 0 does nothing
 * in the _dev forms: no table is built for it.
 * fmx_occurrence_lines: reduces occurrence records to the distinct lines their `pos` fall on.  The input is what
 *                       fmx_occurrences leaves: CSR offsets occ_off[n_groups + 1] over n_occ = occ_off[n_groups] records, the
 *                       records of a group ascending by (pos, len).  OUTPUT is CSR over the same groups: one fmx_line_hit per
 *                       distinct line of a group, ascending by line, out_off[n_groups] == *n_out.  A match that contains a
 *                       break byte counts on the line it BEGINS on.  With a corpus `doc` and raw_off are fmx_corpus_map's of
 *                       the line's start (the record's own `doc` and `group` fields are not read: a line begins in the
 *                       document its hits lie in, and the CSR offsets say the group), raw_len is the raw offset of the end
 *                       less raw_off, line_no is relative to doc_start[doc];
 *                       without one doc = UINT32_MAX, line_no = line + 1, raw_off = start, raw_len = len.
 *                       Capacity as fmx_occurrences: more than cap lines -> FMX_ERR_OVERFLOW with the EXACT total in *n_out,
 *                       nothing written past out[cap - 1]; cap == 0 with out == NULL is the counting call.
 *                       FMX_ERR_ARG, decided before the device is touched: a null handle, occ_off / d_occ_off, out_off or
 *                       n_out; records missing while there are some; n_groups == 0 or > 2^26; n_occ > 2^26; cap >= 2^32; in
 *                       the host form occ_off not non-decreasing or a pos >= n - 1; a corpus whose stream length != n - 1.
 *                       The device form cannot see the records: it reads a pos >= n - 1 as "no line", skips the record and
 *                       raises a flag, and the call returns FMX_ERR_ARG after the launch with nothing reported.  No record
 *                       value leads outside the table or the outputs.  Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under
 *                       a stream capture) and free every temporary on every path; the need (16 bytes per record and the
 *                       scan's block totals) is checked against the free HBM first.
 * fmx_lines_last      : the calling thread's last build (device ms of the locate walks, of the keys, the sort and the
 *                       directory) and its last lookup and occurrence-lines call (ms of the lookups, of the compaction); any
 *                       pointer may be NULL. */
typedef struct fmx_line_hit {
  uint32_t group;
  uint32_t doc;     /* UINT32_MAX without a corpus */
  uint64_t line_no; /* 1-based: in the document, or in the text without a corpus */
  uint64_t start;   /* position of the line's first byte */
  uint32_t len;     /* end - start: the line without its break byte, in stream bytes */
  uint32_t n_hits;  /* occurrences that begin on this line */
  uint64_t raw_off; /* raw offset of start in the file; == start without a corpus */
  uint32_t raw_len; /* the line's length in the file; == len without a corpus */
  uint32_t first;   /* index, within the group's occurrence records, of the first hit on this line */
} fmx_line_hit;     /* 48 bytes */
int fmx_lines_prepare(const fmx_index *idx, const uint8_t *breaks, size_t n_breaks);
int fmx_lines_info(const fmx_index *idx, uint64_t *n_breaks_found, uint8_t set[4], uint32_t *n_set, uint32_t *shift,
                   uint64_t *bytes, double *build_ms);
int fmx_lines_batch(const fmx_index *idx, const uint64_t *pos, size_t k, uint64_t *line, uint64_t *start, uint64_t *end);
int fmx_lines_batch_dev(const fmx_index *idx, const void *d_pos, size_t k, void *d_line, void *d_start, void *d_end,
                        void *stream);
int fmx_line_spans(const fmx_index *idx, const uint64_t *line, size_t k, uint64_t *start, uint64_t *end);
int fmx_line_spans_dev(const fmx_index *idx, const void *d_line, size_t k, void *d_start, void *d_end, void *stream);
int fmx_occurrence_lines(const fmx_index *idx, const fmx_corpus *corpus_or_null, const uint64_t *occ_off /* n_groups + 1 */,
                         const fmx_occurrence *occ, size_t n_groups, uint64_t *out_off /* n_groups + 1 */, fmx_line_hit *out,
                         size_t cap, size_t *n_out);
int fmx_occurrence_lines_dev(const fmx_index *idx, const fmx_corpus *corpus_or_null, const void *d_occ_off, const void *d_occ,
                             size_t n_occ, size_t n_groups, void *d_out_off, void *d_out, size_t cap, size_t *n_out,
                             void *stream);
int fmx_lines_last(double *locate_ms, double *sort_ms, double *lookup_ms, double *compact_ms);

/* ---- line queries: all-of, none-of, near and inverted matches over line-hit lists, evaluated on the device.  Beyond the
 * reference.  DESIGN.md 24.
 * INPUT.  hit_off[n_groups + 1] and hits[] are exactly what fmx_occurrence_lines leaves: CSR over groups, the records of a
 * group ascending by line.  The KEY of a record is (doc, line_no), compared as the 64-bit value doc << 32 | line_no (line_no <
 * 2^32 because n < 2^32; without a corpus doc is UINT32_MAX in every record, so the key orders by line_no alone).  Within a
 * group the keys are strictly ascending.
 * A TERM is (group, window, flags).  A line X with key (d, i) SATISFIES a positive term if group `group` holds a record (d, j)
 * with max(1, i - window) <= j <= i + window; the upper end saturates, so a window of UINT32_MAX means "anywhere in the same
 * document" (without a corpus: anywhere in the text).  window == 0 means the same line.  A term with FMX_LQ_NOT set is
 * satisfied when no such record exists.  A window never reaches into another document, because the document is part of the
 * key.
 * A QUERY is an ANCHOR and a list of terms.  The anchor is a group number, or FMX_LQ_ALL_LINES (UINT32_MAX).  The query's
 * CANDIDATES are the anchor group's records, in order; for FMX_LQ_ALL_LINES they are the REAL LINES of the text, in order.  A
 * global line L of the line table (0 <= L <= n_brk) is real unless it is the empty piece behind a final break: without a
 * corpus L is not real if start(L) == n - 1; with a corpus L is not real if start(L) is the position of a document's
 * separator (start(L) == doc_start[d + 1] - 1).  An empty file therefore has no lines, a file that ends in "\n" has as many
 * lines as `wc -l` says, and an unterminated last line counts.  The query's RESULT is the candidates that satisfy every term,
 * in candidate order; a query without terms returns its candidates.
 * OUTPUT is CSR over QUERIES: out_off[n_queries + 1], out_off[n_queries] == *n_out, and fmx_line_hit records.  An output
 * record is the candidate's record with `group` set to the query's index.  For an FMX_LQ_ALL_LINES candidate the record is
 * built from the line table (and the corpus map when given): doc, line_no, start, len, raw_off and raw_len exactly as
 * fmx_occurrence_lines fills them for a hit on that line, n_hits = 0 and first = UINT32_MAX.  The same input gives the same
 * bytes on every run: no atomics decide an order.
 * `grep -v A` is the query (FMX_LQ_ALL_LINES, [(A, 0, FMX_LQ_NOT)]).  The algebra is over the hit lists it is given: a line
 * "holds a match" when a match BEGINS on it, and in mode `disjoint` a match that runs over a line break can hide a later one;
 * a caller who wants -v in grep's strict sense asks for the lists with lineOnly, or in mode `all` / `longest`.
 * q_off[n_queries + 1] is CSR over `terms`; q_off, anchor and terms are HOST memory in both forms (the call uploads them).
 * Capacity as fmx_occurrence_lines: more than cap results -> FMX_ERR_OVERFLOW with the EXACT total in *n_out, nothing written
 * past out[cap - 1]; cap == 0 with out == NULL is the counting call.
 * FMX_ERR_ARG, decided before the device is touched: null hit_off / out_off / n_out / q_off / anchor; terms null while there
 * are some; n_groups == 0 or > 2^26; n_queries == 0 or > 2^16; more than 64 terms in one query; q_off not non-decreasing from
 * 0; an anchor or term group >= n_groups (the anchor may be FMX_LQ_ALL_LINES); flags & ~1 or reserved != 0; cap >= 2^32;
 * n_hits > 2^26; a null handle (refused last); a corpus whose stream length != n - 1; in the host form also hit_off not
 * non-decreasing from 0, or keys not strictly ascending inside a group.  The device form cannot see the records: it downloads
 * hit_off (which must begin at 0, be non-decreasing and end at n_hits), its key kernel raises a flag for a group whose keys
 * do not ascend, and the call returns FMX_ERR_ARG after the launch with nothing reported.  No record value leads outside the
 * inputs, the table or the outputs.  The candidates of all queries together must be < 2^32, otherwise FMX_ERR_OVERFLOW with a
 * message, known on the host before anything candidate-sized is allocated.
 * Both forms ALLOCATE AND SYNCHRONISE (FMX_ERR_HIP under a stream capture, decided before anything is allocated, the capture
 * left valid) and free every temporary on every path; the need -- 8 bytes per hit, 4 per candidate, the scan's block totals,
 * the query tables -- is checked against the free HBM first (FMX_ERR_NOMEM).  Only a query with FMX_LQ_ALL_LINES needs the
 * line table: such a call builds one when absent, with fmx_occurrence_lines's rules ({10} without a corpus, {10, 1} with one;
 * a table that lacks byte 1 combined with a corpus is FMX_ERR_ARG; locate's refusals pass through, so an fmx_open_block
 * handle is FMX_ERR_UNSUPPORTED).  A call without such a query builds no table and changes none.
 * The process-wide key "lq_narrow" (fmx_config_set: on | off, default off: the plain per-lane search measured
 * faster) selects whether a wave whose candidates belong to
 * one query narrows each term's key range by the bounds of its first and last candidate before every lane searches.
 * fmx_line_query_last: the calling thread's last call: device ms of the key packing, of the flags and of scan + emit +
 * offsets, the candidates and the keys probed; any pointer may be NULL. */
#define FMX_LQ_ALL_LINES 0xffffffffu
#define FMX_LQ_NOT 1u
typedef struct fmx_line_term {
  uint32_t group;
  uint32_t window; /* lines on either side; 0: the same line; UINT32_MAX: the same document */
  uint32_t flags;  /* FMX_LQ_NOT */
  uint32_t reserved;
} fmx_line_term;    /* 16 bytes */
int fmx_line_query(const fmx_index *idx, const fmx_corpus *corpus_or_null, const uint64_t *hit_off /* n_groups + 1 */,
                   const fmx_line_hit *hits, size_t n_groups, const uint64_t *q_off /* n_queries + 1 */,
                   const uint32_t *anchor /* n_queries */, const fmx_line_term *terms, size_t n_queries,
                   uint64_t *out_off /* n_queries + 1 */, fmx_line_hit *out, size_t cap, size_t *n_out);
int fmx_line_query_dev(const fmx_index *idx, const fmx_corpus *corpus_or_null, const void *d_hit_off, const void *d_hits,
                       size_t n_hits, size_t n_groups, const uint64_t *q_off, const uint32_t *anchor, const fmx_line_term *terms,
                       size_t n_queries, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream);
int fmx_line_query_last(double *keys_ms, double *flags_ms, double *emit_ms, uint64_t *candidates, uint64_t *probes);

/* One process, several GPUs (the single-process form of SURVEY.md 8e for regexes; one process per GPU uses
 * findex_amd/distributed.py and an RCCL gather instead): the batch is cut into contiguous slices of about equal
 * estimated frontier work (start elements, states and follow entries of each regex), slice r is made resident on
 * idxs[r]'s device (every handle a replica of one index), the slices are matched concurrently from one host thread
 * each with no device-to-device traffic, and the result lists are concatenated: same output as
 * fmx_regex_batch_match on one handle (frontier mode only). */
typedef struct fmx_regex_batch_multi fmx_regex_batch_multi;
int fmx_regex_batch_create_multi(fmx_index *const *idxs, size_t n_idx, fmx_regex *const *res, size_t k,
                                 fmx_regex_batch_multi **out);
int fmx_regex_batch_free_multi(fmx_regex_batch_multi *mb);
int fmx_regex_batch_match_multi(fmx_regex_batch_multi *mb, const fmx_limits *lim, fmx_result *out, size_t cap,
                                size_t *n_out, uint32_t *per_regex_count);

/* Gathers per-device result slices into one host array (the host-side counterpart of the RCCL all-gather): slice r
 * is cnt[r] elements of `elem` bytes at DEVICE pointer d_src[r] on idxs[r]'s device and lands at
 * dst + (cnt[0] + .. + cnt[r-1]) * elem.  The copies of all devices run concurrently and the call returns when all
 * have landed.  For callers that keep their batches on the devices (fmx_*_dev entry points) and search slices on
 * several handles themselves. */
int fmx_gather(fmx_index *const *idxs, size_t n_idx, const void *const *d_src, const size_t *cnt, size_t elem,
               void *dst);

/* ---- the exchange itself: an RCCL all-gather of the ranks' device-resident result slices over xGMI (SURVEY.md 8e:
 * "ncclAllGather of uint64 sp[], ep[] slices after the kernels finish"), for callers below the Python mirror -- a JVM.
 * RCCL is loaded at first use (dlopen); FMX_ERR_UNSUPPORTED when the process has none.
 *   one process per GPU : rank 0 calls fmx_comm_unique_id, ships the 128 bytes to the other ranks by its own
 *                         means, every rank calls fmx_comm_create_rank(its handle, n_ranks, rank, id).
 *   one process, N GPUs : fmx_comm_create_all(one handle per device) -- ncclCommInitAll.
 * fmx_allgather_dev(comm, d_send, d_recv, bytes, producer_streams): every rank contributes `bytes` bytes at d_send[i] and
 * receives all ranks' contributions, in rank order, at d_recv[i] (n_ranks * bytes); the arrays have one entry per LOCAL
 * rank of the communicator (1, or N for fmx_comm_create_all, in the order of `idxs`).
 * fmx_gather_dev(.., root, ..): the same exchange delivered to ONE rank -- every rank sends its slice to `root`, only the
 * root's d_recv entry is written (the others may be NULL): the "final gather of hit intervals" when one rank consumes
 * the answer; with the 8-byte interval form (fmx_search_opts.packed) it moves half of what the all-gather of (sp, ep) did
 * per link and nothing at all into the other ranks.
 * Ordering: the collective runs on the communicator's own streams.  producer_streams[i] (a hipStream_t; one per local
 * rank) is the stream on which the caller enqueued the work that writes d_send[i] -- fmx_search_batch_dev is asynchronous --
 * and that last touched d_recv[i]: the collective waits for everything enqueued there so far (an event, no host
 * synchronisation).  producer_streams == NULL: the caller vouches that d_send and d_recv are idle (it has synchronised).
 * Both calls return when the exchange has completed on every local rank, so anything enqueued afterwards may read d_recv.
 * Slices of different lengths (regex result lists): gather the counts first, then the payload padded to the longest, as
 * findex_amd/distributed.py all_gather_varlen does. */
#define FMX_COMM_ID_BYTES 128
typedef struct fmx_comm fmx_comm;
int fmx_comm_unique_id(void *id /* FMX_COMM_ID_BYTES */);
int fmx_comm_create_rank(const fmx_index *idx, int n_ranks, int rank, const void *id, fmx_comm **out);
int fmx_comm_create_all(fmx_index *const *idxs, size_t n_idx, fmx_comm **out);
int fmx_comm_info(const fmx_comm *comm, int *n_ranks, int *n_local);
int fmx_comm_free(fmx_comm *comm);
int fmx_allgather_dev(fmx_comm *comm, const void *const *d_send, void *const *d_recv, size_t bytes,
                      void *const *producer_streams);
int fmx_gather_dev(fmx_comm *comm, const void *const *d_send, void *const *d_recv, size_t bytes, int root,
                   void *const *producer_streams);

/* ---- statistics (since open or the last reset; device counters are read with a sync).
 * rank_queries counts occ(c,i) evaluations in the REFERENCE's terms: two per backward step (findex.scala:26-27,
 * 32-36), one per occ_batch operand or LF step -- the number the Scala path would execute on the same inputs
 * (early exits included), which is what the CPU oracle counts too.  The kernels do less memory work than that:
 * a search's first step needs no block, narrow intervals share one, a single-row step needs one; what they
 * really asked of memory is in the *_requests fields (64-byte one-hot blocks, or in the bytes layout 128-byte
 * BWT blocks and their 4-byte checkpoints, one request each). */
typedef struct fmx_stats_t {
  uint64_t rank_queries;     /* occ evaluations the executed steps stand for (see above) */
  uint64_t backward_steps;   /* getPrevRange-equivalents executed (2 rank queries each) */
  uint64_t launches;         /* kernels launched by this handle */
  double last_kernel_ms;     /* device time of the last host-pointer call's kernel(s), HIP events (calls whose operands
                              * and results fit in 2 KB are not timed: they leave it as it was) */
  uint64_t index_bytes;      /* device bytes held: rank dictionary + BWT + tables */
  uint64_t n_blocks;         /* rank-dictionary blocks per symbol */
  uint32_t n_symbols;        /* symbols that own a bit-vector */
  uint32_t block_bytes;      /* bytes fetched per rank query: 64 (one-hot block) or 132 (BWT block + checkpoint) */
  double build_ms;           /* device time of the kernels that built the rank dictionary at open */
  uint32_t layout;           /* 0 = one-hot bit-vectors, 1 = BWT bytes + checkpoints */
  uint32_t search_residency; /* workgroups per CU the last fmx_search_batch[_dev] launch was sized for (0: none yet); | 0x100 once
                                the kernel's residency census (fmx_prepare) has confirmed the number (the occupancy query can
                                answer one too many: DESIGN.md 3, "residency") */
  uint64_t search_requests;  /* memory requests for rank-dictionary lines issued by fmx_search_batch[_dev]'s kernel */
  /* the regex frontier kernels (fmx_regex_*match*), for their roofline: */
  uint64_t frontier_requests;   /* memory requests for rank-dictionary lines */
  uint64_t frontier_elements;   /* frontier elements stepped (= their backward steps) */
  uint64_t frontier_queue_reads;   /* elements read from the HBM work queues */
  uint64_t frontier_queue_writes;  /* elements appended to the HBM work queues */
  uint64_t frontier_results;    /* results written */
  uint64_t frontier_records;    /* 32-byte state records loaded (none inside a literal stretch) */
  uint64_t ktab_lookups;        /* 16-byte k-mer table entries fetched (each stands for up to ktab_k backward steps) */
  uint32_t ktab_k;              /* K of the k-mer jump table (0: none, or not built yet) */
  uint32_t jump_chars;          /* characters (backward steps) one row-jump-table entry stands for (0: no such table) */
  double tables_build_ms;       /* host time spent building the k-mer table, the row jump table and the select directory
                                 * (at first use or in fmx_prepare): what a handle's first search / first Psi pays on top
                                 * of build_ms */
  uint64_t jump_lookups;        /* row-jump-table lookups (one memory request each) by fmx_search_batch[_dev]'s kernel: an entry
                                 * stands for jump_chars backward steps when the pattern's next jump_chars characters match
                                 * it, a pair of entries ("jump_pairs") for up to twice as many */
  uint64_t jump_bytes;          /* device bytes of the row jump table (0: the handle has none; 16 n, or 32 n with pairs);
                                 * part of index_bytes */
  uint64_t row_lookups;         /* 8-byte row-table words fetched (one or three backward steps of a one-row interval each):
                                 * by the one-row part of fmx_search_batch[_dev] and by the regex frontier */
  uint64_t row_bytes;           /* device bytes of the row table and the three-step row table (0: none); part of index_bytes */
  uint64_t peak_table_build_bytes;   /* most device memory one derived table's build held at once: since round 4 the table
                                      * itself (the row jump table was built through a second buffer of its size before) */
  uint64_t patterns_seen;       /* patterns this handle's literal searches have been asked for (what "tables_after" counts) */
  uint64_t tables_held_bytes;   /* device bytes of all derived tables of this handle now (what "table_budget" counts) */
  uint64_t table_budget_bytes;  /* the handle's budget in bytes (a fraction resolved against the HBM free now); ~0: none */
  uint64_t hbm_free_after_tables;   /* free device memory right after the handle's last table build (hipMemGetInfo; 0: none built) */
  double tables_alloc_ms;       /* of tables_build_ms: the time spent inside hipMalloc for the tables -- ~0 on memory nobody has held
                                 * since the box came up, 45-60 ms per GiB on memory a process released shortly before (the driver
                                 * wipes it first: profiles/r05_alloc.md); the rest of tables_build_ms is the build kernels */
} fmx_stats_t;
int fmx_stats(const fmx_index *idx, fmx_stats_t *out);
/* fmx_stats_t.last_kernel_ms alone, without the device synchronisation and counter read-back of fmx_stats. */
int fmx_last_kernel_ms(const fmx_index *idx, double *ms);
int fmx_stats_reset(fmx_index *idx);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H */
