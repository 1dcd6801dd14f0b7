// fmx_corpus_dev.h -- the corpus map as the units that need it see it (fmx_corpus.hip builds and owns it, fmx_occ.hip reads
// it): the handle's host side, the map's device view, and the searches (fmx_order.h's lower_bound / upper_bound) that turn a
// stream position into (document, offset).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fmx_order.h"

namespace fmx {

struct CoMap {
  const uint32_t *doc_start, *doc_esc, *esc_pos;
  uint64_t n_docs, n_esc, stream_len;
};

// (doc, esc_off, raw_off) of stream position p; false at or past the end of the stream
__device__ __forceinline__ bool co_map(const CoMap &m, uint64_t p, uint32_t &doc, uint64_t &esc_off, uint64_t &raw_off) {
  if (p >= m.stream_len) return false;
  const uint64_t d = upper_bound(m.doc_start, 0, m.n_docs, p) - 1;       // doc_start[0] = 0 <= p
  const uint64_t e = lower_bound(m.esc_pos, 0, m.n_esc, p);
  doc = (uint32_t)d;
  esc_off = p - m.doc_start[d];
  raw_off = esc_off - (e - m.doc_esc[d]);
  return true;
}

struct Corpus {
  int device = 0;
  uint64_t n_docs = 0, stream_len = 0, n_esc = 0;
  uint8_t *d_stream = nullptr;                      // until fmx_corpus_drop_stream
  uint32_t *d_doc_start = nullptr, *d_doc_esc = nullptr, *d_esc_pos = nullptr;
  double build_ms = 0.0;
  ~Corpus() {
    for (void *p : {(void *)d_stream, (void *)d_doc_start, (void *)d_doc_esc, (void *)d_esc_pos})
      if (p) (void)hipFree(p);
  }
  uint64_t bytes() const { return (d_stream ? stream_len : 0) + 8 * (n_docs + 1) + 4 * std::max<uint64_t>(n_esc, 1); }
  CoMap map() const { return CoMap{d_doc_start, d_doc_esc, d_esc_pos, n_docs, n_esc, stream_len}; }
};

// ---- the part the document listing and the ranking share (fmx_corpus.hip): the rows of k intervals as sorted
// (interval, document) keys.  corpus_index_check: `idx` is the index of this corpus' stream, on its device, k fits, and
// `st` is not being captured (`noun`: "document listing", "ranking" -- what the messages call the call).
// corpus_doc_keys: locate (the counts, then the rows), the key interval << doc_bits | document of every row -- the document
// of stream position stream_len - pat_len - SA, n_docs where that is no stream position --, the radix sort over exactly
// the significant bits, the head flags and their inclusive sum.  Allocates from `mem`, checks the room first and
// synchronises `st` once, for the row count; with d_set_off (u64[n_slots + 1], ascending from 0 to k: an interval -> slot map)
// the key is slot << doc_bits | document, slot = the one whose [set_off[slot], set_off[slot + 1]) holds the interval; records ev[0] before the locate, ev[1] after it, ev[2] after the key kernel
// and ev[3] after the sort.  rows == 0: nothing but loc_off is allocated and no event is recorded.
struct DocKeys {
  unsigned long long *loc_off = nullptr;            // [k + 1]: the located rows of the intervals before i
  SortSpace ws;                                     // keys(): the sorted keys
  const uint32_t *incl = nullptr;                   // [rows]: distinct keys up to and including row j (in ws.free_keys())
  uint64_t rows = 0;
  int doc_bits = 0;                                 // documents 0 .. n_docs (n_docs: no document) fit
};
int corpus_index_check(const Corpus *c, const fmx_index *idx, size_t k, hipStream_t st, const char *noun);
// corpus_doc_keys' first step, which the passages share (fmx_passages.hip): loc_off[k + 1] from `mem`, the counting locate,
// one synchronisation of `st` for *n_rows, and the 2^32 - 2 limit ("<noun> of .. rows")
int corpus_locate_count(const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, uint64_t max_per, hipStream_t st,
                        const char *noun, DevMem &mem, unsigned long long **loc_off, uint64_t *n_rows);
int corpus_doc_keys(const Corpus *c, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, uint64_t pat_len,
                    uint64_t max_per, hipStream_t st, const char *noun, DevMem &mem, Events<5> &ev, DocKeys &out,
                    const unsigned long long *d_set_off = nullptr, uint64_t n_slots = 0);

// ---- the shapes of a call's term slots, which the ranking and the passages check alike (fmx_rank.hip); `noun` heads the
// messages.  rank_check_tables: q_off starts at 0, never decreases and ends at n_terms, at most 64 slots per query, the
// weights (when given) finite; *max_slots: the longest query's.  rank_check_sets: set_off cuts the n_iv intervals into the slots.
int rank_check_tables(const char *noun, const uint64_t *q_off, size_t n_queries, size_t n_terms, const double *weights,
                      uint64_t *max_slots);
int rank_check_sets(const char *noun, const uint64_t *set_off, size_t n_terms, size_t n_iv);

}  // namespace fmx
