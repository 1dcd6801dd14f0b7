// fmx_lines_dev.h -- the line table as the units that read it see it (fmx_lines.hip builds and owns it, fmx_linequery.hip
// reads it): its device view, the lookups over it, and the one definition of "the record of a line".
#pragma once
#include <fmx.h>

#include "fmx_corpus_dev.h"
#include "fmx_host.h"

namespace fmx {

struct LinesDev {
  const uint32_t *brk, *dir;
  uint64_t n_brk, len;                               // len = n - 1, the bytes of the text
  uint32_t shift;
};

inline LinesDev lines_dev(const Index *h) {
  return LinesDev{static_cast<const uint32_t *>(h->lin.brk), static_cast<const uint32_t *>(h->lin.dir), h->lin.n_brk, h->n - 1,
                  h->lin.shift};
}

__device__ __forceinline__ uint64_t lin_line(const LinesDev &L, uint64_t p) {      // p < len
  const uint64_t b = p >> L.shift;
  uint64_t lo = L.dir[b], hi = L.dir[b + 1];
  hi = hi < L.n_brk ? hi : L.n_brk;
  lo = lo < hi ? lo : hi;
  return lower_bound(L.brk, lo, hi, p);
}
__device__ __forceinline__ uint64_t lin_start(const LinesDev &L, uint64_t line) { return line ? (uint64_t)L.brk[line - 1] + 1 : 0; }
__device__ __forceinline__ uint64_t lin_end(const LinesDev &L, uint64_t line) { return line < L.n_brk ? (uint64_t)L.brk[line] : L.len; }

// The record of global line l (l <= n_brk) but for group, n_hits and first, which are the caller's.
__device__ __forceinline__ fmx_line_hit lin_record(const LinesDev &L, uint64_t l, int has_map, const CoMap &m) {
  const uint64_t s = lin_start(L, l), e = lin_end(L, l);
  fmx_line_hit o;
  o.group = 0;
  o.doc = 0xffffffffu;
  o.line_no = l + 1;
  o.start = s;
  o.len = (uint32_t)(e - s);
  o.n_hits = 0;
  o.raw_off = s;
  o.raw_len = o.len;
  o.first = 0xffffffffu;
  if (has_map) {
    // the line begins in the document its hits lie in (the separator before it is a break), and ends on a break byte of
    // that document, which no escape pair contains
    uint32_t d = 0xffffffffu, d2;
    uint64_t eo, ro = ~0ull, ro2 = ~0ull;
    if (co_map(m, s, d, eo, ro)) {
      o.line_no = l - lin_line(L, m.doc_start[d]) + 1;
      if (!co_map(m, e, d2, eo, ro2)) ro2 = ro + (e - s);
    }
    o.doc = d;
    o.raw_off = ro;
    o.raw_len = (uint32_t)(ro2 - ro);
  }
  return o;
}

}  // namespace fmx
