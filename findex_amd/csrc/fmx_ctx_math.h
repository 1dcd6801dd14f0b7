// fmx_ctx_math.h -- the mask arithmetic of the context filter (fmx_context.hip), shared by host and device and
// tested exhaustively on the host (tests/native/ctx_math.cpp).
//
// A record's candidate rows [a, b) are cut into CHUNKS of `chunk` rows (a power of two, a multiple of kCtxLane) that begin
// at a multiple of kCtxLane at or below a, so every lane's kCtxLane rows are one aligned load of the BWT.  A lane holds a
// PASS MASK m: bit i set <=> row (lane's first row + i) is a row of the record AND its byte is in the class.  Runs of set
// bits are what the filter reports: a HEAD is a passing row whose predecessor does not pass, a TAIL one whose successor
// does not.  The predecessor of a mask's bit 0 and the successor of its top bit come in as carries: the pass bit of that
// row when it is a row of the same record, else 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FMX_CTX_HD __host__ __device__ inline
#else
#define FMX_CTX_HD inline
#endif

namespace fmx {

constexpr uint32_t kCtxLane = 16;                    // rows (BWT bytes) per lane and load

// bits [lo, hi) of a `width`-bit mask (width <= 32), both ends clipped to the width
FMX_CTX_HD uint32_t ctx_range_mask(uint64_t lo, uint64_t hi, uint32_t width) {
  if (hi > width) hi = width;
  if (lo >= hi) return 0u;
  const uint32_t upto_hi = hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u);
  return upto_hi & ~((1u << lo) - 1u);              // lo < hi <= 32: lo <= 31
}

// the bits of the `width` rows from `row0` on that are rows of [a, b)
FMX_CTX_HD uint32_t ctx_valid_mask(uint64_t row0, uint64_t a, uint64_t b, uint32_t width) {
  const uint64_t lo = a > row0 ? a - row0 : 0, hi = b > row0 ? b - row0 : 0;
  return ctx_range_mask(lo, hi, width);
}

// run heads of a pass mask: carry_in = the pass bit of the row before bit 0 (0 when that row is not of the record)
FMX_CTX_HD uint32_t ctx_heads(uint32_t m, uint32_t carry_in) { return m & ~((m << 1) | (carry_in & 1u)); }

// run tails of a `width`-bit pass mask: carry_out = the pass bit of the row behind bit width - 1 (0: not of the record)
FMX_CTX_HD uint32_t ctx_tails(uint32_t m, uint32_t carry_out, uint32_t width) {
  return m & ~((m >> 1) | ((carry_out & 1u) << (width - 1)));
}

// the first row of a record's first chunk, the number of its chunks, and the rows of chunk c that are the record's
FMX_CTX_HD uint64_t ctx_chunk_base(uint64_t a) { return a & ~(uint64_t)(kCtxLane - 1); }
FMX_CTX_HD uint64_t ctx_chunk_count(uint64_t a, uint64_t b, uint64_t chunk) {
  return a < b ? (b - ctx_chunk_base(a) + chunk - 1) / chunk : 0;
}
FMX_CTX_HD uint64_t ctx_chunk_first(uint64_t a, uint64_t c, uint64_t chunk) { return ctx_chunk_base(a) + c * chunk; }

}  // namespace fmx
