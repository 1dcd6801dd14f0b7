// fmx_rank_math.h -- the arithmetic of ranked retrieval (fmx_rank.hip), for the host and the device alike:
// the BM25 term exactly as include/fmx.h states it (IEEE double, every operation rounded once, none contracted into an
// FMA), the default weight, and the monotone map between a double and the u64 key the selection compares.  Plain
// functions that need no device: tests/native/rank_math.cpp checks them on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>

#ifdef __HIPCC__
#define FMX_RANK_HD __host__ __device__ __forceinline__
#else
#define FMX_RANK_HD inline
#endif
// hipcc contracts a * b + c into an FMA by default: not inside these functions
#ifdef __clang__
#define FMX_RANK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FMX_RANK_NO_CONTRACT
#endif

namespace fmx {

constexpr uint32_t kRankMaxTop = 1024;              // results per query: what one workgroup sorts in LDS
constexpr uint32_t kRankMaxSlots = 64;              // term slots per query

// nd = k1 * ((1 - b) + b * len / avglen); a corpus of empty documents (avglen == 0) has r = 0
FMX_RANK_HD double rank_norm(uint64_t len, double avglen, double k1, double b) {
  FMX_RANK_NO_CONTRACT
  const double r = avglen == 0.0 ? 0.0 : (double)len / avglen;
  const double s = b * r;
  const double t = (1.0 - b) + s;
  return k1 * t;
}

// c(t) = w * ((tf * (k1 + 1)) / (tf + nd))
FMX_RANK_HD double rank_term(double w, uint64_t tf, double k1, double nd) {
  FMX_RANK_NO_CONTRACT
  const double f = (double)tf;
  const double num = f * (k1 + 1.0);
  const double den = f + nd;
  const double q = num / den;
  return w * q;
}

FMX_RANK_HD double rank_add(double acc, double c) {
  FMX_RANK_NO_CONTRACT
  return acc + c;
}

// The usual order-preserving map of a double's bits: a < b as doubles <=> key(a) < key(b) as u64 (for -0.0 < +0.0 too)
FMX_RANK_HD uint64_t rank_key(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

FMX_RANK_HD double rank_unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &u, 8);
  return x;
}

// w(t) = log(1 + (N - df + 0.5) / (df + 0.5)), on the host
inline double rank_weight(uint64_t n_docs, uint64_t df) {
  return std::log(1.0 + ((double)(n_docs - df) + 0.5) / ((double)df + 0.5));
}

}  // namespace fmx
