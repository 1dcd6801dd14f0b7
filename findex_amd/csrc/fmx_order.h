// fmx_order.h -- the order step the feature calls share: sort (key, value) pairs, scan flags, number the
// distinct keys, compact to CSR.  The workspaces as records, the searches as device helpers, and the small kernels that
// several units would otherwise each write out, every one behind a launcher that launches and returns hipGetLastError().
// fmx_order.hip holds the kernels; the sizes are in fmx_order_math.h.
#pragma once
#include "fmx_host.h"

namespace fmx {

// ---- device helpers: the binary searches over an ascending a[lo, hi)
template <typename T>
__device__ __forceinline__ uint64_t lower_bound(const T *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v) {   // first i: a[i] >= v
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename T>
__device__ __forceinline__ uint64_t upper_bound(const T *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v) {   // first i: a[i] > v
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- the scan's scratch: in place over len u32, sum or max, inclusive or exclusive; only enqueues on `st`
struct ScanSpace {
  uint32_t *partials = nullptr;
  static uint64_t bytes(uint64_t len) { return scan_space_bytes(len); }
  int alloc(DevMem &mem, uint64_t len, const char *what) { return mem.take((void **)&partials, bytes(len), what); }
  hipError_t sum(uint32_t *d, uint64_t len, bool exclusive, hipStream_t st) const { return run(d, len, kScanSum, exclusive, partials, st); }
  hipError_t max(uint32_t *d, uint64_t len, bool exclusive, hipStream_t st) const { return run(d, len, kScanMax, exclusive, partials, st); }

 private:
  static hipError_t run(uint32_t *d, uint64_t len, int op, bool exclusive, uint32_t *partials, hipStream_t st);
};

// ---- the sort's workspace: LSD radix sort of up to m (u64 key, u32 value) pairs, 8 bits per pass, stable; m < 2^32.
// The caller's key kernel writes keys() / vals(); after sort() these are the sorted pair, and free_keys() / free_vals()
// the other pair, the caller's to reuse.  scan() scans up to m elements with the scratch the sort's own scan uses.
struct SortSpace {
  int passes = 0;                               // of the last sort: 3 launches each
  static uint64_t bytes(uint64_t m) { return sort_space_bytes(m); }
  int alloc(DevMem &mem, uint64_t m, const char *what);
  unsigned long long *keys() const { return k_[cur_]; }
  uint32_t *vals() const { return v_[cur_]; }
  unsigned long long *free_keys() const { return k_[cur_ ^ 1]; }
  uint32_t *free_vals() const { return v_[cur_ ^ 1]; }
  void swap() { cur_ ^= 1; }                    // the caller wrote the next sort's input into the free pair
  // the free value buffer leaves the workspace and `p`, a buffer of the same size, takes its place
  uint32_t *trade_free_vals(uint32_t *p) { std::swap(p, v_[cur_ ^ 1]); return p; }
  hipError_t sort(uint64_t m, int bits, hipStream_t st);      // the first m pairs by the keys' low `bits` bits
  const ScanSpace &scan() const { return scan_; }

 private:
  unsigned long long *k_[2] = {nullptr, nullptr};
  uint32_t *v_[2] = {nullptr, nullptr};
  uint32_t *hist_ = nullptr;
  ScanSpace scan_;
  int cur_ = 0;
};

// ---- launchers of the shared kernels
// out[3 j .. 3 j + 2] = stage[3 val[j] .. ], j < rows: 24-byte records into sorted order (val clamped below rows)
hipError_t launch_gather3(const unsigned long long *stage, const uint32_t *val, uint64_t rows, unsigned long long *out, hipStream_t st);
// out_off[i] = the first sorted key that is not below i << shift, i = 0 .. k; out_off[k] = rows without forming k << shift
// (which need not fit).  key == nullptr with rows == 0: all zero.
hipError_t launch_csr_off(const unsigned long long *key, uint64_t rows, uint64_t k, int shift, unsigned long long *out_off, hipStream_t st);
// head[j] = 1 where key[j] differs from key[j - 1] (and at j == 0), else 0
hipError_t launch_heads(const unsigned long long *key, uint64_t rows, uint32_t *head, hipStream_t st);

// The classes of rows that share their first L bytes, from the LCP array (fmx_repeats.hip, fmx_ngrams.hip):
// stops: P[t] = t + 1 where T[t] = s[m - 1 - t] is the stop byte, else 0
hipError_t launch_stops(const uint8_t *s, uint64_t m, uint32_t stop, uint32_t *P, hipStream_t st);
// class heads: A[r] = r + 1 where a class begins (r == 0 or LCP[r - 1] < L), else 0; B[r] = 0 unless B is null
hipError_t launch_class_heads(const uint32_t *lcp, uint64_t n, uint32_t L, uint32_t *A, uint32_t *B, hipStream_t st);
// class maxima: A the max-scanned heads; B[head] = the largest SA of the class, over the classes of two rows and more
hipError_t launch_class_max(const uint32_t *lcp, const uint32_t *sa, const uint32_t *A, uint64_t n, uint32_t L, uint32_t *B, hipStream_t st);

}  // namespace fmx
