// fmx_order.hip -- the scan, the radix sort and the small order kernels of fmx_order.h.
//
// Radix sort: 8-bit digits, one pass = k_ord_hist (per 4096-key tile histogram, digit-major) + exclusive scan +
// k_ord_scatter (stable: a tile goes through in 256-key chunks, each key's place among its digit's keys from eight
// wave ballots).  Everything is u32 index / u64 key; a loop index is u64, so positions >= 2^31 stay unsigned throughout.
// Scan: 2048 elements per block, the block totals scanned recursively.  No library sort, no host sort.
#include "fmx_order.h"

namespace fmx {

constexpr int kOrdThreads = 256;

__device__ __forceinline__ uint32_t scan_op(int op, uint32_t a, uint32_t b) { return op == kScanMax ? (a > b ? a : b) : a + b; }

// ---- LSD radix sort of (u64 key, u32 value), 8 bits per pass
__global__ __launch_bounds__(kOrdThreads) void k_ord_hist(const unsigned long long *__restrict__ key, uint64_t m, int shift,
                                                          uint32_t *__restrict__ hist /* [256][ntiles] */, uint64_t ntiles) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kRadixTile;
  for (uint32_t c = 0; c < kRadixTile; c += kOrdThreads) {
    const uint64_t idx = base + c + threadIdx.x;
    if (idx < m) atomicAdd(&h[(key[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// hist: the exclusive scan of k_ord_hist's output = where this tile's first key of each digit goes.  Stable: inside a
// 256-key chunk a key's place is its lane rank among the wave's keys of its digit (eight ballots) plus the counts of
// the waves before it; chunks follow each other through base[].
__global__ __launch_bounds__(kOrdThreads) void k_ord_scatter(const unsigned long long *__restrict__ kin,
                                                             const uint32_t *__restrict__ vin,
                                                             unsigned long long *__restrict__ kout,
                                                             uint32_t *__restrict__ vout, uint64_t m, int shift,
                                                             const uint32_t *__restrict__ hist, uint64_t ntiles) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[kOrdThreads / 64][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1;
  base[tid] = hist[(uint64_t)tid * ntiles + blockIdx.x];
  const uint64_t tile = (uint64_t)blockIdx.x * kRadixTile;
  for (uint32_t c = 0; c < kRadixTile; c += kOrdThreads) {
    const uint64_t idx = tile + c + tid;
    const bool valid = idx < m;
    const unsigned long long k = valid ? kin[idx] : 0ull;
    const uint32_t v = valid ? vin[idx] : 0u;
    const uint32_t d = (uint32_t)(k >> shift) & 255u;
    for (int w = 0; w < kOrdThreads / 64; w++) wc[w][tid] = 0;
    __syncthreads();
    unsigned long long mm = __ballot(valid);
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bb = __ballot(bit);
      mm &= bit ? bb : ~bb;
    }
    const uint32_t r = (uint32_t)__popcll(mm & lt);
    if (valid && r == 0) wc[wave][d] = (uint32_t)__popcll(mm);
    __syncthreads();
    if (valid) {
      uint32_t dst = base[d] + r;
      for (int w = 0; w < wave; w++) dst += wc[w][d];
      kout[dst] = k;
      vout[dst] = v;
    }
    __syncthreads();
    uint32_t add = 0;
    for (int w = 0; w < kOrdThreads / 64; w++) add += wc[w][tid];
    base[tid] += add;
    __syncthreads();
  }
}

// ---- scans of u32 (sum or max; inclusive or exclusive), 2048 elements per block, block totals scanned recursively
__global__ __launch_bounds__(kOrdThreads) void k_ord_scan_tile(uint32_t *__restrict__ d, uint64_t len,
                                                               uint32_t *__restrict__ sums, int op, int exclusive) {
  __shared__ uint32_t t[kOrdThreads];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * 8;
  uint32_t x[8], acc = 0;                   // 0 is the identity of both operators
  for (int e = 0; e < 8; e++) {
    x[e] = base + e < len ? d[base + e] : 0u;
    acc = scan_op(op, acc, x[e]);
  }
  t[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 1; off < kOrdThreads; off <<= 1) {
    const uint32_t y = (int)threadIdx.x >= off ? t[threadIdx.x - off] : 0u;
    __syncthreads();
    t[threadIdx.x] = scan_op(op, t[threadIdx.x], y);
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? t[threadIdx.x - 1] : 0u;
  for (int e = 0; e < 8; e++) {
    const uint32_t before = run;
    run = scan_op(op, run, x[e]);
    if (base + e < len) d[base + e] = exclusive ? before : run;
  }
  if (threadIdx.x == kOrdThreads - 1) sums[blockIdx.x] = t[kOrdThreads - 1];
}

__global__ __launch_bounds__(kOrdThreads) void k_ord_scan_add(uint32_t *__restrict__ d, uint64_t len,
                                                              const uint32_t *__restrict__ sums, int op) {
  const uint32_t carry = sums[blockIdx.x];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
  for (uint32_t e = threadIdx.x; e < kScanTile; e += kOrdThreads)
    if (base + e < len) d[base + e] = scan_op(op, carry, d[base + e]);
}

hipError_t ScanSpace::run(uint32_t *d, uint64_t len, int op, bool exclusive, uint32_t *partials, hipStream_t st) {
  if (len == 0) return hipSuccess;
  const uint64_t nb = (len + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(k_ord_scan_tile, dim3((unsigned)nb), dim3(kOrdThreads), 0, st, d, len, partials, op, exclusive ? 1 : 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || nb == 1) return e;
  // the block totals: their exclusive scan (a max's exclusive prefix is the max of the blocks before)
  if ((e = run(partials, nb, op, true, partials + nb, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_ord_scan_add, dim3((unsigned)nb), dim3(kOrdThreads), 0, st, d, len, partials, op);
  return hipGetLastError();
}

int SortSpace::alloc(DevMem &mem, uint64_t m, const char *what) {
  int rc;
  if ((rc = mem.take((void **)&k_[0], 8 * m, what)) || (rc = mem.take((void **)&k_[1], 8 * m, what)) ||
      (rc = mem.take((void **)&v_[0], 4 * m, what)) || (rc = mem.take((void **)&v_[1], 4 * m, what)) ||
      (rc = mem.take((void **)&hist_, 4 * sort_hist_words(m), what)))
    return rc;
  return scan_.alloc(mem, sort_scan_len(m), what);
}

hipError_t SortSpace::sort(uint64_t m, int bits, hipStream_t st) {
  const uint64_t nt = radix_tiles(m);
  passes = 0;
  for (int shift = 0; shift < bits; shift += 8) {
    hipLaunchKernelGGL(k_ord_hist, dim3((unsigned)nt), dim3(kOrdThreads), 0, st, keys(), m, shift, hist_, nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = scan_.sum(hist_, 256 * nt, true, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ord_scatter, dim3((unsigned)nt), dim3(kOrdThreads), 0, st, keys(), vals(), free_keys(), free_vals(), m, shift,
                       hist_, nt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    swap();
    ++passes;
  }
  return hipSuccess;
}

// ---- gather, CSR offsets, head flags
__global__ __launch_bounds__(kOrdThreads) void k_ord_gather3(const unsigned long long *__restrict__ stage,
                                                             const uint32_t *__restrict__ val, uint64_t rows,
                                                             unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const uint64_t s = val[j] < rows ? val[j] : rows - 1;
#pragma unroll
    for (int w = 0; w < 3; w++) out[3 * j + w] = stage[3 * s + w];
  }
}

__global__ __launch_bounds__(kOrdThreads) void k_ord_csr_off(const unsigned long long *__restrict__ key, uint64_t rows, uint64_t k,
                                                             int shift, unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= k; i += stride)
    out_off[i] = i < k ? lower_bound(key, 0, rows, i << shift) : rows;      // (k << shift need not fit)
}

__global__ __launch_bounds__(kOrdThreads) void k_ord_heads(const unsigned long long *__restrict__ key, uint64_t rows,
                                                           uint32_t *__restrict__ head) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride)
    head[j] = j == 0 || key[j] != key[j - 1] ? 1u : 0u;
}

hipError_t launch_gather3(const unsigned long long *stage, const uint32_t *val, uint64_t rows, unsigned long long *out, hipStream_t st) {
  hipLaunchKernelGGL(k_ord_gather3, dim3(flat_grid(rows)), dim3(kOrdThreads), 0, st, stage, val, rows, out);
  return hipGetLastError();
}

hipError_t launch_csr_off(const unsigned long long *key, uint64_t rows, uint64_t k, int shift, unsigned long long *out_off, hipStream_t st) {
  hipLaunchKernelGGL(k_ord_csr_off, dim3(flat_grid(k + 1)), dim3(kOrdThreads), 0, st, key, rows, k, shift, out_off);
  return hipGetLastError();
}

hipError_t launch_heads(const unsigned long long *key, uint64_t rows, uint32_t *head, hipStream_t st) {
  hipLaunchKernelGGL(k_ord_heads, dim3(flat_grid(rows, 8192)), dim3(kOrdThreads), 0, st, key, rows, head);
  return hipGetLastError();
}

// ---- classes of rows from the LCP array
__global__ __launch_bounds__(kOrdThreads) void k_stops(const uint8_t *__restrict__ s, uint64_t m, uint32_t stop,
                                                       uint32_t *__restrict__ P) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride)
    P[t] = s[m - 1 - t] == stop ? (uint32_t)t + 1u : 0u;
}

__global__ __launch_bounds__(kOrdThreads) void k_class_heads(const uint32_t *__restrict__ lcp, uint64_t n, uint32_t L,
                                                             uint32_t *__restrict__ A, uint32_t *__restrict__ B) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    A[r] = (r == 0 || lcp[r - 1] < L) ? (uint32_t)r + 1u : 0u;
    if (B) B[r] = 0u;
  }
}

// The lanes of a wave hold consecutive rows, so a class is a stretch of lanes: a segmented max over the wave, then one
// atomicMax per class and wave.  The loop's trip count is the same for every lane of a workgroup: all 64 lanes shuffle.
// (LCP[n - 1] is 0, so the guard on the last row changes nothing; it keeps the read inside what the row itself says.)
__global__ __launch_bounds__(kOrdThreads) void k_class_max(const uint32_t *__restrict__ lcp, const uint32_t *__restrict__ sa,
                                                           const uint32_t *__restrict__ A, uint64_t n, uint32_t L,
                                                           uint32_t *__restrict__ B) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const uint32_t last = (uint32_t)(n - 1);
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += stride) {
    const uint64_t r = b + threadIdx.x;
    const bool rep = r < n && ((r > 0 && lcp[r - 1] >= L) || (r < n - 1 && lcp[r] >= L));
    const uint32_t key = rep ? A[r] : 0u;                     // >= 1 for a row of a class of two rows and more
    uint32_t val = rep ? min(sa[r], last) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ok = __shfl_up(key, d, 64), ov = __shfl_up(val, d, 64);
      if (lane >= d && ok == key) val = max(val, ov);
    }
    const uint32_t next = __shfl_down(key, 1, 64);
    if (rep && (lane == 63 || next != key)) atomicMax(&B[min(key - 1u, last)], val);
  }
}

hipError_t launch_stops(const uint8_t *s, uint64_t m, uint32_t stop, uint32_t *P, hipStream_t st) {
  hipLaunchKernelGGL(k_stops, dim3(flat_grid(m)), dim3(kOrdThreads), 0, st, s, m, stop, P);
  return hipGetLastError();
}

hipError_t launch_class_heads(const uint32_t *lcp, uint64_t n, uint32_t L, uint32_t *A, uint32_t *B, hipStream_t st) {
  hipLaunchKernelGGL(k_class_heads, dim3(flat_grid(n)), dim3(kOrdThreads), 0, st, lcp, n, L, A, B);
  return hipGetLastError();
}

hipError_t launch_class_max(const uint32_t *lcp, const uint32_t *sa, const uint32_t *A, uint64_t n, uint32_t L, uint32_t *B, hipStream_t st) {
  hipLaunchKernelGGL(k_class_max, dim3(flat_grid(n)), dim3(kOrdThreads), 0, st, lcp, sa, A, n, L, B);
  return hipGetLastError();
}

}  // namespace fmx
