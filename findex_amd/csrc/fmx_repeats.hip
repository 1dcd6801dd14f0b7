// fmx_repeats.hip -- the repeated stretches of the indexed text from the LCP array (fmx.h: repeats).
//
// T is the text of m = n - 1 bytes, s = reverse(T) + sentinel, SA and LCP as fmx_locate.hip and fmx_lcp.hip have them.  The
// window T[t .. t + L) is s[p .. p + L) with p = m - t - L, the prefix of the suffix of the row with SA == p.  The rows whose
// suffixes share their first L bytes are a maximal run of rows with LCP[r] >= L between neighbours: a CLASS; LCP[r] >= L
// implies that both suffixes have L bytes in front of the sentinel, so every row of such a run is a window.
//
// One call: the inversion (SA and s), the stop scan when there is a stop byte, then per threshold L (the stops, the class
// heads and the class maxima are fmx_order.h's kernels, shared with fmx_ngrams.hip)
//
//   class heads    : A[r] = r + 1 where a class begins (r == 0 or LCP[r - 1] < L), else 0; B[r] = 0.  A max-scan turns A
//                    into (head row of r's class) + 1: the class id.
//   class maxima   : B[head] = the largest SA of the class, over the rows of repeated classes only (LCP[r - 1] >= L or
//                    LCP[r] >= L).  The lanes of a wave hold consecutive rows, so a class is a stretch of lanes: a segmented
//                    max over the wave first, one atomicMax per class and wave -- a run of one letter is ONE class of n rows.
//   k_rep_scatter  : flag8[t] = 1 for the rows to flag (all of a repeated class, or all but the one with the largest SA: the
//                    smallest t), t = m - SA - L: one byte scattered per row.  The last row of a class (LCP[r] < L) knows
//                    the class' size (r - head + 1) and answers for it in the summary: classes, windows, the largest class
//                    as one 64-bit max of size << 32 | ~(smallest t).  It asks the stop scan whether the class is eligible.
//   k_rep_seed     : in text order, B[t] = t + 1 where a flagged and eligible window starts, else 0 (a window holds a stop
//                    byte iff the last stop byte at or before t + L - 1 is at t or later: P[t + L - 1] > t).  A max-scan
//                    turns B into (the last flagged start at or before t) + 1; byte t is covered iff it is less than L past it.
//   k_rep_bounds   : A[t] = 1 where a range begins (t covered, t - 1 not), and the covered bytes.  A sum-scan numbers the
//                    ranges.
//   k_rep_write    : the first byte of a range writes its start, the last its end, at out[base + number], below cap only.
//
// Every pass streams over n rows or m bytes except the one scatter; every atomic is a max or an integer sum, so the same
// input gives the same bytes.  Every value read from SA is clamped below n, and a window is used only when p + L <= m: an SA
// that is no suffix array gives unspecified flags, never an access outside the buffers.  A and B are reused between row
// order and text order (m < n).  The host reads each threshold's total and summary before the next threshold begins.
#include <fmx.h>

#include <string>

#include "fmx_order.h"

namespace fmx {

static_assert(FMX_REPEATS_TILE == kScanTile, "FMX_REPEATS_TILE is the scan's block: what the tests place their edges at");
static_assert(sizeof(fmx_repeat_opts) == 8 && sizeof(fmx_repeat_range) == 16 && sizeof(fmx_repeat_summary) == 48, "fmx.h");

constexpr int kRepThreads = 256;

// res[0] classes, res[1] flagged windows, res[2] max of size << 32 | (0xFFFFFFFF - smallest t)
__global__ __launch_bounds__(kRepThreads) void k_rep_scatter(const uint32_t *__restrict__ lcp, const uint32_t *__restrict__ sa,
                                                             const uint32_t *__restrict__ A, const uint32_t *__restrict__ B,
                                                             const uint32_t *__restrict__ P, uint64_t n, uint32_t L,
                                                             uint32_t later, uint8_t *__restrict__ flag8,
                                                             unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_cls[kRepThreads / 64], s_win[kRepThreads / 64], s_best[kRepThreads / 64];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, m = n - 1;
  const uint32_t last = (uint32_t)(n - 1);
  unsigned long long cls = 0, win = 0, best = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    const bool below = r > 0 && lcp[r - 1] >= L, here = lcp[r] >= L;
    if (!below && !here) continue;
    const uint32_t head = min(A[r] - 1u, last);
    const uint64_t pmax = min(B[head], last), p = min(sa[r], last);
    if (p + L <= m && !(later && p == pmax)) flag8[m - p - L] = 1;
    if (!here && pmax + L <= m) {                             // the class' last row: its size, its smallest t
      const uint64_t size = r - head + 1, tmin = m - L - pmax;
      if (P == nullptr || P[tmin + L - 1] <= tmin) {
        cls += 1;
        win += later ? size - 1 : size;
        best = max(best, (unsigned long long)((size << 32) | (0xFFFFFFFFull - tmin)));
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cls += (unsigned long long)__shfl_xor(cls, d, 64);
    win += (unsigned long long)__shfl_xor(win, d, 64);
    best = max(best, (unsigned long long)__shfl_xor(best, d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    s_cls[threadIdx.x >> 6] = cls;
    s_win[threadIdx.x >> 6] = win;
    s_best[threadIdx.x >> 6] = best;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kRepThreads / 64; w++) {
      cls += s_cls[w];
      win += s_win[w];
      best = max(best, s_best[w]);
    }
    if (cls) atomicAdd(res, cls);
    if (win) atomicAdd(res + 1, win);
    if (best) atomicMax(res + 2, best);
  }
}

__global__ __launch_bounds__(kRepThreads) void k_rep_seed(const uint8_t *__restrict__ flag8, const uint32_t *__restrict__ P,
                                                          uint64_t m, uint32_t L, uint32_t *__restrict__ B) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
    bool f = flag8[t] != 0;
    if (f && P) f = P[min(t + L - 1, m - 1)] <= t;
    B[t] = f ? (uint32_t)t + 1u : 0u;
  }
}

// B: the scanned starts.  Byte t is covered iff a flagged window starts at most L - 1 bytes before it.
__device__ __forceinline__ bool rep_covered(const uint32_t *__restrict__ B, uint64_t t, uint32_t L) {
  const uint32_t b = B[t];
  return b != 0 && t + 1 - b < L;
}

// res[3]: the covered bytes
__global__ __launch_bounds__(kRepThreads) void k_rep_bounds(const uint32_t *__restrict__ B, uint64_t m, uint32_t L,
                                                            uint32_t *__restrict__ A, unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_cov[kRepThreads / 64];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long cov = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
    const bool c = rep_covered(B, t, L);
    A[t] = c && !(t > 0 && rep_covered(B, t - 1, L)) ? 1u : 0u;
    cov += c ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cov += (unsigned long long)__shfl_xor(cov, d, 64);
  if ((threadIdx.x & 63) == 0) s_cov[threadIdx.x >> 6] = cov;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kRepThreads / 64; w++) cov += s_cov[w];
    if (cov) atomicAdd(res + 3, cov);
  }
}

// A: the inclusive sum of the range starts, so a covered byte's range is number A[t] - 1 of this threshold
__global__ __launch_bounds__(kRepThreads) void k_rep_write(const uint32_t *__restrict__ B, const uint32_t *__restrict__ A, uint64_t m,
                                                           uint32_t L, uint64_t base, uint64_t cap,
                                                           unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
    if (!rep_covered(B, t, L)) continue;
    const uint32_t a = A[t];
    const uint64_t at = base + a - 1;
    if (a == 0 || at >= cap) continue;
    if (!(t > 0 && rep_covered(B, t - 1, L))) out[2 * at] = t;
    if (!(t + 1 < m && rep_covered(B, t + 1, L))) out[2 * at + 1] = t + 1;
  }
}

// ---------------------------------------------------------------- host side
struct RepeatsInfo {
  double invert_ms = 0.0, class_ms = 0.0, cover_ms = 0.0, compact_ms = 0.0;
};

// the device bytes a build of the LCP array takes while it runs (lcp_prepare's own sum)
static uint64_t lcp_build_bytes(const Index *h) {
  const uint64_t n = h->n;
  return 4 * n + 4 * n + lcp_text_bytes(n) + lcp_core_bytes(n) + locate_invert_text_bytes(h);
}

// the device bytes repeats_run allocates, the inversion's temporaries included
static uint64_t repeats_bytes(const Index *h, bool stop) {
  const uint64_t n = h->n;
  return 4 * n + lcp_text_bytes(n) + 8 * n + (stop ? 4 * n : 0) + n + ScanSpace::bytes(n) + 64 + locate_invert_text_bytes(h);
}

static bool lcp_built(const Index *h) {
  std::lock_guard<std::mutex> lk(h->lcp.mu);
  return h->lcp.ready;
}

// the free device bytes a call needs: its own, beside the LCP array when that is still to be built, or that build's
static uint64_t repeats_need(const Index *h, bool stop) {
  const uint64_t own = repeats_bytes(h, stop);
  return lcp_built(h) ? own : std::max(own + 4 * h->n, lcp_build_bytes(h));
}

// The whole call on `st`, outputs in device memory: off[k + 1] (host) and sum[k] (host, may be null) are filled, d_out gets
// the records below cap.  Allocates, synchronises `st`, frees its temporaries on every path.
static int repeats_run(const Index *h, const uint32_t *min_len, size_t k, uint32_t later, uint32_t stop, void *d_out, uint64_t cap,
                       hipStream_t st, uint64_t *off, fmx_repeat_summary *sum, RepeatsInfo *info) {
  *info = RepeatsInfo{};
  const uint64_t n = h->n, m = n - 1;
  off[0] = 0;
  bool any = false;
  for (size_t j = 0; j < k; j++) any = any || min_len[j] <= m;
  if (!any) {                                                  // every threshold is longer than the text
    for (size_t j = 0; j < k; j++) {
      off[j + 1] = 0;
      if (sum) sum[j] = fmx_repeat_summary{};
    }
    return FMX_OK;
  }
  int rc = device_room(repeats_need(h, stop != 0), "fmx_repeats");
  if (rc) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, st))) return rc;
  const uint32_t *lcp = static_cast<const uint32_t *>(h->lcp.lcp);
  Events<6> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  uint32_t *sa = nullptr, *A = nullptr, *B = nullptr, *P = nullptr;
  ScanSpace scan;
  uint8_t *s = nullptr, *flag8 = nullptr;
  unsigned long long *res = nullptr;
  DEV_ALLOC(mem, sa, 4 * n, "repeats suffix array");
  DEV_ALLOC(mem, s, lcp_text_bytes(n), "repeats text");
  DEV_ALLOC(mem, A, 4 * n, "repeats classes");
  DEV_ALLOC(mem, B, 4 * n, "repeats classes");
  if (stop) DEV_ALLOC(mem, P, 4 * n, "repeats stop scan");
  DEV_ALLOC(mem, flag8, n, "repeats flags");
  if ((rc = scan.alloc(mem, n, "repeats scan"))) return rc;
  DEV_ALLOC(mem, res, 64, "repeats summary");
  uint64_t launches = 0;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  HIP_TRY(hipMemsetAsync(s, 0, lcp_text_bytes(n), st), "hipMemsetAsync");
  if ((rc = locate_invert_text(h, st, sa, s))) return rc;
  if (stop) {
    HIP_TRY(launch_stops(s, m, stop, P, st), "k_rep_stops");
    HIP_TRY(scan.max(P, m, false, st), "scan");
    launches++;
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  info->invert_ms = ev.ms(0, 1);
  const unsigned grid_n = flat_grid(n), grid_m = flat_grid(m);
  for (size_t j = 0; j < k; j++) {
    const uint32_t L = min_len[j];
    fmx_repeat_summary sm{};
    if (L <= m) {
      uint32_t total = 0;
      unsigned long long host[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemsetAsync(res, 0, 64, st), "hipMemsetAsync");
      HIP_TRY(hipMemsetAsync(flag8, 0, n, st), "hipMemsetAsync");
      HIP_TRY(ev.record(2, st), "hipEventRecord");
      HIP_TRY(launch_class_heads(lcp, n, L, A, B, st), "k_rep_heads");
      HIP_TRY(scan.max(A, n, false, st), "scan");
      HIP_TRY(launch_class_max(lcp, sa, A, n, L, B, st), "k_rep_classmax");
      LAUNCH("k_rep_scatter", k_rep_scatter, dim3(grid_n), dim3(kRepThreads), st, lcp, sa, A, B, P, n, L, later, flag8, res);
      HIP_TRY(ev.record(3, st), "hipEventRecord");
      LAUNCH("k_rep_seed", k_rep_seed, dim3(grid_m), dim3(kRepThreads), st, flag8, P, m, L, B);
      HIP_TRY(scan.max(B, m, false, st), "scan");
      LAUNCH("k_rep_bounds", k_rep_bounds, dim3(grid_m), dim3(kRepThreads), st, B, m, L, A, res);
      HIP_TRY(ev.record(4, st), "hipEventRecord");
      HIP_TRY(scan.sum(A, m, false, st), "scan");
      LAUNCH("k_rep_write", k_rep_write, dim3(grid_m), dim3(kRepThreads), st, B, A, m, L, off[j], cap,
             static_cast<unsigned long long *>(d_out));
      HIP_TRY(ev.record(5, st), "hipEventRecord");
      HIP_TRY(hipMemcpyAsync(&total, A + (m - 1), 4, hipMemcpyDeviceToHost, st), "D2H(ranges)");
      HIP_TRY(hipMemcpyAsync(host, res, 32, hipMemcpyDeviceToHost, st), "D2H(summary)");
      HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
      launches += 9;
      info->class_ms += ev.ms(2, 3);
      info->cover_ms += ev.ms(3, 4);
      info->compact_ms += ev.ms(4, 5);
      sm.ranges = total;
      sm.covered_bytes = host[3];
      sm.classes = host[0];
      sm.windows = host[1];
      sm.largest_class = host[2] >> 32;
      sm.largest_class_pos = host[0] ? 0xFFFFFFFFull - (host[2] & 0xFFFFFFFFull) : 0;
    }
    off[j + 1] = off[j] + sm.ranges;
    if (sum) sum[j] = sm;
  }
  std::lock_guard<std::mutex> lk(h->mu);
  h->launches += launches;
  return FMX_OK;
}

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static thread_local RepeatsInfo g_repeats_last;

// What refuses a call before the device is touched; the mode and the stop byte as the kernels take them.
static int repeats_args(const fmx_index *idx, const uint32_t *min_len, size_t k, const fmx_repeat_opts *opts, const void *out_off,
                        const void *out, size_t cap, const size_t *n_out, uint32_t *later, uint32_t *stop) {
  *later = 0;
  *stop = 0;
  if (!idx) return arg_fail("repeats: the handle is null");
  if (!min_len || !out_off || !n_out) return arg_fail("repeats: min_len, out_off or n_out is null");
  if (k == 0 || k > FMX_REPEATS_MAX_LEVELS) return arg_fail("repeats: 1 .. 64 thresholds per call");
  for (size_t j = 0; j < k; j++)
    if (min_len[j] == 0) return arg_fail("repeats: a threshold must be at least 1");
  if (opts) {
    if (opts->mode > FMX_REPEATS_LATER) return arg_fail("fmx_repeat_opts.mode: FMX_REPEATS_ALL or FMX_REPEATS_LATER");
    if (opts->reserved[0] != 0 || opts->reserved[1] != 0 || opts->reserved[2] != 0) return arg_fail("fmx_repeat_opts.reserved must be 0");
    *later = opts->mode;
    *stop = opts->stop;
  }
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("repeats: cap must be below 2^32");
  if (cap && !out) return arg_fail("repeats: out is null");
  return lcp_check(H(idx));
}

extern "C" {

int fmx_repeats_dev(const fmx_index *idx, const uint32_t *min_len, size_t k, const fmx_repeat_opts *opts, void *d_out_off,
                    void *d_out, size_t cap, size_t *n_out, fmx_repeat_summary *summary, void *stream) {
  uint32_t later, stop;
  int rc = repeats_args(idx, min_len, k, opts, d_out_off, d_out, cap, n_out, &later, &stop);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_repeats_dev"))) return rc;
  uint64_t off[FMX_REPEATS_MAX_LEVELS + 1];
  if ((rc = repeats_run(h, min_len, k, later, stop, d_out, cap, st, off, summary, &g_repeats_last))) return rc;
  HIP_TRY(hipMemcpyAsync(d_out_off, off, 8 * (k + 1), hipMemcpyHostToDevice, st), "H2D(offsets)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  *n_out = (size_t)off[k];
  return off[k] > cap ? csr_overflow("repeats", off[k], cap) : FMX_OK;
}

int fmx_repeats(const fmx_index *idx, const uint32_t *min_len, size_t k, const fmx_repeat_opts *opts, uint64_t *out_off,
                fmx_repeat_range *out, size_t cap, size_t *n_out, fmx_repeat_summary *summary) {
  uint32_t later, stop;
  int rc = repeats_args(idx, min_len, k, opts, out_off, out, cap, n_out, &later, &stop);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  fmx_repeat_range *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  const uint64_t outs = sizeof(fmx_repeat_range) * (uint64_t)cap + 16;
  if ((rc = device_room(outs + repeats_need(h, stop != 0), "fmx_repeats"))) return rc;
  DEV_ALLOC(hc.mem, d_out, outs, "repeat ranges");
  uint64_t off[FMX_REPEATS_MAX_LEVELS + 1];
  if ((rc = repeats_run(h, min_len, k, later, stop, d_out, cap, hc.own.s, off, summary, &g_repeats_last))) return rc;
  for (size_t j = 0; j <= k; j++) out_off[j] = off[j];
  *n_out = (size_t)off[k];
  if (off[k] > cap) return csr_overflow("repeats", off[k], cap);
  if ((rc = hc.download(off[k] ? out : nullptr, d_out, sizeof(fmx_repeat_range) * off[k], "D2H(ranges)"))) return rc;
  return hc.sync();
}

int fmx_repeats_last(double *invert_ms, double *class_ms, double *cover_ms, double *compact_ms) {
  if (invert_ms) *invert_ms = g_repeats_last.invert_ms;
  if (class_ms) *class_ms = g_repeats_last.class_ms;
  if (cover_ms) *cover_ms = g_repeats_last.cover_ms;
  if (compact_ms) *compact_ms = g_repeats_last.compact_ms;
  return FMX_OK;
}

}  // extern "C"
