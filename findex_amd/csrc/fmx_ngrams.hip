// fmx_ngrams.hip -- the distinct windows of L bytes of the indexed text and how often each occurs, from the LCP array
// (fmx.h: n-grams).
//
// T, m, s, SA, LCP, window, eligible and class as fmx_repeats.hip has them: the rows whose suffixes share their first L bytes
// are a maximal run of rows with LCP[r] >= L between neighbours.  The run [head, last] IS the suffix-array interval of the
// window, its length the window's count, its largest SA value p the first occurrence t = m - L - p.  A run of ONE row is a
// window only when its suffix has L bytes in front of the sentinel (p + L <= m); exactly min(L, n) rows have not, and each
// of them is a run of its own.
//
// One call: with positions the inversion (SA and s) and, with a stop byte, the stop scan; then per length L (the stops, the
// class heads and the class maxima are fmx_order.h's kernels, shared with fmx_repeats.hip)
//
//   class heads   : A[r] = r + 1 where a run begins (r == 0 or LCP[r - 1] < L), else 0; B[r] = 0.  A max-scan turns A into
//                   (head row of r's run) + 1.
//   class maxima  : (positions only) B[head] = the largest SA of the run, over the runs of two rows and more: a segmented
//                   max over the wave, then one atomicMax per run and wave.  A run of one row has its own SA.
//   k_ng_class    : the last row of a run (LCP[r] < L) knows the size r - head + 1.  It decides whether the run is a window
//                   (p + L <= m; without positions every run passes and the host takes the min(L, n) short rows off the
//                   sums) and eligible (the stop scan), feeds the summary (wave, LDS, one atomic per workgroup; the largest
//                   class as one 64-bit max of count << 32 | ~sp) and the spectrum, and writes S[r] = 1 when the class is
//                   selected (count >= min_count), else 0.  A sum-scan turns S into slot + 1.
//                   The spectrum: singletons are counted per wave by ballot and popcount; counts below FMX_NGRAMS_LDS_BINS
//                   go to a histogram in LDS that is flushed with one global add per bin that is not 0; a count at or above
//                   that bound goes straight to a global 64-bit add -- there are at most n / bound such classes.
//   k_ng_write    : (by row) the selected class of slot j writes its record at out[base + j], below `records` and cap.
//   k_ng_keys     : (by count) K[slot] = (largest - count) << bits(n - 1) | sp, V[slot] = slot, F[slot] = first position; a
//   k_ng_emit       radix sort over the selected classes only, then record i is gathered from pair i.  The key is that of
//                   fmx.h, (0xFFFFFFFF - count) << 32 | sp, less the bits that are the same in every key: fewer passes.
//
// Every pass streams over n rows; every atomic is a max or an integer sum, so the same input gives the same bytes.  Every
// value read from SA is clamped below n and every head to its row: an SA that is no suffix array gives unspecified records,
// never an access outside the buffers.  The host reads each length's summary and selected count before the next begins.
#include <fmx.h>

#include <string>

#include "fmx_order.h"

namespace fmx {

static_assert(sizeof(fmx_ngram_opts) == 32 && sizeof(fmx_ngram) == 24 && sizeof(fmx_ngram_summary) == 64, "fmx.h");
static_assert(FMX_NGRAMS_LDS_BINS >= 2 && FMX_NGRAMS_LDS_BINS <= 4096, "the histogram of one workgroup lives in LDS");

constexpr int kNgThreads = 256;
constexpr uint32_t kNgLdsBins = FMX_NGRAMS_LDS_BINS;
constexpr uint64_t kNgNone = ~0ull;

// What the last row of a run knows of its class
struct NgClass {
  uint32_t head;
  uint64_t size, first;         // first: the smallest t (POS only)
  bool ok;                      // a window, and eligible
};

template <bool POS>
__device__ __forceinline__ NgClass ng_class(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ A,
                                            const uint32_t *__restrict__ B, const uint32_t *__restrict__ P, uint64_t n, uint32_t L,
                                            uint64_t r) {
  NgClass c;
  const uint64_t m = n - 1;
  c.head = min(A[r] - 1u, (uint32_t)r);
  c.size = r - c.head + 1;
  c.first = kNgNone;
  c.ok = true;
  if (POS) {
    const uint64_t p = min(c.size == 1 ? sa[r] : B[c.head], (uint32_t)m);
    c.ok = p + L <= m;
    if (c.ok) {
      c.first = m - L - p;
      if (P != nullptr) c.ok = P[c.first + L - 1] <= c.first;
    }
  }
  return c;
}

// res[0] classes, res[1] windows, res[2] singletons, res[3] max of count << 32 | (0xFFFFFFFF - sp).  Without positions the
// runs of one row are left out of res[3] (which of them are windows is not known) and counted in the others all the same.
// spec: bins 64-bit counters, or null.  The loop's trip count is the same for every lane of a workgroup: all 64 lanes ballot.
template <bool POS>
__global__ __launch_bounds__(kNgThreads) void k_ng_class(const uint32_t *__restrict__ lcp, const uint32_t *__restrict__ sa,
                                                         const uint32_t *__restrict__ A, const uint32_t *__restrict__ B,
                                                         const uint32_t *__restrict__ P, uint64_t n, uint32_t L, uint64_t min_count,
                                                         uint32_t bins, uint32_t *__restrict__ S,
                                                         unsigned long long *__restrict__ spec, unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_cls[kNgThreads / 64], s_win[kNgThreads / 64], s_one[kNgThreads / 64], s_best[kNgThreads / 64];
  __shared__ uint32_t s_hist[kNgLdsBins];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const bool hist = spec != nullptr && bins != 0;
  if (hist) {
    for (uint32_t i = threadIdx.x; i < kNgLdsBins; i += kNgThreads) s_hist[i] = 0u;
    __syncthreads();
  }
  unsigned long long cls = 0, win = 0, one = 0, best = 0;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += stride) {
    const uint64_t r = b + threadIdx.x;
    NgClass c;
    c.ok = false;
    c.size = 0;
    c.head = 0;
    if (r < n && (r == n - 1 || lcp[r] < L)) c = ng_class<POS>(sa, A, B, P, n, L, r);
    if (r < n) S[r] = c.ok && c.size >= min_count ? 1u : 0u;
    const unsigned long long ones = __ballot(c.ok && c.size == 1);
    if (lane == 0) one += (unsigned long long)__popcll(ones);
    if (!c.ok) continue;
    cls += 1;
    win += c.size;
    if (POS || c.size > 1) best = max(best, (unsigned long long)((c.size << 32) | (0xFFFFFFFFull - c.head)));
    if (hist && c.size > 1) {
      const uint32_t bin = c.size < bins ? (uint32_t)c.size : 0u;
      if (c.size < kNgLdsBins) atomicAdd(&s_hist[bin], 1u);
      else atomicAdd(spec + bin, 1ull);
    }
  }
  if (hist && lane == 0 && one) atomicAdd(&s_hist[1u < bins ? 1u : 0u], (uint32_t)one);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cls += (unsigned long long)__shfl_xor(cls, d, 64);
    win += (unsigned long long)__shfl_xor(win, d, 64);
    best = max(best, (unsigned long long)__shfl_xor(best, d, 64));
  }
  if (lane == 0) {
    s_cls[threadIdx.x >> 6] = cls;
    s_win[threadIdx.x >> 6] = win;
    s_one[threadIdx.x >> 6] = one;
    s_best[threadIdx.x >> 6] = best;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kNgThreads / 64; w++) {
      cls += s_cls[w];
      win += s_win[w];
      one += s_one[w];
      best = max(best, s_best[w]);
    }
    if (cls) atomicAdd(res, cls);
    if (win) atomicAdd(res + 1, win);
    if (one) atomicAdd(res + 2, one);
    if (best) atomicMax(res + 3, best);
  }
  if (hist)
    for (uint32_t i = threadIdx.x; i < kNgLdsBins && i < bins; i += kNgThreads) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(spec + i, (unsigned long long)v);
    }
}

// S: the inclusive sum of the select flags, so the selected class whose last row is r has slot S[r] - 1
__device__ __forceinline__ bool ng_slot(const uint32_t *__restrict__ S, uint64_t r, uint32_t *slot) {
  const uint32_t s = S[r], before = r ? S[r - 1] : 0u;
  *slot = s - 1u;
  return s != before;
}

template <bool POS>
__global__ __launch_bounds__(kNgThreads) void k_ng_write(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ A,
                                                         const uint32_t *__restrict__ B, const uint32_t *__restrict__ S, uint64_t n,
                                                         uint32_t L, uint64_t records, uint64_t base, uint64_t cap,
                                                         unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    uint32_t slot;
    if (!ng_slot(S, r, &slot) || slot >= records || base + slot >= cap) continue;
    const NgClass c = ng_class<POS>(sa, A, B, nullptr, n, L, r);
    unsigned long long *o = out + 3 * (base + slot);
    o[0] = c.head;
    o[1] = c.size;
    o[2] = c.first;
  }
}

// selected: the number of slots; F may be null (no positions)
template <bool POS>
__global__ __launch_bounds__(kNgThreads) void k_ng_keys(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ A,
                                                        const uint32_t *__restrict__ B, const uint32_t *__restrict__ S, uint64_t n,
                                                        uint32_t L, uint64_t selected, uint64_t largest, int sp_bits,
                                                        unsigned long long *__restrict__ K, uint32_t *__restrict__ V,
                                                        uint32_t *__restrict__ F) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    uint32_t slot;
    if (!ng_slot(S, r, &slot) || slot >= selected) continue;
    const NgClass c = ng_class<POS>(sa, A, B, nullptr, n, L, r);
    K[slot] = ((unsigned long long)(c.size < largest ? largest - c.size : 0) << sp_bits) | c.head;
    V[slot] = slot;
    if (POS) F[slot] = (uint32_t)c.first;
  }
}

__global__ __launch_bounds__(kNgThreads) void k_ng_emit(const unsigned long long *__restrict__ K, const uint32_t *__restrict__ V,
                                                        const uint32_t *__restrict__ F, uint64_t count, uint64_t selected,
                                                        uint64_t largest, int sp_bits, uint64_t base,
                                                        unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const unsigned long long key = K[i];
    unsigned long long *o = out + 3 * (base + i);
    o[0] = key & ((1ull << sp_bits) - 1);
    o[1] = largest - (key >> sp_bits);
    const uint64_t v = V[i];
    o[2] = F ? (unsigned long long)F[v < selected ? v : selected - 1] : kNgNone;
  }
}

// The rows of the L shortest suffixes, M[step % c * nchk + step / c] for step < L, that are at most L -> flag
__global__ __launch_bounds__(kNgThreads) void k_ng_short_mark(const uint64_t *__restrict__ M, uint64_t L, uint64_t c, uint64_t nchk,
                                                              uint8_t *__restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c * nchk; i += stride) {
    const uint64_t step = (i % nchk) * c + i / nchk, row = M[i];
    if (step < L && row <= L) flag[row] = 1;
  }
}

__global__ __launch_bounds__(kNgThreads) void k_ng_short_mex(const uint8_t *__restrict__ flag, uint64_t L,
                                                             unsigned long long *__restrict__ res) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= L; r += stride)
    if (!flag[r]) atomicMin(res, (unsigned long long)r);
}

// ---------------------------------------------------------------- host side
struct NgramsInfo {
  double invert_ms = 0.0, class_ms = 0.0, select_ms = 0.0, sort_ms = 0.0;
};

struct NgOpts {
  uint32_t order = FMX_NGRAMS_BY_ROW, bins = 0, stop = 0;
  bool pos = true;
  uint64_t min_count = 2, top = 0;
};

// the device bytes a build of the LCP array takes while it runs (lcp_prepare's own sum)
static uint64_t ng_lcp_build_bytes(const Index *h) {
  const uint64_t n = h->n;
  return 4 * n + 4 * n + lcp_text_bytes(n) + lcp_core_bytes(n) + locate_invert_text_bytes(h);
}

// the device bytes ngrams_run allocates before a length's selected classes are known, the inversion's temporaries included
static uint64_t ngrams_bytes(const Index *h, const NgOpts &o) {
  const uint64_t n = h->n;
  uint64_t b = 8 * n + ScanSpace::bytes(n) + 64 + 8 * (uint64_t)o.bins;               // A, S, the scan, the summary, the spectrum
  if (o.pos) b += 4 * n + lcp_text_bytes(n) + 4 * n + (o.stop ? 4 * n : 0) + locate_invert_text_bytes(h);   // SA, s, B, P
  return b;
}

// ... and the sort's, for `sel` selected classes
static uint64_t ngrams_sort_bytes(uint64_t sel, bool pos) { return SortSpace::bytes(sel) + (pos ? 4 * sel : 0); }

static uint64_t ngrams_need(const Index *h, const NgOpts &o) {
  const uint64_t own = ngrams_bytes(h, o);
  bool built;
  {
    std::lock_guard<std::mutex> lk(h->lcp.mu);
    built = h->lcp.ready;
  }
  return built ? own : std::max(own + 4 * h->n, ng_lcp_build_bytes(h));
}

// Without positions and without a class of two windows: the largest class is a singleton, the one of the smallest row whose
// suffix has L bytes.  The L rows that have not are row 0 and its first L - 1 LF images: a walk of L - 1 dependent steps, run as
// ceil(L / c) walks of c steps one after the other (c about sqrt(L)) and then c - 1 launches that step every walk's start once.
static int ngrams_first_long_row(const Index *h, uint64_t L, hipStream_t st, uint64_t *row, uint64_t *launches) {
  uint64_t c = 1;
  while (c * c < L) c++;
  const uint64_t nchk = (L + c - 1) / c;
  int rc = device_room(8 * c * nchk + L + 1 + 8, "fmx_ngrams");
  if (rc) return rc;
  DevMem mem;
  uint64_t *M = nullptr;
  uint8_t *flag = nullptr;
  unsigned long long *best = nullptr;
  DEV_ALLOC(mem, M, 8 * c * nchk, "ngrams short rows");
  DEV_ALLOC(mem, flag, L + 1, "ngrams short rows");
  DEV_ALLOC(mem, best, 8, "ngrams short rows");
  HIP_TRY(hipMemsetAsync(M, 0, 8 * c * nchk, st), "hipMemsetAsync");
  HIP_TRY(hipMemsetAsync(flag, 0, L + 1, st), "hipMemsetAsync");
  HIP_TRY(hipMemsetAsync(best, 0xFF, 8, st), "hipMemsetAsync");
  for (uint64_t i = 0; i + 1 < nchk; i++) HIP_TRY(launch_lf_walk(h, M + i, 1, (uint32_t)c, nullptr, M + i + 1, st), "k_lf_walk");
  for (uint64_t j = 0; j + 1 < c && j + 1 < L; j++) {
    const uint64_t walks = (L - j - 1 + c - 1) / c;             // the starts i with i c + j + 1 < L
    HIP_TRY(launch_lf_walk(h, M + j * nchk, walks, 1, nullptr, M + (j + 1) * nchk, st), "k_lf_walk");
  }
  LAUNCH("k_ng_short_mark", k_ng_short_mark, dim3(flat_grid(c * nchk)), dim3(kNgThreads), st, M, L, c, nchk, flag);
  LAUNCH("k_ng_short_mex", k_ng_short_mex, dim3(flat_grid(L + 1)), dim3(kNgThreads), st, flag, L, best);
  unsigned long long got = 0;
  HIP_TRY(hipMemcpyAsync(&got, best, 8, hipMemcpyDeviceToHost, st), "D2H(short rows)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  *row = got;
  *launches += nchk + c + 1;
  return FMX_OK;
}

// The whole call on `st`, records in device memory: off[k + 1] (host), sum[k] (host, may be null) and spectrum[k * bins] (host)
// are filled, d_out gets the records below cap.  Allocates, synchronises `st`, frees its temporaries on every path.
static int ngrams_run(const Index *h, const uint32_t *lengths, size_t k, const NgOpts &o, void *d_out, uint64_t cap, hipStream_t st,
                      uint64_t *off, fmx_ngram_summary *sum, uint64_t *spectrum, NgramsInfo *info) {
  *info = NgramsInfo{};
  const uint64_t n = h->n, m = n - 1;
  off[0] = 0;
  bool any = false;
  for (size_t j = 0; j < k; j++) any = any || lengths[j] <= m;
  for (size_t j = 0; j < k && o.bins; j++) std::fill(spectrum + j * o.bins, spectrum + (j + 1) * o.bins, 0ull);
  if (!any) {                                                  // every length is longer than the text
    for (size_t j = 0; j < k; j++) {
      off[j + 1] = 0;
      if (sum) {
        sum[j] = fmx_ngram_summary{};
        if (!o.pos) sum[j].largest_pos = kNgNone;
      }
    }
    return FMX_OK;
  }
  int rc = device_room(ngrams_need(h, o), "fmx_ngrams");
  if (rc) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, st))) return rc;
  const uint32_t *lcp = static_cast<const uint32_t *>(h->lcp.lcp);
  Events<8> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  uint32_t *sa = nullptr, *A = nullptr, *B = nullptr, *S = nullptr, *P = nullptr;
  ScanSpace scan;
  uint8_t *s = nullptr;
  unsigned long long *res = nullptr, *spec = nullptr;
  DEV_ALLOC(mem, A, 4 * n, "ngrams classes");
  DEV_ALLOC(mem, S, 4 * n, "ngrams slots");
  if ((rc = scan.alloc(mem, n, "ngrams scan"))) return rc;
  DEV_ALLOC(mem, res, 64, "ngrams summary");
  if (o.bins) DEV_ALLOC(mem, spec, 8 * (uint64_t)o.bins, "ngrams spectrum");
  uint64_t launches = 0;
  if (o.pos) {
    DEV_ALLOC(mem, sa, 4 * n, "ngrams suffix array");
    DEV_ALLOC(mem, s, lcp_text_bytes(n), "ngrams text");
    DEV_ALLOC(mem, B, 4 * n, "ngrams classes");
    if (o.stop) DEV_ALLOC(mem, P, 4 * n, "ngrams stop scan");
    HIP_TRY(ev.record(0, st), "hipEventRecord");
    HIP_TRY(hipMemsetAsync(s, 0, lcp_text_bytes(n), st), "hipMemsetAsync");
    if ((rc = locate_invert_text(h, st, sa, s))) return rc;
    if (o.stop) {
      HIP_TRY(launch_stops(s, m, o.stop, P, st), "k_ng_stops");
      HIP_TRY(scan.max(P, m, false, st), "scan");
      launches++;
    }
    HIP_TRY(ev.record(1, st), "hipEventRecord");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    info->invert_ms = ev.ms(0, 1);
  }
  const unsigned grid_n = flat_grid(n);
  const int sp_bits = bits_for(n - 1);
  unsigned long long *out = static_cast<unsigned long long *>(d_out);
  for (size_t j = 0; j < k; j++) {
    const uint32_t L = lengths[j];
    fmx_ngram_summary sm{};
    if (!o.pos) sm.largest_pos = kNgNone;
    if (L <= m) {
      uint32_t selected = 0;
      unsigned long long host[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemsetAsync(res, 0, 64, st), "hipMemsetAsync");
      if (o.bins) HIP_TRY(hipMemsetAsync(spec, 0, 8 * (uint64_t)o.bins, st), "hipMemsetAsync");
      HIP_TRY(ev.record(2, st), "hipEventRecord");
      HIP_TRY(launch_class_heads(lcp, n, L, A, B, st), "k_ng_heads");
      HIP_TRY(scan.max(A, n, false, st), "scan");
      if (o.pos) {
        HIP_TRY(launch_class_max(lcp, sa, A, n, L, B, st), "k_ng_classmax");
        LAUNCH("k_ng_class", k_ng_class<true>, dim3(grid_n), dim3(kNgThreads), st, lcp, sa, A, B, P, n, L, o.min_count, o.bins, S, spec, res);
      } else {
        LAUNCH("k_ng_class", k_ng_class<false>, dim3(grid_n), dim3(kNgThreads), st, lcp, sa, A, B, P, n, L, o.min_count, o.bins, S, spec, res);
      }
      HIP_TRY(ev.record(3, st), "hipEventRecord");
      HIP_TRY(scan.sum(S, n, false, st), "scan");
      HIP_TRY(ev.record(4, st), "hipEventRecord");
      HIP_TRY(hipMemcpyAsync(&selected, S + (n - 1), 4, hipMemcpyDeviceToHost, st), "D2H(selected)");
      HIP_TRY(hipMemcpyAsync(host, res, 32, hipMemcpyDeviceToHost, st), "D2H(summary)");
      if (o.bins) HIP_TRY(hipMemcpyAsync(spectrum + j * o.bins, spec, 8 * (uint64_t)o.bins, hipMemcpyDeviceToHost, st), "D2H(spectrum)");
      HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
      launches += o.pos ? 7 : 6;
      info->class_ms += ev.ms(2, 3);
      info->select_ms += ev.ms(3, 4);
      // ---- the summary; without positions the L rows whose suffixes are shorter than L passed as singletons
      const uint64_t shorts = o.pos ? 0 : L;
      sm.selected = selected;
      sm.records = o.top ? std::min<uint64_t>(o.top, selected) : selected;
      sm.distinct = host[0] - shorts;
      sm.windows = host[1] - shorts;
      sm.singletons = host[2] - shorts;
      if (o.bins && shorts) spectrum[j * o.bins + (o.bins > 1 ? 1 : 0)] -= shorts;
      uint64_t largest = host[3] >> 32, largest_sp = 0xFFFFFFFFull - (host[3] & 0xFFFFFFFFull);
      if (!host[3] && sm.distinct) {                           // (without positions: nothing occurs twice)
        largest = 1;
        if ((rc = ngrams_first_long_row(h, L, st, &largest_sp, &launches))) return rc;
      }
      if (sm.distinct) {
        sm.largest_count = largest;
        sm.largest_sp = largest_sp;
        if (o.pos) {
          uint32_t p = 0;
          HIP_TRY(hipMemcpyAsync(&p, (largest == 1 ? sa : B) + std::min<uint64_t>(largest_sp, m), 4, hipMemcpyDeviceToHost, st), "D2H(largest)");
          HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
          sm.largest_pos = (uint64_t)p + L <= m ? m - L - p : 0;
        }
      }
      // ---- the records
      const uint64_t base = off[j];
      const uint64_t room = cap > base ? cap - base : 0, writes = std::min(sm.records, room);
      if (writes && o.order == FMX_NGRAMS_BY_ROW) {
        HIP_TRY(ev.record(5, st), "hipEventRecord");
        if (o.pos) LAUNCH("k_ng_write", k_ng_write<true>, dim3(grid_n), dim3(kNgThreads), st, sa, A, B, S, n, L, sm.records, base, cap, out);
        else LAUNCH("k_ng_write", k_ng_write<false>, dim3(grid_n), dim3(kNgThreads), st, sa, A, B, S, n, L, sm.records, base, cap, out);
        HIP_TRY(ev.record(6, st), "hipEventRecord");
        HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
        launches++;
        info->select_ms += ev.ms(5, 6);
      } else if (writes) {
        const uint64_t sel = selected;
        if ((rc = device_room(ngrams_sort_bytes(sel, o.pos), "fmx_ngrams (the sort)"))) return rc;
        DevMem sortmem;
        SortSpace ws;
        uint32_t *F = nullptr;
        if ((rc = ws.alloc(sortmem, sel, "ngrams sort"))) return rc;
        if (o.pos) DEV_ALLOC(sortmem, F, 4 * sel, "ngrams first positions");
        HIP_TRY(ev.record(5, st), "hipEventRecord");
        if (o.pos) LAUNCH("k_ng_keys", k_ng_keys<true>, dim3(grid_n), dim3(kNgThreads), st, sa, A, B, S, n, L, sel, largest, sp_bits, ws.keys(), ws.vals(), F);
        else LAUNCH("k_ng_keys", k_ng_keys<false>, dim3(grid_n), dim3(kNgThreads), st, sa, A, B, S, n, L, sel, largest, sp_bits, ws.keys(), ws.vals(), F);
        HIP_TRY(ev.record(6, st), "hipEventRecord");
        const int bits = sp_bits + bits_for(largest - std::min<uint64_t>(o.min_count, largest));
        HIP_TRY(ws.sort(sel, bits, st), "radix sort");
        HIP_TRY(ev.record(7, st), "hipEventRecord");
        LAUNCH("k_ng_emit", k_ng_emit, dim3(flat_grid(writes)), dim3(kNgThreads), st, ws.keys(), ws.vals(), F, writes, sel, largest,
               sp_bits, base, out);
        HIP_TRY(ev.record(0, st), "hipEventRecord");                    // (the inversion's pair of events is free by now)
        HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");      // the sort's buffers go with this block
        launches += 2 + 3 * (uint64_t)ws.passes;
        info->select_ms += ev.ms(5, 6) + ev.ms(7, 0);
        info->sort_ms += ev.ms(6, 7);
      }
    }
    off[j + 1] = off[j] + sm.records;
    if (sum) sum[j] = sm;
  }
  std::lock_guard<std::mutex> lk(h->mu);
  h->launches += launches;
  return FMX_OK;
}

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static thread_local NgramsInfo g_ngrams_last;

// What refuses a call before the device is touched; the options as the kernels take them.
static int ngrams_args(const fmx_index *idx, const uint32_t *lengths, size_t k, const fmx_ngram_opts *opts, const void *out_off,
                       const void *out, size_t cap, const size_t *n_out, const uint64_t *spectrum, NgOpts *o) {
  *o = NgOpts{};
  if (!idx) return arg_fail("ngrams: the handle is null");
  if (!lengths || !out_off || !n_out) return arg_fail("ngrams: lengths, out_off or n_out is null");
  if (k == 0 || k > FMX_NGRAMS_MAX_LEVELS) return arg_fail("ngrams: 1 .. 64 lengths per call");
  for (size_t j = 0; j < k; j++)
    if (lengths[j] == 0) return arg_fail("ngrams: a length must be at least 1");
  if (opts) {
    if (opts->order > FMX_NGRAMS_BY_COUNT) return arg_fail("fmx_ngram_opts.order: FMX_NGRAMS_BY_ROW or FMX_NGRAMS_BY_COUNT");
    if (opts->flags & ~FMX_NGRAMS_NO_POS) return arg_fail("fmx_ngram_opts.flags: FMX_NGRAMS_NO_POS is the only flag");
    if (opts->min_count == 0) return arg_fail("fmx_ngram_opts.min_count must be at least 1");
    if ((opts->flags & FMX_NGRAMS_NO_POS) && (opts->stop != 0 || opts->min_count < 2))
      return arg_fail("FMX_NGRAMS_NO_POS: only without a stop byte and with min_count >= 2");
    if (opts->spectrum_bins > FMX_NGRAMS_MAX_BINS) return arg_fail("fmx_ngram_opts.spectrum_bins: at most 65536");
    if (opts->spectrum_bins != 0 && !spectrum) return arg_fail("ngrams: spectrum_bins without a spectrum");
    if (opts->reserved[0] != 0 || opts->reserved[1] != 0 || opts->reserved[2] != 0) return arg_fail("fmx_ngram_opts.reserved must be 0");
    o->order = opts->order;
    o->pos = !(opts->flags & FMX_NGRAMS_NO_POS);
    o->min_count = opts->min_count;
    o->top = opts->top;
    o->bins = opts->spectrum_bins;
    o->stop = opts->stop;
  }
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("ngrams: cap must be below 2^32");
  if (cap && !out) return arg_fail("ngrams: out is null");
  return lcp_check(H(idx));
}

extern "C" {

int fmx_ngrams_dev(const fmx_index *idx, const uint32_t *lengths, size_t k, const fmx_ngram_opts *opts, void *d_out_off, void *d_out,
                   size_t cap, size_t *n_out, fmx_ngram_summary *summary, uint64_t *spectrum, void *stream) {
  NgOpts o;
  int rc = ngrams_args(idx, lengths, k, opts, d_out_off, d_out, cap, n_out, spectrum, &o);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_ngrams_dev"))) return rc;
  uint64_t off[FMX_NGRAMS_MAX_LEVELS + 1];
  if ((rc = ngrams_run(h, lengths, k, o, d_out, cap, st, off, summary, spectrum, &g_ngrams_last))) return rc;
  HIP_TRY(hipMemcpyAsync(d_out_off, off, 8 * (k + 1), hipMemcpyHostToDevice, st), "H2D(offsets)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  *n_out = (size_t)off[k];
  return off[k] > cap ? csr_overflow("ngrams", off[k], cap) : FMX_OK;
}

int fmx_ngrams(const fmx_index *idx, const uint32_t *lengths, size_t k, const fmx_ngram_opts *opts, uint64_t *out_off, fmx_ngram *out,
               size_t cap, size_t *n_out, fmx_ngram_summary *summary, uint64_t *spectrum) {
  NgOpts o;
  int rc = ngrams_args(idx, lengths, k, opts, out_off, out, cap, n_out, spectrum, &o);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  fmx_ngram *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  const uint64_t outs = sizeof(fmx_ngram) * (uint64_t)cap + 16;
  if ((rc = device_room(outs + ngrams_need(h, o), "fmx_ngrams"))) return rc;
  DEV_ALLOC(hc.mem, d_out, outs, "ngram records");
  uint64_t off[FMX_NGRAMS_MAX_LEVELS + 1];
  if ((rc = ngrams_run(h, lengths, k, o, d_out, cap, hc.own.s, off, summary, spectrum, &g_ngrams_last))) return rc;
  for (size_t j = 0; j <= k; j++) out_off[j] = off[j];
  *n_out = (size_t)off[k];
  if (off[k] > cap) return csr_overflow("ngrams", off[k], cap);
  if ((rc = hc.download(off[k] ? out : nullptr, d_out, sizeof(fmx_ngram) * off[k], "D2H(records)"))) return rc;
  return hc.sync();
}

int fmx_ngrams_last(double *invert_ms, double *class_ms, double *select_ms, double *sort_ms) {
  if (invert_ms) *invert_ms = g_ngrams_last.invert_ms;
  if (class_ms) *class_ms = g_ngrams_last.class_ms;
  if (select_ms) *select_ms = g_ngrams_last.select_ms;
  if (sort_ms) *sort_ms = g_ngrams_last.sort_ms;
  return FMX_OK;
}

}  // extern "C"
