// fmx_sufsort.hip -- index construction: text -> suffix array -> BWT + EOF row + counts, on the device.
//
// The reference builds its BWT with BWTMerger2.merge over a FileBWTReader (bwtmerger.scala:654-1261): the input file is
// reversed (copyReverse, :1106-1108), sorted block by block and merged on disk, and sa2BWT (:782-810) writes row i as the
// byte before suffix SA[i], with the row of the whole string (the EOF row) filled by a neighbour's byte.  Here the whole
// string s = reverse(text) + 0 is suffix-sorted in HBM by prefix doubling:
//
//   round 1  : every suffix keyed by its first 8 bytes (big-endian u64, 0 past the end), one LSD radix sort -> h = 8.
//              0 is the unique smallest symbol, so a suffix whose first 8 bytes reach the sentinel is already alone.
//   round r  : only the suffixes still in groups of two or more (the ACTIVE list, in SA order) are re-sorted, keyed by
//              (rank[i], rank[i + h]) packed into 2 * ceil(log2 n) bits; rank[i] is the SA position of the head of i's
//              group, so an active group occupies the same SA positions before and after its members are re-sorted.
//              Then the new group heads are flagged, max-scanned and scattered into rank[], singletons leave the list.
//   emit     : bwt[j] = s[sa[j] - 1]; the row with sa[j] == 0 is eof; the 256-entry histogram of the text.
//
// The radix sort and the scans are fmx_order.h's (SortSpace).  Everything is u32 index / u64 key; a loop index is u64, so
// positions >= 2^31 stay unsigned throughout.
//
// Working set (bytes per suffix, n = len + 1): s (1) + sa (4) + rank (4) + two key buffers (16) + two value buffers (8)
// + the active list (4) = 37, plus the digit histograms (1/4) and the scan partials (< 1/500).  The host-pointer entry
// points add the text and the BWT in HBM (2).  No library sort, no host sort.
#include <fmx.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fmx_order.h"

namespace fmx {

constexpr int kSaThreads = 256;

static unsigned sa_grid(uint64_t m) {
  const uint64_t b = (m + kSaThreads - 1) / kSaThreads;
  return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

// s[j] = text[len - 1 - j], s[len .. len + 7] = 0 (the sentinel and the padding the first-round keys read);
// *zero != 0 when the text holds a 0 byte.
__global__ __launch_bounds__(kSaThreads) void k_sa_reverse(const uint8_t *__restrict__ text, uint64_t len,
                                                           uint8_t *__restrict__ s, uint32_t *__restrict__ zero) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool z = false;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < len + 8; j += stride) {
    if (j < len) {
      const uint8_t c = text[len - 1 - j];
      z |= c == 0;
      s[j] = c;
    } else {
      s[j] = 0;
    }
  }
  if (z) atomicOr(zero, 1u);
}

// round 1: key = s[i .. i + 7] big-endian, value = i
__global__ __launch_bounds__(kSaThreads) void k_sa_init(const uint8_t *__restrict__ s, uint64_t n,
                                                        unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    unsigned long long k = 0;
    for (int t = 0; t < 8; t++) k = (k << 8) | s[i + t];
    key[i] = k;
    val[i] = (uint32_t)i;
  }
}

// round r: active suffix i = sa[ap[k]] keyed by (rank[i], rank[i + h]); i + h < n for every active suffix (a suffix whose
// h-prefix reaches the sentinel is alone in its group), the bound below only keeps a broken invariant in bounds
__global__ __launch_bounds__(kSaThreads) void k_sa_keys(const uint32_t *__restrict__ ap, uint64_t m,
                                                        const uint32_t *__restrict__ sa, const uint32_t *__restrict__ rank,
                                                        uint64_t n, uint64_t h, int bits,
                                                        unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const uint32_t i = sa[ap[k]];
    const uint64_t i2 = (uint64_t)i + h;
    const uint32_t r2 = i2 < n ? rank[i2] : 0u;
    key[k] = ((unsigned long long)rank[i] << bits) | r2;
    val[k] = i;
  }
}

// ---- group heads and ranks
__device__ __forceinline__ bool sa_head(const unsigned long long *key, uint64_t k) { return k == 0 || key[k] != key[k - 1]; }

__global__ __launch_bounds__(kSaThreads) void k_sa_heads(const unsigned long long *__restrict__ key, uint64_t m,
                                                         uint32_t *__restrict__ hp) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride)
    hp[k] = sa_head(key, k) ? (uint32_t)k : 0u;
}

// hp: the max-scanned heads (index of k's group head in the sorted list).  ap == nullptr in round 1 (the list is all of
// SA, position k).  Writes sa and rank; keep[k] = 1 when k's group has two members or more.
__global__ __launch_bounds__(kSaThreads) void k_sa_rank(const unsigned long long *__restrict__ key,
                                                        const uint32_t *__restrict__ val, const uint32_t *__restrict__ hp,
                                                        const uint32_t *__restrict__ ap, uint64_t m,
                                                        uint32_t *__restrict__ sa, uint32_t *__restrict__ rank,
                                                        uint32_t *__restrict__ keep) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const uint32_t i = val[k];
    const uint32_t pos = ap ? ap[k] : (uint32_t)k;
    sa[pos] = i;
    rank[i] = ap ? ap[hp[k]] : hp[k];
    const bool single = sa_head(key, k) && (k + 1 == m || key[k + 1] != key[k]);
    keep[k] = single ? 0u : 1u;
  }
}

// incl: the inclusive sum of keep; the kept SA positions move to the front of the next active list, in order
__global__ __launch_bounds__(kSaThreads) void k_sa_compact(const uint32_t *__restrict__ incl, const uint32_t *__restrict__ ap,
                                                           uint64_t m, uint32_t *__restrict__ ap_next) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const uint32_t before = k ? incl[k - 1] : 0u;
    if (incl[k] != before) ap_next[before] = ap ? ap[k] : (uint32_t)k;
  }
}

// ---- the BWT: bwt[j] = s[sa[j] - 1], eof = the row with sa[j] == 0, counts = the histogram of the other rows
__global__ __launch_bounds__(kSaThreads) void k_sa_emit(const uint8_t *__restrict__ s, const uint32_t *__restrict__ sa,
                                                        uint64_t n, uint8_t *__restrict__ bwt,
                                                        unsigned long long *__restrict__ out /* [0] eof, [1..256] counts */) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    const uint32_t p = sa[j];
    if (p == 0) {
      out[0] = j;
    } else {
      const uint8_t c = s[p - 1];
      bwt[j] = c;
      atomicAdd(&h[c], 1u);
    }
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&out[1 + threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// the EOF row's filler, sa2BWT (bwtmerger.scala:799-806): the byte of the row above, of the row below for eof == 0
__global__ void k_sa_eof_fill(const uint8_t *__restrict__ s, const uint32_t *__restrict__ sa, uint64_t n,
                              uint8_t *__restrict__ bwt, const unsigned long long *__restrict__ out) {
  const uint64_t e = out[0];
  if (e >= n || n < 2) return;
  const uint32_t q = e > 0 ? sa[e - 1] : sa[1];
  bwt[e] = q ? s[q - 1] : 0;
}

// ---- host side
namespace {

// FMX_SUFSORT_LOG=<file>: one JSON line per construction appended to the file (tools/build_text_bench.py reads it)
struct RoundLog { uint64_t h, active; int passes; float ms; double bytes; };

void write_log(const char *path, uint64_t n, double alloc_ms, double total_ms, const std::vector<RoundLog> &rounds,
               uint64_t peak) {
  FILE *f = std::fopen(path, "a");
  if (!f) return;
  std::fprintf(f, "{\"n\": %llu, \"peak_bytes\": %llu, \"alloc_ms\": %.3f, \"total_ms\": %.3f, \"rounds\": [",
               (unsigned long long)n, (unsigned long long)peak, alloc_ms, total_ms);
  for (size_t r = 0; r < rounds.size(); r++)
    std::fprintf(f, "%s{\"h\": %llu, \"active\": %llu, \"passes\": %d, \"kernel_ms\": %.3f, \"bytes\": %.0f}", r ? ", " : "",
                 (unsigned long long)rounds[r].h, (unsigned long long)rounds[r].active, rounds[r].passes, rounds[r].ms,
                 rounds[r].bytes);
  std::fprintf(f, "]}\n");
  std::fclose(f);
}

// Modelled bytes of one round over m keys with `passes` radix passes (what the kernels read and write once each):
// keys/init 24 m, per pass hist 8 m + scatter 24 m, heads 12 m, scans ~16 m, rank 28 m, compact 12 m.
double round_bytes(uint64_t m, int passes, bool first) {
  return (double)m * ((first ? 21.0 : 24.0) + 32.0 * passes + 12.0 + 16.0 + 28.0 + 12.0);
}

}  // namespace

uint64_t sufsort_peak_bytes(uint64_t len, bool sa_given) {
  const uint64_t n = len + 1;
  // s, sa, rank, the active list, the sort's workspace, the results
  return (n + 8) + (sa_given ? 0 : 4 * n) + 4 * n + 4 * n + SortSpace::bytes(n) + 8 * 257 + 4096;
}

// The construction proper (include/fmx.h, fmx_bwt_from_text_dev): d_text[len] -> d_bwt[len + 1], eof, counts, and the
// suffix array of s into d_sa when it is given.  Arguments are checked by the caller; `extra` device bytes the caller
// still has to allocate are counted in the free-memory check.  Synchronises `st`.
int sufsort_bwt(const void *d_text, uint64_t len, void *d_bwt, void *d_sa_user, uint64_t *eof, int64_t counts[256],
                hipStream_t st, uint64_t extra) {
  const uint64_t n = len + 1;
  const uint64_t peak = sufsort_peak_bytes(len, d_sa_user != nullptr);
  if (const int rc = device_room(peak + extra, "suffix sort of " + std::to_string(len) + " bytes")) return rc;
  const char *log_path = std::getenv("FMX_SUFSORT_LOG");
  const auto t0 = std::chrono::steady_clock::now();
  DevMem mem;
  uint8_t *s = nullptr;
  uint32_t *sa = nullptr, *rank = nullptr, *ap = nullptr, *flag = nullptr;
  unsigned long long *out = nullptr;
  SortSpace ws;
  DEV_ALLOC(mem, s, n + 8, "suffix sort");
  if (d_sa_user) sa = static_cast<uint32_t *>(d_sa_user);
  else DEV_ALLOC(mem, sa, 4 * n, "suffix sort");
  DEV_ALLOC(mem, rank, 4 * n, "suffix sort");
  DEV_ALLOC(mem, ap, 4 * n, "suffix sort");
  if (const int rc = ws.alloc(mem, n, "suffix sort")) return rc;
  DEV_ALLOC(mem, out, 8 * 257 + 8, "suffix sort");
  flag = reinterpret_cast<uint32_t *>(out + 257);
  const double alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const char *const launch = "suffix sort kernel launch";
  const dim3 block(kSaThreads);
  Events<2> ev;
  if (log_path) HIP_TRY(ev.create(), "hipEventCreate");
  std::vector<RoundLog> rounds;
  HIP_TRY(hipMemsetAsync(out, 0, 8 * 257 + 8, st), "hipMemsetAsync");
  LAUNCH(launch, k_sa_reverse, dim3(sa_grid(n + 8)), block, st, static_cast<const uint8_t *>(d_text), len, s, flag);
  uint32_t zero = 0;
  HIP_TRY(hipMemcpyAsync(&zero, flag, 4, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (zero) {
    set_error("the text contains byte 0 (findex's readers escape it; counts[0] must be 0)");
    return FMX_ERR_UNSUPPORTED;
  }
  const int bits = bits_for(n - 1);           // significant bits of a rank
  uint64_t m = n, h = 0;
  uint32_t *list = nullptr;                   // the active list (SA positions); nullptr in round 1: all of them
  while (m > 0) {
    if (log_path) HIP_TRY(ev.record(0, st), "hipEventRecord");
    const dim3 grid(sa_grid(m));
    if (h == 0) LAUNCH(launch, k_sa_init, grid, block, st, s, n, ws.keys(), ws.vals());
    else LAUNCH(launch, k_sa_keys, grid, block, st, list, m, sa, rank, n, h, bits, ws.keys(), ws.vals());
    HIP_TRY(ws.sort(m, h == 0 ? 64 : 2 * bits, st), "radix sort");
    // the free key buffer holds the heads (first m u32) and the keep flags (next m u32)
    uint32_t *hp = reinterpret_cast<uint32_t *>(ws.free_keys()), *keep = hp + m;
    LAUNCH(launch, k_sa_heads, grid, block, st, ws.keys(), m, hp);
    HIP_TRY(ws.scan().max(hp, m, false, st), "scan");
    LAUNCH(launch, k_sa_rank, grid, block, st, ws.keys(), ws.vals(), hp, list, m, sa, rank, keep);
    HIP_TRY(ws.scan().sum(keep, m, false, st), "scan");
    // the next list goes to the free value buffer
    uint32_t *next = ws.free_vals();
    LAUNCH(launch, k_sa_compact, grid, block, st, keep, list, m, next);
    uint32_t m_next = 0;
    HIP_TRY(hipMemcpyAsync(&m_next, keep + (m - 1), 4, hipMemcpyDeviceToHost, st), "D2H");
    if (log_path) HIP_TRY(ev.record(1, st), "hipEventRecord");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (log_path) rounds.push_back({h == 0 ? 8 : 2 * h, m, ws.passes, ev.ms(0, 1), round_bytes(m, ws.passes, h == 0)});
    if ((uint64_t)m_next >= m && h != 0) {    // a round that separates nothing would loop for ever
      set_error("suffix sort made no progress (internal error)");
      return FMX_ERR_HIP;
    }
    // ... and the old list's buffer becomes a value buffer in its place
    list = ap = ws.trade_free_vals(ap);
    m = m_next;
    h = h == 0 ? 8 : 2 * h;
  }
  LAUNCH(launch, k_sa_emit, dim3(sa_grid(n)), block, st, s, sa, n, static_cast<uint8_t *>(d_bwt), out);
  LAUNCH(launch, k_sa_eof_fill, dim3(1), dim3(1), st, s, sa, n, static_cast<uint8_t *>(d_bwt), out);
  unsigned long long host_out[257];
  HIP_TRY(hipMemcpyAsync(host_out, out, sizeof host_out, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  *eof = host_out[0];
  for (int c = 0; c < 256; c++) counts[c] = (int64_t)host_out[1 + c];
  if (log_path)
    write_log(log_path, n, alloc_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
              rounds, peak);
  return FMX_OK;
}

}  // namespace fmx
