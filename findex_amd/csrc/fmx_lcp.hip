// fmx_lcp.hip -- the LCP array of s = reverse(text) + sentinel on the device.
//
// LCP[r] = length of the longest common prefix of the suffixes of rows r and r + 1 (r < n - 1), LCP[n - 1] = 0: a row is
// paired with the row BELOW it, the convention of Util.bwtFm2LCP (util.scala:153-212) and LCPCreator (bwtmerger.scala:
// 558-652).  The reference fills the array with one sequential Kasai loop; here it is the Phi algorithm of Kärkkäinen,
// Manzini and Puglisi with the successor in place of the predecessor, so that the row convention needs no shift:
//
//   k_lcp_phi    : phi[SA[r]] = SA[r + 1] (r < n - 1), kNone for SA[n - 1]: n random 4-byte stores.
//   k_lcp_plcp   : in TEXT order, plcp[i] = lcp(s[i..], s[phi[i]..]), written over phi[i].  The successor of i + 1 shares at
//                  least plcp[i] - 1 bytes with it (the suffixes i + 1 and phi[i] + 1 share that many and the successor lies
//                  between them), so a lane that takes consecutive positions carries h from one to the next and compares
//                  from there: a lane takes a run of kRun positions and keeps it in registers; only the run's first
//                  position is compared from nothing.  A comparison takes 8 bytes of either side per step.  (Two forms
//                  that compare fewer positions from nothing -- the run starts computed first by a kernel of their own,
//                  and several runs in a row per lane -- measured slower on text: DESIGN.md §13.)
//   k_lcp_gather : LCP[r] = plcp[SA[r]], LCP[n - 1] = 0, and in the same pass the largest entry with the first row that
//                  holds it (one 64-bit atomicMax of lcp << 32 | ~row per workgroup) and the sum of all entries.
//
// Separate launches on the caller's stream; no workgroup waits for another.  Every value read from SA or phi is clamped
// below n before it becomes an address, and a comparison stops at the end of s whatever the bytes say: an SA that is no
// suffix array gives unspecified values, never an access outside the buffers.  Inputs with long repeats are correct and
// terminate but are not fast: a run of one letter of length n costs about n^2 / 256 steps of 8 bytes (n / kRun comparisons
// from nothing, n / 2 bytes each on average).
#include <fmx.h>

#include <chrono>
#include <string>

#include "fmx_host.h"

namespace fmx {

constexpr int kLcpThreads = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kRun = 16;                        // positions per lane in k_lcp_plcp: four 16-byte loads and stores of phi / plcp
constexpr uint64_t kTextPad = 16;               // readable zero bytes behind s (an 8-byte load may begin at n - 1)

static unsigned lcp_grid(int cu_count, uint64_t work) {
  uint64_t want = (work + kLcpThreads - 1) / kLcpThreads;
  const uint64_t cap = (uint64_t)(cu_count > 0 ? cu_count : 256) * 32;
  if (want < 1) want = 1;
  return (unsigned)(want < cap ? want : cap);
}

// s[j] = text[len - 1 - j], zeros from s[len] (the sentinel) to the end of the padding
__global__ __launch_bounds__(kLcpThreads) void k_lcp_reverse(const uint8_t *__restrict__ text, uint64_t len, uint8_t *__restrict__ s) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < len + 1 + kTextPad; j += stride)
    s[j] = j < len ? text[len - 1 - j] : (uint8_t)0;
}

__global__ __launch_bounds__(kLcpThreads) void k_lcp_phi(const uint32_t *__restrict__ sa, uint64_t n, uint32_t *__restrict__ phi) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t last = (uint32_t)(n - 1);
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    const uint32_t a = min(sa[r], last);
    phi[a] = r + 1 < n ? sa[r + 1] : kNone;
  }
}

__device__ __forceinline__ unsigned long long load8(const uint8_t *p) {
  unsigned long long x;
  __builtin_memcpy(&x, p, 8);
  return x;
}

// lcp(s[a..], s[b..]) given that the first h bytes are equal; never reads at or behind s[n + 8] and never answers more
// than n - max(a, b).  b == kNone (no successor) or out of range: 0.
__device__ __forceinline__ uint32_t lcp_extend(const uint8_t *__restrict__ s, uint64_t n, uint32_t a, uint32_t b, uint32_t h) {
  if (b >= n) return 0;
  const uint64_t room = n - max(a, b);          // >= 1
  uint64_t t = min((uint64_t)h, room);
  const uint8_t *pa = s + a, *pb = s + b;
  while (t < room) {
    const unsigned long long x = load8(pa + t) ^ load8(pb + t);
    if (x) {
      t += (uint64_t)(__builtin_ctzll(x) >> 3);
      break;
    }
    t += 8;
  }
  return (uint32_t)min(t, room);
}

// A lane takes one run of kRun consecutive positions (four 16-byte loads of phi, four 16-byte stores of plcp, the run in
// registers) and carries h from each position to the next: only the run's first position is compared from nothing.  The
// lanes of a wave take neighbouring runs, so a wave reads one stretch of s and of phi.  phi is padded to a multiple of kRun
// entries.
__global__ __launch_bounds__(kLcpThreads) void k_lcp_plcp(const uint8_t *__restrict__ s, uint64_t n, uint32_t *__restrict__ phi,
                                                          uint64_t nruns) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nruns; j += stride) {
    uint4 *line = reinterpret_cast<uint4 *>(phi + j * kRun);
    uint32_t w[kRun];
#pragma unroll
    for (int q = 0; q < kRun / 4; q++) {
      const uint4 v = line[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    uint32_t h = 0;
#pragma unroll
    for (int t = 0; t < kRun; t++) {
      const uint64_t i = j * kRun + t;
      h = i < n ? lcp_extend(s, n, (uint32_t)i, w[t], h) : 0u;
      w[t] = h;
      h = h > 0 ? h - 1 : 0u;
    }
#pragma unroll
    for (int q = 0; q < kRun / 4; q++) line[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

// res[0]: max over rows of lcp << 32 | (0xFFFFFFFF - row) -- the largest entry, the smallest row among equals; res[1]: the sum
__global__ __launch_bounds__(kLcpThreads) void k_lcp_gather(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ plcp, uint64_t n,
                                                            uint32_t *__restrict__ lcp, unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_best[kLcpThreads / 64], s_sum[kLcpThreads / 64];
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t last = (uint32_t)(n - 1);
  unsigned long long best = 0, sum = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    const uint32_t v = r < last ? plcp[min(sa[r], last)] : 0u;
    lcp[r] = v;
    sum += v;
    best = max(best, ((unsigned long long)v << 32) | (0xFFFFFFFFu - (uint32_t)r));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    best = max(best, (unsigned long long)__shfl_xor(best, d, 64));
    sum += (unsigned long long)__shfl_xor(sum, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_best[threadIdx.x >> 6] = best;
    s_sum[threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kLcpThreads / 64; w++) {
      best = max(best, s_best[w]);
      sum += s_sum[w];
    }
    atomicMax(res, best);
    atomicAdd(res + 1, sum);
  }
}

// getLCP for a batch: out[q] = LCP[rows[q]], UINT32_MAX for a row >= n
__global__ __launch_bounds__(kLcpThreads) void k_lcp_rows(const uint32_t *__restrict__ lcp, uint64_t n, const uint64_t *__restrict__ rows,
                                                          uint64_t k, uint32_t *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < k; q += stride) {
    const uint64_t r = rows[q];
    out[q] = r < n ? lcp[r] : kNone;
  }
}

// ---------------------------------------------------------------- host side
uint64_t lcp_text_bytes(uint64_t n) { return n + kTextPad; }

uint64_t lcp_core_bytes(uint64_t n) { return ((n + kRun - 1) / kRun) * kRun * 4 + 64; }

void lcp_reverse_text(const uint8_t *d_text, uint64_t len, uint8_t *d_s, int cu_count, hipStream_t st) {
  k_lcp_reverse<<<lcp_grid(cu_count, len + 1 + kTextPad), kLcpThreads, 0, st>>>(d_text, len, d_s);
}

int lcp_core(const uint8_t *d_s, uint64_t n, const uint32_t *d_sa, uint32_t *d_lcp, int cu_count, hipStream_t st, LcpInfo *info) {
  struct Tmp {
    void *phi = nullptr, *res = nullptr;
    ~Tmp() {
      if (phi) (void)hipFree(phi);
      if (res) (void)hipFree(res);
    }
  } tmp;
  const uint64_t nruns = (n + kRun - 1) / kRun;
  hipError_t e = hipMalloc(&tmp.phi, nruns * kRun * 4);
  if (e == hipSuccess) e = hipMalloc(&tmp.res, 64);
  if (e != hipSuccess) {
    set_error(std::string("hipMalloc(LCP): ") + hipGetErrorString(e));
    return FMX_ERR_NOMEM;
  }
  uint32_t *phi = static_cast<uint32_t *>(tmp.phi);
  unsigned long long *res = static_cast<unsigned long long *>(tmp.res);
  Events<4> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  HIP_TRY(hipMemsetAsync(res, 0, 64, st), "hipMemsetAsync");
  // the entries no row names (the padding; all of them when d_sa is no permutation) read as "no successor"
  HIP_TRY(hipMemsetAsync(phi, 0xFF, nruns * kRun * 4, st), "hipMemsetAsync");
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  k_lcp_phi<<<lcp_grid(cu_count, n), kLcpThreads, 0, st>>>(d_sa, n, phi);
  HIP_TRY(hipGetLastError(), "k_lcp_phi");
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  k_lcp_plcp<<<lcp_grid(cu_count, nruns), kLcpThreads, 0, st>>>(d_s, n, phi, nruns);
  HIP_TRY(hipGetLastError(), "k_lcp_plcp");
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  k_lcp_gather<<<lcp_grid(cu_count, n), kLcpThreads, 0, st>>>(d_sa, phi, n, d_lcp, res);
  HIP_TRY(hipGetLastError(), "k_lcp_gather");
  HIP_TRY(ev.record(3, st), "hipEventRecord");
  unsigned long long host[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(host, res, 16, hipMemcpyDeviceToHost, st), "D2H(LCP summary)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (info) {
    info->max = (uint32_t)(host[0] >> 32);
    info->max_row = 0xFFFFFFFFull - (host[0] & 0xFFFFFFFFull);
    info->sum = host[1];
    for (int i = 0; i < 3; i++) info->phase_ms[i] = ev.ms(i, i + 1);
  }
  return FMX_OK;
}

// ---------------------------------------------------------------- the handle's array
int lcp_check(const Index *h) {
  if (h->block_mode) {
    set_error("the LCP array needs the index of one text: fmx_open_block handles (one merge block) have no suffix array");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n >= (1ull << 32)) {
    set_error("X.lcp holds 4-byte entries and the array is built over u32 positions: n must be < 2^32");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

// The handle's array into h->lcp: s and the suffix array by the inversion (fmx_locate.hip), then the core.
static int lcp_build(const Index *h, hipStream_t st, DevMem &mem) {
  const uint64_t n = h->n;
  int rc = device_room(4 * n + 4 * n + lcp_text_bytes(n) + lcp_core_bytes(n) + locate_invert_text_bytes(h), "the LCP array");
  if (rc) return rc;
  uint32_t *lcp = nullptr, *sa = nullptr;
  uint8_t *s = nullptr;
  DEV_ALLOC(mem, lcp, 4 * n, "LCP");
  DEV_ALLOC(mem, sa, 4 * n, "LCP");
  DEV_ALLOC(mem, s, lcp_text_bytes(n), "LCP");
  HIP_TRY(hipMemsetAsync(s, 0, lcp_text_bytes(n), st), "hipMemsetAsync");
  if ((rc = locate_invert_text(h, st, sa, s))) return rc;
  LcpInfo info;
  if ((rc = lcp_core(s, n, sa, lcp, h->cu_count, st, &info))) return rc;
  mem.keep(lcp);
  h->lcp.lcp = lcp;
  h->lcp.bytes = 4 * n;
  h->lcp.max = info.max;
  h->lcp.max_row = info.max_row;
  h->lcp.sum = info.sum;
  return FMX_OK;
}

int lcp_prepare(const Index *h, hipStream_t st) {
  if (const int rc = lcp_check(h)) return rc;
  return build_locked(h->lcp, st, "the LCP array is built by fmx_prepare(FMX_PREPARE_LCP) or a first LCP call outside a stream capture",
                      [&](DevMem &mem) { return lcp_build(h, st, mem); });
}

hipError_t launch_lcp_gather(const Index *h, const void *d_rows, uint64_t k, void *d_out, hipStream_t st) {
  if (!k) return hipSuccess;
  k_lcp_rows<<<lcp_grid(h->cu_count, k), kLcpThreads, 0, st>>>(static_cast<const uint32_t *>(h->lcp.lcp), h->n,
                                                              static_cast<const uint64_t *>(d_rows), k, static_cast<uint32_t *>(d_out));
  return hipGetLastError();
}

}  // namespace fmx
