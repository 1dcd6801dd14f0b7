// fmx_mstat.hip -- matching statistics and maximal exact matches of long queries.
//
// The batch is k patterns back to back in `pat`; the outputs are parallel to `pat`.  For byte j of pattern q, with
// e = j - off[q] + 1 and L = min(e, max_len), the reference's loop (findex.scala:15-31) runs from (0, n) over pat[j],
// pat[j - 1], .. and stops before the first step whose result is empty, after L steps at the latest: len[j] is the number of
// steps completed, (sp[j], ep[j]) the interval after the last of them.  Every position is a backward search of its own.
//
// A WORKGROUP takes tiles of kMsTile consecutive positions, grid-strided.  It stages the tile's bytes and the max_len bytes in
// front of them in LDS (a step never waits for a dependent byte load from memory), and for every position of the tile the
// number of steps it may make at most (the owner search over the offsets, once per position).  Each of the four WAVES owns a
// quarter of the tile; its lane groups (16 quads, or 8 octets on the bytes layout) own one end position each.  Every round
// each live group makes one step; a group whose walk has ended writes its result and, at the top of the loop, draws the
// wave's next position from a wave-uniform cursor: a ballot of the groups that want one and a popcount prefix.  A wave's time
// is then the sum of its walks over its groups, not its groups times the longest walk.
//
// The MEMs of a batch are its statistics compacted: k_mem_flag marks the positions that end a reported match, the scan of
// fmx_host.h turns the flags into output slots, k_mem_write writes the 32-byte records and the CSR offsets.  A pattern's hits
// come by ascending end: the order of the positions themselves, so the same input gives the same bytes on every run.
#include <fmx.h>

#include <algorithm>
#include <string>

#include "fmx_device.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kMsThreads = 256;
constexpr int kMsWaves = kMsThreads / 64;
constexpr uint32_t kMsTile = FMX_MSTAT_TILE;                // positions per tile: four waves of 128
constexpr uint32_t kMsWaveTile = kMsTile / kMsWaves;
constexpr uint32_t kMsMaxLen = FMX_MSTAT_MAX_LEN;

struct MsShared {
  uint64_t cf[256];
  uint16_t slot[256];
  uint16_t lim[kMsTile];                                   // per position of the tile: min(e, max_len); 0: no pattern covers it
  uint8_t buf[kMsMaxLen + kMsTile];                        // pat[tile_lo - halo .. tile_hi)
};

// The pattern that owns position j: the largest q with off[q] <= j, when j < off[q + 1].  Whatever the offsets hold, the
// search stays inside off[0 .. k] and *start <= j: k (no owner) otherwise.
__device__ __forceinline__ uint64_t ms_owner(const uint64_t *__restrict__ off, uint64_t k, uint64_t j, uint64_t *start) {
  uint64_t lo = 0, hi = k + 1;                             // the first index whose offset exceeds j
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] <= j) lo = mid + 1; else hi = mid;
  }
  *start = 0;
  if (lo == 0 || lo > k) return k;
  const uint64_t b = off[lo - 1];
  if (b > j) return k;
  *start = b;
  return lo - 1;
}

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kMsThreads) void k_mstat(DevIndex ix, const uint8_t *__restrict__ pat,
                                                      const uint64_t *__restrict__ off, uint64_t k, uint64_t n_bytes,
                                                      uint32_t max_len, uint32_t *__restrict__ out_len,
                                                      uint64_t *__restrict__ out_sp, uint64_t *__restrict__ out_ep,
                                                      unsigned long long *__restrict__ counters) {
  __shared__ MsShared sh;
  for (int c = threadIdx.x; c < 256; c += kMsThreads) {
    sh.cf[c] = ix.cf[c];
    sh.slot[c] = ix.slot[c];
  }
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const bool lead = lc.t == 0;
  const unsigned long long below = (1ull << (lane & ~(uint32_t)(G - 1))) - 1ull;    // the lanes in front of this group
  unsigned long long steps = 0, reqs = 0;                  // counted by the lane that leads the group
  const uint64_t ntiles = (n_bytes + kMsTile - 1) / kMsTile;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t tile_lo = tile * kMsTile;
    const uint32_t tile_n = (uint32_t)min_u64(kMsTile, n_bytes - tile_lo);
    const uint32_t halo = (uint32_t)min_u64(max_len, tile_lo);
    __syncthreads();                                       // the tile before this one is through (and cf / slot are there)
    for (uint32_t b = threadIdx.x; b < halo + tile_n; b += kMsThreads) sh.buf[b] = pat[tile_lo - halo + b];
    for (uint32_t p = threadIdx.x; p < tile_n; p += kMsThreads) {
      uint64_t start;
      const uint64_t q = ms_owner(off, k, tile_lo + p, &start);
      sh.lim[p] = q < k ? (uint16_t)min_u64(tile_lo + p - start + 1, max_len) : (uint16_t)0;
    }
    __syncthreads();
    const uint32_t wend = (uint32_t)min_u64(tile_n, (wv + 1) * kMsWaveTile);
    uint32_t cursor = wv * kMsWaveTile;                    // wave-uniform: the wave's next position that nobody owns
    bool want = true, live = false;                        // both the same in all lanes of a group
    uint32_t p = 0, i = 0, lim = 0;
    uint64_t sp = 0, ep = 0;
    for (;;) {
      const unsigned long long need = __builtin_amdgcn_ballot_w64(want && lead);
      if (need) {
        if (want) {
          const uint32_t np = cursor + (uint32_t)__popcll(need & below);
          want = false;
          if (np < wend) {
            p = np;
            lim = sh.lim[np];
            i = 0;
            sp = 0;
            ep = ix.n;
            live = true;
          }
        }
        cursor = (uint32_t)min_u64(wend, cursor + (uint32_t)__popcll(need));
      }
      if (!__builtin_amdgcn_ballot_w64(live)) break;
      if (live) {
        bool fin = lim == 0;
        if (!fin) {
          const uint32_t c = sh.buf[halo + p - i];
          const uint16_t sl = sh.slot[c];
          uint64_t s = sp, t = ep;
          const uint32_t r = t - s == 1 ? single_row_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, t)
                                        : backward_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, t);
          if (lead) { steps++; reqs += r; }
          if (s < t) {
            sp = s;
            ep = t;
            i++;
            fin = i == lim;
          } else {
            fin = true;
          }
        }
        if (fin) {
          if (lead) {
            const uint64_t j = tile_lo + p;
            out_len[j] = i;
            if (out_sp) out_sp[j] = sp;
            if (out_ep) out_ep[j] = ep;
          }
          live = false;
          want = true;
        }
      }
    }
  }
  counters_add(counters, 2ull * steps, steps, reqs);
}

// flag[j] = 1 where byte j ends a reported match: len[j] >= min_len (>= 1) and the match does not go on with byte j + 1.
// The first byte of a pattern has len <= 1, so len[j + 1] <= len[j] holds at every pattern edge by itself; flag[n_bytes] = 0
// is the slot the scan leaves the total in.
__global__ __launch_bounds__(256) void k_mem_flag(const uint32_t *__restrict__ len, uint64_t n_bytes, uint32_t min_len,
                                                  uint32_t *__restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= n_bytes; j += stride) {
    uint32_t f = 0;
    if (j < n_bytes) {
      const uint32_t l = len[j];
      f = l >= min_len && (j + 1 == n_bytes || len[j + 1] <= l) ? 1u : 0u;
    }
    flag[j] = f;
  }
}

// slot[] = the exclusive scan of the flags (slot[n_bytes] = the total).  The record of every flagged position below cap, and
// out_off[q] = the hits in front of pattern q's first byte.
__global__ __launch_bounds__(256) void k_mem_write(const uint32_t *__restrict__ slot, const uint32_t *__restrict__ len,
                                                   const uint64_t *__restrict__ sp, const uint64_t *__restrict__ ep,
                                                   const uint64_t *__restrict__ off, uint64_t k, uint64_t n_bytes,
                                                   uint64_t cap, unsigned long long *__restrict__ out_off,
                                                   uint4 *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t j = t0; j < n_bytes; j += stride) {
    const uint32_t at = slot[j];
    if (slot[j + 1] == at || at >= cap) continue;
    uint64_t start;
    const uint64_t q = ms_owner(off, k, j, &start);
    const uint64_t end = j - start + 1, s = sp[j], e = ep[j];
    out[2 * (uint64_t)at] = make_uint4((uint32_t)q, len[j], (uint32_t)end, (uint32_t)(end >> 32));
    out[2 * (uint64_t)at + 1] = make_uint4((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)e, (uint32_t)(e >> 32));
  }
  for (uint64_t q = t0; q <= k; q += stride) out_off[q] = slot[min_u64(off[q], n_bytes)];
}

template <bool WIDE, uint32_t LAYOUT>
static hipError_t ms_launch(const Index *h, const uint8_t *pat, const uint64_t *off, uint64_t k, uint64_t n_bytes,
                            uint32_t max_len, uint32_t *len, uint64_t *sp, uint64_t *ep, unsigned long long *counters,
                            hipStream_t st) {
  uint32_t grid = 0;
  const hipError_t he = resident_grid<k_mstat<WIDE, LAYOUT>>(h, kMsThreads, n_bytes, kMsTile, &grid);
  if (he != hipSuccess) return he;
  hipLaunchKernelGGL((k_mstat<WIDE, LAYOUT>), dim3(grid), dim3(kMsThreads), 0, st, h->dev, pat, off, k, n_bytes, max_len, len, sp,
                     ep, counters);
  return hipGetLastError();
}

static int mstat_check(const Index *h) {
  if (h->block_mode) {
    set_error("matching statistics: not for fmx_open_block handles");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

// The statistics of the n_bytes pattern bytes, device pointers throughout (d_sp / d_ep may be null); it only enqueues on `st`;
// counters == nullptr: the handle's own.
static hipError_t mstat_enqueue(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint64_t n_bytes,
                                uint32_t max_len, void *d_len, void *d_sp, void *d_ep, unsigned long long *counters,
                                hipStream_t st) {
  if (n_bytes == 0) return hipSuccess;
  hipError_t he = hipSuccess;
#define FMX_MS_CALL(W, L) \
  he = ms_launch<W, L>(h, static_cast<const uint8_t *>(d_pat), static_cast<const uint64_t *>(d_off), k, n_bytes, max_len, \
                       static_cast<uint32_t *>(d_len), static_cast<uint64_t *>(d_sp), static_cast<uint64_t *>(d_ep), \
                       counters ? counters : h->d_counters, st)
  FMX_LAYOUT_DISPATCH(h, FMX_MS_CALL);
#undef FMX_MS_CALL
  return he;
}

// the device bytes mstat_run allocates
static uint64_t mstat_bytes(uint64_t n_bytes, bool mems) {
  uint64_t need = kMeteredBytes;
  if (mems) need += 20 * n_bytes + 4 * (n_bytes + 1) + ScanSpace::bytes(n_bytes + 1) + 64;
  return need;
}

struct MstatInfo {
  uint64_t total = 0, steps = 0, requests = 0;
  double walk_ms = 0.0, compact_ms = 0.0;       // device events: k_mstat, the flag / scan / write steps
};

// mstat_enqueue with the call's own counters and timing, and, with `mems`, the compaction into d_out_off[k + 1] / d_out[cap]
// (the statistics are then temporaries of the call, d_len / d_sp / d_ep ignored); allocates, synchronises `st`, frees its
// temporaries on every path.  info->total is the exact number of hits; records past cap are not written.
static int mstat_run(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint64_t n_bytes, uint32_t max_len,
                     uint32_t min_len, void *d_len, void *d_sp, void *d_ep, bool mems, void *d_out_off, void *d_out,
                     uint64_t cap, hipStream_t st, MstatInfo *info) {
  *info = MstatInfo{};
  int rc = device_room(mstat_bytes(n_bytes, mems), mems ? "fmx_mems_batch" : "fmx_match_stats_batch");
  if (rc) return rc;
  Events<3> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  Metered own;
  uint32_t *len = static_cast<uint32_t *>(d_len), *flag = nullptr;
  ScanSpace scan;
  uint64_t *sp = static_cast<uint64_t *>(d_sp), *ep = static_cast<uint64_t *>(d_ep);
  if ((rc = own.alloc(mem, "matching statistics"))) return rc;
  if (mems) {
    DEV_ALLOC(mem, len, 4 * n_bytes, "MEM statistics");
    DEV_ALLOC(mem, sp, 8 * n_bytes, "MEM statistics");
    DEV_ALLOC(mem, ep, 8 * n_bytes, "MEM statistics");
    DEV_ALLOC(mem, flag, 4 * (n_bytes + 1), "MEM flags");
    if ((rc = scan.alloc(mem, n_bytes + 1, "MEM scan"))) return rc;
  }
  if ((rc = own.zero(st))) return rc;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (n_bytes) {
    HIP_TRY(mstat_enqueue(h, d_pat, d_off, k, n_bytes, max_len, len, sp, ep, own.mine, st), "k_mstat");
    if ((rc = own.fold(h, 1, st))) return rc;                // counter [1]: the backward steps
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  uint32_t total = 0;
  if (mems) {
    LAUNCH("k_mem_flag", k_mem_flag, dim3(flat_grid(n_bytes + 1)), dim3(256), st, len, n_bytes, min_len, flag);
    HIP_TRY(scan.sum(flag, n_bytes + 1, true, st), "scan");
    LAUNCH("k_mem_write", k_mem_write, dim3(flat_grid(std::max<uint64_t>(n_bytes, k + 1))), dim3(256), st, flag, len, sp, ep,
           static_cast<const uint64_t *>(d_off), k, n_bytes, cap, static_cast<unsigned long long *>(d_out_off),
           static_cast<uint4 *>(d_out));
    HIP_TRY(ev.record(2, st), "hipEventRecord");
    HIP_TRY(hipMemcpyAsync(&total, flag + n_bytes, 4, hipMemcpyDeviceToHost, st), "D2H");
  }
  MeterCounts cnt;
  if ((rc = own.finish(h, st, n_bytes ? 1 : 0, &cnt))) return rc;
  info->walk_ms = ev.ms(0, 1);
  if (mems) info->compact_ms = ev.ms(1, 2);
  info->total = total;
  info->steps = cnt.steps;
  info->requests = cnt.requests;
  return FMX_OK;
}

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static thread_local MstatInfo g_mstat_last;

// What refuses a call before the device is touched; max_len and min_len as the kernels take them.
static int mstat_args(const fmx_index *idx, size_t k, uint64_t n_bytes, const fmx_mstat_opts *opts, uint32_t *max_len,
                      uint32_t *min_len) {
  *max_len = FMX_MSTAT_MAX_LEN;
  *min_len = 1;
  if (opts) {
    if (opts->max_len > FMX_MSTAT_MAX_LEN) return arg_fail("fmx_mstat_opts.max_len: 1 .. 4096 (0 = the maximum)");
    if (opts->reserved[0] != 0 || opts->reserved[1] != 0) return arg_fail("fmx_mstat_opts.reserved must be 0");
    if (opts->max_len) *max_len = opts->max_len;
    if (opts->min_len > *max_len) return arg_fail("fmx_mstat_opts: min_len > max_len");
    if (opts->min_len) *min_len = opts->min_len;
  }
  if ((uint64_t)k > (1ull << 26)) return arg_fail("matching statistics: at most 2^26 patterns per call");
  if (n_bytes >= (1ull << 32)) return arg_fail("matching statistics: n_bytes must be below 2^32");
  if (!idx) return arg_fail("matching statistics: the handle is null");
  return mstat_check(H(idx));
}

// the host forms' offsets: off[0] == 0, non-decreasing; *n_bytes = off[k]
static int mstat_host_offsets(const uint64_t *off, size_t k, uint64_t *n_bytes) {
  *n_bytes = 0;
  if ((uint64_t)k > (1ull << 26)) return FMX_OK;           // (refused by mstat_args, with its own message)
  if (k && !off) return arg_fail("null argument");
  if (k && off[0] != 0) return arg_fail("matching statistics: off[0] must be 0");
  if (k && !offsets_monotonic(off, 0, k)) return arg_fail("pattern offsets must be non-decreasing");
  *n_bytes = k ? off[k] : 0;
  return FMX_OK;
}

static int mems_args(const void *out_off, const void *out, size_t cap, const size_t *n_out) {
  if (!n_out) return arg_fail("mems: n_out is null");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("mems: cap must be below 2^32");
  if (!out_off || (cap && !out)) return arg_fail("null argument");
  return FMX_OK;
}

extern "C" {

int fmx_match_stats_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, uint64_t n_bytes,
                              const fmx_mstat_opts *opts, void *d_len, void *d_sp, void *d_ep, void *stream) {
  uint32_t max_len, min_len;
  if (n_bytes && !d_len) return arg_fail("matching statistics: d_len is null");
  int rc = mstat_args(idx, k, n_bytes, opts, &max_len, &min_len);
  if (rc) return rc;
  if (n_bytes && (!d_pat || !d_off)) return arg_fail("null argument");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HIP_TRY(mstat_enqueue(h, d_pat, d_off, k, n_bytes, max_len, d_len, d_sp, d_ep, nullptr, (hipStream_t)stream), "k_mstat");
  return FMX_OK;
}

int fmx_match_stats_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_mstat_opts *opts,
                          uint32_t *out_len, uint64_t *out_sp, uint64_t *out_ep) {
  uint32_t max_len, min_len;
  uint64_t n_bytes;
  int rc = mstat_host_offsets(off, k, &n_bytes);
  if (rc) return rc;
  if (n_bytes && n_bytes < (1ull << 32) && (!out_len || !pat)) return arg_fail("matching statistics: null argument");
  if ((rc = mstat_args(idx, k, n_bytes, opts, &max_len, &min_len))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  const uint64_t outs = n_bytes * (4 + (out_sp ? 8 : 0) + (out_ep ? 8 : 0));
  if ((rc = device_room(mstat_bytes(n_bytes, false) + n_bytes + 8 * ((uint64_t)k + 1) + outs + 64, "fmx_match_stats_batch"))) return rc;
  HostCall hc;
  void *d_pat = nullptr;
  uint64_t *d_off = nullptr, *d_sp = nullptr, *d_ep = nullptr;
  uint32_t *d_len = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("patterns", pat, n_bytes, "offsets", off, k, false, &d_pat, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_len, 4 * n_bytes, "matching statistics");
  if (out_sp) DEV_ALLOC(hc.mem, d_sp, 8 * n_bytes, "matching statistics");
  if (out_ep) DEV_ALLOC(hc.mem, d_ep, 8 * n_bytes, "matching statistics");
  rc = mstat_run(h, d_pat, d_off, k, n_bytes, max_len, min_len, d_len, d_sp, d_ep, false, nullptr, nullptr, 0, hc.own.s, &g_mstat_last);
  if (rc || !n_bytes) return rc;
  if ((rc = hc.download(out_len, d_len, 4 * n_bytes, "D2H(len)")) || (rc = hc.download(out_sp, d_sp, 8 * n_bytes, "D2H(sp)")) ||
      (rc = hc.download(out_ep, d_ep, 8 * n_bytes, "D2H(ep)")))
    return rc;
  return hc.sync();
}

int fmx_mems_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, uint64_t n_bytes,
                       const fmx_mstat_opts *opts, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  uint32_t max_len, min_len;
  int rc = mems_args(d_out_off, d_out, cap, n_out);
  if (rc) return rc;
  if ((rc = mstat_args(idx, k, n_bytes, opts, &max_len, &min_len))) return rc;
  if (!d_off || (n_bytes && !d_pat)) return arg_fail("null argument");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  if ((rc = not_capturing((hipStream_t)stream, "a MEM call"))) return rc;
  rc = mstat_run(h, d_pat, d_off, k, n_bytes, max_len, min_len, nullptr, nullptr, nullptr, true, d_out_off, d_out, cap,
                 (hipStream_t)stream, &g_mstat_last);
  if (rc) return rc;
  *n_out = (size_t)g_mstat_last.total;
  return g_mstat_last.total > cap ? csr_overflow("mems", g_mstat_last.total, cap) : FMX_OK;
}

int fmx_mems_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_mstat_opts *opts,
                   uint64_t *out_off, fmx_mem_hit *out, size_t cap, size_t *n_out) {
  uint32_t max_len, min_len;
  uint64_t n_bytes;
  int rc = mems_args(out_off, out, cap, n_out);
  if (rc) return rc;
  if ((rc = mstat_host_offsets(off, k, &n_bytes))) return rc;
  if (n_bytes && n_bytes < (1ull << 32) && !pat) return arg_fail("pat is null");
  if ((rc = mstat_args(idx, k, n_bytes, opts, &max_len, &min_len))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  if ((rc = device_room(mstat_bytes(n_bytes, true) + n_bytes + 16 * ((uint64_t)k + 1) + sizeof(fmx_mem_hit) * (uint64_t)cap + 64,
                        "fmx_mems_batch"))) return rc;
  HostCall hc;
  void *d_pat = nullptr;
  uint64_t *d_off = nullptr, *d_out_off = nullptr;
  fmx_mem_hit *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("patterns", pat, n_bytes, "offsets", off, k, false, &d_pat, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out_off, 8 * ((uint64_t)k + 1), "MEM offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_mem_hit) * cap, "MEM hits");
  rc = mstat_run(h, d_pat, d_off, k, n_bytes, max_len, min_len, nullptr, nullptr, nullptr, true, d_out_off, d_out, cap, hc.own.s,
                 &g_mstat_last);
  if (rc) return rc;
  const uint64_t total = g_mstat_last.total;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("mems", total, cap);
  return hc.download_csr(out_off, d_out_off, k, out, d_out, total, sizeof(fmx_mem_hit));
}

int fmx_mstat_last(double *walk_ms, double *compact_ms, uint64_t *steps, uint64_t *requests) {
  if (walk_ms) *walk_ms = g_mstat_last.walk_ms;
  if (compact_ms) *compact_ms = g_mstat_last.compact_ms;
  if (steps) *steps = g_mstat_last.steps;
  if (requests) *requests = g_mstat_last.requests;
  return FMX_OK;
}

}  // extern "C"
