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
#include <atomic>
#include <string>

#include "fmx_device.h"
#include "fmx_host.h"

namespace fmx {

constexpr int kMsThreads = 256;
constexpr int kMsWaves = kMsThreads / 64;
constexpr uint32_t kMsTile = FMX_MSTAT_TILE;                // positions per tile: four waves of 128
constexpr uint32_t kMsWaveTile = kMsTile / kMsWaves;
constexpr uint32_t kMsMaxLen = FMX_MSTAT_MAX_LEN;
constexpr uint32_t kMsLineWords = 32;                      // the call's own words: [16] steps, [17] requests

struct MsShared {
  uint64_t cf[256];
  uint16_t slot[256];
  uint16_t lim[kMsTile];                                   // per position of the tile: min(e, max_len); 0: no pattern covers it
  uint8_t buf[kMsMaxLen + kMsTile];                        // pat[tile_lo - halo .. tile_hi)
};

__device__ __forceinline__ uint64_t ms_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

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
    const uint32_t tile_n = (uint32_t)ms_min(kMsTile, n_bytes - tile_lo);
    const uint32_t halo = (uint32_t)ms_min(max_len, tile_lo);
    __syncthreads();                                       // the tile before this one is through (and cf / slot are there)
    for (uint32_t b = threadIdx.x; b < halo + tile_n; b += kMsThreads) sh.buf[b] = pat[tile_lo - halo + b];
    for (uint32_t p = threadIdx.x; p < tile_n; p += kMsThreads) {
      uint64_t start;
      const uint64_t q = ms_owner(off, k, tile_lo + p, &start);
      sh.lim[p] = q < k ? (uint16_t)ms_min(tile_lo + p - start + 1, max_len) : (uint16_t)0;
    }
    __syncthreads();
    const uint32_t wend = (uint32_t)ms_min(tile_n, (wv + 1) * kMsWaveTile);
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
        cursor = (uint32_t)ms_min(wend, cursor + (uint32_t)__popcll(need));
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

// The call's counter slots into the handle's, and their sums into the call's line (the host and MEM forms).
__global__ __launch_bounds__(256) void k_mstat_fold(const unsigned long long *__restrict__ mine,
                                                    unsigned long long *__restrict__ counters,
                                                    unsigned long long *__restrict__ line) {
  const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
  unsigned long long v[3] = {0, 0, 0};
  if (sl < kCounterSlots) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      v[j] = mine[(size_t)sl * kCounterStride + j];
      if (v[j]) atomicAdd(counters + (size_t)sl * kCounterStride + j, v[j]);
    }
  }
  const unsigned long long s1 = wave_sum(v[1]), s2 = wave_sum(v[2]);
  if ((threadIdx.x & 63u) == 0) {
    if (s1) atomicAdd(line + 16, s1);
    if (s2) atomicAdd(line + 17, s2);
  }
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
  for (uint64_t q = t0; q <= k; q += stride) out_off[q] = slot[ms_min(off[q], n_bytes)];
}

static uint32_t ms_grid(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, 4096)); }

template <bool WIDE, uint32_t LAYOUT>
static hipError_t ms_launch(const Index *h, const uint8_t *pat, const uint64_t *off, uint64_t k, uint64_t n_bytes,
                            uint32_t max_len, uint32_t *len, uint64_t *sp, uint64_t *ep, unsigned long long *counters,
                            hipStream_t st) {
  static std::atomic<int> cached{0};                       // per instantiation: the query is made once
  int per_cu = cached.load(std::memory_order_relaxed);
  if (per_cu <= 0) {
    const hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_mstat<WIDE, LAYOUT>, kMsThreads, 0);
    if (he != hipSuccess) return he;
    per_cu = std::max(per_cu, 1);
    cached.store(per_cu, std::memory_order_relaxed);
  }
  const uint64_t resident = (uint64_t)per_cu * (uint64_t)std::max(h->cu_count, 1);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident, (n_bytes + kMsTile - 1) / kMsTile));
  hipLaunchKernelGGL((k_mstat<WIDE, LAYOUT>), dim3(grid), dim3(kMsThreads), 0, st, h->dev, pat, off, k, n_bytes, max_len, len, sp,
                     ep, counters);
  return hipGetLastError();
}

int mstat_check(const Index *h) {
  if (h->block_mode) {
    set_error("matching statistics: not for fmx_open_block handles");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

hipError_t mstat_enqueue(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint64_t n_bytes, uint32_t max_len,
                         void *d_len, void *d_sp, void *d_ep, unsigned long long *counters, hipStream_t st) {
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

uint64_t mstat_bytes(uint64_t n_bytes, bool mems) {
  uint64_t need = kCounterBytes + 8 * kMsLineWords;
  if (mems) need += 20 * n_bytes + 4 * (n_bytes + 1) + 4 * scan_partials(n_bytes + 1) + 64;
  return need;
}

int mstat_room(uint64_t need, const char *what) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
  if (need > free_b) {
    set_error(std::string(what) + " needs " + std::to_string((unsigned long long)need) + " bytes of device memory, " +
              std::to_string((unsigned long long)free_b) + " are free");
    return FMX_ERR_NOMEM;
  }
  return FMX_OK;
}

int mstat_run(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint64_t n_bytes, uint32_t max_len,
              uint32_t min_len, void *d_len, void *d_sp, void *d_ep, bool mems, void *d_out_off, void *d_out, uint64_t cap,
              hipStream_t st, MstatInfo *info) {
  *info = MstatInfo{};
  int rc = mstat_room(mstat_bytes(n_bytes, mems), mems ? "fmx_mems_batch" : "fmx_match_stats_batch");
  if (rc) return rc;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t *ev; ~EvGuard() { for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]); } } evg{ev};
  for (int i = 0; i < 3; i++) HIP_TRY(hipEventCreate(&ev[i]), "hipEventCreate");
  DevMem mem;
  unsigned long long *line = nullptr, *mine = nullptr;
  uint32_t *len = static_cast<uint32_t *>(d_len), *flag = nullptr, *partials = nullptr;
  uint64_t *sp = static_cast<uint64_t *>(d_sp), *ep = static_cast<uint64_t *>(d_ep);
  DEV_ALLOC(mem, line, 8 * kMsLineWords, "matching statistics");
  DEV_ALLOC(mem, mine, kCounterBytes, "matching statistics");
  if (mems) {
    DEV_ALLOC(mem, len, 4 * n_bytes, "MEM statistics");
    DEV_ALLOC(mem, sp, 8 * n_bytes, "MEM statistics");
    DEV_ALLOC(mem, ep, 8 * n_bytes, "MEM statistics");
    DEV_ALLOC(mem, flag, 4 * (n_bytes + 1), "MEM flags");
    DEV_ALLOC(mem, partials, 4 * scan_partials(n_bytes + 1), "MEM scan");
  }
  HIP_TRY(hipMemsetAsync(line, 0, 8 * kMsLineWords, st), "memset");
  HIP_TRY(hipMemsetAsync(mine, 0, kCounterBytes, st), "memset");
  HIP_TRY(hipEventRecord(ev[0], st), "hipEventRecord");
  if (n_bytes) {
    HIP_TRY(mstat_enqueue(h, d_pat, d_off, k, n_bytes, max_len, len, sp, ep, mine, st), "k_mstat");
    hipLaunchKernelGGL(k_mstat_fold, dim3(kCounterSlots / 256), dim3(256), 0, st, mine, h->d_counters, line);
    HIP_TRY(hipGetLastError(), "k_mstat_fold");
  }
  HIP_TRY(hipEventRecord(ev[1], st), "hipEventRecord");
  unsigned long long words[kMsLineWords];
  uint32_t total = 0;
  if (mems) {
    hipLaunchKernelGGL(k_mem_flag, dim3(ms_grid(n_bytes + 1)), dim3(256), 0, st, len, n_bytes, min_len, flag);
    HIP_TRY(hipGetLastError(), "k_mem_flag");
    HIP_TRY(scan_u32(flag, n_bytes + 1, kScanSum, true, partials, st), "scan");
    hipLaunchKernelGGL(k_mem_write, dim3(ms_grid(std::max<uint64_t>(n_bytes, k + 1))), dim3(256), 0, st, flag, len, sp, ep,
                       static_cast<const uint64_t *>(d_off), k, n_bytes, cap, static_cast<unsigned long long *>(d_out_off),
                       static_cast<uint4 *>(d_out));
    HIP_TRY(hipGetLastError(), "k_mem_write");
    HIP_TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    HIP_TRY(hipMemcpyAsync(&total, flag + n_bytes, 4, hipMemcpyDeviceToHost, st), "D2H");
  }
  HIP_TRY(hipMemcpyAsync(words, line, sizeof words, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the temporaries go when this returns
  {
    std::lock_guard<std::mutex> lk(h->mu);
    h->launches += n_bytes ? 1 : 0;
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
  info->walk_ms = ms;
  if (mems) {
    (void)hipEventElapsedTime(&ms, ev[1], ev[2]);
    info->compact_ms = ms;
  }
  info->total = total;
  info->steps = words[16];
  info->requests = words[17];
  return FMX_OK;
}

}  // namespace fmx
