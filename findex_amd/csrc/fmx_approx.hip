// fmx_approx.hip -- approximate search: literal patterns with up to three substituted bytes.
//
// A hit of pattern P (m bytes, matched last byte first) with budget e and substitution range [lo, hi] is a string Q of m
// bytes that differs from P in d <= e positions, holds a byte of the range at each of them, and whose exact backward search
// ends with a non-empty interval; it is reported as (pattern, d, sp, ep).  The search is a depth-first walk over the
// backward steps: at a node (i bytes left, d mismatches, sp, ep) with d < e every symbol c != P[i - 1] of the range that
// occurs in the index is a substitution child, and the step with P[i - 1] itself is the match child.
//
// One WAVE owns one pattern at a time.  Its lane groups (16 quads, or 8 octets on the bytes layout) take one candidate
// symbol each per round.  A child that has used up the budget (d + 1 == e) is an exact tail: the group that found it
// walks it to the end of the pattern by itself and reports it.  A child with budget left is written to the node's frame
// on the wave's stack in LDS (a node that pushes has d <= e - 2: at most two frames), and the wave descends into the
// round's children one at a time; the match child is taken last, as the continuation of the loop.
// The one-row rule: a node of exactly one row has one non-empty child, the symbol BWT'[sp] (0 on the EOF row, which no
// range holds) -- where that symbol is a candidate other than P[i - 1] the node tries it and nothing else; otherwise it
// makes the match step alone, like a node without budget.
//
// Hits go to a staging area of `cap` records in the order they are found (one atomic per wave and round, positions from
// a ballot prefix; appends past cap are counted, not written); a radix sort of pattern << 38 | sp with the staging index
// as value, a gather and a binary search per pattern put them into their CSR order, which depends on nothing but the input.
#include <fmx.h>

#include <algorithm>
#include <string>

#include "fmx_device.h"
#include "fmx_host.h"

namespace fmx {

constexpr int kApThreads = 256;                // four waves: four patterns per workgroup
constexpr int kApWaves = kApThreads / 64;
constexpr uint32_t kApFrames = 2;              // nodes that push have d = 0 .. e - 2
constexpr int kApRowBits = 38;                 // rows are below 2^38, patterns below 2^26: the sort key
constexpr uint32_t kApLineWords = 32;          // the call's own words: [0] hits (a 128-byte line of its own), [16] steps, [17] requests

struct ApFrame {
  uint64_t sp, ep, i;                          // the node: its interval and the pattern bytes it has left
  uint32_t round, nchild, child, pad;          // the next symbol round; this round's children and the next one to walk
  uint64_t csp[16], cep[16];
};

struct ApShared {
  uint64_t cf[256];
  uint16_t slot[256];
  uint8_t cand[256];                           // the symbols of the range that occur in the index, ascending
  uint32_t ncand;
  ApFrame fr[kApWaves][kApFrames];
};

// writes and reads of the wave's frame by different lanes
__device__ __forceinline__ void ap_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Appends the hits of the lanes with `flag` (called by the whole wave).
__device__ __forceinline__ void ap_emit(bool flag, uint64_t q, uint32_t d, uint64_t sp, uint64_t ep, uint32_t lane,
                                        unsigned long long *__restrict__ stage, uint64_t cap,
                                        unsigned long long *__restrict__ total) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  if (!m) return;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(total, (unsigned long long)__popcll(m));
  base = __shfl(base, 0, 64);
  if (flag) {
    const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < cap) {
      stage[3 * pos] = (unsigned long long)(uint32_t)q | ((unsigned long long)d << 32);
      stage[3 * pos + 1] = sp;
      stage[3 * pos + 2] = ep;
    }
  }
}

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kApThreads) void k_approx(DevIndex ix, const uint8_t *__restrict__ pat,
                                                       const uint64_t *__restrict__ off, uint64_t k, uint32_t e,
                                                       uint32_t sub_lo, uint32_t sub_hi, unsigned long long *__restrict__ stage,
                                                       uint64_t cap, unsigned long long *__restrict__ total,
                                                       unsigned long long *__restrict__ counters) {
  __shared__ ApShared sh;
  for (int c = threadIdx.x; c < 256; c += kApThreads) {
    sh.cf[c] = ix.cf[c];
    sh.slot[c] = ix.slot[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t nc = 0;
    if (e)
      for (uint32_t c = sub_lo; c <= sub_hi && c < 256u; c++)
        if (sh.slot[c] < kSlotEof) sh.cand[nc++] = (uint8_t)c;
    sh.ncand = nc;
  }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  constexpr uint32_t NG = 64 / G;
  const LaneConst lc = lane_const<G>();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, g = lane / G;
  const bool lead = lc.t == 0;
  ApFrame *fr = sh.fr[wv];
  const uint64_t nwaves = (uint64_t)gridDim.x * kApWaves;
  unsigned long long steps = 0, reqs = 0;                    // counted by the lane that leads the group (lane 0 for the wave's own steps)
  auto step = [&](uint32_t c, uint64_t &s, uint64_t &t, bool count) {
    const uint16_t sl = sh.slot[c];
    const uint32_t r = t - s == 1 ? single_row_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, t)
                                  : backward_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, t);
    if (count) { steps++; reqs += r; }
  };
  for (uint64_t q = (uint64_t)blockIdx.x * kApWaves + wv; q < k; q += nwaves) {
    const uint64_t b = off[q], en = off[q + 1];
    const uint8_t *P = pat + b;
    uint64_t i = en > b ? en - b : 0, sp = 0, ep = ix.n;
    uint32_t d = 0, depth = 0, round = 0;
    bool node = true;                                        // false: take the next child of the top frame, or leave it
    for (;;) {
      if (!node) {
        if (depth == 0) break;
        ApFrame &f = fr[depth - 1];
        const uint32_t ch = f.child;
        node = true;
        if (ch < f.nchild) {                                 // the next child of the round
          sp = f.csp[ch & 15u];
          ep = f.cep[ch & 15u];
          i = f.i - 1;
          d = depth;
          round = 0;
          ap_wave_sync();
          if (lane == 0) f.child = ch + 1;
          ap_wave_sync();
        } else {                                             // back at the node: its later rounds, then its match child
          depth--;
          sp = f.sp;
          ep = f.ep;
          i = f.i;
          d = depth;
          round = f.round;
        }
        continue;
      }
      if (i == 0) {                                          // the pattern is through: a hit with d mismatches
        ap_emit(lane == 0, q, d, sp, ep, lane, stage, cap, total);
        node = false;
        continue;
      }
      const uint32_t pc = P[i - 1];
      const bool one = ep - sp == 1;
      uint32_t bsym = 0;
      if (d < e) {
        uint32_t nc = sh.ncand;
        if (one) {                                           // the one-row rule
          bsym = sp == ix.eof ? 0u : (uint32_t)ix.bwt[sp];
          nc = (bsym != pc && bsym >= sub_lo && bsym <= sub_hi && sh.slot[bsym] < kSlotEof) ? 1u : 0u;
        }
        bool pushed = false;
        while ((uint64_t)round * NG < nc) {
          const uint32_t ci = round * NG + g;
          round++;
          const uint32_t c = one ? bsym : (uint32_t)sh.cand[ci < nc ? ci : 0u];
          const bool act = ci < nc && c != pc;
          uint64_t s = sp, t = ep;
          bool hit = false;
          if (act) {
            step(c, s, t, lead);
            hit = s < t;
            if (d + 1 == e) {                                // an exact tail: this group alone, to the end of the pattern
              for (uint64_t j = i - 1; hit && j > 0; j--) {
                step(P[j - 1], s, t, lead);
                hit = s < t;
              }
            }
          }
          if (d + 1 == e) {
            ap_emit(hit && lead, q, d + 1, s, t, lane, stage, cap, total);
            continue;
          }
          const unsigned long long m = __builtin_amdgcn_ballot_w64(hit && lead);
          if (!m) continue;
          ApFrame &f = fr[d & (kApFrames - 1u)];
          if (hit && lead) {
            const uint32_t at = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) & 15u;
            f.csp[at] = s;
            f.cep[at] = t;
          }
          if (lane == 0) {
            f.sp = sp;
            f.ep = ep;
            f.i = i;
            f.round = round;
            f.nchild = (uint32_t)__popcll(m);
            f.child = 0;
          }
          ap_wave_sync();
          depth = d + 1;
          pushed = true;
          break;
        }
        if (pushed) { node = false; continue; }
        if (one && nc) { node = false; continue; }           // the node tried its row's symbol: no match child
      }
      step(pc, sp, ep, lane == 0);                           // the match child: every group makes the same step
      i--;
      round = 0;
      if (!(sp < ep)) node = false;
    }
  }
  // the call's own counters: private slots, folded into the handle's afterwards (k_approx_fold)
  counters_add(counters, 2ull * steps, steps, reqs);
}

// The call's counter slots into the handle's, and their sums into the call's line.
__global__ __launch_bounds__(256) void k_approx_fold(const unsigned long long *__restrict__ mine,
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

__global__ __launch_bounds__(256) void k_approx_keys(const unsigned long long *__restrict__ stage, uint64_t rows,
                                                     unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    key[j] = ((stage[3 * j] & 0xFFFFFFFFull) << kApRowBits) | stage[3 * j + 1];
    val[j] = (uint32_t)j;
  }
}

__global__ __launch_bounds__(256) void k_approx_gather(const unsigned long long *__restrict__ stage,
                                                       const uint32_t *__restrict__ val, uint64_t rows,
                                                       unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const uint64_t s = val[j] < rows ? val[j] : rows - 1;
#pragma unroll
    for (int w = 0; w < 3; w++) out[3 * j + w] = stage[3 * s + w];
  }
}

// out_off[i] = hits of the patterns before i: the first sorted key that is not below i << 38 (key == nullptr: none at all)
__global__ __launch_bounds__(256) void k_approx_off(const unsigned long long *__restrict__ key, uint64_t rows, uint64_t k,
                                                    unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= k; i += stride) {
    const unsigned long long want = (unsigned long long)i << kApRowBits;
    uint64_t lo = 0, hi = rows;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    out_off[i] = lo;
  }
}

static uint32_t ap_grid(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, 4096)); }

template <bool WIDE, uint32_t LAYOUT>
static hipError_t ap_launch(const Index *h, const uint8_t *pat, const uint64_t *off, uint64_t k, uint32_t e, uint32_t lo,
                            uint32_t hi, unsigned long long *stage, uint64_t cap, unsigned long long *line,
                            unsigned long long *mine, hipStream_t st) {
  int per_cu = 0;
  hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_approx<WIDE, LAYOUT>, kApThreads, 0);
  if (he != hipSuccess) return he;
  const uint64_t resident = (uint64_t)std::max(per_cu, 1) * (uint64_t)std::max(h->cu_count, 1);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident, (k + kApWaves - 1) / kApWaves));
  hipLaunchKernelGGL((k_approx<WIDE, LAYOUT>), dim3(grid), dim3(kApThreads), 0, st, h->dev, pat, off, k, e, lo, hi, stage, cap,
                     line, mine);
  return hipGetLastError();
}

int approx_check(const Index *h) {
  if (h->block_mode) {
    set_error("approximate search: not for fmx_open_block handles");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n >= (1ull << kApRowBits)) {
    set_error("approximate search: the index has 2^38 rows or more");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

int approx_search(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint32_t e, uint32_t lo, uint32_t hi,
                  void *d_out_off, void *d_out, uint64_t cap, hipStream_t st, ApproxInfo *info) {
  *info = ApproxInfo{};
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t *ev; ~EvGuard() { for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]); } } evg{ev};
  for (int i = 0; i < 3; i++) HIP_TRY(hipEventCreate(&ev[i]), "hipEventCreate");
  DevMem mem;
  unsigned long long *stage = nullptr, *line = nullptr, *mine = nullptr;
  DEV_ALLOC(mem, stage, 24 * cap, "approx staging");
  DEV_ALLOC(mem, line, 8 * kApLineWords, "approx");
  DEV_ALLOC(mem, mine, kCounterBytes, "approx");
  HIP_TRY(hipMemsetAsync(line, 0, 8 * kApLineWords, st), "memset");
  HIP_TRY(hipMemsetAsync(mine, 0, kCounterBytes, st), "memset");
  HIP_TRY(hipEventRecord(ev[0], st), "hipEventRecord");
  if (k) {
#define FMX_AP_CALL(W, L) \
  HIP_TRY((ap_launch<W, L>(h, static_cast<const uint8_t *>(d_pat), static_cast<const uint64_t *>(d_off), k, e, lo, hi, stage, \
                           cap, line, mine, st)), "k_approx")
    FMX_LAYOUT_DISPATCH(h, FMX_AP_CALL);
#undef FMX_AP_CALL
    hipLaunchKernelGGL(k_approx_fold, dim3(kCounterSlots / 256), dim3(256), 0, st, mine, h->d_counters, line);
    HIP_TRY(hipGetLastError(), "k_approx_fold");
  }
  HIP_TRY(hipEventRecord(ev[1], st), "hipEventRecord");
  unsigned long long words[kApLineWords];
  HIP_TRY(hipMemcpyAsync(words, line, sizeof words, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  {
    std::lock_guard<std::mutex> lk(h->mu);
    h->launches += k ? 1 : 0;
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
  info->search_ms = ms;
  info->total = words[0];
  info->steps = words[16];
  info->requests = words[17];
  if (info->total > cap) return FMX_OK;                      // the caller reports the overflow; nothing is ordered
  const uint64_t rows = info->total;
  unsigned long long *out_off = static_cast<unsigned long long *>(d_out_off);
  if (rows == 0) {
    hipLaunchKernelGGL(k_approx_off, dim3(ap_grid(k + 1)), dim3(256), 0, st, nullptr, 0ull, k, out_off);
    HIP_TRY(hipGetLastError(), "k_approx_off");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return FMX_OK;
  }
  const uint64_t nt = radix_tiles(rows), hist_words = 256 * nt, parts = scan_partials(std::max<uint64_t>(rows, hist_words));
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr, *hist = nullptr, *partials = nullptr;
  DEV_ALLOC(mem, k0, 8 * rows, "approx sort");
  DEV_ALLOC(mem, k1, 8 * rows, "approx sort");
  DEV_ALLOC(mem, v0, 4 * rows, "approx sort");
  DEV_ALLOC(mem, v1, 4 * rows, "approx sort");
  DEV_ALLOC(mem, hist, 4 * hist_words, "approx sort");
  DEV_ALLOC(mem, partials, 4 * parts, "approx sort");
  hipLaunchKernelGGL(k_approx_keys, dim3(ap_grid(rows)), dim3(256), 0, st, stage, rows, k0, v0);
  HIP_TRY(hipGetLastError(), "k_approx_keys");
  int k_bits = 1;
  while (k_bits < 26 && ((k - 1) >> k_bits) != 0) k_bits++;
  unsigned long long *key = k0, *key_alt = k1;
  uint32_t *val = v0, *val_alt = v1;
  int passes = 0;
  HIP_TRY(radix_sort(&key, &val, &key_alt, &val_alt, rows, kApRowBits + k_bits, hist, partials, st, &passes), "radix sort");
  hipLaunchKernelGGL(k_approx_gather, dim3(ap_grid(rows)), dim3(256), 0, st, stage, val, rows,
                     static_cast<unsigned long long *>(d_out));
  HIP_TRY(hipGetLastError(), "k_approx_gather");
  hipLaunchKernelGGL(k_approx_off, dim3(ap_grid(k + 1)), dim3(256), 0, st, key, rows, k, out_off);
  HIP_TRY(hipGetLastError(), "k_approx_off");
  HIP_TRY(hipEventRecord(ev[2], st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the temporaries go when this returns
  (void)hipEventElapsedTime(&ms, ev[1], ev[2]);
  info->sort_ms = ms;
  return FMX_OK;
}

}  // namespace fmx
