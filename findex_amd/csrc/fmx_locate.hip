// fmx_locate.hip -- locate: text positions of suffix-array rows from a sampled suffix array.
//
// s = reverse(text) + sentinel, n = len + 1 rows; SA[eof] = 0, SA[0] = n - 1, SA[LF r] = SA[r] - 1 for r != eof
// (Util.bwtFm2sa, util.scala:213-224; SACreator, bwtmerger.scala:535-556).  A handle keeps the rows whose SA is a
// multiple of the rate s: MARKS, a bit-vector over rows in the one-hot rank-block format (fmx_device.h: 64 bytes =
// 8-byte count of the set bits before the block + 448 bits), and SAMPLES, their SA values in row order (u32 when
// n <= 2^32, else u64).  locate(r) walks LF from r until a marked row: SA[r] = samples[rank(marks, r')] + steps.
//
// The samples are built from the BWT alone, by parallel inversion:
//   * starts: row 0 and the rows whose hash falls below a threshold (about n / 1024 of them, at most ~2^22): "is this
//     a start" costs no memory request.  Enumerated in row order (a count per run of rows, a host scan, a write);
//   * pass 1: one lane group per start walks LF to the next start and records which start that is and how far;
//   * list ranking by pointer jumping: every start's distance to row 0 along the cycle.  The cycle through row 0 must
//     be n rows long -- otherwise the input is not the BWT of one text (FMX_ERR_FORMAT);
//   * pass 2: every segment is walked again with its absolute SA known; the row of each SA value v % s == 0 goes to
//     tmp[v / s], from which the marks, their block counts and the samples follow.
// Both passes make two requests per LF step (the BWT byte, then the rank line(s)): 4 n requests for a build.
#include <fmx.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "fmx_device.h"
#include "fmx_host.h"

namespace fmx {

constexpr int kLocThreads = 256;
constexpr uint64_t kRunRows = 1024;            // rows per thread when the starts are enumerated
constexpr uint32_t kNoNext = 0xFFFFFFFFu;

struct LocTables {
  uint64_t cf[256];
  uint16_t slot[256];
};

__device__ __forceinline__ void loc_stage(const DevIndex &ix, LocTables &tb) {
  for (int c = threadIdx.x; c < 256; c += blockDim.x) {
    tb.cf[c] = ix.cf[c];
    tb.slot[c] = ix.slot[c];
  }
  __syncthreads();
}

// The start predicate: row 0, and rows whose 32-bit hash falls below `thresh`.
__device__ __forceinline__ bool inv_start(uint64_t r, uint32_t thresh) {
  uint64_t x = (r + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  return r == 0 || (uint32_t)x < thresh;
}

// One LF step for W walks of the lane group at once: all BWT bytes, then all rank lines, are requested before any is
// used.  Inactive walks make no request.
template <bool WIDE, uint32_t LAYOUT, int W>
__device__ __forceinline__ void lf_steps(const DevIndex &ix, const LocTables &tb, const LaneConst &lc, uint64_t (&r)[W],
                                         const bool (&act)[W]) {
  uint32_t b[W];
#pragma unroll
  for (int j = 0; j < W; j++) b[j] = act[j] ? (r[j] == ix.eof ? 0u : (uint32_t)ix.bwt[r[j]]) : 0u;
  RankReq q[W];
#pragma unroll
  for (int j = 0; j < W; j++) {
    q[j] = rank_issue<LAYOUT>(ix, act[j] ? tb.slot[b[j]] : kSlotNone, r[j], lc);
  }
#pragma unroll
  for (int j = 0; j < W; j++)
    if (act[j]) r[j] = tb.cf[b[j]] + rank_complete<WIDE, LAYOUT>(q[j], b[j], lc);
}

// ---------------------------------------------------------------- starts
__global__ __launch_bounds__(kLocThreads) void k_inv_count(uint64_t n, uint32_t thresh, uint32_t *__restrict__ cnt,
                                                          uint64_t runs) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < runs; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = t * kRunRows, hi = min(n, lo + kRunRows);
    uint32_t c = 0;
    for (uint64_t r = lo; r < hi; r++) c += inv_start(r, thresh) ? 1u : 0u;
    cnt[t] = c;
  }
}

__global__ __launch_bounds__(kLocThreads) void k_inv_list(uint64_t n, uint32_t thresh, const uint64_t *__restrict__ off,
                                                         uint64_t runs, uint64_t *__restrict__ starts) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < runs; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = t * kRunRows, hi = min(n, lo + kRunRows);
    uint64_t o = off[t];
    for (uint64_t r = lo; r < hi; r++)
      if (inv_start(r, thresh)) starts[o++] = r;
  }
}

// ---------------------------------------------------------------- pass 1: segments
// Walk q goes from starts[q] to the next start (at most n steps: a walk from a start returns to it at the latest).
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kLocThreads) void k_inv_segments(DevIndex ix, const uint64_t *__restrict__ starts, uint64_t S,
                                                             uint32_t thresh, uint32_t *__restrict__ next,
                                                             uint64_t *__restrict__ dist) {
  __shared__ LocTables tb;
  loc_stage(ix, tb);
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t ng = (uint64_t)gridDim.x * (kLocThreads / G);
  for (uint64_t q0 = ((uint64_t)blockIdx.x * kLocThreads + threadIdx.x) / G; q0 < S; q0 += 2 * ng) {
    const uint64_t qq[2] = {q0, q0 + ng};
    uint64_t r[2], d[2] = {0, 0};
    bool act[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      act[j] = qq[j] < S;
      r[j] = act[j] ? starts[qq[j]] : 0;
    }
    while (act[0] || act[1]) {
      lf_steps<WIDE, LAYOUT, 2>(ix, tb, lc, r, act);
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (act[j]) {
          d[j]++;
          act[j] = !inv_start(r[j], thresh) && d[j] < ix.n;
        }
    }
    if (lc.t == 0) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (qq[j] >= S) continue;
        uint64_t lo = 0, hi = S;                       // the start reached: lower bound in the sorted list
        while (lo < hi) {
          const uint64_t mid = (lo + hi) >> 1;
          if (starts[mid] < r[j]) lo = mid + 1; else hi = mid;
        }
        next[qq[j]] = lo < S && starts[lo] == r[j] ? (uint32_t)lo : kNoNext;
        dist[qq[j]] = d[j];
      }
    }
  }
}

// ---------------------------------------------------------------- list ranking (Wyllie): D[i] = rows from start i to row 0
__global__ __launch_bounds__(kLocThreads) void k_inv_rank_init(const uint32_t *__restrict__ next, const uint64_t *__restrict__ dist,
                                                              uint64_t S, uint32_t *__restrict__ nx, uint64_t *__restrict__ D) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t j = next[i];
    nx[i] = j == 0 ? kNoNext : j;                      // the segment that ends at row 0 ends the list
    D[i] = dist[i];
  }
}

__global__ __launch_bounds__(kLocThreads) void k_inv_rank_round(const uint32_t *__restrict__ nx0, const uint64_t *__restrict__ D0,
                                                               uint64_t S, uint32_t *__restrict__ nx1, uint64_t *__restrict__ D1) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t j = nx0[i];
    if (j == kNoNext || j >= S) {
      nx1[i] = kNoNext;
      D1[i] = D0[i];
    } else {
      nx1[i] = nx0[j];
      D1[i] = D0[i] + D0[j];
    }
  }
}

// ---------------------------------------------------------------- pass 2: every row with its SA
// Segment q: rows starts[q], LF starts[q], ... (dist[q] of them) with SA D[q] - 1, D[q] - 2, ...  The row of every SA
// value v with v % rate == 0 goes to tmp[v / rate]; with sa_be set instead, every row's SA goes there as a big-endian
// u32 (the X.sa file, rate 1).  TEXT (the LCP array's build, fmx_lcp.hip): every row's SA goes to sa_ne as a native u32
// and the row's BWT byte, which is s[SA - 1], to s_out -- the inversion walks s backwards, so it can write it down.
template <bool WIDE, uint32_t LAYOUT, bool TEXT>
__global__ __launch_bounds__(kLocThreads) void k_inv_fill(DevIndex ix, const uint64_t *__restrict__ starts, uint64_t S,
                                                         const uint64_t *__restrict__ dist, const uint64_t *__restrict__ D,
                                                         uint32_t rate, uint64_t *__restrict__ tmp, uint32_t *__restrict__ sa_be,
                                                         uint32_t *__restrict__ sa_ne, uint8_t *__restrict__ s_out) {
  __shared__ LocTables tb;
  loc_stage(ix, tb);
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t ng = (uint64_t)gridDim.x * (kLocThreads / G);
  for (uint64_t q0 = ((uint64_t)blockIdx.x * kLocThreads + threadIdx.x) / G; q0 < S; q0 += 2 * ng) {
    const uint64_t qq[2] = {q0, q0 + ng};
    uint64_t r[2], v[2], left[2];
    uint32_t ph[2];
    bool act[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      act[j] = qq[j] < S;
      r[j] = act[j] ? starts[qq[j]] : 0;
      left[j] = act[j] ? dist[qq[j]] : 0;
      v[j] = act[j] ? D[qq[j]] - 1 : 0;
      ph[j] = (uint32_t)(v[j] % rate);                 // steps to the next sampled SA value
      act[j] = act[j] && left[j] > 0;
    }
    while (act[0] || act[1]) {
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (act[j] && lc.t == 0) {
          if (TEXT) {
            sa_ne[r[j]] = (uint32_t)v[j];
            if (v[j] > 0 && v[j] < ix.n) s_out[v[j] - 1] = ix.bwt[r[j]];
          } else if (sa_be) sa_be[r[j]] = __builtin_bswap32((uint32_t)v[j]);
          else if (ph[j] == 0) tmp[v[j] / rate] = r[j];
        }
      bool mv[2];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (act[j]) {
          left[j]--;
          ph[j] = ph[j] == 0 ? rate - 1 : ph[j] - 1;
        }
        mv[j] = act[j] && left[j] > 0;
      }
      lf_steps<WIDE, LAYOUT, 2>(ix, tb, lc, r, mv);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (mv[j]) v[j]--;
        act[j] = mv[j];
      }
    }
  }
}

// ---------------------------------------------------------------- marks and samples from tmp
__device__ __forceinline__ void mark_pos(uint64_t r, uint64_t &blk, uint32_t &rem) {
  blk = r / kBlockBits;
  rem = (uint32_t)(r - blk * kBlockBits);
}

__global__ __launch_bounds__(kLocThreads) void k_mark_set(const uint64_t *__restrict__ tmp, uint64_t m, uint32_t *__restrict__ marks) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t b;
    uint32_t rem;
    mark_pos(tmp[j], b, rem);
    atomicOr(marks + b * 16 + 2 + (rem >> 5), 1u << (rem & 31u));
  }
}

__global__ __launch_bounds__(kLocThreads) void k_mark_count(const uint32_t *__restrict__ marks, uint64_t nb, uint32_t *__restrict__ cnt) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t c = 0;
#pragma unroll
    for (int d = 2; d < 16; d++) c += __popc(marks[b * 16 + d]);
    cnt[b] = c;
  }
}

__global__ __launch_bounds__(kLocThreads) void k_mark_headers(const uint64_t *__restrict__ pre, uint64_t nb, uint64_t *__restrict__ marks64) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x)
    marks64[b * 8] = pre[b];
}

// samples[rank(marks, tmp[j])] = j * rate
__global__ __launch_bounds__(kLocThreads) void k_mark_samples(const uint64_t *__restrict__ tmp, uint64_t m, const uint32_t *__restrict__ marks,
                                                             uint32_t rate, int wide, void *__restrict__ samples) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t b;
    uint32_t rem;
    mark_pos(tmp[j], b, rem);
    const uint32_t *blk = marks + b * 16;
    uint64_t rank = *reinterpret_cast<const uint64_t *>(blk);
#pragma unroll
    for (int d = 2; d < 16; d++) {
      const uint32_t first = 32u * (d - 2);
      const uint32_t w = blk[d];
      if (rem >= first + 32u) rank += __popc(w);
      else if (rem > first) rank += __popc(w & ((1u << (rem - first)) - 1u));
    }
    const uint64_t val = j * (uint64_t)rate;
    if (wide) static_cast<uint64_t *>(samples)[rank] = val;
    else static_cast<uint32_t *>(samples)[rank] = (uint32_t)val;
  }
}

// ---------------------------------------------------------------- the locate kernel
// Per step of a walk, two dependent round trips and three requests: (1) the marks block of the row and its BWT byte
// (one-hot: the byte; bytes layout: the row's 128-byte block line, which is also the line its rank query needs), then
// (2) the rank line of that byte (one-hot: the symbol's block; bytes layout: the checkpoint).  A marked row ends the walk
// with one more request, its sample.  W walks per lane group are stepped together; the group takes W new rows when all
// W have ended.  (A form in which an ended walk took the group's next row at once measured the same -- 1.07 against
// 1.05 ms for 1 M rows, DESIGN.md §12 -- and was left out.)
struct LocDev {
  const uint4 *marks;
  const void *samples;
  uint32_t wide;       // samples are u64
};

constexpr int kLocW = 2;

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kLocThreads) void k_locate(DevIndex ix, LocDev ld, const uint64_t *rows, uint64_t k,
                                                       const uint64_t *k_dev, uint64_t *out) {
  __shared__ LocTables tb;
  loc_stage(ix, tb);
  constexpr int G = Lay<LAYOUT>::G;
  constexpr int W = kLocW;
  const LaneConst lc = lane_const<G>();
  const LaneConst lm = lane_const<4>();            // the marks block is read by quads (an octet reads it twice: one request)
  if (k_dev) k = min(k, *k_dev);
  const uint64_t ng = (uint64_t)gridDim.x * (kLocThreads / G);
  const uint64_t g = ((uint64_t)blockIdx.x * kLocThreads + threadIdx.x) / G;
  uint64_t q[W], r[W];
  uint32_t steps[W];
  bool act[W], bad[W];
#pragma unroll
  for (int j = 0; j < W; j++) {
    q[j] = g + (uint64_t)j * ng;
    act[j] = q[j] < k;
    r[j] = act[j] ? rows[q[j]] : 0;
    bad[j] = r[j] >= ix.n;
    if (bad[j]) r[j] = ix.eof;                       // marked (SA 0): ends at once, reported as UINT64_MAX
    steps[j] = 0;
  }
  while (true) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < W; j++) any = any || act[j];
    if (!any) break;
    // round trip 1: marks block + BWT byte (bytes layout: the block line) of every active walk
    uint4 mw[W], bl[W];
    uint32_t rem[W], byte[W];
#pragma unroll
    for (int j = 0; j < W; j++) {
      mw[j] = make_uint4(0, 0, 0, 0);
      bl[j] = make_uint4(0, 0, 0, 0);
      byte[j] = 0;
      rem[j] = 0;
      if (act[j]) {
        uint32_t blk;
        split448(r[j], blk, rem[j]);
        mw[j] = load_line16((uint64_t)(uintptr_t)ld.marks + (uint64_t)blk * kBlockBytes + lm.t * 16u);
        if (LAYOUT == kLayoutBytes) bl[j] = load_line16((uint64_t)(uintptr_t)ix.bwt + (r[j] >> 7) * kByteBlock + lc.t * 16u);
        else byte[j] = ix.bwt[r[j]];
      }
    }
    // marked rows: sample + steps; the others take an LF step (round trip 2)
    RankReq rq[W];
    bool stepping[W];
#pragma unroll
    for (int j = 0; j < W; j++) {
      stepping[j] = false;
      rq[j].kind = 0;
      rq[j].sup = 0;
      if (!act[j]) continue;
      if (payload_bit(mw[j], rem[j], lm)) {
        const uint64_t rank = rank_finish<WIDE>(mw[j], rem[j], lm);
        if (lc.t == 0) {
          const uint64_t sa = ld.wide ? static_cast<const uint64_t *>(ld.samples)[rank]
                                      : (uint64_t) static_cast<const uint32_t *>(ld.samples)[rank];
          out[q[j]] = bad[j] ? ~0ull : sa + steps[j];
        }
        act[j] = false;
        continue;
      }
      stepping[j] = true;
      if (LAYOUT == kLayoutBytes) {
        // the byte of row r from the block line: lane (rem & 127) >> 4 holds it
        const uint32_t rr = (uint32_t)r[j] & 127u;
        const uint32_t bidx = rr & 15u, comp = bidx >> 2;
        const uint32_t sh = 32u * (comp & 1u);
        const uint32_t lo = (uint32_t)((((uint64_t)bl[j].y << 32) | bl[j].x) >> sh);
        const uint32_t hi = (uint32_t)((((uint64_t)bl[j].w << 32) | bl[j].z) >> sh);
        const uint32_t word = (uint32_t)((((uint64_t)hi << 32) | lo) >> (16u * (comp & 2u)));
        const uint32_t bt = __builtin_amdgcn_ubfe(word, 8u * (bidx & 3u), 8u);
        byte[j] = group_or<8>((rr >> 4) == lc.t ? bt : 0u);
        const uint32_t c = r[j] == ix.eof ? 0u : byte[j];
        byte[j] = c;
        const uint16_t s = tb.slot[c];
        if (s < kSlotEof) {
          const uint64_t blk = r[j] >> 7;
          rq[j].kind = 1;
          rq[j].w = bl[j];
          rq[j].rem = rr;
          rq[j].chk = lc.t == 0 ? ix.chk[blk * ix.nslots + s] : 0u;
          rq[j].sup = ix.sup ? ix.sup[(blk >> kSuperShift) * ix.nslots + s] : 0ull;
        } else {
          rq[j].sup = (s == kSlotEof && r[j] > ix.eof) ? 1 : 0;
        }
      } else {
        const uint32_t c = r[j] == ix.eof ? 0u : byte[j];
        byte[j] = c;
        rq[j] = rank_issue<LAYOUT>(ix, tb.slot[c], r[j], lc);
      }
    }
#pragma unroll
    for (int j = 0; j < W; j++)
      if (stepping[j]) {
        r[j] = tb.cf[byte[j]] + rank_complete<WIDE, LAYOUT>(rq[j], byte[j], lc);
        steps[j]++;
      }
    // next rows
    bool all_done = true;
#pragma unroll
    for (int j = 0; j < W; j++) all_done = all_done && !act[j];
#pragma unroll
    for (int j = 0; j < W; j++) {
      if (act[j] || !all_done) continue;
      if (q[j] >= k) continue;                        // this slot ran out of rows
      q[j] += (uint64_t)W * ng;
      if (q[j] >= k) continue;
      r[j] = rows[q[j]];
      bad[j] = r[j] >= ix.n;
      if (bad[j]) r[j] = ix.eof;
      steps[j] = 0;
      act[j] = true;
    }
  }
}

// ---------------------------------------------------------------- intervals: offsets and rows
// One workgroup: off[i] = sum of min(ep - sp, max_per) over the intervals before i, off[k] = the total.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_loc_scan(const uint64_t *__restrict__ sp, const uint64_t *__restrict__ ep, uint64_t k,
                                                          uint64_t max_per, uint64_t *__restrict__ off) {
  __shared__ uint64_t part[kScanThreads / 64];
  __shared__ uint64_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  for (uint64_t base = 0; base < k; base += kScanThreads) {
    const uint64_t i = base + threadIdx.x;
    uint64_t c = 0;
    if (i < k) {
      const uint64_t a = sp[i], b = ep[i];
      c = b > a ? min(b - a, max_per) : 0;
    }
    uint64_t x = c;                                  // inclusive scan in the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) part[wv] = x;
    __syncthreads();
    uint64_t before = carry_s;
    for (uint32_t w = 0; w < wv; w++) before += part[w];
    if (i < k) off[i] = before + x - c;
    __syncthreads();
    if (threadIdx.x == kScanThreads - 1) carry_s = before + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) off[k] = carry_s;
}

// One wave per interval: pos[off[i] + t] = sp[i] + t for the rows below cap (the locate kernel then works in place).
__global__ __launch_bounds__(kLocThreads) void k_loc_expand(const uint64_t *__restrict__ sp, const uint64_t *__restrict__ off, uint64_t k,
                                                           uint64_t cap, uint64_t *__restrict__ pos) {
  const uint64_t nw = (uint64_t)gridDim.x * (kLocThreads / 64);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t i = ((uint64_t)blockIdx.x * kLocThreads + threadIdx.x) / 64; i < k; i += nw) {
    const uint64_t o = off[i], c = off[i + 1] - o, a = sp[i];
    for (uint64_t t = lane; t < c && o + t < cap; t += 64) pos[o + t] = a + t;
  }
}

// ---------------------------------------------------------------- host side
static inline unsigned loc_grid(const Index *h, uint64_t work, int per_block) {
  uint64_t want = (work + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)h->cu_count * 8;
  if (want < 1) want = 1;
  return (unsigned)(want < cap ? want : cap);
}

static inline unsigned flat_grid(const Index *h, uint64_t work) {
  uint64_t want = (work + kLocThreads - 1) / kLocThreads;
  const uint64_t cap = (uint64_t)h->cu_count * 32;
  if (want < 1) want = 1;
  return (unsigned)(want < cap ? want : cap);
}

// How many starts: about n / 1024 (at least 4096 where n allows, at most 2^22); the threshold of the 32-bit hash.
static void start_plan(uint64_t n, uint64_t *target, uint32_t *thresh) {
  uint64_t t = std::min<uint64_t>(std::max<uint64_t>(n >> 10, 4096), 1ull << 22);
  t = std::min<uint64_t>(t, std::max<uint64_t>(n / 8, 1));
  *target = t;
  const double f = (double)t / (double)n * 4294967296.0;
  *thresh = f >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)f;
}

// Device bytes of the inversion's temporaries for n rows at `rate` (rate 0: the X.sa form, no marks or samples).
static uint64_t inv_temp_bytes(uint64_t n, uint32_t rate) {
  uint64_t target;
  uint32_t thresh;
  start_plan(n, &target, &thresh);
  const uint64_t smax = 2 * target + 1024;          // the starts are a binomial count around target: twice is never reached in practice
  const uint64_t runs = (n + kRunRows - 1) / kRunRows;
  uint64_t b = runs * 12 + smax * (8 + 4 + 8 + 2 * 4 + 2 * 8);
  if (rate) {
    const uint64_t m = (n - 1) / rate + 1, nb = n / kBlockBits + 1;
    b += m * 8 + nb * 12;
  }
  return b;
}

static uint64_t sample_bytes(uint64_t n, uint32_t rate) {
  const uint64_t m = (n - 1) / rate + 1, nb = n / kBlockBits + 1;
  return nb * kBlockBytes + m * (n > (1ull << 32) ? 8 : 4);
}

// The inversion: every segment's SA, then pass 2 into tmp (rate != 0) or into sa_be (X.sa).  Synchronises `st`.
static int invert(const Index *h, hipStream_t st, DevMem &mem, uint32_t rate, uint64_t *tmp, uint32_t *sa_be,
                  uint32_t *sa_ne = nullptr, uint8_t *s_out = nullptr) {
  const uint64_t n = h->n;
  uint64_t target;
  uint32_t thresh;
  start_plan(n, &target, &thresh);
  const uint64_t runs = (n + kRunRows - 1) / kRunRows;
  uint32_t *d_cnt = nullptr;
  uint64_t *d_off = nullptr, *d_starts = nullptr;
  DEV_ALLOC(mem, d_cnt, runs * 4, "locate samples");
  DEV_ALLOC(mem, d_off, runs * 8, "locate samples");
  k_inv_count<<<flat_grid(h, runs), kLocThreads, 0, st>>>(n, thresh, d_cnt, runs);
  HIP_TRY(hipGetLastError(), "k_inv_count");
  std::vector<uint32_t> cnt(runs);
  std::vector<uint64_t> off(runs);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, runs * 4, hipMemcpyDeviceToHost, st), "D2H(counts)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  uint64_t S = 0;
  for (uint64_t t = 0; t < runs; t++) { off[t] = S; S += cnt[t]; }
  if (S > 2 * target + 1024) {
    set_error("locate: " + std::to_string(S) + " segment starts, more than the build planned for");
    return FMX_ERR_NOMEM;
  }
  DEV_ALLOC(mem, d_starts, S * 8, "locate samples");
  HIP_TRY(hipMemcpyAsync(d_off, off.data(), runs * 8, hipMemcpyHostToDevice, st), "H2D(offsets)");
  k_inv_list<<<flat_grid(h, runs), kLocThreads, 0, st>>>(n, thresh, d_off, runs, d_starts);
  HIP_TRY(hipGetLastError(), "k_inv_list");
  // pass 1
  uint32_t *d_next = nullptr, *nx0 = nullptr, *nx1 = nullptr;
  uint64_t *d_dist = nullptr, *D0 = nullptr, *D1 = nullptr;
  DEV_ALLOC(mem, d_next, S * 4, "locate samples");
  DEV_ALLOC(mem, d_dist, S * 8, "locate samples");
  DEV_ALLOC(mem, nx0, S * 4, "locate samples");
  DEV_ALLOC(mem, nx1, S * 4, "locate samples");
  DEV_ALLOC(mem, D0, S * 8, "locate samples");
  DEV_ALLOC(mem, D1, S * 8, "locate samples");
#define SEG(W, L)                                                                                          \
  k_inv_segments<W, L><<<loc_grid(h, S, kLocThreads / Lay<L>::G), kLocThreads, 0, st>>>(h->dev, d_starts, S, thresh, \
                                                                                        d_next, d_dist)
  FMX_LAYOUT_DISPATCH(h, SEG);
#undef SEG
  HIP_TRY(hipGetLastError(), "k_inv_segments");
  // list ranking
  k_inv_rank_init<<<flat_grid(h, S), kLocThreads, 0, st>>>(d_next, d_dist, S, nx0, D0);
  HIP_TRY(hipGetLastError(), "k_inv_rank_init");
  int rounds = 1;
  while (rounds < 63 && (1ull << rounds) < S + 1) rounds++;
  for (int i = 0; i < rounds; i++) {
    k_inv_rank_round<<<flat_grid(h, S), kLocThreads, 0, st>>>(nx0, D0, S, nx1, D1);
    std::swap(nx0, nx1);
    std::swap(D0, D1);
  }
  HIP_TRY(hipGetLastError(), "k_inv_rank_round");
  uint64_t cyc = 0;
  HIP_TRY(hipMemcpyAsync(&cyc, D0, 8, hipMemcpyDeviceToHost, st), "D2H(cycle)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (cyc != n) {
    set_error("locate: the LF cycle through row 0 has " + std::to_string(cyc) + " of the index's " + std::to_string(n) +
              " rows -- not the BWT of one text (an i.i.d. byte string has several LF cycles)");
    return FMX_ERR_FORMAT;
  }
  // pass 2
#define FILL(W, L)                                                                                                      \
  do {                                                                                                                  \
    if (sa_ne)                                                                                                          \
      k_inv_fill<W, L, true><<<loc_grid(h, S, kLocThreads / Lay<L>::G), kLocThreads, 0, st>>>(h->dev, d_starts, S, d_dist, D0, \
                                                                                              1u, nullptr, nullptr, sa_ne, s_out); \
    else                                                                                                                \
      k_inv_fill<W, L, false><<<loc_grid(h, S, kLocThreads / Lay<L>::G), kLocThreads, 0, st>>>(h->dev, d_starts, S, d_dist, D0, \
                                                                                               rate ? rate : 1u, tmp, sa_be, nullptr, nullptr); \
  } while (0)
  FMX_LAYOUT_DISPATCH(h, FILL);
#undef FILL
  HIP_TRY(hipGetLastError(), "k_inv_fill");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  return FMX_OK;
}

static int loc_supported(const Index *h) {
  if (h->block_mode) {
    set_error("locate needs the index of one text: fmx_open_block handles (one merge block) have no suffix array");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n >= kOneHotMaxN) {
    set_error("locate: indexes of 2^37 rows and more are not supported");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

int locate_check(const Index *h) { return loc_supported(h); }

// The samples at the handle's rate into h->loc: the inversion, the marks as rank blocks, the samples in row order.
static int locate_build(const Index *h, hipStream_t st, DevMem &mem) {
  const uint64_t n = h->n;
  const uint32_t rate = (uint32_t)h->policy.locate_sample.load(std::memory_order_relaxed);
  const uint64_t m = (n - 1) / rate + 1, nb = n / kBlockBits + 1;
  const bool wide = n > (1ull << 32);
  const uint64_t keep = sample_bytes(n, rate);
  int rc = device_room(inv_temp_bytes(n, rate) + keep, "the locate samples");
  if (rc) return rc;
  void *d_marks = nullptr, *d_samples = nullptr;
  uint64_t *tmp = nullptr, *d_pre = nullptr;
  uint32_t *d_cnt = nullptr;
  DEV_ALLOC(mem, d_marks, nb * kBlockBytes, "locate samples");
  DEV_ALLOC(mem, d_samples, m * (wide ? 8 : 4), "locate samples");
  DEV_ALLOC(mem, tmp, m * 8, "locate samples");
  DEV_ALLOC(mem, d_cnt, nb * 4, "locate samples");
  DEV_ALLOC(mem, d_pre, nb * 8, "locate samples");
  if ((rc = invert(h, st, mem, rate, tmp, nullptr))) return rc;
  HIP_TRY(hipMemsetAsync(d_marks, 0, nb * kBlockBytes, st), "hipMemset(marks)");
  k_mark_set<<<flat_grid(h, m), kLocThreads, 0, st>>>(tmp, m, (uint32_t *)d_marks);
  k_mark_count<<<flat_grid(h, nb), kLocThreads, 0, st>>>((const uint32_t *)d_marks, nb, d_cnt);
  HIP_TRY(hipGetLastError(), "k_mark_count");
  std::vector<uint32_t> cnt(nb);
  std::vector<uint64_t> pre(nb);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, nb * 4, hipMemcpyDeviceToHost, st), "D2H(mark counts)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  uint64_t acc = 0;
  for (uint64_t b = 0; b < nb; b++) { pre[b] = acc; acc += cnt[b]; }
  if (acc != m) {
    set_error("locate: " + std::to_string(acc) + " rows marked, " + std::to_string(m) + " expected -- not the BWT of one text");
    return FMX_ERR_FORMAT;
  }
  HIP_TRY(hipMemcpyAsync(d_pre, pre.data(), nb * 8, hipMemcpyHostToDevice, st), "H2D(mark counts)");
  k_mark_headers<<<flat_grid(h, nb), kLocThreads, 0, st>>>(d_pre, nb, (uint64_t *)d_marks);
  k_mark_samples<<<flat_grid(h, m), kLocThreads, 0, st>>>(tmp, m, (const uint32_t *)d_marks, rate, wide ? 1 : 0, d_samples);
  HIP_TRY(hipGetLastError(), "k_mark_samples");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  mem.keep(d_marks);
  mem.keep(d_samples);
  h->loc.marks = d_marks;
  h->loc.samples = d_samples;
  h->loc.rate = rate;
  h->loc.wide = wide;
  h->loc.bytes = keep;
  return FMX_OK;
}

int locate_prepare(const Index *h, hipStream_t st) {
  if (const int rc = loc_supported(h)) return rc;
  return build_locked(h->loc, st, "the locate samples are built by fmx_prepare(FMX_PREPARE_LOCATE) or a first locate call outside a stream capture",
                      [&](DevMem &mem) { return locate_build(h, st, mem); });
}

int locate_write_sa(const Index *h, hipStream_t st, uint32_t *d_sa_be) {
  int rc = loc_supported(h);
  if (rc) return rc;
  DevMem mem;
  return invert(h, st, mem, 0, nullptr, d_sa_be);
}

uint64_t locate_write_sa_bytes(const Index *h) { return inv_temp_bytes(h->n, 0) + h->n * 4; }

// The LCP array's inputs (fmx_lcp.hip): d_sa[row] = SA[row] and d_s[v] = s[v] for v < n - 1; the caller has zeroed d_s, so
// the sentinel s[n - 1] = 0 is there already.
int locate_invert_text(const Index *h, hipStream_t st, uint32_t *d_sa, uint8_t *d_s) {
  int rc = loc_supported(h);
  if (rc) return rc;
  DevMem mem;
  return invert(h, st, mem, 0, nullptr, nullptr, d_sa, d_s);
}

uint64_t locate_invert_text_bytes(const Index *h) { return inv_temp_bytes(h->n, 0); }

// The inverse-SA samples' input (fmx_extract.hip): pass 2's tmp itself, into the caller's array.
int locate_invert_rows(const Index *h, hipStream_t st, uint32_t rate, uint64_t *d_tmp) {
  int rc = loc_supported(h);
  if (rc) return rc;
  DevMem mem;
  return invert(h, st, mem, rate, d_tmp, nullptr);
}

uint64_t locate_invert_rows_bytes(const Index *h) { return inv_temp_bytes(h->n, 0); }

static LocDev loc_dev(const Index *h) {
  LocDev ld;
  ld.marks = (const uint4 *)h->loc.marks;
  ld.samples = h->loc.samples;
  ld.wide = h->loc.wide ? 1u : 0u;
  return ld;
}

static hipError_t launch_locate_k(const Index *h, const void *d_rows, uint64_t k, const uint64_t *k_dev, void *d_out,
                                  hipStream_t st) {
  if (!k) return hipSuccess;
  const LocDev ld = loc_dev(h);
#define CALL(W, L)                                                                                                   \
  k_locate<W, L><<<loc_grid(h, (k + kLocW - 1) / kLocW, kLocThreads / Lay<L>::G), kLocThreads, 0, st>>>(           \
      h->dev, ld, (const uint64_t *)d_rows, k, k_dev, (uint64_t *)d_out)
  FMX_LAYOUT_DISPATCH(h, CALL);
#undef CALL
  return hipGetLastError();
}

hipError_t launch_locate(const Index *h, const void *d_rows, uint64_t k, void *d_out, hipStream_t st) {
  return launch_locate_k(h, d_rows, k, nullptr, d_out, st);
}

hipError_t launch_locate_intervals(const Index *h, const void *d_sp, const void *d_ep, uint64_t k, uint64_t max_per,
                                   void *d_off, void *d_pos, uint64_t cap, hipStream_t st) {
  k_loc_scan<<<1, kScanThreads, 0, st>>>((const uint64_t *)d_sp, (const uint64_t *)d_ep, k, max_per ? max_per : ~0ull,
                                         (uint64_t *)d_off);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !cap || !k) return e;
  k_loc_expand<<<loc_grid(h, k, kLocThreads / 64), kLocThreads, 0, st>>>((const uint64_t *)d_sp, (const uint64_t *)d_off, k,
                                                                         cap, (uint64_t *)d_pos);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_locate_k(h, d_pos, cap, (const uint64_t *)d_off + k, d_pos, st);
}

}  // namespace fmx
