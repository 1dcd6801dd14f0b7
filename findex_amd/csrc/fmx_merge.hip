// fmx_merge.hip -- append: new text B merged into the index of A on the device (include/fmx.h, "append").
//
// The reference grows an index by BWTMerger2.merge (bwtmerger.scala:654-1261): sort a block, compute for each of its
// suffixes how many suffixes of the existing index lie before it (calcGaps, :981-1023: one chain of rank steps), interleave.
// Here, with R = reverse(B) and s_T = R . s_A:
//
//   piece       : tail(A, M) + B suffix-sorted by the existing construction (fmx_sufsort.hip), its LCP array by fmx_lcp.hip.
//                 The rows with SA < b, in order, are the order of the new suffixes X_j = R[j..] . s_A among themselves --
//                 provided no comparison reached the piece's end: k_mrg_check.
//   k_mrg_walk  : r_j = rows of A below X_j.  r_b = A's eof row, r_j = C[c] + rank(c, r_{j+1}) with c = R[j]: b dependent
//                 steps.  One lane group per segment of S positions starts W positions early with the interval [0, n) and
//                 walks left; with sp == ep the value is r_j, and an empty interval stays empty.  Positions of the segment
//                 whose interval is not empty are its right end: nun[segment] counts them.
//   k_mrg_fixup : one walker per maximal run of such positions, from the exact rank to the run's right, across segments.
//                 The runs are read from nun[], which this kernel never writes: which group walks what does not depend on
//                 timing.
//   k_mrg_place : new suffix of kept rank q -> output row pos[q] = r_j + q, its byte R[j - 1] (j == 0: the new eof row).
//   k_mrg_mono  : pos[] must increase strictly and stay below n + b (an internal error otherwise; it also keeps
//                 k_mrg_emit inside its buffers).
//   k_mrg_emit  : per tile of FMX_MERGE_TILE output rows: binary search for the tile's first new suffix, marks in LDS, a
//                 prefix count, the next rows of A (staged through LDS with 16-byte loads) with A's eof row replaced.
//
// Every kernel is a separate launch on the caller's stream; none waits for another workgroup; all sums are integer atomics.
#include <fmx.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "fmx_device.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kMrgThreads = 256;
constexpr uint32_t kMrgTile = FMX_MERGE_TILE;
constexpr uint32_t kMrgRowsPerThread = kMrgTile / kMrgThreads;       // 16: one 16-byte store
static_assert(kMrgRowsPerThread == 16, "k_mrg_emit writes one uint4 per thread");
constexpr uint64_t kUnresolved = ~0ull;
// words of the result buffer
constexpr int kResBad = 0, kResEofQ = 1, kResEofRow = 2, kResFixSteps = 3, kResFixLongest = 4, kResFixRuns = 5, kResHist = 8;
constexpr int kResWords = kResHist + 256;

static unsigned mrg_grid(uint64_t items, int cu_count) {
  const uint64_t want = (items + kMrgThreads - 1) / kMrgThreads;
  const uint64_t cap = (uint64_t)std::max(cu_count, 1) * 16;
  return (unsigned)std::max<uint64_t>(1, std::min(want, cap));
}

// piece = tail(A, M) + B; tail_rev = s_A[0 .. M) as the Psi walk wrote it (A's last byte first)
__global__ __launch_bounds__(kMrgThreads) void k_mrg_piece(const uint8_t *__restrict__ tail_rev, uint64_t M,
                                                           const uint8_t *__restrict__ text, uint64_t b,
                                                           uint8_t *__restrict__ piece) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M + b; i += stride)
    piece[i] = i < M ? tail_rev[M - 1 - i] : text[i - M];
}

// A new suffix p < b whose common prefix with a neighbouring row reaches position b + M of the piece's s was compared
// against the piece's sentinel, not against the rest of s_A: the piece is too short.
__global__ __launch_bounds__(kMrgThreads) void k_mrg_check(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ lcp,
                                                           uint64_t np, uint64_t b, uint64_t M,
                                                           unsigned long long *__restrict__ res) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < np; r += stride) {
    const uint64_t p = sa[r];
    if (p >= b) continue;
    const uint32_t above = r ? lcp[r - 1] : 0u, below = lcp[r];
    bad |= p + (uint64_t)max(above, below) >= b + M;
  }
  if (bad) atomicOr(res + kResBad, 1ull);
}

__global__ __launch_bounds__(kMrgThreads) void k_mrg_keep(const uint32_t *__restrict__ sa, uint64_t np, uint64_t b,
                                                          uint32_t *__restrict__ keep) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < np; r += stride) keep[r] = sa[r] < b ? 1u : 0u;
}

// 256-bin histogram of B into res[kResHist ..]
__global__ __launch_bounds__(kMrgThreads) void k_mrg_hist(const uint8_t *__restrict__ text, uint64_t b,
                                                          unsigned long long *__restrict__ res) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t per = 1ull << 16;                 // bytes per stretch: the 32-bit bins cannot overflow
  for (uint64_t c0 = (uint64_t)blockIdx.x * per; c0 < b; c0 += (uint64_t)gridDim.x * per) {
    const uint64_t c1 = min_u64(c0 + per, b);
    for (uint64_t i = c0 + threadIdx.x; i < c1; i += kMrgThreads) atomicAdd(&h[text[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(res + kResHist + threadIdx.x, (unsigned long long)h[threadIdx.x]);
    h[threadIdx.x] = 0;
    __syncthreads();
  }
}

// C[c] + rank(c, r): the backward step of an empty interval [r, r)
template <bool WIDE, uint32_t LAYOUT>
__device__ __forceinline__ uint64_t mrg_step1(const DevIndex &ix, const uint64_t *s_cf, const uint16_t *s_slot, uint32_t c,
                                              uint64_t r, const LaneConst &lc) {
  return s_cf[c] + rank_excl<WIDE, LAYOUT>(ix, c, s_slot[c], r, lc);
}

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kMrgThreads) void k_mrg_walk(DevIndex ix, const uint8_t *__restrict__ text, uint64_t b, uint32_t S,
                                                          uint32_t W, uint64_t nseg, uint64_t *__restrict__ rank,
                                                          uint32_t *__restrict__ nun) {
  __shared__ uint64_t s_cf[256];
  __shared__ uint16_t s_slot[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) { s_cf[c] = ix.cf[c]; s_slot[c] = ix.slot[c]; }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t ngroups = (uint64_t)gridDim.x * (kMrgThreads / G);
  for (uint64_t seg = ((uint64_t)blockIdx.x * kMrgThreads + threadIdx.x) / G; seg < nseg; seg += ngroups) {
    const uint64_t lo = seg * S, hi = min_u64(lo + S, b), start = min_u64(hi + W, b);
    uint64_t sp = 0, ep = ix.n;
    if (start == b) sp = ep = ix.eof;              // r_b: s_A itself is the row A's eof names
    uint32_t un = 0;
    for (uint64_t j = start; j-- > lo;) {
      const uint32_t c = text[b - 1 - j];          // R[j]
      if (sp == ep) {
        sp = ep = mrg_step1<WIDE, LAYOUT>(ix, s_cf, s_slot, c, sp, lc);
      } else {
        backward_step<WIDE, LAYOUT>(ix, c, s_slot[c], s_cf[c], lc, sp, ep);
      }
      if (j < hi) {
        const bool exact = sp == ep;
        if (lc.t == 0) rank[j] = exact ? sp : kUnresolved;
        un += exact ? 0u : 1u;
      }
    }
    if (lc.t == 0) nun[seg] = un;
  }
}

// Segment `seg` ends a run when its right end is unresolved and the position right of it (the left end of segment seg + 1)
// is exact.  The walker then takes the unresolved right ends of seg, seg - 1, .. for as long as each segment before was
// unresolved throughout.
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kMrgThreads) void k_mrg_fixup(DevIndex ix, const uint8_t *__restrict__ text, uint64_t b, uint32_t S,
                                                           uint64_t nseg, uint64_t *__restrict__ rank,
                                                           const uint32_t *__restrict__ nun, unsigned long long *__restrict__ res) {
  __shared__ uint64_t s_cf[256];
  __shared__ uint16_t s_slot[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) { s_cf[c] = ix.cf[c]; s_slot[c] = ix.slot[c]; }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t ngroups = (uint64_t)gridDim.x * (kMrgThreads / G);
  for (uint64_t seg = ((uint64_t)blockIdx.x * kMrgThreads + threadIdx.x) / G; seg + 1 < nseg; seg += ngroups) {
    if (nun[seg] == 0) continue;
    const uint64_t right_lo = (seg + 1) * S, right_len = min_u64(right_lo + S, b) - right_lo;
    if (nun[seg + 1] == right_len) continue;       // the run goes on to the right: its walker starts there
    uint64_t r = rank[right_lo];                   // exact, and no walker writes it
    uint64_t steps = 0;
    for (uint64_t s = seg;; s--) {
      const uint64_t lo = s * S, hi = min_u64(lo + S, b);
      const uint64_t cnt = nun[s];
      for (uint64_t j = hi; j-- > hi - cnt;) {
        r = mrg_step1<WIDE, LAYOUT>(ix, s_cf, s_slot, text[b - 1 - j], r, lc);
        if (lc.t == 0) rank[j] = r;
      }
      steps += cnt;
      if (cnt < hi - lo || s == 0 || nun[s - 1] == 0) break;
    }
    if (lc.t == 0) {
      atomicAdd(res + kResFixSteps, (unsigned long long)steps);
      atomicMax(res + kResFixLongest, (unsigned long long)steps);
      atomicAdd(res + kResFixRuns, 1ull);
    }
  }
}

// excl = the exclusive sum of keep: row r of the piece with SA = p < b is new suffix X_p with kept rank excl[r]
__global__ __launch_bounds__(kMrgThreads) void k_mrg_place(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ excl,
                                                           uint64_t np, const uint8_t *__restrict__ text, uint64_t b,
                                                           const uint64_t *__restrict__ rank, uint64_t *__restrict__ pos,
                                                           uint8_t *__restrict__ nb, unsigned long long *__restrict__ res) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < np; r += stride) {
    const uint64_t p = sa[r];
    if (p >= b) continue;
    const uint64_t q = excl[r];
    if (q >= b) continue;                          // (a broken scan stays in bounds; k_mrg_mono then sees a hole)
    pos[q] = rank[p] + q;
    nb[q] = p ? text[b - p] : (uint8_t)0;          // R[p - 1]
    if (p == 0) res[kResEofQ] = q;
  }
}

__global__ __launch_bounds__(kMrgThreads) void k_mrg_mono(const uint64_t *__restrict__ pos, uint64_t b, uint64_t nT,
                                                          unsigned long long *__restrict__ res) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < b; q += stride) {
    const uint64_t p = pos[q];
    bad |= p >= nT || (q && pos[q - 1] >= p);
  }
  if (bad) atomicOr(res + kResBad, 2ull);
}

__global__ __launch_bounds__(kMrgThreads) void k_mrg_emit(const uint8_t *__restrict__ bwt_a, uint64_t n_a, uint64_t eof_a,
                                                          const uint8_t *__restrict__ text, const uint64_t *__restrict__ pos,
                                                          const uint8_t *__restrict__ nb, uint64_t b, uint64_t nT,
                                                          uint8_t *__restrict__ out, int aligned) {
  __shared__ uint4 s_mark4[kMrgTile / 16];
  __shared__ uint8_t s_new[kMrgTile];
  __shared__ uint4 s_a4[kMrgTile / 16 + 1];
  __shared__ uint32_t s_wave[kMrgThreads / 64];
  uint8_t *s_mark = reinterpret_cast<uint8_t *>(s_mark4);
  const uint8_t *s_a = reinterpret_cast<const uint8_t *>(s_a4);
  const uint32_t tid = threadIdx.x;
  const uint64_t ntiles = (nT + kMrgTile - 1) / kMrgTile;
  const uint8_t eof_byte = text[0];                // A's eof row now stands before R's last byte
  const uint64_t a_pad = (n_a + 15) & ~15ull;      // readable: the handle's BWT is padded to whole 128-byte blocks
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t t0 = tile * kMrgTile, t1 = min_u64(t0 + kMrgTile, nT);
    uint64_t lo = 0, hi = b;                       // q0 = the first new suffix at or after row t0
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (pos[mid] < t0) lo = mid + 1; else hi = mid;
    }
    const uint64_t q0 = lo;
    s_mark4[tid] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for (uint64_t q = q0 + tid; q < b; q += kMrgThreads) {
      const uint64_t p = pos[q];
      if (p >= t1) break;
      s_mark[p - t0] = 1;
      s_new[p - t0] = nb[q];
    }
    // the rows of A this tile takes begin at a0: q0 new suffixes stand before row t0
    const uint64_t a0 = t0 - q0, ab = a0 & ~15ull;
    for (uint32_t u = tid; u < kMrgTile / 16 + 1; u += kMrgThreads) {
      const uint64_t at = ab + 16ull * u;
      s_a4[u] = at < a_pad ? *reinterpret_cast<const uint4 *>(bwt_a + at) : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    const uint4 m = s_mark4[tid];
    const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
    const uint32_t cnt = ((mw[0] + mw[1] + mw[2] + mw[3]) * 0x01010101u) >> 24;      // 16 bytes of 0 / 1
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
      if ((int)(tid & 63u) >= d) incl += y;
    }
    if ((tid & 63u) == 63u) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - cnt;
    for (uint32_t w = 0; w < (tid >> 6); w++) before += s_wave[w];
    const uint32_t my = tid * kMrgRowsPerThread;
    uint32_t ai = (uint32_t)(a0 - ab) + my - before;          // byte of the stage that holds my first row of A
    const uint64_t eof_at = eof_a - ab;                       // (wraps to a value no ai has when eof_a < ab)
    uint32_t ow[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const bool is_new = (mw[i >> 2] >> (8 * (i & 3))) & 1u;
      uint32_t v;
      if (is_new) {
        v = s_new[my + i];
      } else {
        v = (uint64_t)ai == eof_at ? eof_byte : s_a[ai];
        ai++;
      }
      ow[i >> 2] |= v << (8 * (i & 3));
    }
    const uint64_t row0 = t0 + my;
    if (aligned && row0 + 16 <= t1) {
      *reinterpret_cast<uint4 *>(out + row0) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++)
        if (row0 + i < t1) out[row0 + i] = (uint8_t)(ow[i >> 2] >> (8 * (i & 3)));
    }
    __syncthreads();
  }
}

// the new eof row's filler (sa2BWT, bwtmerger.scala:799-806): the byte of the row above, of the row below for row 0
__global__ void k_mrg_eof_fill(const uint64_t *__restrict__ pos, uint64_t b, uint64_t nT, uint8_t *__restrict__ out,
                               unsigned long long *__restrict__ res) {
  const uint64_t q = res[kResEofQ];
  if (q >= b) { atomicOr(res + kResBad, 4ull); return; }
  const uint64_t e = pos[q];
  if (e >= nT) { atomicOr(res + kResBad, 4ull); return; }
  out[e] = e ? out[e - 1] : out[1];                // nT >= 3
  res[kResEofRow] = e;
}

// ---------------------------------------------------------------- host side
namespace {

thread_local fmx_merge_stats g_merge_last = {};

struct MergeOpts {
  uint64_t context, max_context;
  uint32_t segment, warmup;
};

constexpr uint64_t kMaxPiece = 0xfffffffeull;       // the suffix sort's limit

int resolve_opts(const fmx_merge_opts *o, uint64_t len, MergeOpts *r) {
  r->context = FMX_MERGE_CONTEXT;
  r->max_context = ~0ull;
  r->segment = FMX_MERGE_SEGMENT;
  r->warmup = FMX_MERGE_WARMUP;
  if (o) {
    for (uint32_t w : o->reserved)
      if (w) return arg_fail("fmx_merge_opts.reserved must be 0");
    if (o->context) r->context = o->context;
    if (o->max_context) r->max_context = o->max_context;
    if (o->segment) { r->segment = o->segment; r->warmup = o->warmup; }
  }
  if (len > kMaxPiece || r->context > kMaxPiece - len) {
    set_error("append of " + std::to_string(len) + " bytes with a context of " + std::to_string(r->context) +
              ": the piece takes at most 2^32 - 2 bytes (u32 suffix indices)");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

// What is decided before the device is touched (include/fmx.h lists the order).
int merge_args(const fmx_index *idx, const void *text, uint64_t len, const uint8_t *host_text, const fmx_merge_opts *opts,
               const void *out, uint64_t *n_t, MergeOpts *mo) {
  if (!text) return arg_fail("text is null");
  if (!out) return arg_fail("output is null");
  if (len == 0) return arg_fail("len must be >= 1");
  if (const int rc = resolve_opts(opts, len, mo)) return rc;
  if (host_text && std::memchr(host_text, 0, (size_t)len)) {
    set_error("the text contains byte 0 (findex's readers escape it; counts[0] must be 0)");
    return FMX_ERR_UNSUPPORTED;
  }
  if (!idx) return arg_fail("idx is null");
  const Index *h = H(idx);
  if (h->block_mode) {
    set_error("append needs the index of one text: fmx_open_block handles (one merge block) are not one");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n + len >= (1ull << 38)) {
    set_error("append: n + len >= 2^38 is not supported");
    return FMX_ERR_UNSUPPORTED;
  }
  *n_t = h->n + len;
  return FMX_OK;
}

uint64_t piece_hold_bytes(uint64_t M, uint64_t b) {          // what a piece keeps while it is built and checked
  const uint64_t np = M + b + 1;
  return (M + 16) + (M + b) + np + 4 * np + 4 * np + 64;      // tail, text, BWT, suffix array, LCP / keep
}
uint64_t piece_temp_bytes(uint64_t M, uint64_t b) {          // the largest of its temporaries
  const uint64_t np = M + b + 1;
  return std::max<uint64_t>({sufsort_peak_bytes(M + b, true), lcp_text_bytes(np) + lcp_core_bytes(np), ScanSpace::bytes(np)});
}
uint64_t place_bytes(uint64_t b, uint64_t nseg) { return 8 * b + 8 * b + b + 4 * nseg + 8 * kResWords + 256; }

struct Piece {                  // the device buffers of one piece; freed with the object
  DevMem mem;
  uint8_t *tail = nullptr, *text = nullptr, *bwt = nullptr;
  uint32_t *sa = nullptr, *lcp = nullptr;
};

template <bool WIDE, uint32_t LAYOUT>
hipError_t launch_walks(const Index *h, const uint8_t *d_text, uint64_t b, const MergeOpts &mo, uint64_t nseg, uint64_t *rank,
                        uint32_t *nun, unsigned long long *res, Events<8> &ev, hipStream_t st) {
  constexpr int G = Lay<LAYOUT>::G;
  const uint64_t per_block = kMrgThreads / G;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nseg + per_block - 1) / per_block, (uint64_t)std::max(h->cu_count, 1) * 64));
  hipError_t e;
  if ((e = ev.record(2, st)) != hipSuccess) return e;
  k_mrg_walk<WIDE, LAYOUT><<<grid, kMrgThreads, 0, st>>>(h->dev, d_text, b, mo.segment, mo.warmup, nseg, rank, nun);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = ev.record(3, st)) != hipSuccess) return e;
  k_mrg_fixup<WIDE, LAYOUT><<<grid, kMrgThreads, 0, st>>>(h->dev, d_text, b, mo.segment, nseg, rank, nun, res);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return ev.record(4, st);
}

// The merge proper: d_text[b] appended to h, the merged BWT (h->n + b bytes) into d_out.  Arguments are checked by the caller;
// `extra` = device bytes the caller still allocates, counted in the free-memory check.  Synchronises `st`.
int merge_core(const Index *h, const uint8_t *d_text, uint64_t b, const MergeOpts &mo, uint8_t *d_out, uint64_t *eof,
               int64_t counts[256], hipStream_t st, uint64_t extra) {
  const uint64_t n_a = h->n, a = n_a - 1, n_t = n_a + b;
  const uint64_t S = mo.segment, nseg = (b + S - 1) / S;
  fmx_merge_stats stats = {};
  Events<8> ev;                 // 0 .. 1 piece, 2 .. 3 walk, 3 .. 4 fix-up, 5 .. 6 order and emit
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *res = nullptr;
  uint64_t *d_sps = nullptr;
  uint32_t *d_tail_len = nullptr;
  // ---- the piece, with a longer tail of A until no comparison of a new suffix reaches its end
  uint64_t context = mo.context;
  Piece *piece = nullptr;
  struct PieceGuard { Piece *&p; ~PieceGuard() { delete p; } } guard{piece};
  uint64_t M = 0;
  bool first = true;
  for (;;) {
    M = std::min(a, context);
    delete piece;
    piece = nullptr;
    const uint64_t need = piece_hold_bytes(M, b) + piece_temp_bytes(M, b) + place_bytes(b, nseg) + extra;
    stats.need_bytes = need;
    if (const int rc = device_room(need, "append of " + std::to_string(b) + " bytes with a context of " + std::to_string(M))) return rc;
    if (first) {
      DEV_ALLOC(mem, res, 8 * kResWords, "append");
      DEV_ALLOC(mem, d_sps, 8, "append");
      DEV_ALLOC(mem, d_tail_len, 4, "append");
      HIP_TRY(hipMemsetAsync(res, 0, 8 * kResWords, st), "hipMemsetAsync");
      HIP_TRY(hipMemcpyAsync(d_sps, &h->eof, 8, hipMemcpyHostToDevice, st), "H2D(eof)");
      HIP_TRY(ev.record(0, st), "hipEventRecord");
      first = false;
    }
    piece = new Piece();
    const uint64_t np = M + b + 1;
    DEV_ALLOC(piece->mem, piece->tail, M + 16, "append piece");
    DEV_ALLOC(piece->mem, piece->text, M + b, "append piece");
    DEV_ALLOC(piece->mem, piece->bwt, np, "append piece");
    DEV_ALLOC(piece->mem, piece->sa, 4 * np, "append piece");
    DEV_ALLOC(piece->mem, piece->lcp, 4 * np, "append piece");
    if (M) {
      // s_A[0 .. M): the first bytes of the rows eof, Psi eof, Psi^2 eof, .. (the path of fmx_next_substr)
      const hipError_t he = launch_next_substr(h, d_sps, 1, (uint32_t)M, piece->tail, d_tail_len, st);
      if (he == hipErrorStreamCaptureUnsupported) return FMX_ERR_HIP;
      HIP_TRY(he, "select directory / k_next_substr");
      uint32_t got = 0;
      HIP_TRY(hipMemcpyAsync(&got, d_tail_len, 4, hipMemcpyDeviceToHost, st), "D2H(tail length)");
      HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
      if (got != M) {
        set_error("the index is not the BWT of one text: its Psi walk from the eof row ends after " + std::to_string(got) + " bytes");
        return FMX_ERR_FORMAT;
      }
    }
    k_mrg_piece<<<mrg_grid(M + b, h->cu_count), kMrgThreads, 0, st>>>(piece->tail, M, d_text, b, piece->text);
    HIP_TRY(hipGetLastError(), "k_mrg_piece");
    uint64_t p_eof = 0;
    int64_t p_counts[256];
    if (const int rc = sufsort_bwt(piece->text, M + b, piece->bwt, piece->sa, &p_eof, p_counts, st, 0)) return rc;
    stats.rounds++;
    if (M == a) break;          // the piece is all of A + B: nothing to check
    {
      DevMem tmp;
      uint8_t *s = nullptr;
      DEV_ALLOC(tmp, s, lcp_text_bytes(np), "append piece");
      lcp_reverse_text(piece->text, M + b, s, h->cu_count, st);
      HIP_TRY(hipGetLastError(), "k_lcp_reverse");
      if (const int rc = lcp_core(s, np, piece->sa, piece->lcp, h->cu_count, st, nullptr)) return rc;
    }
    k_mrg_check<<<mrg_grid(np, h->cu_count), kMrgThreads, 0, st>>>(piece->sa, piece->lcp, np, b, M, res);
    HIP_TRY(hipGetLastError(), "k_mrg_check");
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, res + kResBad, 8, hipMemcpyDeviceToHost, st), "D2H(check)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (!bad) break;
    HIP_TRY(hipMemsetAsync(res + kResBad, 0, 8, st), "hipMemsetAsync");
    const uint64_t next = context > kMaxPiece / 2 ? kMaxPiece : 2 * context;
    if (next > mo.max_context || std::min(a, next) > kMaxPiece - b) {
      set_error("append: B repeats the end of A beyond a context of " + std::to_string(M) + " bytes; the next piece needs context " +
                std::to_string(next) + (next > mo.max_context ? ", above max_context " + std::to_string(mo.max_context)
                                                                : std::string(", beyond the suffix sort's 2^32 - 2 bytes")));
      return FMX_ERR_UNSUPPORTED;
    }
    context = next;
  }
  stats.context = M;
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  const uint64_t np = M + b + 1;
  // ---- gap ranks
  uint64_t *rank = nullptr, *pos = nullptr;
  uint32_t *nun = nullptr;
  ScanSpace scan;
  uint8_t *nb = nullptr;
  DEV_ALLOC(mem, rank, 8 * b, "append ranks");
  DEV_ALLOC(mem, pos, 8 * b, "append rows");
  DEV_ALLOC(mem, nb, b, "append bytes");
  DEV_ALLOC(mem, nun, 4 * nseg, "append segments");
  if (const int arc = scan.alloc(mem, np, "append scan")) return arc;
  hipError_t he = hipSuccess;
#define MRG_WALKS(WIDE, LAYOUT) he = launch_walks<WIDE, LAYOUT>(h, d_text, b, mo, nseg, rank, nun, res, ev, st)
  FMX_LAYOUT_DISPATCH(h, MRG_WALKS);
#undef MRG_WALKS
  HIP_TRY(he, "k_mrg_walk / k_mrg_fixup");
  {                                                // what the walk kernel steps: every position once, and each segment's warm-up
    uint64_t full = nseg;                          // segments 0 .. full - 1 have all W positions to their right
    stats.walk_steps = b;
    while (full > 0) {
      const uint64_t hi = std::min(full * S, b);
      if (b - hi >= mo.warmup) break;
      stats.walk_steps += b - hi;
      full--;
    }
    stats.walk_steps += full * mo.warmup;
  }
  // ---- order of the new suffixes, rows, emit
  HIP_TRY(ev.record(5, st), "hipEventRecord");
  uint32_t *keep = piece->lcp;                     // (the check is done: the LCP buffer holds the keep flags and their sum)
  k_mrg_keep<<<mrg_grid(np, h->cu_count), kMrgThreads, 0, st>>>(piece->sa, np, b, keep);
  HIP_TRY(hipGetLastError(), "k_mrg_keep");
  HIP_TRY(scan.sum(keep, np, true, st), "scan");
  k_mrg_place<<<mrg_grid(np, h->cu_count), kMrgThreads, 0, st>>>(piece->sa, keep, np, d_text, b, rank, pos, nb, res);
  HIP_TRY(hipGetLastError(), "k_mrg_place");
  k_mrg_mono<<<mrg_grid(b, h->cu_count), kMrgThreads, 0, st>>>(pos, b, n_t, res);
  HIP_TRY(hipGetLastError(), "k_mrg_mono");
  unsigned long long host_res[kResWords];
  HIP_TRY(hipMemcpyAsync(host_res, res, 8, hipMemcpyDeviceToHost, st), "D2H(check)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (host_res[kResBad]) {
    set_error("append: the new suffixes' rows do not increase along their order (internal error)");
    return FMX_ERR_HIP;
  }
  const uint64_t ntiles = (n_t + kMrgTile - 1) / kMrgTile;
  const unsigned egrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)std::max(h->cu_count, 1) * 32));
  const int aligned = ((uintptr_t)d_out & 15u) == 0;
  k_mrg_emit<<<egrid, kMrgThreads, 0, st>>>(h->dev.bwt, n_a, h->eof, d_text, pos, nb, b, n_t, d_out, aligned);
  HIP_TRY(hipGetLastError(), "k_mrg_emit");
  k_mrg_eof_fill<<<1, 1, 0, st>>>(pos, b, n_t, d_out, res);
  HIP_TRY(hipGetLastError(), "k_mrg_eof_fill");
  k_mrg_hist<<<mrg_grid(b, h->cu_count), kMrgThreads, 0, st>>>(d_text, b, res);
  HIP_TRY(hipGetLastError(), "k_mrg_hist");
  HIP_TRY(ev.record(6, st), "hipEventRecord");
  HIP_TRY(hipMemcpyAsync(host_res, res, sizeof host_res, hipMemcpyDeviceToHost, st), "D2H(result)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (host_res[kResBad]) {
    set_error("append: the new eof row lies outside the merged index (internal error)");
    return FMX_ERR_HIP;
  }
  *eof = host_res[kResEofRow];
  counts[0] = 0;
  for (int c = 1; c < 256; c++) counts[c] = h->counts[c] + (int64_t)host_res[kResHist + c];
  stats.piece_ms = ev.ms(0, 1);
  stats.walk_ms = ev.ms(2, 3);
  stats.fixup_ms = ev.ms(3, 4);
  stats.emit_ms = ev.ms(5, 6);
  stats.fixup_steps = host_res[kResFixSteps];
  stats.longest_run = host_res[kResFixLongest];
  stats.runs = host_res[kResFixRuns];
  g_merge_last = stats;
  return FMX_OK;
}

// device bytes fmx_open_dev takes for an index of n rows over `nslots` symbols, at the least (the bytes layout)
uint64_t handle_bytes_floor(uint64_t n, uint32_t nslots) {
  return (n / kByteBlock + 2) * kByteBlock + (uint64_t)nslots * (n / kByteBlock + 1) * 4 + kCounterBytes + kCensusBytes + kTixBytes;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_append_text_dev(const fmx_index *idx, const void *d_text, uint64_t len, const fmx_merge_opts *opts, void *d_bwt_out,
                        uint64_t *eof, int64_t counts[256], void *stream) {
  MergeOpts mo;
  uint64_t n_t = 0;
  if (!eof || !counts) return arg_fail("null argument");
  int rc = merge_args(idx, d_text, len, nullptr, opts, d_bwt_out, &n_t, &mo);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "append"))) return rc;
  return merge_core(h, static_cast<const uint8_t *>(d_text), len, mo, static_cast<uint8_t *>(d_bwt_out), eof, counts, st, 0);
}

int fmx_append_text(const fmx_index *idx, const uint8_t *text, uint64_t len, const fmx_merge_opts *opts, fmx_index **out) {
  MergeOpts mo;
  uint64_t n_t = 0;
  if (out) *out = nullptr;
  int rc = merge_args(idx, text, len, text, opts, out, &n_t, &mo);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  uint32_t nslots = 0;
  {
    bool seen[256] = {false};
    for (uint64_t i = 0; i < len; i++) seen[text[i]] = true;
    for (int c = 1; c < 256; c++) nslots += (seen[c] || h->counts[c]) ? 1u : 0u;
  }
  DevMem mem;
  StreamGuard own;
  HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
  const uint64_t extra = len + n_t + handle_bytes_floor(n_t, nslots);
  if ((rc = device_room(extra, "append: the merged index of " + std::to_string(n_t) + " rows"))) return rc;
  uint8_t *d_text = nullptr, *d_out = nullptr;
  DEV_ALLOC(mem, d_text, len, "append text");
  DEV_ALLOC(mem, d_out, n_t, "append output");
  HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, own.s), "H2D(text)");
  uint64_t eof = 0;
  int64_t counts[256];
  if ((rc = merge_core(h, d_text, len, mo, d_out, &eof, counts, own.s, handle_bytes_floor(n_t, nslots)))) return rc;
  return fmx_open_dev(d_out, n_t, eof, counts, h->device, own.s, out);
}

int fmx_merge_last(fmx_merge_stats *out) {
  if (!out) return arg_fail("out is null");
  *out = g_merge_last;
  return FMX_OK;
}

}  // extern "C"
