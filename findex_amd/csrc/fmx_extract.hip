// fmx_extract.hip -- text by position from inverse-SA samples.
//
// s = reverse(text) + sentinel, n = len + 1 rows; SA[0] = n - 1, SA[LF r] = SA[r] - 1 (fmx_locate.hip).  The row with
// SA == v (v >= 1) holds the BWT byte s[v - 1] = text[n - 1 - v], so an LF walk from it emits text[n - 1 - v], text[n - v], ..:
// the text FORWARDS.  A handle keeps ISA SAMPLES at a rate `rate` (the key "extract_sample"): isa[j] = the row with
// SA == j * rate, j = 0 .. (n - 1) / rate (u32 when n <= 2^32, else u64) -- pass 2 of the locate inversion's tmp, packed; or,
// when the handle's locate samples exist at the same rate, one scatter pass over their marks (isa[samples[k] / rate] = the
// k-th marked row), no inversion.
//
// To emit from text offset t: v = n - 1 - t, up = ceil(v / rate) * rate; when up <= n - 1 the walk starts at isa[up / rate] and
// skips up - v steps, otherwise it starts at row 0 (SA n - 1) and skips n - 1 - v.  A range is cut into PIECES at every t with
// (n - 1 - t) % rate == 0 (and at tile edges): each piece is a walk of its own, at most rate - 1 skipped plus rate emitted
// steps, a loop on a counter.  A long range is as many independent walks as it has pieces.
//
// The batch is k ranges: range q is the off[q + 1] - off[q] text bytes from text offset pos[q], written at out[off[q] ..).  A
// WORKGROUP takes tiles of kExTile consecutive OUTPUT bytes, grid-strided.  Each thread finds the range that owns its output
// byte (a search over the offsets, its result clamped to 0 .. k - 1), computes t and decides whether its byte heads a piece:
// the tile's first byte, a range's first byte, or (n - 1 - t) % rate == 0.  A head computes its piece -- start row, steps to
// skip, bytes to emit, all clamped -- and appends it to the tile's piece list in LDS.  The lane groups (quads, or octets on the
// bytes layout) then draw pieces from a cursor in LDS and walk them, one LF step a round, putting their bytes into the tile in
// LDS; the workgroup writes the tile with 16-byte stores.  A byte with t >= n - 1, or that no range covers, is 0 and costs no
// walk.  Nothing is written outside out[0 .. n_bytes), and no operand value forms an address outside the index.
#include <fmx.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "fmx_device.h"
#include "fmx_host.h"

namespace fmx {

constexpr int kExThreads = 256;
constexpr uint32_t kExTile = FMX_EXTRACT_TILE;             // output bytes per tile
static_assert(kExTile == 1024, "a piece's start and length are packed into 10 bits each");
static_assert(kExTile == 4 * kExThreads, "the tile is cleared one dword per thread");

struct ExDev {
  const void *isa;
  uint64_t m;          // entries of isa: (n - 1) / rate + 1
  uint32_t rate;
  uint32_t wide;       // entries are u64
};

struct ExShared {
  uint64_t cf[256];
  uint16_t slot[256];
  uint64_t row[kExTile];                                   // per piece: the row its walk starts on
  uint32_t meta[kExTile];                                  // first byte in the tile | (bytes - 1) << 10 | steps to skip << 20
  __attribute__((aligned(16))) uint8_t tile[kExTile];
  uint32_t np, cursor;
};

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kExThreads) void k_extract(DevIndex ix, ExDev xd, const uint64_t *__restrict__ pos,
                                                        const uint64_t *__restrict__ off, uint64_t k, uint64_t n_bytes,
                                                        uint8_t *__restrict__ out, unsigned long long *__restrict__ counters) {
  __shared__ ExShared sh;
  for (int c = threadIdx.x; c < 256; c += kExThreads) {
    sh.cf[c] = ix.cf[c];
    sh.slot[c] = ix.slot[c];
  }
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const bool lead = lc.t == 0;
  const uint64_t last = ix.n - 1;                          // the text's length; also the largest row
  const uint32_t s = xd.rate;
  unsigned long long steps = 0, reqs = 0;                  // counted by the lane that leads the group
  const uint64_t ntiles = (n_bytes + kExTile - 1) / kExTile;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t tile_lo = tile * kExTile;
    const uint32_t tile_n = (uint32_t)min_u64(kExTile, n_bytes - tile_lo);
    __syncthreads();                                       // the tile before this one is written (and cf / slot are there)
    if (threadIdx.x == 0) {
      sh.np = 0;
      sh.cursor = 0;
    }
    reinterpret_cast<uint32_t *>(sh.tile)[threadIdx.x] = 0u;
    __syncthreads();
    // ---- heads: one piece per head, its walk fully described
    for (uint32_t p = threadIdx.x; p < tile_n; p += kExThreads) {
      const uint64_t j = tile_lo + p;
      uint64_t lo = 0, hi = k - 1;                         // the largest q in 0 .. k - 1 with off[q] <= j (0 when there is none)
      while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid - 1;
      }
      const uint64_t rs = off[lo], re = off[lo + 1];
      if (j < rs || j >= re) continue;                     // no range covers the byte: 0
      const uint64_t p0 = pos[lo], d = j - rs;
      if (p0 >= last || d >= last - p0) continue;          // t >= n - 1: 0, no walk
      const uint64_t v = last - (p0 + d);                  // 1 .. n - 1
      const uint64_t vq = v / s;
      const uint32_t ph = (uint32_t)(v - vq * s);
      if (!(p == 0 || d == 0 || ph == 0)) continue;
      // the bytes up to the next cut: the tile's end, the range's end, the next t with (n - 1 - t) % s == 0
      const uint32_t len = (uint32_t)min_u64(min_u64(tile_n - p, re - j), ph ? ph : s);
      const uint64_t uj = vq + (ph ? 1u : 0u);             // ceil(v / s)
      uint64_t row = 0;
      uint32_t skip;
      if (uj < xd.m) {                                     // uj * s <= n - 1: a sample
        row = xd.wide ? static_cast<const uint64_t *>(xd.isa)[uj] : (uint64_t) static_cast<const uint32_t *>(xd.isa)[uj];
        skip = ph ? s - ph : 0u;
      } else {                                             // row 0, SA n - 1; fewer than s steps away
        skip = (uint32_t)(last - v);
      }
      const uint32_t at = atomicAdd(&sh.np, 1u);           // at most one piece per byte of the tile
      sh.row[at] = min_u64(row, last);
      sh.meta[at] = p | ((len - 1u) << 10) | ((uint32_t)min_u64(skip, s - 1u) << 20);
    }
    __syncthreads();
    // ---- walks: a group draws a piece, steps it skip + len times, draws the next
    const uint32_t np = sh.np;
    bool live = false, done = false;                       // the same in all lanes of a group
    uint32_t wp = 0, left = 0, skip = 0;
    uint64_t r = 0;
    for (;;) {
      if (!live && !done) {
        const uint32_t idx = group_bcast<G, 0>(lead ? atomicAdd(&sh.cursor, 1u) : 0u);
        if (idx < np) {
          const uint32_t m = sh.meta[idx];
          r = sh.row[idx];
          wp = m & 1023u;
          skip = m >> 20;
          left = ((m >> 10) & 1023u) + 1u + skip;          // <= 2 s - 1
          live = true;
        } else {
          done = true;
        }
      }
      if (!__builtin_amdgcn_ballot_w64(live)) break;
      if (live) {
        const uint32_t b = r == ix.eof ? 0u : (uint32_t)ix.bwt[r];
        const RankReq q = rank_issue<LAYOUT>(ix, sh.slot[b], r, lc);
        if (skip) {
          skip--;
        } else {
          if (lead) sh.tile[wp] = (uint8_t)b;
          wp++;
        }
        r = min_u64(sh.cf[b] + rank_complete<WIDE, LAYOUT>(q, b, lc), last);
        if (lead) {
          steps++;
          reqs += 1u + (q.kind ? (LAYOUT == kLayoutBytes ? 2u : 1u) : 0u);
        }
        left--;
        live = left != 0;
      }
    }
    __syncthreads();
    // ---- the tile, 16 bytes per store where the destination allows
    uint8_t *dst = out + tile_lo;
    if (((uintptr_t)dst & 15u) == 0) {
      for (uint32_t c = threadIdx.x * 16u; c < tile_n; c += kExThreads * 16u) {
        if (c + 16u <= tile_n) {
          *reinterpret_cast<uint4 *>(dst + c) = *reinterpret_cast<const uint4 *>(sh.tile + c);
        } else {
          for (uint32_t e = c; e < tile_n; e++) dst[e] = sh.tile[e];
        }
      }
    } else {
      for (uint32_t c = threadIdx.x; c < tile_n; c += kExThreads) dst[c] = sh.tile[c];
    }
  }
  counters_add(counters, steps, 0ull, reqs);
}

// ---------------------------------------------------------------- the samples
// isa[j] = tmp[j], a row below n
__global__ __launch_bounds__(256) void k_isa_pack(const uint64_t *__restrict__ tmp, uint64_t m, uint64_t n, int wide,
                                                  void *__restrict__ isa) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = min_u64(tmp[j], n - 1);
    if (wide) static_cast<uint64_t *>(isa)[j] = r;
    else static_cast<uint32_t *>(isa)[j] = (uint32_t)r;
  }
}

// From the locate samples at the same rate: the k-th set bit of the marks is a row r with SA samples[k]: isa[samples[k] / rate] = r.
__global__ __launch_bounds__(256) void k_isa_scatter(const uint32_t *__restrict__ marks, uint64_t nb, uint64_t n,
                                                     const void *__restrict__ samples, int swide, uint32_t rate, uint64_t m,
                                                     int wide, void *__restrict__ isa) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t rank = *reinterpret_cast<const uint64_t *>(marks + b * 16);
    for (uint32_t d = 2; d < 16; d++) {
      uint32_t w = marks[b * 16 + d];
      for (uint32_t i = 0; i < 32u && w; i++) {            // one round per set bit
        const uint32_t bit = (uint32_t)__builtin_ctz(w);
        w &= w - 1u;
        const uint64_t r = b * kBlockBits + 32u * (d - 2) + bit, kk = rank++;
        if (kk >= m || r >= n) continue;
        const uint64_t sa = swide ? static_cast<const uint64_t *>(samples)[kk] : (uint64_t) static_cast<const uint32_t *>(samples)[kk];
        const uint64_t j = sa / rate;
        if (j >= m) continue;
        if (wide) static_cast<uint64_t *>(isa)[j] = r;
        else static_cast<uint32_t *>(isa)[j] = (uint32_t)r;
      }
    }
  }
}

int extract_check(const Index *h) {
  if (h->block_mode) {
    set_error("extraction needs the index of one text: fmx_open_block handles (one merge block) have no suffix array");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n >= kOneHotMaxN) {
    set_error("extraction: indexes of 2^37 rows and more are not supported");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

// The samples at the handle's rate into h->ext.
static int extract_build(const Index *h, hipStream_t st, DevMem &mem) {
  const uint64_t n = h->n;
  const uint32_t rate = (uint32_t)h->policy.extract_sample.load(std::memory_order_relaxed);
  const uint64_t m = (n - 1) / rate + 1, nb = n / kBlockBits + 1;
  const bool wide = n > (1ull << 32);
  const uint64_t keep = m * (wide ? 8 : 4);
  // the locate samples at the same rate hold the same pairs (row, SA): no inversion then
  std::unique_lock<std::mutex> ll(h->loc.mu);
  const bool from_locate = h->loc.ready && h->loc.rate == rate;
  if (!from_locate) ll.unlock();
  int rc = device_room(keep + (from_locate ? 0 : m * 8 + locate_invert_rows_bytes(h)), "the extract samples", "need");
  if (rc) return rc;
  void *d_isa = nullptr;
  DEV_ALLOC(mem, d_isa, keep, "extract samples");
  if (from_locate) {
    HIP_TRY(hipMemsetAsync(d_isa, 0, keep, st), "hipMemset(extract samples)");
    hipLaunchKernelGGL(k_isa_scatter, dim3(flat_grid(nb, 8192)), dim3(256), 0, st, static_cast<const uint32_t *>(h->loc.marks), nb, n,
                       static_cast<const void *>(h->loc.samples), h->loc.wide ? 1 : 0, rate, m, wide ? 1 : 0, d_isa);
    HIP_TRY(hipGetLastError(), "k_isa_scatter");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    ll.unlock();
  } else {
    uint64_t *tmp = nullptr;
    DEV_ALLOC(mem, tmp, m * 8, "extract samples");
    HIP_TRY(hipMemsetAsync(tmp, 0, m * 8, st), "hipMemset(extract samples)");
    if ((rc = locate_invert_rows(h, st, rate, tmp))) return rc;
    hipLaunchKernelGGL(k_isa_pack, dim3(flat_grid(m, 8192)), dim3(256), 0, st, static_cast<const uint64_t *>(tmp), m, n, wide ? 1 : 0, d_isa);
    HIP_TRY(hipGetLastError(), "k_isa_pack");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  }
  mem.keep(d_isa);
  h->ext.isa = d_isa;
  h->ext.rate = rate;
  h->ext.wide = wide;
  h->ext.bytes = keep;
  return FMX_OK;
}

int extract_prepare(const Index *h, hipStream_t st) {
  if (const int rc = extract_check(h)) return rc;
  return build_locked(h->ext, st, "the extract samples are built by fmx_prepare(FMX_PREPARE_EXTRACT) or a first extract call outside a stream capture",
                      [&](DevMem &mem) { return extract_build(h, st, mem); });
}

// ---------------------------------------------------------------- launches
template <bool WIDE, uint32_t LAYOUT>
static hipError_t ex_launch(const Index *h, const ExDev &xd, const uint64_t *pos, const uint64_t *off, uint64_t k, uint64_t n_bytes,
                            uint8_t *out, unsigned long long *counters, hipStream_t st) {
  uint32_t grid = 0;
  const hipError_t he = resident_grid<k_extract<WIDE, LAYOUT>>(h, kExThreads, n_bytes, kExTile, &grid);
  if (he != hipSuccess) return he;
  hipLaunchKernelGGL((k_extract<WIDE, LAYOUT>), dim3(grid), dim3(kExThreads), 0, st, h->dev, xd, pos, off, k, n_bytes, out, counters);
  return hipGetLastError();
}

// The k ranges' n_bytes bytes into d_out, device pointers throughout; it needs the samples built and only enqueues on `st`;
// counters == nullptr: the handle's own.
static hipError_t extract_enqueue(const Index *h, const void *d_pos, const void *d_off, uint64_t k, uint64_t n_bytes, void *d_out,
                                  unsigned long long *counters, hipStream_t st) {
  if (n_bytes == 0 || k == 0) return hipSuccess;
  ExDev xd;
  xd.isa = h->ext.isa;
  xd.rate = h->ext.rate;
  xd.m = (h->n - 1) / h->ext.rate + 1;
  xd.wide = h->ext.wide ? 1u : 0u;
  hipError_t he = hipSuccess;
#define FMX_EX_CALL(W, L) \
  he = ex_launch<W, L>(h, xd, static_cast<const uint64_t *>(d_pos), static_cast<const uint64_t *>(d_off), k, n_bytes, \
                       static_cast<uint8_t *>(d_out), counters ? counters : h->d_counters, st)
  FMX_LAYOUT_DISPATCH(h, FMX_EX_CALL);
#undef FMX_EX_CALL
  return he;
}

struct ExtractInfo {
  uint64_t steps = 0, requests = 0;
  double ms = 0.0;                              // device events around k_extract
};

static uint64_t extract_bytes() { return kMeteredBytes; }     // the device bytes extract_run allocates

// extract_enqueue with the call's own counters and timing; allocates, synchronises `st`, frees its temporaries on every path.
static int extract_run(const Index *h, const void *d_pos, const void *d_off, uint64_t k, uint64_t n_bytes, void *d_out,
                       hipStream_t st, ExtractInfo *info) {
  *info = ExtractInfo{};
  Events<2> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  Metered own;
  int rc;
  if ((rc = own.alloc(mem, "extraction")) || (rc = own.zero(st))) return rc;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  HIP_TRY(extract_enqueue(h, d_pos, d_off, k, n_bytes, d_out, own.mine, st), "k_extract");
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  if ((rc = own.fold(h, 0, st))) return rc;                  // counter [0]: the rank queries, one per LF step
  MeterCounts cnt;
  if ((rc = own.finish(h, st, 1, &cnt))) return rc;
  info->ms = ev.ms(0, 1);
  info->steps = cnt.steps;
  info->requests = cnt.requests;
  return FMX_OK;
}

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static thread_local ExtractInfo g_extract_last;

extern "C" {

int fmx_extract_text_batch(const fmx_index *idx, const uint64_t *pos, const uint64_t *off, size_t k, uint8_t *out) {
  if ((uint64_t)k > (1ull << 26)) return arg_fail("extract: at most 2^26 ranges per call");
  if (k && (!pos || !off)) return arg_fail("extract: null argument");
  if (k && off[0] != 0) return arg_fail("extract: off[0] must be 0");
  if (k && !offsets_monotonic(off, 0, k)) return arg_fail("extract: range offsets must be non-decreasing");
  const uint64_t n_bytes = k ? off[k] : 0;
  if (n_bytes >= (1ull << 32)) return arg_fail("extract: n_bytes = off[k] must be below 2^32");
  if (n_bytes && !out) return arg_fail("extract: null argument (out)");
  if (!idx) return arg_fail("extract: the handle is null");
  const Index *h = H(idx);
  int rc = extract_check(h);
  if (rc) return rc;
  const uint64_t len = h->n - 1;
  for (size_t q = 0; q < k; q++) {
    const uint64_t l = off[q + 1] - off[q];
    if (pos[q] > len || l > len - pos[q]) return arg_fail("extract: a range runs past the text (pos + length <= n - 1)");
  }
  if (!n_bytes) return FMX_OK;
  if ((rc = use_device(h))) return rc;
  if ((rc = ensure_built(h, h->ext, extract_prepare, nullptr))) return rc;
  if ((rc = device_room(extract_bytes() + n_bytes + 16 * ((uint64_t)k + 1) + 64, "fmx_extract_text_batch"))) return rc;
  HostCall hc;
  void *d_pos = nullptr;
  uint64_t *d_off = nullptr;
  uint8_t *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("positions", pos, 8 * (uint64_t)k, "offsets", off, k, false, &d_pos, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out, n_bytes, "text");
  rc = extract_run(h, d_pos, d_off, k, n_bytes, d_out, hc.own.s, &g_extract_last);
  if (rc) return rc;
  if ((rc = hc.download(out, d_out, n_bytes, "D2H(text)"))) return rc;
  return hc.sync();
}

int fmx_extract_text_batch_dev(const fmx_index *idx, const void *d_pos, const void *d_off, size_t k, uint64_t n_bytes,
                               void *d_out, void *stream) {
  if ((uint64_t)k > (1ull << 26)) return arg_fail("extract: at most 2^26 ranges per call");
  if (n_bytes >= (1ull << 32)) return arg_fail("extract: n_bytes must be below 2^32");
  if (k && n_bytes && (!d_pos || !d_off || !d_out)) return arg_fail("extract: null argument");
  if (!idx) return arg_fail("extract: the handle is null");
  const Index *h = H(idx);
  int rc = extract_check(h);
  if (rc) return rc;
  if (!k || !n_bytes) return FMX_OK;
  if ((rc = use_device(h))) return rc;
  if ((rc = ensure_built(h, h->ext, extract_prepare, (hipStream_t)stream))) return rc;
  HIP_TRY(extract_enqueue(h, d_pos, d_off, k, n_bytes, d_out, nullptr, (hipStream_t)stream), "k_extract");
  return FMX_OK;
}

int fmx_extract_info(const fmx_index *idx, uint32_t *rate, uint64_t *bytes, double *build_ms) {
  if (!idx) return arg_fail("null argument");
  const Index *h = H(idx);
  std::lock_guard<std::mutex> lk(h->ext.mu);
  if (rate) *rate = h->ext.ready ? h->ext.rate : (uint32_t)h->policy.extract_sample.load(std::memory_order_relaxed);
  if (bytes) *bytes = h->ext.ready ? h->ext.bytes : 0;
  if (build_ms) *build_ms = h->ext.ready ? h->ext.build_ms : 0.0;
  return FMX_OK;
}

int fmx_extract_last(double *ms, uint64_t *steps, uint64_t *requests) {
  if (ms) *ms = g_extract_last.ms;
  if (steps) *steps = g_extract_last.steps;
  if (requests) *requests = g_extract_last.requests;
  return FMX_OK;
}

}  // extern "C"
