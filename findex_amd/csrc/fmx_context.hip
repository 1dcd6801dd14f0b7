// fmx_context.hip -- the context filter: rows of (group, len, sp, ep) records whose neighbouring text bytes are in a class
// (include/fmx.h: fmx_context_filter, fmx_search_context_batch).  Whole-word matching is the class "not a word
// byte" on both sides.  The text is not in HBM and is not needed: the byte BEHIND an occurrence is the BWT byte of its row, and
// the byte IN FRONT is matched by the search itself (the rows of aX are rows of X).
//
//   check   : k_ctx_check    a bad record raises a flag; the longest FMX_CTX_START record of the call (a max, no order)
//   chain   : k_ctx_chain    LF^j(0), j = 0 .. that length, by one lane group: the row whose occurrence begins at text offset 0
//   ranges  : k_ctx_ranges   record -> its candidate rows [a, b) and its chunks (fmx_ctx_math.h); a scan gives each record its
//                            first chunk (fmx_order.h, ScanSpace)
//   count   : k_ctx_pass<0>  one wave per chunk of 1024 rows, one aligned 16-byte BWT load per lane, the class test against
//                            the 256-bit set in scalar registers; pass mask -> run heads and tails per chunk
//   scan    : two scans over the chunks: the heads and the tails before each
//   emit    : k_ctx_pass<1>  the same masks again; the i-th head writes group, len and run_sp of output slot i, the i-th tail
//                            its run_ep -- a run may span chunks, waves and workgroups without communication
//             k_ctx_off      out_off[i] = the heads before the first chunk of record i * stride
// The only atomics add up totals (chunks, rows, runs) that no order depends on: the same input gives the same bytes.
#include <fmx.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fmx_ctx_math.h"
#include "fmx_classes.h"
#include "fmx_fold.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kCtxThreads = 256;
constexpr uint32_t kCtxChunk = 64 * kCtxLane;        // rows per chunk: one wave, one load per lane
constexpr uint64_t kCtxMaxRecords = 1ull << 26;      // records of one filter call, whoever makes them
constexpr uint32_t kCtxSlots = 64;                   // totals are added up in this many words, 128 bytes apart
constexpr uint32_t kCtxSlotStride = 16;
constexpr uint64_t kCtxNoRow = ~0ull;
static_assert(sizeof(fmx_result) == 24, "record size is ABI");

struct CtxClass {                                    // the 256-bit set, by value: scalar registers
  unsigned long long w0, w1, w2, w3;
};
__device__ __forceinline__ uint32_t ctx_in(const CtxClass &s, uint32_t c) {
  const unsigned long long lo = (c & 64u) ? s.w1 : s.w0, hi = (c & 64u) ? s.w3 : s.w2;
  return (uint32_t)(((c & 128u) ? hi : lo) >> (c & 63u)) & 1u;
}
__device__ __forceinline__ uint32_t ctx_in4(const CtxClass &s, uint32_t w) {      // the four bytes of a dword -> 4 bits
  return ctx_in(s, w & 255u) | (ctx_in(s, (w >> 8) & 255u) << 1) | (ctx_in(s, (w >> 16) & 255u) << 2) | (ctx_in(s, w >> 24) << 3);
}

__device__ __forceinline__ bool ctx_bad(const fmx_result &r, uint32_t md) {
  return r.len > FMX_OCC_MAX_LEN || r.sp > r.ep || ((md & FMX_CTX_START) && (md & 127u));
}

// bad[0] = 1 for a bad record; bad[1] = the longest FMX_CTX_START record
__global__ __launch_bounds__(kCtxThreads) void k_ctx_check(const fmx_result *__restrict__ rec, const uint8_t *__restrict__ mode,
                                                           uint64_t k, uint32_t *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t longest = 0, any = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
    const fmx_result r = rec[i];
    const uint32_t md = mode ? mode[i] : 0u;
    if (ctx_bad(r, md)) any = 1;
    else if ((md & FMX_CTX_START) && r.len > longest) longest = r.len;
  }
  if (any) bad[0] = 1u;
  if (longest) atomicMax(bad + 1, longest);
}

// chain[j] = LF^j(0) for j <= min(len, n - 1), kCtxNoRow behind: one lane group walks, every other group of the wave idles along
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(64) void k_ctx_chain(DevIndex ix, uint32_t len, unsigned long long *__restrict__ chain) {
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const bool writer = threadIdx.x == 0;
  uint64_t r = 0;
  if (writer) chain[0] = 0;
  for (uint32_t j = 1; j <= len; j++) {
    if ((uint64_t)j > ix.n - 1) {
      if (writer) chain[j] = kCtxNoRow;
      continue;
    }
    const uint32_t c = r == ix.eof ? 0u : ix.bwt[r];
    r = ix.cf[c] + rank_excl<WIDE, LAYOUT>(ix, c, ix.slot[c], r, lc);
    if (r >= ix.n) r = ix.n - 1;                     // an index that is not the BWT of one text stays inside itself
    if (writer) chain[j] = r;
  }
}

// a[i], b[i] = the candidate rows of record i; nch[i] = its chunks (nch[k] = 0); tot[slot]: chunks, tot[slot + 1]: rows
__global__ __launch_bounds__(kCtxThreads) void k_ctx_ranges(const fmx_result *__restrict__ rec, const uint8_t *__restrict__ mode,
                                                            uint64_t k, uint64_t n, const unsigned long long *__restrict__ chain,
                                                            uint32_t chain_len, unsigned long long *__restrict__ a,
                                                            unsigned long long *__restrict__ b, uint32_t *__restrict__ nch,
                                                            unsigned long long *__restrict__ tot) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long chunks = 0, rows = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= k; i += stride) {
    if (i == k) {
      nch[i] = 0;
      continue;
    }
    const fmx_result r = rec[i];
    const uint32_t md = mode ? mode[i] : 0u, lead = md & 127u;
    uint64_t lo = 0, hi = 0;
    if (!ctx_bad(r, md) && r.len > lead && r.sp < r.ep && r.sp < n) {
      if (md & FMX_CTX_START) {
        if (r.len <= chain_len && chain[r.len] == r.sp) {
          lo = r.sp;
          hi = r.sp + 1;
        }
      } else {
        lo = r.sp;
        hi = r.ep < n ? r.ep : n;
      }
    }
    a[i] = lo;
    b[i] = hi;
    const uint64_t c = ctx_chunk_count(lo, hi, kCtxChunk);
    nch[i] = (uint32_t)c;
    chunks += c;
    rows += hi - lo;
  }
  chunks = wave_sum(chunks);
  rows = wave_sum(rows);
  if ((threadIdx.x & 63u) == 0 && chunks) {
    unsigned long long *t = tot + (size_t)(blockIdx.x % kCtxSlots) * kCtxSlotStride;
    atomicAdd(t, chunks);
    atomicAdd(t + 1, rows);
  }
}

// One wave per chunk.  EMIT == 0: heads[c], tails[c] = the run heads and tails of chunk c, tot[slot + 2] += the heads.
// EMIT == 1: heads[] and tails[] hold their exclusive sums, and the runs are written (nothing past out[cap - 1]).
template <int EMIT>
__global__ __launch_bounds__(kCtxThreads) void k_ctx_pass(const uint8_t *__restrict__ bwt, const fmx_result *__restrict__ rec,
                                                          const uint8_t *__restrict__ mode,
                                                          const unsigned long long *__restrict__ a,
                                                          const unsigned long long *__restrict__ b,
                                                          const uint32_t *__restrict__ choff, uint64_t k, uint64_t n_chunks,
                                                          CtxClass cls, uint32_t *__restrict__ heads, uint32_t *__restrict__ tails,
                                                          fmx_result *__restrict__ out, uint64_t cap,
                                                          unsigned long long *__restrict__ tot) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (kCtxThreads / 64);
  unsigned long long found = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * (kCtxThreads / 64) + (threadIdx.x >> 6); c < n_chunks; c += waves) {
    const uint64_t j = upper_bound(choff, 0, k + 1, c) - 1;          // choff[0] = 0 <= c < choff[k]: a record with chunks
    const uint64_t lo = a[j], hi = b[j];
    const uint64_t row0 = ctx_chunk_first(lo, c - choff[j], kCtxChunk) + (uint64_t)lane * kCtxLane;
    const uint32_t valid = ctx_valid_mask(row0, lo, hi, kCtxLane);
    uint32_t m = 0;
    if (valid) {                                     // a row of the record lies in these 16: they are inside the padded BWT
      const uint4 w = *reinterpret_cast<const uint4 *>(bwt + row0);
      m = (ctx_in4(cls, w.x) | (ctx_in4(cls, w.y) << 4) | (ctx_in4(cls, w.z) << 8) | (ctx_in4(cls, w.w) << 12)) & valid;
    }
    // the pass bits of the rows next to this lane's: the neighbour lanes', and at the chunk's ends one byte each
    uint32_t cin = (uint32_t)__shfl_up((int)m, 1, 64) >> (kCtxLane - 1);
    uint32_t cout = (uint32_t)__shfl_down((int)m, 1, 64) & 1u;
    if (lane == 0) cin = row0 > lo ? ctx_in(cls, bwt[row0 - 1]) : 0u;
    if (lane == 63) cout = row0 + kCtxLane < hi ? ctx_in(cls, bwt[row0 + kCtxLane]) : 0u;
    uint32_t h = ctx_heads(m, cin), t = ctx_tails(m, cout, kCtxLane);
    const uint32_t cnt = (uint32_t)__popc(h) | ((uint32_t)__popc(t) << 16);      // at most 8 of each per lane, 512 per wave
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (!EMIT) {
      if (lane == 63) {
        heads[c] = incl & 0xffffu;
        tails[c] = incl >> 16;
        found += incl & 0xffffu;
      }
      continue;
    }
    const uint32_t excl = incl - cnt;
    uint64_t hs = (uint64_t)heads[c] + (excl & 0xffffu), ts = (uint64_t)tails[c] + (excl >> 16);
    if (h | t) {
      const fmx_result r = rec[j];
      const uint32_t len = r.len - (mode ? (mode[j] & 127u) : 0u);
      while (h) {
        const uint32_t i = (uint32_t)__ffs((int)h) - 1u;
        h &= h - 1u;
        if (hs < cap) {
          out[hs].regex = r.regex;
          out[hs].len = len;
          out[hs].sp = row0 + i;
        }
        hs++;
      }
      while (t) {
        const uint32_t i = (uint32_t)__ffs((int)t) - 1u;
        t &= t - 1u;
        if (ts < cap) out[ts].ep = row0 + i + 1;
        ts++;
      }
    }
  }
  if (!EMIT && found) atomicAdd(tot + (size_t)(blockIdx.x % kCtxSlots) * kCtxSlotStride + 2, found);
}

// out_off[i] = the runs before record i * stride, i = 0 .. m (hscan: the heads before each chunk, and behind the last)
__global__ __launch_bounds__(kCtxThreads) void k_ctx_off(const uint32_t *__restrict__ choff, const uint32_t *__restrict__ hscan,
                                                         uint64_t m, uint64_t stride_rec, unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += stride) out_off[i] = hscan[choff[i * stride_rec]];
}

// ---- fmx_search_context_batch: the expansion of the patterns and the record list
struct CtxExpand {
  const void *pat;                                   // uint8_t bytes, or the uint16_t elements of the class search (§30)
  const unsigned long long *off;
  uint64_t k, n_left;                                // patterns; left bytes a >= 1 that occur, ascending, in lefts[]
  const uint8_t *lefts;
};

// Pattern i (a string of s, as fmx_search_batch takes it) -> 1 + n_left strings: itself, then itself with each left byte
// appended (a in front of the text string is a behind its reverse).  flag[0] = 1 for an empty pattern, a byte 0, offsets
// that do not ascend or a pattern above FMX_OCC_MAX_LEN - 1 bytes; nothing is written outside the expansion's buffers.
template <class T>
__global__ __launch_bounds__(kCtxThreads) void k_ctx_expand(CtxExpand e, T *__restrict__ xpat,
                                                            unsigned long long *__restrict__ xoff, uint32_t *__restrict__ flag) {
  const uint64_t per = e.n_left + 1, total = e.k * per, stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t o0 = e.off[0], ok_ = e.off[e.k];
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x <= total; x += stride) {
    const uint64_t i = x / per, v = x - i * per;
    uint64_t ob = e.off[i], oe = i < e.k ? e.off[i + 1] : ob;
    bool bad = ob < o0 || ob > ok_ || oe < ob || oe > ok_ || ok_ < o0;
    if (bad) ob = oe = o0;
    const uint64_t len = oe - ob, at = per * (ob - o0) + i * e.n_left + (v ? len + (v - 1) * (len + 1) : 0);
    xoff[x] = at;
    if (x == total) {
      if (bad) flag[0] = 1u;
      continue;
    }
    if (len == 0 || len > FMX_OCC_MAX_LEN - 1) bad = true;
    if (!bad) {
      for (uint64_t t = 0; t < len; t++) {
        const T c = static_cast<const T *>(e.pat)[ob + t];
        if (c == 0) bad = true;
        xpat[at + t] = c;
      }
      if (v) xpat[at + len] = e.lefts[v - 1];
    }
    if (bad) flag[0] = 1u;
  }
}

// the record list: per pattern the plain interval under FMX_CTX_START (empty when the text may not begin there), then the
// intervals of its left bytes with lead 1
__global__ __launch_bounds__(kCtxThreads) void k_ctx_records(const unsigned long long *__restrict__ xoff,
                                                             const unsigned long long *__restrict__ sp,
                                                             const unsigned long long *__restrict__ ep, uint64_t k, uint64_t per,
                                                             int start, fmx_result *__restrict__ rec, uint8_t *__restrict__ mode) {
  const uint64_t total = k * per, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
    const uint64_t i = x / per, v = x - i * per;
    fmx_result r;
    r.regex = (uint32_t)i;
    r.len = (uint32_t)(xoff[x + 1] - xoff[x]);
    r.sp = sp[x];
    r.ep = ep[x];
    if (r.sp > r.ep || (v == 0 && !start)) r.sp = r.ep = 0;
    rec[x] = r;
    mode[x] = v ? 1u : (start ? (uint8_t)FMX_CTX_START : 0u);
  }
}

// ---- fmx_search_context_fold_batch: the fold search (fmx_fold.hip) in the place of the exact one
// lead[x] = 1 for the expansion's strings with a left byte: that byte's step is exact whatever the map says
__global__ __launch_bounds__(kCtxThreads) void k_ctx_leads(uint64_t total, uint64_t per, uint8_t *__restrict__ lead) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) lead[x] = x % per ? 1u : 0u;
}

// the fold search's records -> the filter's: the lead bit out of len into the mode; a plain record is an occurrence at the
// text's beginning or nothing
__global__ __launch_bounds__(kCtxThreads) void k_ctx_fold_modes(fmx_result *__restrict__ rec, uint64_t rows, int start,
                                                                uint8_t *__restrict__ mode) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const uint32_t tag = rec[j].len;
    const bool lead = (tag & kFoldLeadBit) != 0;
    rec[j].len = tag & ~kFoldLeadBit;
    if (!lead && !start) rec[j].sp = rec[j].ep = 0;
    mode[j] = lead ? 1u : (start ? (uint8_t)FMX_CTX_START : 0u);
  }
}

// out_off[i] = the runs before the first record of pattern i
__global__ __launch_bounds__(kCtxThreads) void k_ctx_recut(const unsigned long long *__restrict__ rec_off,
                                                           const unsigned long long *__restrict__ run_off, uint64_t k,
                                                           unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= k; i += stride) out_off[i] = run_off[rec_off[i]];
}

namespace {

struct CtxLast {
  double ms[3] = {0.0, 0.0, 0.0};                    // search, chain, count + scan + emit
  uint64_t rows = 0, runs = 0;
};
thread_local CtxLast g_ctx_last;

int ctx_handle(const fmx_index *idx, const char *who) {
  if (!idx) return arg_fail("context filter: the handle is null");
  const Index *h = H(idx);
  if (h->block_mode) {
    set_error(std::string(who) + ": fmx_open_block handles are not supported");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

template <bool W, uint32_t L>
void ctx_chain_launch(const Index *h, uint32_t len, unsigned long long *chain, hipStream_t st) {
  hipLaunchKernelGGL((k_ctx_chain<W, L>), dim3(1), dim3(64), 0, st, h->dev, len, chain);
}

// The filter on `st`: d_rec, d_mode (or null), d_out_off (u64[m + 1], m = k / stride_rec) and d_out in device memory.
// out_off is over every stride_rec-th record.  Allocates, synchronises, frees its temporaries on every path.
int ctx_run(const Index *h, const fmx_result *d_rec, const uint8_t *d_mode, uint64_t k, uint64_t stride_rec, const uint64_t right[4],
            unsigned long long *d_out_off, fmx_result *d_out, uint64_t cap, hipStream_t st, uint64_t *total) {
  const uint64_t m = stride_rec ? k / stride_rec : 0;
  uint64_t launches = 0;
  auto done = [&]() {
    std::lock_guard<std::mutex> lk(h->mu);
    h->launches += launches;
  };
  int rc = device_room(20 * (k + 1) + ScanSpace::bytes(k + 1) + 8 * kCtxSlots * kCtxSlotStride + 8192, "fmx_context_filter");
  if (rc) return rc;
  Events<4> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *a = nullptr, *b = nullptr, *tot = nullptr, *chain = nullptr;
  uint32_t *choff = nullptr, *bad = nullptr, *heads = nullptr, *tails = nullptr;
  ScanSpace rscan, cscan;
  DEV_ALLOC(mem, a, 8 * k, "context filter");
  DEV_ALLOC(mem, b, 8 * k, "context filter");
  DEV_ALLOC(mem, choff, 4 * (k + 1), "context filter");
  DEV_ALLOC(mem, bad, 16, "context filter");
  DEV_ALLOC(mem, tot, 8 * kCtxSlots * kCtxSlotStride, "context filter");
  if ((rc = rscan.alloc(mem, k + 1, "context filter"))) return rc;
  HIP_TRY(hipMemsetAsync(bad, 0, 16, st), "hipMemsetAsync");
  HIP_TRY(hipMemsetAsync(tot, 0, 8 * kCtxSlots * kCtxSlotStride, st), "hipMemsetAsync");
  uint32_t bad_h[2] = {0, 0};
  if (k) {
    LAUNCH("k_ctx_check", k_ctx_check, dim3(flat_grid(k)), dim3(kCtxThreads), st, d_rec, d_mode, k, bad);
    launches++;
    HIP_TRY(hipMemcpyAsync(bad_h, bad, 8, hipMemcpyDeviceToHost, st), "D2H(flag)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  }
  if (bad_h[0]) {
    done();
    return arg_fail("context filter: a record with len > FMX_OCC_MAX_LEN, sp > ep, or FMX_CTX_START with a lead");
  }
  // ---- the chain LF^j(0), as far as the longest FMX_CTX_START record
  const uint32_t chain_len = bad_h[1];
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (chain_len) {
    if ((rc = device_room(8 * ((uint64_t)chain_len + 1) + 4096, "fmx_context_filter"))) return rc;
    DEV_ALLOC(mem, chain, 8 * ((uint64_t)chain_len + 1), "context filter");
#define FMX_CTX_CHAIN(W, L) ctx_chain_launch<W, L>(h, chain_len, chain, st)
    FMX_LAYOUT_DISPATCH(h, FMX_CTX_CHAIN);
#undef FMX_CTX_CHAIN
    HIP_TRY(hipGetLastError(), "k_ctx_chain");
    launches++;
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  // ---- ranges, chunks
  LAUNCH("k_ctx_ranges", k_ctx_ranges, dim3(flat_grid(k + 1)), dim3(kCtxThreads), st, d_rec, d_mode, k, h->n, chain, chain_len, a, b, choff,
         tot);
  HIP_TRY(rscan.sum(choff, k + 1, true, st), "scan");
  launches += 3;
  std::vector<unsigned long long> tot_h(kCtxSlots * kCtxSlotStride, 0ull);
  HIP_TRY(hipMemcpyAsync(tot_h.data(), tot, 8 * tot_h.size(), hipMemcpyDeviceToHost, st), "D2H(totals)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  uint64_t n_chunks = 0, rows = 0;
  for (uint32_t s = 0; s < kCtxSlots; s++) {
    n_chunks += tot_h[s * kCtxSlotStride];
    rows += tot_h[s * kCtxSlotStride + 1];
  }
  g_ctx_last.rows = rows;
  if (n_chunks >= 0xffffffffull) {
    done();
    set_error("context filter: " + std::to_string(rows) + " rows in " + std::to_string(n_chunks) + " chunks, at most 2^32 - 2 chunks per call");
    return FMX_ERR_OVERFLOW;
  }
  if ((rc = device_room(8 * (n_chunks + 1) + ScanSpace::bytes(n_chunks + 1) + 4096, "fmx_context_filter"))) {
    done();
    return rc;
  }
  DEV_ALLOC(mem, heads, 4 * (n_chunks + 1), "context filter");
  DEV_ALLOC(mem, tails, 4 * (n_chunks + 1), "context filter");
  if ((rc = cscan.alloc(mem, n_chunks + 1, "context filter"))) return rc;
  HIP_TRY(hipMemsetAsync(heads + n_chunks, 0, 4, st), "hipMemsetAsync");
  HIP_TRY(hipMemsetAsync(tails + n_chunks, 0, 4, st), "hipMemsetAsync");
  const CtxClass cls{right[0], right[1], right[2], right[3]};
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_chunks + 3) / 4, (uint64_t)std::max(h->cu_count, 1) * 8));
  uint64_t runs = 0;
  if (n_chunks) {
    LAUNCH("k_ctx_pass", k_ctx_pass<0>, dim3(grid), dim3(kCtxThreads), st, h->dev.bwt, d_rec, d_mode, a, b, choff, k, n_chunks, cls, heads,
           tails, d_out, cap, tot);
    launches++;
    HIP_TRY(hipMemcpyAsync(tot_h.data(), tot, 8 * tot_h.size(), hipMemcpyDeviceToHost, st), "D2H(totals)");
  }
  HIP_TRY(cscan.sum(heads, n_chunks + 1, true, st), "scan");
  HIP_TRY(cscan.sum(tails, n_chunks + 1, true, st), "scan");
  launches += 4;
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (n_chunks)
    for (uint32_t s = 0; s < kCtxSlots; s++) runs += tot_h[s * kCtxSlotStride + 2];
  g_ctx_last.runs = runs;
  *total = runs;
  if (runs >= 0xffffffffull) {                       // the run slots are numbered in 32 bits: the exact total, and no output
    done();
    return csr_overflow("context filter (at most 2^32 - 2 runs per call)", runs, cap);
  }
  LAUNCH("k_ctx_off", k_ctx_off, dim3(flat_grid(m + 1)), dim3(kCtxThreads), st, choff, heads, m, stride_rec, d_out_off);
  launches++;
  if (n_chunks && cap && runs) {
    LAUNCH("k_ctx_pass", k_ctx_pass<1>, dim3(grid), dim3(kCtxThreads), st, h->dev.bwt, d_rec, d_mode, a, b, choff, k, n_chunks, cls, heads,
           tails, d_out, cap, tot);
    launches++;
  }
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
  g_ctx_last.ms[1] = chain_len ? ev.ms(0, 1) : 0.0;
  g_ctx_last.ms[2] = ev.ms(1, 2);
  done();
  return FMX_OK;
}

int ctx_filter_args(const void *rec, size_t k, const uint64_t *right, const void *out_off, const void *out, size_t cap,
                    const size_t *n_out) {
  if (!right || !out_off || !n_out) return arg_fail("context filter: right, out_off or n_out is null");
  if ((uint64_t)k > kCtxMaxRecords) return arg_fail("context filter: at most 2^26 records per call");
  if (k && !rec) return arg_fail("context filter: the records are null");
  if (cap && !out) return arg_fail("context filter: out is null");
  return FMX_OK;
}

int ctx_opts_check(const fmx_context_opts *o) {
  if (!o) return arg_fail("search_context: opts is null");
  if (o->flags != 0 || o->reserved != 0) return arg_fail("fmx_context_opts.flags and .reserved must be 0");
  return FMX_OK;
}

// The search with context on `st`; everything in device memory, the patterns already checked as far as the caller can.
// pat_bytes = d_off[k] - d_off[0].  fold_map (256 bytes, or null: the exact search): the search under that map instead, with
// fold_len the longest expanded pattern (the left byte included), FMX_FOLD_MAX_LEN where the lengths are not known.
// cc (or null): the class search (fmx_classes.hip) instead -- d_pat holds uint16_t elements, pat_bytes counts elements, the left
// byte is appended as a LITERAL element, and fold_len is in elements.  Lead bit, `per`, modes, filter and re-cut are the fold path's.
struct CtxClasses {
  const std::vector<ClassRec> *packed;
  uint32_t largest;
};
int ctx_search(const Index *h, const fmx_index *idx, const void *d_pat, const unsigned long long *d_off, uint64_t k,
               uint64_t pat_bytes, const fmx_context_opts &o, const uint8_t *fold_map, const CtxClasses *cc, uint32_t fold_len,
               unsigned long long *d_out_off, fmx_result *d_out, uint64_t cap, hipStream_t st, uint64_t *total) {
  uint8_t lefts[256];
  uint64_t n_left = 0;
  for (uint32_t c = 1; c < 256; c++)
    if (((o.left[c >> 6] >> (c & 63)) & 1) && h->counts[c] > 0) lefts[n_left++] = (uint8_t)c;
  const uint64_t per = n_left + 1, xk = k * per, xbytes = (per * pat_bytes + k * n_left) * (cc ? 2 : 1);
  if (xk > (1ull << 26)) return arg_fail("search_context: patterns x (left bytes that occur + 1) must be at most 2^26");
  int rc = device_room(xbytes + 8 * (xk + 1) + 16 * xk + 25 * xk + 8 * (xk + 1) + 8192, "fmx_search_context_batch");
  if (rc) return rc;
  Events<2> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  uint8_t *xpat = nullptr, *d_lefts = nullptr, *mode = nullptr;
  unsigned long long *xoff = nullptr, *sp = nullptr, *ep = nullptr;
  fmx_result *rec = nullptr;
  uint32_t *flag = nullptr;
  DEV_ALLOC(mem, xpat, xbytes, "search_context");
  DEV_ALLOC(mem, d_lefts, 256, "search_context");
  DEV_ALLOC(mem, xoff, 8 * (xk + 1), "search_context");
  if (!fold_map && !cc) {
    DEV_ALLOC(mem, sp, 8 * xk, "search_context");
    DEV_ALLOC(mem, ep, 8 * xk, "search_context");
    DEV_ALLOC(mem, rec, sizeof(fmx_result) * xk, "search_context");
    DEV_ALLOC(mem, mode, xk, "search_context");
  }
  DEV_ALLOC(mem, flag, 16, "search_context");
  HIP_TRY(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  HIP_TRY(hipMemcpyAsync(d_lefts, lefts, 256, hipMemcpyHostToDevice, st), "H2D(left bytes)");
  const CtxExpand e{d_pat, d_off, k, n_left, d_lefts};
  if (cc) LAUNCH("k_ctx_expand", k_ctx_expand<uint16_t>, dim3(flat_grid(xk + 1)), dim3(kCtxThreads), st, e, reinterpret_cast<uint16_t *>(xpat), xoff, flag);
  else LAUNCH("k_ctx_expand", k_ctx_expand<uint8_t>, dim3(flat_grid(xk + 1)), dim3(kCtxThreads), st, e, xpat, xoff, flag);
  uint32_t flag_h = 0;
  HIP_TRY(hipMemcpyAsync(&flag_h, flag, 4, hipMemcpyDeviceToHost, st), "D2H(flag)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // lefts[] is on the stack
  {
    std::lock_guard<std::mutex> lk(h->mu);
    h->launches += 1;
  }
  if (flag_h)
    return arg_fail("search_context: an empty pattern, a pattern above 65534 bytes, a byte 0 in a pattern, or offsets that do not ascend");
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (fold_map || cc) {
    // the records are the fold search's hits: their number is known after it -- a second search when the first guess was short
    uint8_t *lead = nullptr;
    unsigned long long *rec_off = nullptr, *run_off = nullptr;
    DEV_ALLOC(mem, rec_off, 8 * (k + 1), "search_context");
    if (per > 1 && !cc) {
      DEV_ALLOC(mem, lead, xk, "search_context");
      LAUNCH("k_ctx_leads", k_ctx_leads, dim3(flat_grid(xk)), dim3(kCtxThreads), st, xk, per, lead);
    }
    FoldInfo info;
    uint64_t rcap = std::min<uint64_t>(2 * xk + 1024, kCtxMaxRecords);
    uint64_t own_launches = 1 + (per > 1 && !cc ? 1 : 0);          // k_ctx_recut, k_ctx_leads; the fold search and the filter count their own
    for (int pass = 0;; pass++) {
      if ((rc = device_room(33 * rcap + 4096, "fmx_search_context_fold_batch"))) return rc;
      DEV_ALLOC(mem, rec, sizeof(fmx_result) * rcap, "search_context");
      if (cc) {
        if ((rc = classes_search(h, xpat, xoff, xk, per, *cc->packed, cc->largest, fold_len, rec_off, rec, rcap, true, st, &info))) return rc;
        classes_set_last(info);
      } else {
        if ((rc = fold_search(h, xpat, xoff, xk, fold_map, lead, per, fold_len, rec_off, rec, rcap, true, st, &info))) return rc;
        fold_set_last(info);
      }
      if (info.total <= rcap) break;
      if (pass || info.total > kCtxMaxRecords) {             // the variants are the filter's records: its limit holds for them
        set_error("search_context_fold: " + std::to_string(info.total) + " variants occur, at most 2^26 records reach the filter in one call");
        return FMX_ERR_ARG;
      }
      rcap = info.total;
    }
    const uint64_t n_rec = info.total;
    DEV_ALLOC(mem, mode, n_rec, "search_context");
    DEV_ALLOC(mem, run_off, 8 * (n_rec + 1), "search_context");
    if (n_rec) {
      LAUNCH("k_ctx_fold_modes", k_ctx_fold_modes, dim3(flat_grid(n_rec)), dim3(kCtxThreads), st, rec, n_rec, (int)(o.left[0] & 1), mode);
      own_launches++;
    }
    rc = ctx_run(h, rec, mode, n_rec, 1, o.right, run_off, d_out, cap, st, total);
    g_ctx_last.ms[0] = info.search_ms + info.sort_ms;
    if (rc) return rc;
    LAUNCH("k_ctx_recut", k_ctx_recut, dim3(flat_grid(k + 1)), dim3(kCtxThreads), st, rec_off, run_off, k, d_out_off);
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
    std::lock_guard<std::mutex> lk(h->mu);
    h->launches += own_launches;
    return FMX_OK;
  }
  if (xk && (rc = fmx_search_batch_dev(idx, xpat, xoff, sp, ep, xk, st))) return rc;
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  if (xk) {
    LAUNCH("k_ctx_records", k_ctx_records, dim3(flat_grid(xk)), dim3(kCtxThreads), st, xoff, sp, ep, k, per, (int)(o.left[0] & 1), rec, mode);
  }
  rc = ctx_run(h, rec, mode, xk, per, o.right, d_out_off, d_out, cap, st, total);
  g_ctx_last.ms[0] = ev.ms(0, 1);
  return rc;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_context_filter_dev(const fmx_index *idx, const void *d_rec, const void *d_mode, size_t k, const uint64_t *right,
                           void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  int rc = ctx_filter_args(d_rec, k, right, d_out_off, d_out, cap, n_out);
  if (rc || (rc = ctx_handle(idx, "fmx_context_filter_dev"))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_context_filter_dev"))) return rc;
  g_ctx_last = CtxLast{};
  uint64_t total = 0;
  if ((rc = ctx_run(h, static_cast<const fmx_result *>(d_rec), static_cast<const uint8_t *>(d_mode), k, 1, right,
                    static_cast<unsigned long long *>(d_out_off), static_cast<fmx_result *>(d_out), cap, st, &total))) {
    if (rc == FMX_ERR_OVERFLOW && total) *n_out = (size_t)total;
    return rc;
  }
  *n_out = (size_t)total;
  return total > cap ? csr_overflow("context filter", total, cap) : FMX_OK;
}

int fmx_context_filter(const fmx_index *idx, const fmx_result *rec, const uint8_t *mode, size_t k, const uint64_t *right,
                       uint64_t *out_off, fmx_result *out, size_t cap, size_t *n_out) {
  int rc = ctx_filter_args(rec, k, right, out_off, out, cap, n_out);
  if (rc) return rc;
  for (size_t i = 0; i < k; i++) {
    if (rec[i].len > FMX_OCC_MAX_LEN) return arg_fail("context filter: a record's len is above FMX_OCC_MAX_LEN (65535)");
    if (rec[i].sp > rec[i].ep) return arg_fail("context filter: a record with sp > ep");
    if (mode && (mode[i] & FMX_CTX_START) && (mode[i] & 127u)) return arg_fail("context filter: FMX_CTX_START needs lead == 0");
  }
  if ((rc = ctx_handle(idx, "fmx_context_filter"))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  if ((rc = hc.open())) return rc;
  const uint64_t kk = k;
  if ((rc = device_room(25 * kk + 8 * (kk + 1) + 24 * (uint64_t)cap + 4096, "fmx_context_filter"))) return rc;
  fmx_result *d_rec = nullptr, *d_out = nullptr;
  uint8_t *d_mode = nullptr;
  unsigned long long *d_off = nullptr;
  DEV_ALLOC(hc.mem, d_rec, sizeof(fmx_result) * kk, "context records");
  DEV_ALLOC(hc.mem, d_off, 8 * (kk + 1), "context offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_result) * (uint64_t)cap, "context runs");
  if (mode) DEV_ALLOC(hc.mem, d_mode, kk, "context modes");
  if (k) {
    HIP_TRY(hipMemcpyAsync(d_rec, rec, sizeof(fmx_result) * kk, hipMemcpyHostToDevice, hc.own.s), "H2D(records)");
    if (mode) HIP_TRY(hipMemcpyAsync(d_mode, mode, kk, hipMemcpyHostToDevice, hc.own.s), "H2D(modes)");
  }
  g_ctx_last = CtxLast{};
  uint64_t total = 0;
  if ((rc = ctx_run(h, d_rec, d_mode, kk, 1, right, d_off, d_out, cap, hc.own.s, &total))) {
    if (rc == FMX_ERR_OVERFLOW && total) *n_out = (size_t)total;
    return rc;
  }
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("context filter", total, cap);
  return hc.download_csr(out_off, d_off, k, out, d_out, total, sizeof(fmx_result));
}

int fmx_context_last(double *search_ms, double *chain_ms, double *filter_ms, uint64_t *rows, uint64_t *runs) {
  if (search_ms) *search_ms = g_ctx_last.ms[0];
  if (chain_ms) *chain_ms = g_ctx_last.ms[1];
  if (filter_ms) *filter_ms = g_ctx_last.ms[2];
  if (rows) *rows = g_ctx_last.rows;
  if (runs) *runs = g_ctx_last.runs;
  return FMX_OK;
}

// both device forms; fold_map: null (the exact search) or the 256 bytes of a checked map
static int ctx_search_dev_form(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_context_opts *opts,
                               const uint8_t *fold_map, const CtxClasses *cc, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  int rc = ctx_opts_check(opts);
  if (rc) return rc;
  if (!d_out_off || !n_out || !d_off || (cap && !d_out)) return arg_fail("search_context: null argument");
  if ((uint64_t)k > (1ull << 26)) return arg_fail("search_context: at most 2^26 patterns per call");
  if ((rc = ctx_handle(idx, "fmx_search_context_batch_dev"))) return rc;
  const Index *h = H(idx);
  if ((fold_map || cc) && (rc = fold_handle_check(h))) return rc;
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_search_context_batch_dev"))) return rc;
  unsigned long long ends[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&ends[0], d_off, 8, hipMemcpyDeviceToHost, st), "D2H(off)");
  HIP_TRY(hipMemcpyAsync(&ends[1], static_cast<const unsigned long long *>(d_off) + k, 8, hipMemcpyDeviceToHost, st), "D2H(off)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (ends[1] < ends[0]) return arg_fail("search_context: offsets that do not ascend");
  if (ends[1] > ends[0] && !d_pat) return arg_fail("search_context: the patterns are null");
  g_ctx_last = CtxLast{};
  uint64_t total = 0;
  if ((rc = ctx_search(h, idx, d_pat, static_cast<const unsigned long long *>(d_off), k, ends[1] - ends[0], *opts, fold_map, cc,
                       FMX_FOLD_MAX_LEN,
                       static_cast<unsigned long long *>(d_out_off), static_cast<fmx_result *>(d_out), cap, st, &total))) {
    if (rc == FMX_ERR_OVERFLOW && total) *n_out = (size_t)total;
    return rc;
  }
  *n_out = (size_t)total;
  return total > cap ? csr_overflow("search_context", total, cap) : FMX_OK;
}

// both host forms
static int ctx_search_host_form(const fmx_index *idx, const void *pat_, const uint64_t *off, size_t k, const fmx_context_opts *opts,
                                const uint8_t *fold_map, const CtxClasses *cc, uint64_t *out_off, fmx_result *out, size_t cap, size_t *n_out) {
  int rc = ctx_opts_check(opts);
  if (rc) return rc;
  if (!out_off || !n_out || !off || (cap && !out)) return arg_fail("search_context: null argument");
  if ((uint64_t)k > (1ull << 26)) return arg_fail("search_context: at most 2^26 patterns per call");
  const uint8_t *pat = static_cast<const uint8_t *>(pat_);      // (cc: uint16_t elements, `bytes` and the offsets count elements)
  const uint16_t *el = static_cast<const uint16_t *>(pat_);
  const uint64_t es = cc ? 2 : 1;
  uint64_t longest = 0;
  for (size_t i = 0; i < k; i++) {
    if (off[i + 1] <= off[i]) return arg_fail("search_context: an empty pattern, or offsets that do not ascend");
    longest = std::max<uint64_t>(longest, off[i + 1] - off[i]);
    if (off[i + 1] - off[i] > FMX_OCC_MAX_LEN - 1) return arg_fail("search_context: a pattern above 65534 bytes");
    if (fold_map && off[i + 1] - off[i] > FMX_FOLD_MAX_LEN - 1) return arg_fail("search_context_fold: a pattern above 254 bytes");
    if (cc && off[i + 1] - off[i] > FMX_CLASS_MAX_ELEMS - 1) return arg_fail("search_context_classes: a pattern above 254 elements");
  }
  const uint64_t bytes = k ? off[k] - off[0] : 0;
  if (bytes && !pat) return arg_fail("search_context: the patterns are null");
  for (uint64_t t = 0; t < bytes; t++) {
    if ((cc ? el[off[0] + t] : pat[off[0] + t]) == 0) return arg_fail("search_context: a byte 0 in a pattern");
    if (cc && el[off[0] + t] >= 256u && (uint64_t)(el[off[0] + t] - 256u) >= cc->packed->size())
      return arg_fail("search_context_classes: an element names a class that is not in the table");
  }
  if ((rc = ctx_handle(idx, "fmx_search_context_batch"))) return rc;
  const Index *h = H(idx);
  if ((fold_map || cc) && (rc = fold_handle_check(h))) return rc;
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  if ((rc = hc.open())) return rc;
  const uint64_t kk = k;
  if ((rc = device_room(es * bytes + 16 * (kk + 1) + 24 * (uint64_t)cap + 4096, "fmx_search_context_batch"))) return rc;
  void *d_pat = nullptr;
  uint64_t *d_off = nullptr;
  unsigned long long *d_out_off = nullptr;
  fmx_result *d_out = nullptr;
  if ((rc = hc.upload("context patterns", pat ? pat + es * off[0] : nullptr, es * bytes, "context offsets", off, k, true, &d_pat, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out_off, 8 * (kk + 1), "context offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_result) * (uint64_t)cap, "context runs");
  g_ctx_last = CtxLast{};
  uint64_t total = 0;
  if (k == 0) {
    out_off[0] = 0;
    *n_out = 0;
    return FMX_OK;
  }
  if ((rc = ctx_search(h, idx, d_pat, reinterpret_cast<const unsigned long long *>(d_off), kk, bytes, *opts, fold_map, cc,
                       (uint32_t)std::min<uint64_t>(longest + 1, FMX_FOLD_MAX_LEN),
                       d_out_off, d_out, cap, hc.own.s, &total))) {
    if (rc == FMX_ERR_OVERFLOW && total) *n_out = (size_t)total;
    return rc;
  }
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("search_context", total, cap);
  return hc.download_csr(out_off, d_out_off, k, out, d_out, total, sizeof(fmx_result));
}

int fmx_search_context_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_context_opts *opts,
                                 void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  return ctx_search_dev_form(idx, d_pat, d_off, k, opts, nullptr, nullptr, d_out_off, d_out, cap, n_out, stream);
}

int fmx_search_context_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_context_opts *opts,
                             uint64_t *out_off, fmx_result *out, size_t cap, size_t *n_out) {
  return ctx_search_host_form(idx, pat, off, k, opts, nullptr, nullptr, out_off, out, cap, n_out);
}

int fmx_search_context_fold_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k,
                                      const fmx_context_opts *ctx, const fmx_fold_opts *fold, void *d_out_off, void *d_out,
                                      size_t cap, size_t *n_out, void *stream) {
  uint8_t map[256];
  int rc = fold_map_check(fold, map);
  if (rc) return rc;
  return ctx_search_dev_form(idx, d_pat, d_off, k, ctx, map, nullptr, d_out_off, d_out, cap, n_out, stream);
}

int fmx_search_context_fold_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k,
                                  const fmx_context_opts *ctx, const fmx_fold_opts *fold, uint64_t *out_off, fmx_result *out,
                                  size_t cap, size_t *n_out) {
  uint8_t map[256];
  int rc = fold_map_check(fold, map);
  if (rc) return rc;
  return ctx_search_host_form(idx, pat, off, k, ctx, map, nullptr, out_off, out, cap, n_out);
}

int fmx_search_context_classes_batch_dev(const fmx_index *idx, const void *d_el, const void *d_el_off, size_t k,
                                         const fmx_context_opts *ctx, const fmx_class_table *tab, void *d_out_off, void *d_out,
                                         size_t cap, size_t *n_out, void *stream) {
  std::vector<ClassRec> packed;
  CtxClasses cc{&packed, 1};
  int rc = classes_table_check(tab, &packed, &cc.largest);
  if (rc) return rc;
  return ctx_search_dev_form(idx, d_el, d_el_off, k, ctx, nullptr, &cc, d_out_off, d_out, cap, n_out, stream);
}

int fmx_search_context_classes_batch(const fmx_index *idx, const uint16_t *el, const uint64_t *el_off, size_t k,
                                     const fmx_context_opts *ctx, const fmx_class_table *tab, uint64_t *out_off, fmx_result *out,
                                     size_t cap, size_t *n_out) {
  std::vector<ClassRec> packed;
  CtxClasses cc{&packed, 1};
  int rc = classes_table_check(tab, &packed, &cc.largest);
  if (rc) return rc;
  return ctx_search_host_form(idx, el, el_off, k, ctx, nullptr, &cc, out_off, out, cap, n_out);
}

}  // extern "C"
