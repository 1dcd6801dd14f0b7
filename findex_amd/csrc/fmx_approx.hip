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

#include "fmx_approx.h"
#include "fmx_device.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kApThreads = 256;                // four waves: four patterns per workgroup
constexpr int kApWaves = kApThreads / 64;
constexpr uint32_t kApFrames = 2;              // nodes that push have d = 0 .. e - 2
constexpr int kApRowBits = 38;                 // rows are below 2^38, patterns below 2^26: the sort key

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

// (ap_wave_sync and ap_emit: fmx_approx.h, shared with fmx_edit.hip)

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
  // the call's own counters: private slots, folded into the handle's afterwards (k_counters_fold: fmx_host.h, Metered)
  counters_add(counters, 2ull * steps, steps, reqs);
}

__global__ __launch_bounds__(256) void k_approx_keys(const unsigned long long *__restrict__ stage, uint64_t rows,
                                                     unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    key[j] = ((stage[3 * j] & 0xFFFFFFFFull) << kApRowBits) | stage[3 * j + 1];
    val[j] = (uint32_t)j;
  }
}

template <bool WIDE, uint32_t LAYOUT>
static hipError_t ap_launch(const Index *h, const uint8_t *pat, const uint64_t *off, uint64_t k, uint32_t e, uint32_t lo,
                            uint32_t hi, unsigned long long *stage, uint64_t cap, unsigned long long *total,
                            unsigned long long *mine, hipStream_t st) {
  uint32_t grid = 0;
  const hipError_t he = resident_grid<k_approx<WIDE, LAYOUT>>(h, kApThreads, k, kApWaves, &grid);
  if (he != hipSuccess) return he;
  hipLaunchKernelGGL((k_approx<WIDE, LAYOUT>), dim3(grid), dim3(kApThreads), 0, st, h->dev, pat, off, k, e, lo, hi, stage, cap,
                     total, mine);
  return hipGetLastError();
}

static int approx_check(const Index *h) {
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

struct ApproxInfo {
  uint64_t total = 0, steps = 0, requests = 0;
  double search_ms = 0.0, sort_ms = 0.0;      // device events: the search kernel, the ordering step
};

// The hits of k patterns within e substitutions from [lo, hi], device pointers throughout; allocates, synchronises `st`, frees
// its temporaries on every path.  info->total is the exact number of hits; when it exceeds cap nothing is ordered and
// d_out_off / d_out are unspecified.
static int approx_search(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint32_t e, uint32_t lo, uint32_t hi,
                         void *d_out_off, void *d_out, uint64_t cap, hipStream_t st, ApproxInfo *info) {
  *info = ApproxInfo{};
  Events<3> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *stage = nullptr;
  Metered own;
  int rc;
  DEV_ALLOC(mem, stage, 24 * cap, "approx staging");
  if ((rc = own.alloc(mem, "approx")) || (rc = own.zero(st))) return rc;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (k) {
#define FMX_AP_CALL(W, L) \
  HIP_TRY((ap_launch<W, L>(h, static_cast<const uint8_t *>(d_pat), static_cast<const uint64_t *>(d_off), k, e, lo, hi, stage, \
                           cap, own.line + kLineHits, own.mine, st)), "k_approx")
    FMX_LAYOUT_DISPATCH(h, FMX_AP_CALL);
#undef FMX_AP_CALL
    if ((rc = own.fold(h, 1, st))) return rc;                // counter [1]: the backward steps
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  MeterCounts cnt;
  if ((rc = own.finish(h, st, k ? 1 : 0, &cnt))) return rc;
  info->search_ms = ev.ms(0, 1);
  info->total = cnt.hits;
  info->steps = cnt.steps;
  info->requests = cnt.requests;
  if (info->total > cap) return FMX_OK;                      // the caller reports the overflow; nothing is ordered
  const uint64_t rows = info->total;
  unsigned long long *out_off = static_cast<unsigned long long *>(d_out_off);
  if (rows == 0) {
    HIP_TRY(launch_csr_off(nullptr, 0, k, kApRowBits, out_off, st), "k_approx_off");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return FMX_OK;
  }
  SortSpace ws;
  if ((rc = ws.alloc(mem, rows, "approx sort"))) return rc;
  LAUNCH("k_approx_keys", k_approx_keys, dim3(flat_grid(rows)), dim3(256), st, stage, rows, ws.keys(), ws.vals());
  HIP_TRY(ws.sort(rows, kApRowBits + std::min(26, bits_for(k - 1)), st), "radix sort");      // pattern ids 0 .. k - 1
  HIP_TRY(launch_gather3(stage, ws.vals(), rows, static_cast<unsigned long long *>(d_out), st), "k_approx_gather");
  HIP_TRY(launch_csr_off(ws.keys(), rows, k, kApRowBits, out_off, st), "k_approx_off");
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the temporaries go when this returns
  info->sort_ms = ev.ms(1, 2);
  return FMX_OK;
}

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static thread_local ApproxInfo g_approx_last;

// What refuses a call before the device is touched; the budget and the range as the kernel takes them.
static int approx_args(const fmx_index *idx, size_t k, const fmx_approx_opts *opts, const void *out_off, const void *out, size_t cap,
                       const size_t *n_out, uint32_t *e, uint32_t *lo, uint32_t *hi) {
  if (!n_out) return arg_fail("approx: n_out is null");
  *e = 0; *lo = 1; *hi = 255;
  if (opts) {
    if (opts->max_mismatches > FMX_APPROX_MAX_MISMATCHES) return arg_fail("fmx_approx_opts.max_mismatches: 0 .. 3");
    if (opts->reserved != 0) return arg_fail("fmx_approx_opts.reserved must be 0");
    if ((opts->sub_lo == 0) != (opts->sub_hi == 0)) return arg_fail("fmx_approx_opts: symbol 0 is never substituted (sub_lo >= 1; 0, 0 = the default range)");
    if (opts->sub_lo > opts->sub_hi) return arg_fail("fmx_approx_opts: sub_lo > sub_hi");
    *e = opts->max_mismatches;
    if (opts->sub_lo) { *lo = opts->sub_lo; *hi = opts->sub_hi; }
  }
  if ((uint64_t)k > (1ull << 26)) return arg_fail("approx: at most 2^26 patterns per call");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("approx: cap must be below 2^32");
  if (!out_off || (cap && !out)) return arg_fail("null argument");
  if (!idx) return arg_fail("approx: the handle is null");
  return approx_check(H(idx));
}

extern "C" {

int fmx_search_approx_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_approx_opts *opts,
                                void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  uint32_t e, lo, hi;
  int rc = approx_args(idx, k, opts, d_out_off, d_out, cap, n_out, &e, &lo, &hi);
  if (rc) return rc;
  if (k && !d_off) return arg_fail("null argument");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  if ((rc = not_capturing((hipStream_t)stream, "an approximate search"))) return rc;
  rc = approx_search(h, d_pat, d_off, k, e, lo, hi, d_out_off, d_out, cap, (hipStream_t)stream, &g_approx_last);
  if (rc) return rc;
  *n_out = (size_t)g_approx_last.total;
  return g_approx_last.total > cap ? csr_overflow("search_approx", g_approx_last.total, cap) : FMX_OK;
}

int fmx_search_approx_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_approx_opts *opts,
                            uint64_t *out_off, fmx_approx_hit *out, size_t cap, size_t *n_out) {
  uint32_t e, lo, hi;
  if (k && (uint64_t)k <= (1ull << 26) && off && !offsets_monotonic(off, 0, k)) return arg_fail("pattern offsets must be non-decreasing");
  int rc = approx_args(idx, k, opts, out_off, out, cap, n_out, &e, &lo, &hi);
  if (rc) return rc;
  if (k && !off) return arg_fail("null argument");
  const uint64_t lo_off = k ? off[0] : 0, total_bytes = k ? off[k] - lo_off : 0;
  if (total_bytes && !pat) return arg_fail("pat is null");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  void *d_pat = nullptr;
  uint64_t *d_off = nullptr, *d_out_off = nullptr;
  fmx_approx_hit *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("approx patterns", total_bytes ? pat + lo_off : nullptr, total_bytes, "approx offsets", off, k, true, &d_pat, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out_off, 8 * (k + 1), "approx offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_approx_hit) * cap, "approx hits");
  rc = approx_search(h, d_pat, d_off, k, e, lo, hi, d_out_off, d_out, cap, hc.own.s, &g_approx_last);
  if (rc) return rc;
  const uint64_t total = g_approx_last.total;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("search_approx", total, cap);
  return hc.download_csr(out_off, d_out_off, k, out, d_out, total, sizeof(fmx_approx_hit));
}

int fmx_approx_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests) {
  if (search_ms) *search_ms = g_approx_last.search_ms;
  if (sort_ms) *sort_ms = g_approx_last.sort_ms;
  if (steps) *steps = g_approx_last.steps;
  if (requests) *requests = g_approx_last.requests;
  return FMX_OK;
}

}  // extern "C"
