// fmx_edit.hip -- approximate search with insertions and deletions: edit distance up to two.
//
// A hit of pattern P (m bytes, matched last byte first) with budget e and symbol range A = [lo, hi] is a byte string Q of
// m - e .. m + e bytes whose cheapest alignment with P costs d <= e (fmx.h has the costs) and whose exact backward search
// ends with a non-empty interval; it is reported as (pattern, d, len = |Q|, sp, ep).  The search is a depth-first walk over
// the backward steps, as in fmx_approx.hip, whose nodes are the strings S that occur: a node is (t = |S|, sp, ep, R) with
// R[j] = min(d_A(S, the last j bytes of P), e + 1).  Only the entries with |j - t| <= e can be <= e, so a node keeps the
// five of them around t (kept at five whatever e is: the outer ones are e + 1, dead, for a smaller budget), four bits each.
//
// At a node: R[m] <= e is a hit.  M is the set of the P_j with R[j - 1] <= e (P_j = the j-th byte from the end of P): the
// symbols that continue an alignment for nothing.  The TRIED symbols are
//     min R == e                : M -- every other symbol costs an edit the node does not have;
//     min R <  e, several rows  : the candidates (the symbols of A that occur in the index, ascending), then M's others;
//     min R <  e, one row       : BWT'[sp] (0 on the EOF row) if it is a candidate or in M -- no other child has a row.
// One backward step per tried symbol, lane groups (16 quads, or 8 octets on the bytes layout) taking one symbol each per
// round; a step that comes back empty is still a step.  Every non-empty child is a node; its row follows from R and its symbol
// (ed_child).  Depth ends by itself: at t = m + e the only live entry is R[m] = e and M is empty.
//
// One WAVE owns one pattern at a time.  A round's children go to a frame of the wave's stack and the wave descends into
// them one at a time; a node's only child, found in its last round, is the continuation of the loop and takes no frame.
// Every node with a live row can branch, so the stack is as deep as the walk: kEdFrames frames per wave in device memory,
// allocated per call, read and written wave-uniformly.
//
// Hits are staged and ordered as in fmx_approx.hip: the sort key is pattern << 41 | sp << 3 | (len - m + e).
#include <fmx.h>

#include <algorithm>
#include <string>

#include "fmx_approx.h"
#include "fmx_device.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kEdThreads = 256;                // four waves: four patterns per workgroup
constexpr int kEdWaves = kEdThreads / 64;
constexpr uint32_t kEdFrames = FMX_EDIT_MAX_LEN + FMX_EDIT_MAX_EDITS + 1;   // nodes that push have t = 0 .. m + e - 1
constexpr int kEdRowBits = 38, kEdLenBits = 3; // rows are below 2^38, len - m + e below 8, patterns below 2^23: the sort key
constexpr int kEdBand = 2 * FMX_EDIT_MAX_EDITS + 1;

struct EdFrame {
  uint64_t sp, ep;                             // the node: its interval,
  uint32_t t, band, round, nchild;             // its depth and row; the next symbol round; this round's children
  uint32_t child, pad[3];                      // ... and the next one to walk
  uint64_t csp[16], cep[16];
  uint8_t csym[16];
};
static_assert(sizeof(EdFrame) == 320, "EdFrame");

struct EdShared {
  uint64_t cf[256];
  uint16_t slot[256];
  uint8_t cand[256];                           // the symbols of the range that occur in the index, ascending
  uint32_t ncand;
};

// slot b of a node of depth t holds R[t - 2 + b]
__device__ __forceinline__ uint32_t ed_get(uint32_t band, int b) { return (band >> (4 * b)) & 15u; }

// the row of the empty string: R[j] = j
__device__ __forceinline__ uint32_t ed_root(uint32_t m, uint32_t e) {
  uint32_t band = 0;
#pragma unroll
  for (int b = 0; b < kEdBand; b++) {
    const int j = b - 2;
    const uint32_t v = (j < 0 || (uint32_t)j > m) ? e + 1u : min((uint32_t)j, e + 1u);
    band |= v << (4 * b);
  }
  return band;
}

// byte b of the result = P_(t - 1 + b), what slot b of a node of depth t is compared with (0 where there is none)
__device__ __forceinline__ uint64_t ed_bytes(const uint8_t *__restrict__ P, uint32_t m, uint32_t t) {
  uint64_t pj = 0;
#pragma unroll
  for (int b = 0; b < kEdBand; b++) {
    const int j = (int)t - 1 + b;
    if (j >= 1 && (uint32_t)j <= m) pj |= (uint64_t)P[m - (uint32_t)j] << (8 * b);
  }
  return pj;
}

// The row of the child by symbol c of a node (t, band), pj = ed_bytes(P, m, t):
// R'[j] = min(R[j - 1] + sub(c, P_j), R[j] + ins(c), R'[j - 1] + 1), clipped at e + 1; c outside the range neither stands for
// another byte nor for nothing.
__device__ __forceinline__ uint32_t ed_child(uint32_t band, uint64_t pj, uint32_t t, uint32_t m, uint32_t e, uint32_t c, bool in_a) {
  const uint32_t dead = e + 1u, edit = in_a ? 1u : dead;
  uint32_t out = 0, prev = dead;
#pragma unroll
  for (int b = 0; b < kEdBand; b++) {
    const int j = (int)t - 1 + b;                            // slot b of the child holds R'[j]
    uint32_t v = ed_get(band, b) + (c == ((uint32_t)(pj >> (8 * b)) & 255u) ? 0u : edit);
    if (b + 1 < kEdBand) v = min(v, ed_get(band, b + 1) + edit);
    v = min(v, prev + 1u);
    if (j < 0 || (uint32_t)j > m || v > dead) v = dead;
    out |= v << (4 * b);
    prev = v;
  }
  return out;
}

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kEdThreads) void k_edit(DevIndex ix, const uint8_t *__restrict__ pat,
                                                     const uint64_t *__restrict__ off, uint64_t k, uint32_t e, uint32_t sub_lo,
                                                     uint32_t sub_hi, EdFrame *__restrict__ stack,
                                                     unsigned long long *__restrict__ stage, uint64_t cap,
                                                     unsigned long long *__restrict__ total,
                                                     unsigned long long *__restrict__ too_long,
                                                     unsigned long long *__restrict__ counters) {
  __shared__ EdShared sh;
  for (int c = threadIdx.x; c < 256; c += kEdThreads) {
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
  EdFrame *fr = stack + ((uint64_t)blockIdx.x * kEdWaves + wv) * kEdFrames;
  const uint64_t nwaves = (uint64_t)gridDim.x * kEdWaves;
  unsigned long long steps = 0, reqs = 0;                    // counted by the lane that leads the group
  auto in_range = [&](uint32_t c) { return c >= sub_lo && c <= sub_hi; };
  auto is_cand = [&](uint32_t c) { return in_range(c) && sh.slot[c] < kSlotEof; };
  for (uint64_t q = (uint64_t)blockIdx.x * kEdWaves + wv; q < k; q += nwaves) {
    const uint64_t b0 = off[q], en = off[q + 1];
    if (en > b0 && en - b0 > FMX_EDIT_MAX_LEN) {             // the device form cannot know before: skipped, the call refused
      if (lane == 0) atomicOr(too_long, 1ull);
      continue;
    }
    const uint8_t *P = pat + b0;
    const uint32_t m = en > b0 ? (uint32_t)(en - b0) : 0u;
    uint64_t sp = 0, ep = ix.n;
    uint32_t t = 0, band = ed_root(m, e), depth = 0, round = 0;
    bool node = true, fresh = true;                          // !node: take the next child of the top frame, or leave it
    for (;;) {
      if (!node) {
        if (depth == 0) break;
        EdFrame &f = fr[depth - 1];
        const uint32_t ch = f.child;
        node = true;
        if (ch < f.nchild) {                                 // the next child of the round
          const uint32_t c = f.csym[ch & 15u], pt = f.t;
          sp = f.csp[ch & 15u];
          ep = f.cep[ch & 15u];
          band = ed_child(f.band, ed_bytes(P, m, pt), pt, m, e, c, in_range(c));
          t = pt + 1;
          round = 0;
          fresh = true;
          ap_wave_sync();
          if (lane == 0) f.child = ch + 1;
          ap_wave_sync();
        } else {                                             // back at the node: its later rounds
          depth--;
          sp = f.sp;
          ep = f.ep;
          t = f.t;
          band = f.band;
          round = f.round;
          fresh = false;
        }
        continue;
      }
      const int hb = (int)m - (int)t + 2;                    // the slot of R[m]
      if (fresh && hb >= 0 && hb < kEdBand && ed_get(band, hb) <= e)
        ap_emit(lane == 0, q, ed_get(band, hb) | (t << 16), sp, ep, lane, stage, cap, total);
      // the tried symbols: the first nc0 from the candidate list, then the nex bytes of ex
      const uint64_t pj = ed_bytes(P, m, t);
      uint32_t min_r = e + 1u;
#pragma unroll
      for (int b = 0; b < kEdBand; b++) min_r = min(min_r, ed_get(band, b));
      uint32_t live = 0;                                     // bit b: slot b is <= e and has a pattern byte behind it
#pragma unroll
      for (int b = 0; b < kEdBand; b++) {
        const int j = (int)t - 1 + b;
        if (ed_get(band, b) <= e && j >= 1 && (uint32_t)j <= m) live |= 1u << b;
      }
      const bool budget = min_r < e;
      uint32_t nc0 = 0, nex = 0;
      uint64_t ex = 0;
      if (budget && ep - sp == 1) {                          // the one-row rule
        const uint32_t bsym = sp == ix.eof ? 0u : (uint32_t)ix.bwt[sp];
        bool in = is_cand(bsym);
#pragma unroll
        for (int b = 0; b < kEdBand; b++)
          if ((live >> b & 1u) && ((uint32_t)(pj >> (8 * b)) & 255u) == bsym) in = true;
        ex = bsym;
        nex = in ? 1u : 0u;
      } else {
        nc0 = budget ? sh.ncand : 0u;
#pragma unroll
        for (int b = 0; b < kEdBand; b++) {
          const uint32_t sym = (uint32_t)(pj >> (8 * b)) & 255u;
          bool take = (live >> b & 1u) && !(budget && is_cand(sym));
#pragma unroll
          for (int b2 = 0; b2 < b; b2++)
            if ((live >> b2 & 1u) && ((uint32_t)(pj >> (8 * b2)) & 255u) == sym) take = false;
          if (take) {
            ex |= (uint64_t)sym << (8 * nex);
            nex++;
          }
        }
      }
      const uint32_t nt = nc0 + nex;
      node = false;
      while (round * NG < nt) {
        const uint32_t ci = round * NG + g;
        round++;
        const bool act = ci < nt;
        const uint32_t c = !act ? 0u : ci < nc0 ? (uint32_t)sh.cand[ci] : (uint32_t)(ex >> (8 * (ci - nc0))) & 255u;
        uint64_t s = sp, u = ep;
        bool hit = false;
        if (act) {
          const uint16_t sl = sh.slot[c];
          const uint32_t r = u - s == 1 ? single_row_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, u)
                                        : backward_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, u);
          if (lead) { steps++; reqs += r; }
          hit = s < u;
        }
        const unsigned long long mm = __builtin_amdgcn_ballot_w64(hit && lead);
        if (!mm) continue;
        const uint32_t nch = (uint32_t)__popcll(mm);
        if (nch == 1 && round * NG >= nt) {                  // the only child of the last round: the loop goes on with it
          const int src = __ffsll((long long)mm) - 1;
          const uint32_t cc = (uint32_t)__shfl((int)c, src, 64);
          sp = __shfl(s, src, 64);
          ep = __shfl(u, src, 64);
          band = ed_child(band, pj, t, m, e, cc, in_range(cc));
          t++;
          round = 0;
          fresh = true;
          node = true;
          break;
        }
        if (depth >= kEdFrames) break;                       // (a pushing node has t < m + e: never)
        EdFrame &f = fr[depth];
        if (hit && lead) {
          const uint32_t at = (uint32_t)__popcll(mm & ((1ull << lane) - 1ull)) & 15u;
          f.csp[at] = s;
          f.cep[at] = u;
          f.csym[at] = (uint8_t)c;
        }
        if (lane == 0) {
          f.sp = sp;
          f.ep = ep;
          f.t = t;
          f.band = band;
          f.round = round;
          f.nchild = nch;
          f.child = 0;
        }
        ap_wave_sync();
        depth++;
        break;
      }
    }
  }
  // the call's own counters: private slots, folded into the handle's afterwards (k_counters_fold: fmx_host.h, Metered)
  counters_add(counters, 2ull * steps, steps, reqs);
}

// key = pattern << 41 | sp << 3 | (len - m + e): a pattern's hits by (sp, len)
__global__ __launch_bounds__(256) void k_edit_keys(const unsigned long long *__restrict__ stage, uint64_t rows,
                                                   const uint64_t *__restrict__ off, uint32_t e,
                                                   unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const unsigned long long w = stage[3 * j], q = w & 0xFFFFFFFFull;
    const uint64_t m = off[q + 1] - off[q];
    const unsigned long long rel = ((w >> 48) + e - m) & ((1ull << kEdLenBits) - 1ull);
    key[j] = (q << (kEdRowBits + kEdLenBits)) | (stage[3 * j + 1] << kEdLenBits) | rel;
    val[j] = (uint32_t)j;
  }
}

template <bool WIDE, uint32_t LAYOUT>
static hipError_t ed_grid(const Index *h, uint64_t k, uint32_t *grid) {
  return resident_grid<k_edit<WIDE, LAYOUT>>(h, kEdThreads, k, kEdWaves, grid);
}

static int edit_check(const Index *h) {
  if (h->block_mode) {
    set_error("edit search: not for fmx_open_block handles");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n >= (1ull << kEdRowBits)) {
    set_error("edit search: the index has 2^38 rows or more");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

struct EditInfo {
  uint64_t total = 0, steps = 0, requests = 0;
  double search_ms = 0.0, sort_ms = 0.0;        // device events: the search kernel, the ordering step
};

// The hits of k patterns within e edits over [lo, hi], device pointers throughout; allocates, synchronises `st`, frees its
// temporaries on every path.  info->total is the exact number of hits; when it exceeds cap nothing is ordered and
// d_out_off / d_out are unspecified.  check_len: a pattern of more than FMX_EDIT_MAX_LEN bytes may be among them (the
// device form) -- FMX_ERR_ARG then, after the launch.
static int edit_search(const Index *h, const void *d_pat, const void *d_off, uint64_t k, uint32_t e, uint32_t lo, uint32_t hi,
                       void *d_out_off, void *d_out, uint64_t cap, bool check_len, hipStream_t st, EditInfo *info) {
  *info = EditInfo{};
  uint32_t grid = 1;
  if (k) {
#define FMX_ED_GRID(W, L) HIP_TRY((ed_grid<W, L>(h, k, &grid)), "k_edit")
    FMX_LAYOUT_DISPATCH(h, FMX_ED_GRID);
#undef FMX_ED_GRID
  }
  const uint64_t stack_bytes = k ? (uint64_t)grid * kEdWaves * kEdFrames * sizeof(EdFrame) : 0;
  int rc;
  if ((rc = device_room(24 * cap + stack_bytes + kMeteredBytes + 8, "the edit search"))) return rc;
  Events<3> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *stage = nullptr, *too_long = nullptr;
  EdFrame *stack = nullptr;
  Metered own;
  DEV_ALLOC(mem, stage, 24 * cap, "edit staging");
  DEV_ALLOC(mem, stack, stack_bytes, "edit stacks");
  DEV_ALLOC(mem, too_long, 8, "edit flag");
  if ((rc = own.alloc(mem, "edit")) || (rc = own.zero(st))) return rc;
  HIP_TRY(hipMemsetAsync(too_long, 0, 8, st), "memset");
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (k) {
#define FMX_ED_CALL(W, L)                                                                                                       \
  hipLaunchKernelGGL((k_edit<W, L>), dim3(grid), dim3(kEdThreads), 0, st, h->dev, static_cast<const uint8_t *>(d_pat),          \
                     static_cast<const uint64_t *>(d_off), k, e, lo, hi, stack, stage, cap, own.line + kLineHits, too_long,     \
                     own.mine)
    FMX_LAYOUT_DISPATCH(h, FMX_ED_CALL);
#undef FMX_ED_CALL
    HIP_TRY(hipGetLastError(), "k_edit");
    if ((rc = own.fold(h, 1, st))) return rc;                // counter [1]: the backward steps
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  MeterCounts cnt;
  if ((rc = own.finish(h, st, k ? 1 : 0, &cnt))) return rc;
  info->search_ms = ev.ms(0, 1);
  info->total = cnt.hits;
  info->steps = cnt.steps;
  info->requests = cnt.requests;
  if (check_len && k) {
    unsigned long long flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, too_long, 8, hipMemcpyDeviceToHost, st), "D2H");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (flag) return arg_fail("search_edit: a pattern is longer than 255 bytes");
  }
  if (info->total > cap) return FMX_OK;                      // the caller reports the overflow; nothing is ordered
  const uint64_t rows = info->total;
  unsigned long long *out_off = static_cast<unsigned long long *>(d_out_off);
  if (rows == 0) {
    HIP_TRY(launch_csr_off(nullptr, 0, k, kEdRowBits + kEdLenBits, out_off, st), "k_edit_off");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return FMX_OK;
  }
  SortSpace ws;
  if ((rc = ws.alloc(mem, rows, "edit sort"))) return rc;
  LAUNCH("k_edit_keys", k_edit_keys, dim3(flat_grid(rows)), dim3(256), st, stage, rows, static_cast<const uint64_t *>(d_off), e, ws.keys(),
         ws.vals());
  HIP_TRY(ws.sort(rows, kEdRowBits + kEdLenBits + std::min(23, bits_for(k - 1)), st), "radix sort");      // pattern ids 0 .. k - 1
  HIP_TRY(launch_gather3(stage, ws.vals(), rows, static_cast<unsigned long long *>(d_out), st), "k_edit_gather");
  HIP_TRY(launch_csr_off(ws.keys(), rows, k, kEdRowBits + kEdLenBits, out_off, st), "k_edit_off");
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the temporaries go when this returns
  info->sort_ms = ev.ms(1, 2);
  return FMX_OK;
}

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static thread_local EditInfo g_edit_last;
static_assert(sizeof(fmx_edit_hit) == 24 && sizeof(fmx_edit_opts) == 8, "fmx.h");

// What refuses a call before the device is touched; the budget and the range as the kernel takes them.
static int edit_args(const fmx_index *idx, size_t k, const fmx_edit_opts *opts, const void *out_off, const void *out, size_t cap,
                     const size_t *n_out, uint32_t *e, uint32_t *lo, uint32_t *hi) {
  if (!n_out) return arg_fail("search_edit: n_out is null");
  *e = 0; *lo = 1; *hi = 255;
  if (opts) {
    if (opts->max_edits > FMX_EDIT_MAX_EDITS) return arg_fail("fmx_edit_opts.max_edits: 0 .. 2");
    if (opts->reserved != 0) return arg_fail("fmx_edit_opts.reserved must be 0");
    if ((opts->sub_lo == 0) != (opts->sub_hi == 0)) return arg_fail("fmx_edit_opts: symbol 0 is never inserted or substituted (sub_lo >= 1; 0, 0 = the default range)");
    if (opts->sub_lo > opts->sub_hi) return arg_fail("fmx_edit_opts: sub_lo > sub_hi");
    *e = opts->max_edits;
    if (opts->sub_lo) { *lo = opts->sub_lo; *hi = opts->sub_hi; }
  }
  if ((uint64_t)k > (1ull << 23)) return arg_fail("search_edit: at most 2^23 patterns per call");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("search_edit: cap must be below 2^32");
  if (!out_off || (cap && !out)) return arg_fail("null argument");
  if (!idx) return arg_fail("search_edit: the handle is null");
  return edit_check(H(idx));
}

extern "C" {

int fmx_search_edit_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_edit_opts *opts,
                              void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  uint32_t e, lo, hi;
  int rc = edit_args(idx, k, opts, d_out_off, d_out, cap, n_out, &e, &lo, &hi);
  if (rc) return rc;
  if (k && !d_off) return arg_fail("null argument");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  if ((rc = not_capturing((hipStream_t)stream, "an edit search"))) return rc;
  rc = edit_search(h, d_pat, d_off, k, e, lo, hi, d_out_off, d_out, cap, true, (hipStream_t)stream, &g_edit_last);
  if (rc) return rc;
  *n_out = (size_t)g_edit_last.total;
  return g_edit_last.total > cap ? csr_overflow("search_edit", g_edit_last.total, cap) : FMX_OK;
}

int fmx_search_edit_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_edit_opts *opts,
                          uint64_t *out_off, fmx_edit_hit *out, size_t cap, size_t *n_out) {
  uint32_t e, lo, hi;
  if (k && (uint64_t)k <= (1ull << 23) && off) {
    if (!offsets_monotonic(off, 0, k)) return arg_fail("pattern offsets must be non-decreasing");
    for (size_t q = 0; q < k; q++)
      if (off[q + 1] - off[q] > FMX_EDIT_MAX_LEN) return arg_fail("search_edit: a pattern is longer than 255 bytes");
  }
  int rc = edit_args(idx, k, opts, out_off, out, cap, n_out, &e, &lo, &hi);
  if (rc) return rc;
  if (k && !off) return arg_fail("null argument");
  const uint64_t lo_off = k ? off[0] : 0, total_bytes = k ? off[k] - lo_off : 0;
  if (total_bytes && !pat) return arg_fail("pat is null");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  void *d_pat = nullptr;
  uint64_t *d_off = nullptr, *d_out_off = nullptr;
  fmx_edit_hit *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("edit patterns", total_bytes ? pat + lo_off : nullptr, total_bytes, "edit offsets", off, k, true, &d_pat, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out_off, 8 * (k + 1), "edit offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_edit_hit) * cap, "edit hits");
  rc = edit_search(h, d_pat, d_off, k, e, lo, hi, d_out_off, d_out, cap, false, hc.own.s, &g_edit_last);
  if (rc) return rc;
  const uint64_t total = g_edit_last.total;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("search_edit", total, cap);
  return hc.download_csr(out_off, d_out_off, k, out, d_out, total, sizeof(fmx_edit_hit));
}

int fmx_edit_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests) {
  if (search_ms) *search_ms = g_edit_last.search_ms;
  if (sort_ms) *sort_ms = g_edit_last.sort_ms;
  if (steps) *steps = g_edit_last.steps;
  if (requests) *requests = g_edit_last.requests;
  return FMX_OK;
}

}  // extern "C"
