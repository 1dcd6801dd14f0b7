// fmx_fold.hip -- literal search under a fold map: every case variant of a pattern that occurs.
//
// A fold map sends each byte to the representative of its class.  A hit of pattern P (m bytes, matched last byte first) is a
// string Q of m bytes with fold[Q[j]] == fold[P[j]] at every j whose exact backward search ends with a non-empty interval;
// it is reported as (pattern, m, sp, ep).  The search is a depth-first walk over wave-uniform nodes (i bytes left, sp, ep):
//   singleton : P[i - 1]'s class has one member in the map -- the plain step of the exact search, by every lane group alike;
//   branching : otherwise, with two rows or more, lane group g steps with the g-th member of the class that occurs in the
//               index (a class has at most 8 members: one round of 16 quads or 8 octets).  The wave goes on with the
//               non-empty child of the smallest symbol and pushes the others as {sp, ep, i - 1} onto its stack;
//   one row   : a node of one row whose class is not a singleton has one non-empty child at most, the symbol BWT'[sp] (0 on
//               the EOF row, which no class of two holds): in the class, the node makes that one step; else it dies without one.
// At i == 0 the wave reports the node and pops.  A pattern byte pushes at most 7 entries, so the stack of a wave is 7 entries
// per byte of the call's longest pattern (255 where the host does not know the lengths) in device memory (as fmx_edit.hip's
// frames) and cannot overflow: a pattern longer than the slab was sized for is skipped and flagged.
//
// One WAVE owns one pattern at a time; hits go to a staging area in the order they are found and a radix sort of
// pattern << 38 | sp puts them into their CSR order, which depends on nothing but the input (fmx_approx.hip's scheme).
#include <fmx.h>

#include <algorithm>
#include <string>

#include "fmx_approx.h"
#include "fmx_device.h"
#include "fmx_fold.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kFoThreads = 256;                // four waves: four patterns per workgroup
constexpr int kFoWaves = kFoThreads / 64;
constexpr uint32_t kFoPush = FMX_FOLD_MAX_CLASS - 1;      // stack entries per pattern byte at the most
constexpr int kFoRowBits = kFoldRowBits;       // rows are below 2^38, patterns below 2^26: the sort key

struct FoEntry {
  uint64_t sp, ep, i;
};
static_assert(sizeof(FoEntry) == 24, "a stack entry");

struct FoShared {
  uint64_t cf[256];
  uint16_t slot[256];
  uint8_t fold[256];
  uint8_t size[256];                           // by representative: the members of its class in the map ...
  uint8_t occ[256];                            // ... and how many of them occur in the index,
  uint8_t mem[256][FMX_FOLD_MAX_CLASS];        // ascending
};

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kFoThreads) void k_fold(DevIndex ix, const uint8_t *__restrict__ pat,
                                                     const uint64_t *__restrict__ off, uint64_t k,
                                                     const uint8_t *__restrict__ map, const uint8_t *__restrict__ leads,
                                                     uint64_t per, FoEntry *__restrict__ stack, uint32_t max_len,
                                                     unsigned long long *__restrict__ stage, uint64_t cap,
                                                     unsigned long long *__restrict__ total,
                                                     unsigned long long *__restrict__ too_long,
                                                     unsigned long long *__restrict__ counters) {
  __shared__ FoShared sh;
  for (int c = threadIdx.x; c < 256; c += kFoThreads) {
    sh.cf[c] = ix.cf[c];
    sh.slot[c] = ix.slot[c];
    sh.fold[c] = map[c];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 256; r += kFoThreads) {
    uint32_t size = 0, occ = 0;
    if (sh.fold[r] == r)
      for (uint32_t c = 0; c < 256u; c++)
        if (sh.fold[c] == r) {
          size++;
          if (sh.slot[c] < kSlotEof && occ < FMX_FOLD_MAX_CLASS) sh.mem[r][occ++] = (uint8_t)c;
        }
    sh.size[r] = (uint8_t)min(size, 255u);
    sh.occ[r] = (uint8_t)occ;
  }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, g = lane / G;
  const bool lead = lc.t == 0;
  const uint32_t slab = max_len * kFoPush;                   // entries per wave: what the host sized the stacks for
  FoEntry *st = stack + ((uint64_t)blockIdx.x * kFoWaves + wv) * slab;
  const uint64_t nwaves = (uint64_t)gridDim.x * kFoWaves;
  unsigned long long steps = 0, reqs = 0;                    // counted by the lane that leads the group (lane 0 for the wave's own steps)
  auto step = [&](uint32_t c, uint64_t &s, uint64_t &t, bool count) {
    const uint16_t sl = sh.slot[c];
    const uint32_t r = t - s == 1 ? single_row_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, t)
                                  : backward_step<WIDE, LAYOUT>(ix, c, sl, sh.cf[c], lc, s, t);
    if (count) { steps++; reqs += r; }
  };
  for (uint64_t q = (uint64_t)blockIdx.x * kFoWaves + wv; q < k; q += nwaves) {
    const uint64_t b = off[q], en = off[q + 1];
    if (en > b && en - b > max_len) {                        // the device form cannot know before: skipped, the call refused
      if (lane == 0) atomicOr(too_long, 1ull);
      continue;
    }
    const uint8_t *P = pat + b;
    const uint64_t m = en > b ? en - b : 0;
    const uint64_t ld = leads ? leads[q] : 0u;
    const uint64_t grp = per > 1 ? q / per : q;
    const uint32_t tag = (uint32_t)m | ((per > 1 && ld) ? kFoldLeadBit : 0u);
    uint64_t i = m, sp = 0, ep = ix.n;
    uint32_t top = 0;
    bool node = true;                                        // false: pop the next entry, or leave the pattern
    for (;;) {
      if (!node) {
        if (top == 0) break;
        top--;
        const FoEntry e = st[top];
        sp = e.sp;
        ep = e.ep;
        i = e.i;
        node = true;
        continue;
      }
      if (i == 0) {                                          // the pattern is through: a hit
        ap_emit(lane == 0, grp, tag, sp, ep, lane, stage, cap, total);
        node = false;
        continue;
      }
      const uint32_t pc = P[i - 1], rep = sh.fold[pc];
      if (sh.size[rep] <= 1 || i + ld > m) {                 // a singleton class, or a leading exact step: the exact search's step
        step(pc, sp, ep, lane == 0);
        i--;
        node = sp < ep;
        continue;
      }
      if (ep - sp == 1) {                                    // the one-row rule
        const uint32_t bsym = sp == ix.eof ? 0u : (uint32_t)ix.bwt[sp];
        if (sh.fold[bsym] != rep) {
          node = false;
          continue;
        }
        step(bsym, sp, ep, lane == 0);
        i--;
        node = sp < ep;
        continue;
      }
      const bool act = g < sh.occ[rep];
      const uint32_t c = sh.mem[rep][act ? g : 0u];
      uint64_t s = sp, t = ep;
      bool hit = false;
      if (act) {
        step(c, s, t, lead);
        hit = s < t;
      }
      const unsigned long long mm = __builtin_amdgcn_ballot_w64(hit && lead);
      if (!mm) {
        node = false;
        continue;
      }
      const int src = __ffsll((long long)mm) - 1;            // the lowest group: the smallest symbol
      const uint32_t nch = (uint32_t)__popcll(mm);
      if (nch > 1) {
        if (hit && lead && lane != (uint32_t)src) {
          const uint32_t at = top + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull)) - 1u;
          if (at < slab) st[at] = FoEntry{s, t, i - 1};      // (nch - 1 <= 7 per pattern byte: never past the slab)
        }
        top = min(top + nch - 1u, slab);
        ap_wave_sync();
      }
      sp = __shfl(s, src, 64);
      ep = __shfl(t, src, 64);
      i--;
    }
  }
  // the call's own counters: private slots, folded into the handle's afterwards (k_counters_fold: fmx_host.h, Metered)
  counters_add(counters, 2ull * steps, steps, reqs);
}

// key = group << (38 + tb) | sp << tb | the lead bit (tb == 1 only): a group's hits by sp, the plain record first
__global__ __launch_bounds__(256) void k_fold_keys(const unsigned long long *__restrict__ stage, uint64_t rows, int tb,
                                                   unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const unsigned long long w = stage[3 * j];
    key[j] = ((w & 0xFFFFFFFFull) << (kFoRowBits + tb)) | (stage[3 * j + 1] << tb) | (tb ? w >> 63 : 0ull);
    val[j] = (uint32_t)j;
  }
}

template <bool WIDE, uint32_t LAYOUT>
static hipError_t fo_grid(const Index *h, uint64_t k, uint32_t *grid) {
  return resident_grid<k_fold<WIDE, LAYOUT>>(h, kFoThreads, k, kFoWaves, grid);
}

int fold_handle_check(const Index *h) {
  if (h->block_mode) {
    set_error("fold search: not for fmx_open_block handles");
    return FMX_ERR_UNSUPPORTED;
  }
  if (h->n >= (1ull << kFoRowBits)) {
    set_error("fold search: the index has 2^38 rows or more");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

int fold_map_check(const fmx_fold_opts *opts, uint8_t map[256]) {
  if (!opts) {
    for (int c = 0; c < 256; c++) map[c] = (uint8_t)((c >= 'A' && c <= 'Z') ? c + 32 : c);
    return FMX_OK;
  }
  if (opts->flags != 0 || opts->reserved != 0) return arg_fail("fmx_fold_opts.flags and .reserved must be 0");
  uint32_t size[256] = {0};
  for (int c = 0; c < 256; c++) {
    const uint8_t r = opts->fold[c];
    if (opts->fold[r] != r) return arg_fail("fmx_fold_opts.fold is not idempotent: fold[fold[c]] != fold[c]");
    if ((r == 0) != (c == 0)) return arg_fail("fmx_fold_opts.fold: byte 0 folds to itself and no other byte folds to 0");
    if (++size[r] > FMX_FOLD_MAX_CLASS) return arg_fail("fmx_fold_opts.fold: a class of more than 8 members");
    map[c] = r;
  }
  return FMX_OK;
}

int fold_search(const Index *h, const void *d_pat, const void *d_off, uint64_t k, const uint8_t map[256], const uint8_t *d_lead,
                uint64_t per, uint32_t max_len, void *d_out_off, void *d_out, uint64_t cap, bool check_len, hipStream_t st,
                FoldInfo *info) {
  *info = FoldInfo{};
  max_len = std::min<uint32_t>(std::max<uint32_t>(max_len, 1u), FMX_FOLD_MAX_LEN);
  const int tb = per > 1 ? 1 : 0;
  const uint64_t groups = per > 1 ? k / per : k;
  uint32_t grid = 1;
  if (k) {
#define FMX_FO_GRID(W, L) HIP_TRY((fo_grid<W, L>(h, k, &grid)), "k_fold")
    FMX_LAYOUT_DISPATCH(h, FMX_FO_GRID);
#undef FMX_FO_GRID
  }
  const uint64_t stack_bytes = k ? (uint64_t)grid * kFoWaves * max_len * kFoPush * sizeof(FoEntry) : 0;
  int rc;
  if ((rc = device_room(24 * cap + stack_bytes + kMeteredBytes + 256 + 8, "the fold search"))) return rc;
  Events<3> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *stage = nullptr, *too_long = nullptr;
  FoEntry *stack = nullptr;
  uint8_t *d_map = nullptr;
  Metered own;
  DEV_ALLOC(mem, stage, 24 * cap, "fold staging");
  DEV_ALLOC(mem, stack, stack_bytes, "fold stacks");
  DEV_ALLOC(mem, too_long, 8, "fold flag");
  DEV_ALLOC(mem, d_map, 256, "fold map");
  if ((rc = own.alloc(mem, "fold")) || (rc = own.zero(st))) return rc;
  HIP_TRY(hipMemsetAsync(too_long, 0, 8, st), "memset");
  HIP_TRY(hipMemcpyAsync(d_map, map, 256, hipMemcpyHostToDevice, st), "H2D(fold map)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the map may be on the caller's stack
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (k) {
#define FMX_FO_CALL(W, L)                                                                                                       \
  hipLaunchKernelGGL((k_fold<W, L>), dim3(grid), dim3(kFoThreads), 0, st, h->dev, static_cast<const uint8_t *>(d_pat),          \
                     static_cast<const uint64_t *>(d_off), k, d_map, d_lead, per, stack, max_len, stage, cap,                   \
                     own.line + kLineHits,                                                                                      \
                     too_long, own.mine)
    FMX_LAYOUT_DISPATCH(h, FMX_FO_CALL);
#undef FMX_FO_CALL
    HIP_TRY(hipGetLastError(), "k_fold");
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
    if (flag) return arg_fail("search_fold: a pattern is longer than 255 bytes");
  }
  if (info->total > cap) return FMX_OK;                      // the caller reports the overflow; nothing is ordered
  const uint64_t rows = info->total;
  if ((rc = fold_order(mem, stage, rows, groups, tb, d_out_off, d_out, st))) return rc;
  if (rows) HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the temporaries go when this returns
  if (rows) info->sort_ms = ev.ms(1, 2);
  return FMX_OK;
}

int fold_order(DevMem &mem, unsigned long long *stage, uint64_t rows, uint64_t groups, int tb, void *d_out_off, void *d_out,
               hipStream_t st) {
  unsigned long long *out_off = static_cast<unsigned long long *>(d_out_off);
  if (rows == 0) {
    HIP_TRY(launch_csr_off(nullptr, 0, groups, kFoRowBits + tb, out_off, st), "k_fold_off");
    return FMX_OK;
  }
  SortSpace ws;
  if (const int rc = ws.alloc(mem, rows, "fold sort")) return rc;
  LAUNCH("k_fold_keys", k_fold_keys, dim3(flat_grid(rows)), dim3(256), st, stage, rows, tb, ws.keys(), ws.vals());
  HIP_TRY(ws.sort(rows, kFoRowBits + tb + std::min(26 - tb, bits_for(groups - 1)), st), "radix sort");      // group ids 0 .. groups - 1
  HIP_TRY(launch_gather3(stage, ws.vals(), rows, static_cast<unsigned long long *>(d_out), st), "k_fold_gather");
  HIP_TRY(launch_csr_off(ws.keys(), rows, groups, kFoRowBits + tb, out_off, st), "k_fold_off");
  return FMX_OK;
}

static thread_local FoldInfo g_fold_last;
void fold_set_last(const FoldInfo &info) { g_fold_last = info; }

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static_assert(sizeof(fmx_fold_opts) == 264 && sizeof(fmx_result) == 24, "fmx.h");

// What refuses a call before the device is touched; the map as the kernel takes it.
static int fold_args(const fmx_index *idx, size_t k, const fmx_fold_opts *opts, const void *out_off, const void *out, size_t cap,
                     const size_t *n_out, uint8_t map[256]) {
  if (!n_out) return arg_fail("search_fold: n_out is null");
  int rc = fold_map_check(opts, map);
  if (rc) return rc;
  if ((uint64_t)k > (1ull << 26)) return arg_fail("search_fold: at most 2^26 patterns per call");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("search_fold: cap must be below 2^32");
  if (!out_off || (cap && !out)) return arg_fail("null argument");
  if (!idx) return arg_fail("search_fold: the handle is null");
  return fold_handle_check(H(idx));
}

extern "C" {

int fmx_search_fold_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, size_t k, const fmx_fold_opts *opts,
                              void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  uint8_t map[256];
  int rc = fold_args(idx, k, opts, d_out_off, d_out, cap, n_out, map);
  if (rc) return rc;
  if (k && !d_off) return arg_fail("null argument");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  if ((rc = not_capturing((hipStream_t)stream, "a fold search"))) return rc;
  rc = fold_search(h, d_pat, d_off, k, map, nullptr, 1, FMX_FOLD_MAX_LEN, d_out_off, d_out, cap, true, (hipStream_t)stream, &g_fold_last);
  if (rc) return rc;
  *n_out = (size_t)g_fold_last.total;
  return g_fold_last.total > cap ? csr_overflow("search_fold", g_fold_last.total, cap) : FMX_OK;
}

int fmx_search_fold_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, size_t k, const fmx_fold_opts *opts,
                          uint64_t *out_off, fmx_result *out, size_t cap, size_t *n_out) {
  uint8_t map[256];
  if (k && (uint64_t)k <= (1ull << 26) && off && !offsets_monotonic(off, 0, k)) return arg_fail("pattern offsets must be non-decreasing");
  uint64_t longest = 0;                                      // the stacks are sized by it
  if (off && (uint64_t)k <= (1ull << 26))
    for (size_t i = 0; i < k; i++) {
      if (off[i + 1] - off[i] > FMX_FOLD_MAX_LEN) return arg_fail("search_fold: a pattern is longer than 255 bytes");
      longest = std::max<uint64_t>(longest, off[i + 1] - off[i]);
    }
  int rc = fold_args(idx, k, opts, out_off, out, cap, n_out, map);
  if (rc) return rc;
  if (k && !off) return arg_fail("null argument");
  const uint64_t lo_off = k ? off[0] : 0, total_bytes = k ? off[k] - lo_off : 0;
  if (total_bytes && !pat) return arg_fail("pat is null");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  void *d_pat = nullptr;
  uint64_t *d_off = nullptr, *d_out_off = nullptr;
  fmx_result *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("fold patterns", total_bytes ? pat + lo_off : nullptr, total_bytes, "fold offsets", off, k, true, &d_pat, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out_off, 8 * (k + 1), "fold offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_result) * cap, "fold hits");
  rc = fold_search(h, d_pat, d_off, k, map, nullptr, 1, (uint32_t)longest, d_out_off, d_out, cap, false, hc.own.s, &g_fold_last);
  if (rc) return rc;
  const uint64_t total = g_fold_last.total;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("search_fold", total, cap);
  return hc.download_csr(out_off, d_out_off, k, out, d_out, total, sizeof(fmx_result));
}

int fmx_fold_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests) {
  if (search_ms) *search_ms = g_fold_last.search_ms;
  if (sort_ms) *sort_ms = g_fold_last.sort_ms;
  if (steps) *steps = g_fold_last.steps;
  if (requests) *requests = g_fold_last.requests;
  return FMX_OK;
}

}  // extern "C"
