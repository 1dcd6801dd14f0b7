// fmx_classes.hip -- literal search under string classes: a pattern position stands for a set of byte strings of 1 .. 4 bytes
// (the contract is the comment block in fmx.h).
//
// A pattern is a sequence of elements, matched last first: a literal byte, or a class of the table.  The search is fmx_fold.hip's
// depth-first walk over wave-uniform nodes (elements left, sp, ep, bytes matched) with one new thing: a child is a short chain
// of dependent steps, a member's bytes from its last to its first, not one step.
//   literal, or a class of one member : the bytes as plain steps of the exact search, made by every lane group alike;
//   branching                         : lane group g takes member g and makes its steps, stopping at the first empty interval.
//                                       A class has at most 16 members: one round of 16 quads on the one-hot layout, two rounds
//                                       of 8 octets on the bytes layout.  The wave goes on with the non-empty child of the
//                                       smallest member index over all rounds and pushes the others, at ballot-prefix
//                                       positions, as {sp, ep, elements left | bytes matched << 32};
//   one row                           : on a branching node of one row only the members whose last byte is BWT'[sp] (0 on the EOF
//                                       row, which no member ends with) are stepped -- several may share it; with none the node
//                                       dies without a step.
// When no element is left the wave reports the node with the bytes of its spelling in the record's len, and pops.  An element
// pushes at most (largest class of the table - 1) entries, so a wave's stack of that many entries per element of the longest
// pattern cannot overflow; the kernel clamps all the same.  The class records are read from device memory with uniform loads.
// Staging, the sort key and the ordering step are fmx_fold.hip's (fold_order).
#include <fmx.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fmx_approx.h"
#include "fmx_classes.h"
#include "fmx_device.h"
#include "fmx_fold.h"

namespace fmx {

constexpr int kClThreads = 256;                // four waves: four patterns per workgroup
constexpr int kClWaves = kClThreads / 64;
constexpr unsigned long long kClTooLong = 1, kClNoClass = 2;      // the flag word

struct ClEntry {
  uint64_t sp, ep, at;                         // at = elements left | bytes matched << 32
};
static_assert(sizeof(ClEntry) == 24, "a stack entry");

template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kClThreads) void k_classes(DevIndex ix, const uint16_t *__restrict__ el,
                                                        const uint64_t *__restrict__ off, uint64_t k, uint64_t per,
                                                        const ClassRec *__restrict__ tab, uint32_t n_classes,
                                                        ClEntry *__restrict__ stack, uint32_t slab, uint32_t max_len,
                                                        unsigned long long *__restrict__ stage, uint64_t cap,
                                                        unsigned long long *__restrict__ total,
                                                        unsigned long long *__restrict__ flags,
                                                        unsigned long long *__restrict__ counters) {
  __shared__ uint64_t s_cf[256];
  __shared__ uint16_t s_slot[256];
  for (int c = threadIdx.x; c < 256; c += kClThreads) {
    s_cf[c] = ix.cf[c];
    s_slot[c] = ix.slot[c];
  }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  constexpr uint32_t kGroups = 64 / G;                       // members stepped in one round
  const LaneConst lc = lane_const<G>();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, g = lane / G;
  const bool lead = lc.t == 0;
  ClEntry *st = stack + ((uint64_t)blockIdx.x * kClWaves + wv) * slab;
  const uint64_t nwaves = (uint64_t)gridDim.x * kClWaves;
  unsigned long long steps = 0, reqs = 0;                    // counted by the lane that leads the group (lane 0 for the wave's own steps)
  auto step = [&](uint32_t c, uint64_t &s, uint64_t &t, bool count) {
    const uint16_t sl = s_slot[c];
    const uint32_t r = t - s == 1 ? single_row_step<WIDE, LAYOUT>(ix, c, sl, s_cf[c], lc, s, t)
                                  : backward_step<WIDE, LAYOUT>(ix, c, sl, s_cf[c], lc, s, t);
    if (count) { steps++; reqs += r; }
  };
  for (uint64_t q = (uint64_t)blockIdx.x * kClWaves + wv; q < k; q += nwaves) {
    const uint64_t b = off[q], en = off[q + 1];
    if (en > b && en - b > max_len) {                        // the device form cannot know before: skipped, the call refused
      if (lane == 0) atomicOr(flags, kClTooLong);
      continue;
    }
    const uint16_t *E = el + b;
    // per > 1 (the whole-word expansion, fmx_context.hip): pattern q is a string of group q / per, and one with a left byte
    // behind it -- a LITERAL element, so no step needs to know -- carries the lead bit in its records
    const uint64_t grp = per > 1 ? q / per : q;
    const uint32_t lead_bit = (per > 1 && q % per) ? kFoldLeadBit : 0u;
    uint32_t i = en > b ? (uint32_t)(en - b) : 0u, len = 0, top = 0;
    uint64_t sp = 0, ep = ix.n;
    bool node = true;                                        // false: pop the next entry, or leave the pattern
    for (;;) {
      if (!node) {
        if (top == 0) break;
        top--;
        const ClEntry e = st[top];
        sp = e.sp;
        ep = e.ep;
        i = (uint32_t)e.at;
        len = (uint32_t)(e.at >> 32);
        node = true;
        continue;
      }
      if (i == 0) {                                          // the pattern is through: a hit
        ap_emit(lane == 0, grp, len | lead_bit, sp, ep, lane, stage, cap, total);
        node = false;
        continue;
      }
      const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)E[i - 1]);
      if (e < 256u) {                                        // a literal: the exact search's step
        step(e, sp, ep, lane == 0);
        i--;
        len++;
        node = sp < ep;
        continue;
      }
      if (e - 256u >= n_classes) {                           // (the host form has refused it): the pattern is left, the call refused
        if (lane == 0) atomicOr(flags, kClNoClass);
        break;
      }
      const ClassRec *cr = tab + (e - 256u);
      const uint32_t cnt = min(cr->count, (uint32_t)FMX_CLASS_MAX_MEMBERS);
      if (cnt <= 1) {                                        // one member: its bytes as plain steps
        const uint32_t w = cr->w[0], L = cr->len[0];
        for (uint32_t j = 0; j < L && sp < ep; j++) step((w >> (8u * j)) & 255u, sp, ep, lane == 0);
        i--;
        len += L;
        node = sp < ep;
        continue;
      }
      const bool one = ep - sp == 1;                         // the one-row rule: only a member that ends with the row's symbol
      const uint32_t bsym = (one && sp != ix.eof) ? (uint32_t)ix.bwt[sp] : 0u;
      bool have = false;
      uint64_t csp = 0, cep = 0;
      uint32_t clen = 0;
      for (uint32_t base = 0; base < cnt; base += kGroups) {
        const uint32_t mi = base + g;
        bool act = mi < cnt;
        const uint32_t w = cr->w[act ? mi : 0u], L = cr->len[act ? mi : 0u];
        if (one && (w & 255u) != bsym) act = false;
        uint64_t s = sp, t = ep;
        bool hit = false;
        if (act) {
          for (uint32_t j = 0; j < L; j++) {
            step((w >> (8u * j)) & 255u, s, t, lead);
            if (s >= t) break;
          }
          hit = s < t;
        }
        unsigned long long mm = __builtin_amdgcn_ballot_w64(hit && lead);
        if (!mm) continue;
        if (!have) {                                         // the lowest group of the first round that has one: the smallest member
          const int src = __ffsll((long long)mm) - 1;
          csp = __shfl(s, src, 64);
          cep = __shfl(t, src, 64);
          clen = len + __shfl(L, src, 64);
          have = true;
          mm &= ~(1ull << src);
        }
        const uint32_t nk = (uint32_t)__popcll(mm);
        if (nk) {
          if (hit && lead && ((mm >> lane) & 1ull)) {
            const uint32_t at = top + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
            if (at < slab) st[at] = ClEntry{s, t, (uint64_t)(i - 1u) | ((uint64_t)(len + L) << 32)};      // (never past the slab)
          }
          top = min(top + nk, slab);
          ap_wave_sync();
        }
      }
      if (!have) {
        node = false;
        continue;
      }
      sp = csp;
      ep = cep;
      len = clen;
      i--;
    }
  }
  // the call's own counters: private slots, folded into the handle's afterwards (k_counters_fold: fmx_host.h, Metered)
  counters_add(counters, 2ull * steps, steps, reqs);
}

template <bool WIDE, uint32_t LAYOUT>
static hipError_t cl_grid(const Index *h, uint64_t k, uint32_t *grid) {
  return resident_grid<k_classes<WIDE, LAYOUT>>(h, kClThreads, k, kClWaves, grid);
}

int classes_table_check(const fmx_class_table *tab, std::vector<ClassRec> *packed, uint32_t *largest) {
  packed->clear();
  *largest = 1;
  if (!tab) return FMX_OK;
  if (tab->flags != 0 || tab->reserved != 0) return arg_fail("fmx_class_table.flags and .reserved must be 0");
  if (tab->n_classes > FMX_CLASS_MAX_CLASSES) return arg_fail("fmx_class_table: at most 65280 classes");
  if (tab->n_classes == 0) return FMX_OK;
  if (!tab->cls_off || !tab->mem_off || !tab->mem_bytes) return arg_fail("fmx_class_table: a null array");
  if (tab->cls_off[0] != 0 || tab->mem_off[0] != 0) return arg_fail("fmx_class_table: cls_off[0] and mem_off[0] must be 0");
  auto fail = [](uint64_t c, const char *what) {
    set_error("fmx_class_table: class " + std::to_string(c) + " " + what);
    return (int)FMX_ERR_ARG;
  };
  packed->resize(tab->n_classes);
  for (uint64_t c = 0; c < tab->n_classes; c++) {
    const uint64_t lo = tab->cls_off[c], hi = tab->cls_off[c + 1];
    if (hi <= lo) return fail(c, "has no member");
    if (hi - lo > FMX_CLASS_MAX_MEMBERS) return fail(c, "has more than 16 members");
    ClassRec &r = (*packed)[c];
    r = ClassRec{};
    r.count = (uint32_t)(hi - lo);
    *largest = std::max(*largest, r.count);
    for (uint64_t j = lo; j < hi; j++) {
      const uint64_t a = tab->mem_off[j], z = tab->mem_off[j + 1];
      if (z <= a) return fail(c, "has an empty member");
      if (z - a > FMX_CLASS_MAX_MEMBER_LEN) return fail(c, "has a member of more than 4 bytes");
      uint32_t w = 0;
      for (uint64_t x = a; x < z; x++) {
        if (tab->mem_bytes[x] == 0) return fail(c, "has a member with byte 0");
        w |= (uint32_t)tab->mem_bytes[x] << (8u * (uint32_t)(z - 1 - x));      // the last byte first
      }
      r.w[j - lo] = w;
      r.len[j - lo] = (uint8_t)(z - a);
      for (uint64_t p = lo; p < j; p++) {                    // distinct, and none a prefix of another
        const uint64_t pa = tab->mem_off[p], common = std::min(tab->mem_off[p + 1] - pa, z - a);
        if (std::equal(tab->mem_bytes + pa, tab->mem_bytes + pa + common, tab->mem_bytes + a))
          return fail(c, common == z - a && common == tab->mem_off[p + 1] - pa ? "has the same member twice" : "has a member that is a prefix of another");
      }
    }
  }
  return FMX_OK;
}

int classes_search(const Index *h, const void *d_el, const void *d_off, uint64_t k, uint64_t per, const std::vector<ClassRec> &packed,
                   uint32_t largest, uint32_t max_len, void *d_out_off, void *d_out, uint64_t cap, bool check_flags,
                   hipStream_t st, FoldInfo *info) {
  *info = FoldInfo{};
  const int tb = per > 1 ? 1 : 0;
  const uint64_t groups = per > 1 ? k / per : k;
  max_len = std::min<uint32_t>(std::max<uint32_t>(max_len, 1u), FMX_CLASS_MAX_ELEMS);
  const uint32_t slab = max_len * (std::min<uint32_t>(std::max<uint32_t>(largest, 1u), FMX_CLASS_MAX_MEMBERS) - 1u);
  uint32_t grid = 1;
  if (k) {
#define FMX_CL_GRID(W, L) HIP_TRY((cl_grid<W, L>(h, k, &grid)), "k_classes")
    FMX_LAYOUT_DISPATCH(h, FMX_CL_GRID);
#undef FMX_CL_GRID
  }
  const uint64_t stack_bytes = k ? (uint64_t)grid * kClWaves * slab * sizeof(ClEntry) : 0;
  const uint64_t tab_bytes = packed.size() * sizeof(ClassRec);
  int rc;
  // (the sort space of the ordering step, 24 bytes per hit, is allocated and checked by fold_order once the hits are counted)
  if ((rc = device_room(24 * cap + stack_bytes + tab_bytes + kMeteredBytes + 8, "the class search"))) return rc;
  Events<3> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *stage = nullptr, *flags = nullptr;
  ClEntry *stack = nullptr;
  ClassRec *d_tab = nullptr;
  Metered own;
  DEV_ALLOC(mem, stage, 24 * cap, "classes staging");
  DEV_ALLOC(mem, stack, stack_bytes, "classes stacks");
  DEV_ALLOC(mem, flags, 8, "classes flag");
  DEV_ALLOC(mem, d_tab, tab_bytes, "class table");
  if ((rc = own.alloc(mem, "classes")) || (rc = own.zero(st))) return rc;
  HIP_TRY(hipMemsetAsync(flags, 0, 8, st), "memset");
  if (tab_bytes) HIP_TRY(hipMemcpyAsync(d_tab, packed.data(), tab_bytes, hipMemcpyHostToDevice, st), "H2D(class table)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the table is the caller's vector
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (k) {
#define FMX_CL_CALL(W, L)                                                                                                       \
  hipLaunchKernelGGL((k_classes<W, L>), dim3(grid), dim3(kClThreads), 0, st, h->dev, static_cast<const uint16_t *>(d_el),       \
                     static_cast<const uint64_t *>(d_off), k, per, d_tab, (uint32_t)packed.size(), stack, slab, max_len, stage, cap, \
                     own.line + kLineHits, flags, own.mine)
    FMX_LAYOUT_DISPATCH(h, FMX_CL_CALL);
#undef FMX_CL_CALL
    HIP_TRY(hipGetLastError(), "k_classes");
    if ((rc = own.fold(h, 1, st))) return rc;                // counter [1]: the backward steps
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  MeterCounts cnt;
  if ((rc = own.finish(h, st, k ? 1 : 0, &cnt))) return rc;
  info->search_ms = ev.ms(0, 1);
  info->total = cnt.hits;
  info->steps = cnt.steps;
  info->requests = cnt.requests;
  if (check_flags && k) {
    unsigned long long flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, flags, 8, hipMemcpyDeviceToHost, st), "D2H");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (flag & kClTooLong) return arg_fail("search_classes: a pattern is longer than 255 elements");
    if (flag & kClNoClass) return arg_fail("search_classes: an element names a class that is not in the table");
  }
  if (info->total > cap) return FMX_OK;                      // the caller reports the overflow; nothing is ordered
  const uint64_t rows = info->total;
  if ((rc = fold_order(mem, stage, rows, groups, tb, d_out_off, d_out, st))) return rc;
  if (rows) HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");  // the temporaries go when this returns
  if (rows) info->sort_ms = ev.ms(1, 2);
  return FMX_OK;
}

static thread_local FoldInfo g_classes_last;
void classes_set_last(const FoldInfo &info) { g_classes_last = info; }

}  // namespace fmx

// ---------------------------------------------------------------- the C entry points (fmx.h)
using namespace fmx;

static_assert(sizeof(fmx_class_table) == 40, "fmx.h");

// What refuses a call before the device is touched, the handle apart; the table as the kernel takes it.
static int classes_args(size_t k, const fmx_class_table *tab, const void *out_off, const void *out, size_t cap, const size_t *n_out,
                        std::vector<ClassRec> *packed, uint32_t *largest) {
  if (!n_out) return arg_fail("search_classes: n_out is null");
  int rc = classes_table_check(tab, packed, largest);
  if (rc) return rc;
  if ((uint64_t)k > (1ull << 26)) return arg_fail("search_classes: at most 2^26 patterns per call");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("search_classes: cap must be below 2^32");
  if (!out_off || (cap && !out)) return arg_fail("null argument");
  return FMX_OK;
}

static int classes_handle(const fmx_index *idx) {
  if (!idx) return arg_fail("search_classes: the handle is null");
  return fold_handle_check(H(idx));
}

extern "C" {

int fmx_search_classes_batch_dev(const fmx_index *idx, const void *d_el, const void *d_el_off, size_t k, const fmx_class_table *tab,
                                 void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  std::vector<ClassRec> packed;
  uint32_t largest = 1;
  int rc = classes_args(k, tab, d_out_off, d_out, cap, n_out, &packed, &largest);
  if (rc || (rc = classes_handle(idx))) return rc;
  if (k && !d_el_off) return arg_fail("null argument");
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  if ((rc = not_capturing((hipStream_t)stream, "a class search"))) return rc;
  rc = classes_search(h, d_el, d_el_off, k, 1, packed, largest, FMX_CLASS_MAX_ELEMS, d_out_off, d_out, cap, true, (hipStream_t)stream,
                      &g_classes_last);
  if (rc) return rc;
  *n_out = (size_t)g_classes_last.total;
  return g_classes_last.total > cap ? csr_overflow("search_classes", g_classes_last.total, cap) : FMX_OK;
}

int fmx_search_classes_batch(const fmx_index *idx, const uint16_t *el, const uint64_t *el_off, size_t k, const fmx_class_table *tab,
                             uint64_t *out_off, fmx_result *out, size_t cap, size_t *n_out) {
  const bool sane = el_off && (uint64_t)k <= (1ull << 26);
  if (k && sane && !offsets_monotonic(el_off, 0, k)) return arg_fail("pattern offsets must be non-decreasing");
  uint64_t longest = 0;                                      // the stacks are sized by it
  if (sane)
    for (size_t i = 0; i < k; i++) {
      if (el_off[i + 1] - el_off[i] > FMX_CLASS_MAX_ELEMS) return arg_fail("search_classes: a pattern is longer than 255 elements");
      longest = std::max<uint64_t>(longest, el_off[i + 1] - el_off[i]);
    }
  std::vector<ClassRec> packed;
  uint32_t largest = 1;
  int rc = classes_args(k, tab, out_off, out, cap, n_out, &packed, &largest);
  if (rc) return rc;
  if (k && !el_off) return arg_fail("null argument");
  const uint64_t lo = k ? el_off[0] : 0, total = k ? el_off[k] - lo : 0;
  if (total && !el) return arg_fail("el is null");
  for (uint64_t j = 0; j < total; j++)
    if (el[lo + j] >= 256u && (uint64_t)(el[lo + j] - 256u) >= packed.size()) {
      set_error("search_classes: an element names class " + std::to_string(el[lo + j] - 256u) + ", the table has " +
                std::to_string(packed.size()));
      return FMX_ERR_ARG;
    }
  if ((rc = classes_handle(idx))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  void *d_el = nullptr;
  uint64_t *d_off = nullptr, *d_out_off = nullptr;
  fmx_result *d_out = nullptr;
  if ((rc = hc.open())) return rc;
  if ((rc = hc.upload("class patterns", total ? el + lo : nullptr, 2 * total, "class pattern offsets", el_off, k, true, &d_el, &d_off))) return rc;
  DEV_ALLOC(hc.mem, d_out_off, 8 * (k + 1), "classes offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_result) * cap, "classes hits");
  rc = classes_search(h, d_el, d_off, k, 1, packed, largest, (uint32_t)longest, d_out_off, d_out, cap, false, hc.own.s, &g_classes_last);
  if (rc) return rc;
  const uint64_t hits = g_classes_last.total;
  *n_out = (size_t)hits;
  if (hits > cap) return csr_overflow("search_classes", hits, cap);
  return hc.download_csr(out_off, d_out_off, k, out, d_out, hits, sizeof(fmx_result));
}

int fmx_classes_last(double *search_ms, double *sort_ms, uint64_t *steps, uint64_t *requests) {
  if (search_ms) *search_ms = g_classes_last.search_ms;
  if (sort_ms) *sort_ms = g_classes_last.sort_ms;
  if (steps) *steps = g_classes_last.steps;
  if (requests) *requests = g_classes_last.requests;
  return FMX_OK;
}

}  // extern "C"
