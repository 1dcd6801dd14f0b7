// fmx_occ.hip -- occurrences: (group, len, sp, ep) intervals -> the text occurrences they stand for, reduced and in CSR order
// (fmx.h: fmx_occurrences).  The records are what a regex batch leaves in HBM (fmx_regex_batch_match_dev) or a
// repack of edit, mismatch and exact hits.  All stages run on the device:
//
//   unpack  : k_occ_unpack   records -> sp[], ep[] (ep > n read as n; a bad or empty record gets no rows, a bad one raises a flag)
//   locate  : launch_locate_intervals (fmx_locate.hip): the scan of min(ep - sp, max_per), the expansion, the LF walks
//   keys    : k_occ_keys     row j finds its record by a search in the offsets, forms pos = n - 1 - len - SA, applies the corpus
//                            rule and writes a sort key over (group, pos, len); a dropped row sorts behind everything
//   sort    : SortSpace (fmx_order.h) over the bits the call needs; when group, pos and len do not fit 64 bits, two stable
//             sorts: (pos, len) first, then the group gathered through the permutation (k_occ_regroup)
//   select  : k_occ_spread   the sorted keys as G[] (group) and PL[] (pos << 16 | len)
//             k_occ_heads    ALL: the first of each equal (group, pos, len); LONGEST: the last of each (group, pos) run
//             DISJOINT       the LONGEST set compacted (k_occ_pick), next[] by a lower bound of (group, pos + len)
//                            (k_occ_next), then ceil(log2(rows + 1)) rounds of mark[jump[i]] = 1 for marked i, jump = jump o jump
//                            (k_occ_round): plain stores of the value 1, jump double-buffered
//   compact : a scan (fmx_order.h) over the flags, k_occ_emit (32-byte records, the corpus map's raw offsets), k_occ_off (a lower bound
//             per group)
// No atomics anywhere: the same input gives the same bytes on every run.  Positions are u32 in the keys (n < 2^32).
#include <fmx.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fmx_corpus_dev.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kOccThreads = 256;
constexpr uint32_t kOccNone = 0xffffffffu;           // no next element in the group
constexpr int kOccLenBits = 16;                      // PL = pos << 16 | len; FMX_OCC_MAX_LEN fits
constexpr uint64_t kOccMaxK = 1ull << 26;            // records and groups per call
static_assert(FMX_OCC_MAX_LEN < (1 << kOccLenBits), "len must fit the key");
static_assert(sizeof(fmx_occurrence) == 32 && sizeof(fmx_result) == 24, "record sizes are ABI");

__global__ __launch_bounds__(kOccThreads) void k_occ_unpack(const fmx_result *__restrict__ rec, uint64_t k, uint64_t n,
                                                            uint64_t n_groups, unsigned long long *__restrict__ sp,
                                                            unsigned long long *__restrict__ ep, uint32_t *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
    const fmx_result r = rec[i];
    uint64_t a = r.sp, b = r.ep < n ? r.ep : n;
    if (r.regex >= n_groups || r.len > FMX_OCC_MAX_LEN || r.sp > r.ep) {
      *bad = 1u;
      a = b = 0;
    } else if (r.len == 0 || a >= b) {
      a = b = 0;
    }
    sp[i] = a;
    ep[i] = b;
  }
}

struct OccKeyForm {
  int wide;                  // 1: key = pos << 16 | len and the group goes to grp[]; 0: key = group << (pb + lb) | pos << lb | len
  int pb, lb;
};

// sa[j] = SA of the j-th located row, off[] the rows before each record.  A dropped row: group n_groups, pos 0, len 0.
__global__ __launch_bounds__(kOccThreads) void k_occ_keys(const unsigned long long *__restrict__ sa, uint64_t rows,
                                                          const unsigned long long *__restrict__ off, uint64_t k,
                                                          const fmx_result *__restrict__ rec, uint64_t n, uint64_t n_groups,
                                                          int has_map, CoMap m, OccKeyForm f,
                                                          unsigned long long *__restrict__ key, uint32_t *__restrict__ val,
                                                          uint32_t *__restrict__ grp) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const uint64_t i = upper_bound(off, 0, k + 1, j) - 1;
    const uint64_t s = sa[j], len = rec[i].len;
    uint64_t g = n_groups, pos = 0, ln = 0;
    if (s < n && s + len <= n - 1) {
      const uint64_t p = n - 1 - len - s;
      bool keep = true;
      if (has_map) {
        uint32_t d;
        uint64_t eo, ro;
        keep = co_map(m, p, d, eo, ro) && p + len + 1 <= (uint64_t)m.doc_start[d + 1];
      }
      if (keep) {
        g = rec[i].regex;
        pos = p;
        ln = len;
      }
    }
    if (f.wide) {
      key[j] = (pos << kOccLenBits) | ln;
      grp[j] = (uint32_t)g;
    } else {
      key[j] = (g << (f.pb + f.lb)) | (pos << f.lb) | ln;
    }
    val[j] = (uint32_t)j;
  }
}

// the wide form between its two sorts: (pos, len) sorted in key[] with the permutation in val[] -> pl[] keeps them, the
// second sort's key is the group of the row each came from and its value the place in pl[]
__global__ __launch_bounds__(kOccThreads) void k_occ_regroup(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ val,
                                                             const uint32_t *__restrict__ grp, uint64_t rows,
                                                             unsigned long long *__restrict__ pl, unsigned long long *__restrict__ key2,
                                                             uint32_t *__restrict__ val2) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += stride) {
    pl[t] = key[t];
    key2[t] = grp[val[t]];
    val2[t] = (uint32_t)t;
  }
}

// the sorted keys as G[] and PL[].  wide: key = the group, val = the place in pl_in[]
__global__ __launch_bounds__(kOccThreads) void k_occ_spread(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ val,
                                                            const unsigned long long *__restrict__ pl_in, uint64_t rows, OccKeyForm f,
                                                            uint32_t *__restrict__ G, unsigned long long *__restrict__ PL) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += stride) {
    const unsigned long long kk = key[t];
    if (f.wide) {
      G[t] = (uint32_t)kk;
      PL[t] = pl_in[val[t]];
    } else {
      const uint64_t ln = kk & ((1ull << f.lb) - 1), pos = (kk >> f.lb) & ((1ull << f.pb) - 1);
      G[t] = (uint32_t)(kk >> (f.pb + f.lb));
      PL[t] = (pos << kOccLenBits) | ln;
    }
  }
}

// longest == 0: the first of each equal (group, pos, len); else the last of each (group, pos) run (len ascends inside a run)
__global__ __launch_bounds__(kOccThreads) void k_occ_heads(const uint32_t *__restrict__ G, const unsigned long long *__restrict__ PL,
                                                           uint64_t rows, uint32_t n_groups, int longest, uint32_t *__restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += stride) {
    const uint32_t g = G[t];
    uint32_t fl = 0;
    if (g < n_groups) {
      if (longest) fl = t + 1 == rows || G[t + 1] != g || (PL[t + 1] >> kOccLenBits) != (PL[t] >> kOccLenBits) ? 1u : 0u;
      else fl = t == 0 || G[t - 1] != g || PL[t - 1] != PL[t] ? 1u : 0u;
    }
    flag[t] = fl;
  }
}

// the flagged elements side by side: incl = the inclusive sum of the flags
__global__ __launch_bounds__(kOccThreads) void k_occ_pick(const uint32_t *__restrict__ G, const unsigned long long *__restrict__ PL,
                                                          const uint32_t *__restrict__ incl, uint64_t rows, uint32_t *__restrict__ cG,
                                                          unsigned long long *__restrict__ cPL) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += stride) {
    const uint32_t c = incl[t];
    if (c == (t ? incl[t - 1] : 0u)) continue;
    cG[c - 1] = G[t];
    cPL[c - 1] = PL[t];
  }
}

// jump[i] = the first element of i's group that begins at or behind i's end (kOccNone: none); mark = each group's first
__global__ __launch_bounds__(kOccThreads) void k_occ_next(const uint32_t *__restrict__ cG, const unsigned long long *__restrict__ cPL,
                                                          const uint32_t *__restrict__ m_dev, uint32_t *__restrict__ jump,
                                                          uint32_t *__restrict__ mark) {
  const uint64_t m = *m_dev, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const uint32_t g = cG[i];
    const uint64_t pl = cPL[i], end = (pl >> kOccLenBits) + (pl & ((1ull << kOccLenBits) - 1));
    uint64_t lo = i + 1, hi = m;                     // len >= 1: the next one lies behind i
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      const uint32_t gm = cG[mid];
      if (gm < g || (gm == g && (cPL[mid] >> kOccLenBits) < end)) lo = mid + 1;
      else hi = mid;
    }
    jump[i] = lo < m && cG[lo] == g ? (uint32_t)lo : kOccNone;
    mark[i] = i == 0 || cG[i - 1] != g ? 1u : 0u;
  }
}

// One doubling round.  A mark is only ever set on an element of its group's chain (a marked element's jump is one), so a
// mark seen early does no harm; jump is read from one buffer and written to the other, which keeps the distances exact.
__global__ __launch_bounds__(kOccThreads) void k_occ_round(const uint32_t *__restrict__ m_dev, const uint32_t *__restrict__ jump,
                                                           uint32_t *__restrict__ jump_out, uint32_t *mark) {
  const uint64_t m = *m_dev, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const uint32_t j = jump[i];
    if (j == kOccNone || j >= m) {
      jump_out[i] = kOccNone;
      continue;
    }
    if (mark[i]) mark[j] = 1u;
    jump_out[i] = jump[j];
  }
}

// the marks as flags over all `rows` slots (the slots behind the m elements: 0), ready for the scan
__global__ __launch_bounds__(kOccThreads) void k_occ_marks(const uint32_t *__restrict__ m_dev, const uint32_t *__restrict__ mark,
                                                           uint64_t rows, uint32_t *__restrict__ flag) {
  const uint64_t m = *m_dev, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) flag[i] = i < m ? mark[i] : 0u;
}

// len_dev != null: the arrays hold *len_dev elements (the compacted set).  incl = the inclusive sum of the flags.
__global__ __launch_bounds__(kOccThreads) void k_occ_emit(const uint32_t *__restrict__ G, const unsigned long long *__restrict__ PL,
                                                          const uint32_t *__restrict__ incl, uint64_t len,
                                                          const uint32_t *__restrict__ len_dev, int has_map, CoMap m, uint64_t cap,
                                                          fmx_occurrence *__restrict__ out) {
  if (len_dev) len = *len_dev;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < len; t += stride) {
    const uint32_t c = incl[t];
    if (c == (t ? incl[t - 1] : 0u)) continue;
    const uint64_t slot = (uint64_t)c - 1;
    if (slot >= cap) continue;
    const uint64_t pl = PL[t], pos = pl >> kOccLenBits, ln = pl & ((1ull << kOccLenBits) - 1);
    fmx_occurrence o;
    o.group = G[t];
    o.len = (uint32_t)ln;
    o.pos = pos;
    o.doc = 0xffffffffu;
    o.raw_len = (uint32_t)ln;
    o.raw_off = pos;
    if (has_map) {
      uint32_t d = 0xffffffffu, d2;
      uint64_t eo, ro = ~0ull, ro2 = ~0ull;
      (void)co_map(m, pos, d, eo, ro);
      (void)co_map(m, pos + ln - 1, d2, eo, ro2);
      o.doc = d;
      o.raw_off = ro;
      o.raw_len = (uint32_t)(ro2 + 1 - ro);
    }
    out[slot] = o;
  }
}

// out_off[g] = the occurrences of the groups before g, g = 0 .. n_groups
__global__ __launch_bounds__(kOccThreads) void k_occ_off(const uint32_t *__restrict__ G, const uint32_t *__restrict__ incl, uint64_t len,
                                                         const uint32_t *__restrict__ len_dev, uint64_t n_groups,
                                                         unsigned long long *__restrict__ out_off) {
  if (len_dev) len = *len_dev;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= n_groups; g += stride) {
    const uint64_t j = len ? lower_bound(G, 0, len, g) : 0;
    out_off[g] = j ? incl[j - 1] : 0u;
  }
}

namespace {

struct OccInfo {
  double phase_ms[4] = {0, 0, 0, 0};                 // locate, sort, select, compact
  uint64_t rows = 0;
};
thread_local OccInfo g_occ_last;

// Device bytes of a call beside the sort's workspace: per row the SA values (8), the flags (4), and with DISJOINT the
// compacted set, two jump buffers and the marks (24); the group array of the two-sort form (4); per record the two interval
// ends and the offset (24).
uint64_t occ_row_bytes(uint32_t mode, bool wide) { return 12 + (mode == FMX_OCC_DISJOINT ? 24 : 0) + (wide ? 4 : 0); }

// What the arguments alone decide (both forms), before a handle is looked at.
int occ_args(const void *rec, size_t k, size_t n_groups, const fmx_occ_opts *opts, const void *out_off, const void *out, size_t cap,
             const size_t *n_out) {
  if (!out_off || !n_out) return arg_fail("occurrences: out_off or n_out is null");
  if (opts) {
    if (opts->mode > FMX_OCC_DISJOINT) return arg_fail("fmx_occ_opts.mode: FMX_OCC_ALL, FMX_OCC_LONGEST or FMX_OCC_DISJOINT");
    if (opts->reserved != 0) return arg_fail("fmx_occ_opts.reserved must be 0");
  }
  if ((uint64_t)k > kOccMaxK) return arg_fail("occurrences: at most 2^26 records per call");
  if (n_groups == 0 || (uint64_t)n_groups > kOccMaxK) return arg_fail("occurrences: n_groups must be 1 .. 2^26");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("occurrences: cap must be below 2^32");
  if (k && !rec) return arg_fail("occurrences: the records are null");
  if (cap && !out) return arg_fail("occurrences: out is null");
  return FMX_OK;
}

// The handles, last: a null one, those locate refuses, n >= 2^32, a corpus that is not this index's.
int occ_handles(const fmx_index *idx, const fmx_corpus *corpus) {
  if (!idx) return arg_fail("occurrences: the handle is null");
  const Index *h = H(idx);
  int rc = locate_check(h);
  if (rc) return rc;
  if (h->n >= (1ull << 32)) {
    set_error("occurrences: indexes of 2^32 rows and more are not supported (positions are 32 bits in the sort key)");
    return FMX_ERR_UNSUPPORTED;
  }
  if (corpus) {
    const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
    if (h->n != c->stream_len + 1) return arg_fail("occurrences: the index is not the index of this corpus (n != stream length + 1)");
    if (h->device != c->device) return arg_fail("occurrences: the index and the corpus live on different devices");
  }
  return FMX_OK;
}

// The whole call on `st`: d_rec, d_out_off and d_out in device memory.  len_bits: the bits a record's len may take.
// Allocates, synchronises `st`, frees its temporaries on every path; *total = the occurrences found.
int occ_run(const Index *h, const Corpus *c, const fmx_result *d_rec, uint64_t k, uint64_t n_groups, uint32_t mode, uint64_t max_per,
            int len_bits, unsigned long long *d_out_off, fmx_occurrence *d_out, uint64_t cap, hipStream_t st, uint64_t *total) {
  g_occ_last = OccInfo{};
  const uint64_t n = h->n;
  int rc = device_room(24 * k + 4096, "fmx_occurrences");
  if (rc) return rc;
  if ((rc = ensure_built(h, h->loc, locate_prepare, st))) return rc;
  const CoMap map = c ? c->map() : CoMap{nullptr, nullptr, nullptr, 0, 0, 0};
  const int has_map = c ? 1 : 0;
  Events<5> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  unsigned long long *sp = nullptr, *ep = nullptr, *off = nullptr;
  uint32_t *bad = nullptr;
  DEV_ALLOC(mem, sp, 8 * k, "occurrences");
  DEV_ALLOC(mem, ep, 8 * k, "occurrences");
  DEV_ALLOC(mem, off, 8 * (k + 1), "occurrences");
  DEV_ALLOC(mem, bad, 16, "occurrences");
  uint64_t launches = 0;
  HIP_TRY(hipMemsetAsync(bad, 0, 16, st), "hipMemsetAsync");
  if (k) {
    LAUNCH("k_occ_unpack", k_occ_unpack, dim3(flat_grid(k)), dim3(kOccThreads), st, d_rec, k, n, n_groups, sp, ep, bad);
    launches++;
  }
  // the row counts first (no positions: cap 0), then room for exactly that many
  HIP_TRY(launch_locate_intervals(h, sp, ep, k, max_per, off, nullptr, 0, st), "k_loc_scan");
  launches++;
  unsigned long long rows = 0;
  uint32_t bad_h = 0;
  HIP_TRY(hipMemcpyAsync(&rows, off + k, 8, hipMemcpyDeviceToHost, st), "D2H(rows)");
  HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st), "D2H(flag)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  auto done = [&]() {
    std::lock_guard<std::mutex> lk(h->mu);
    h->launches += launches;
  };
  if (bad_h) {
    done();
    return arg_fail("occurrences: a record with group >= n_groups, len > FMX_OCC_MAX_LEN or sp > ep");
  }
  g_occ_last.rows = rows;
  if (rows >= (1ull << 32)) {
    done();
    set_error("occurrences: " + std::to_string(rows) + " rows to locate, at most 2^32 - 1 per call: lower max_per");
    return FMX_ERR_OVERFLOW;
  }
  if (rows == 0) {
    LAUNCH("k_occ_off", k_occ_off, dim3(flat_grid(n_groups + 1)), dim3(kOccThreads), st, nullptr, nullptr, 0ull, nullptr, n_groups,
           d_out_off);
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    launches++;
    done();
    *total = 0;
    return FMX_OK;
  }
  OccKeyForm f;
  f.pb = bits_for(n);
  f.lb = len_bits;
  const int gb = bits_for(n_groups);                 // groups 0 .. n_groups (n_groups: a dropped row)
  f.wide = f.pb + f.lb + gb > 64 ? 1 : 0;
  if ((rc = device_room(occ_row_bytes(mode, f.wide) * rows + SortSpace::bytes(rows) + 8192, "fmx_occurrences"))) {
    done();
    return rc;
  }
  unsigned long long *pos = nullptr, *cPL = nullptr;
  uint32_t *flag = nullptr, *grp = nullptr, *cG = nullptr, *ja = nullptr, *jb = nullptr, *mark = nullptr;
  SortSpace ws;
  DEV_ALLOC(mem, pos, 8 * rows, "occurrences");
  if ((rc = ws.alloc(mem, rows, "occurrences"))) return rc;
  DEV_ALLOC(mem, flag, 4 * rows, "occurrences");
  if (f.wide) DEV_ALLOC(mem, grp, 4 * rows, "occurrences");
  if (mode == FMX_OCC_DISJOINT) {
    DEV_ALLOC(mem, cPL, 8 * rows, "occurrences");
    DEV_ALLOC(mem, cG, 4 * rows, "occurrences");
    DEV_ALLOC(mem, ja, 4 * rows, "occurrences");
    DEV_ALLOC(mem, jb, 4 * rows, "occurrences");
    DEV_ALLOC(mem, mark, 4 * rows, "occurrences");
  }
  const dim3 grid(flat_grid(rows)), block(kOccThreads);
  // ---- locate
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  HIP_TRY(launch_locate_intervals(h, sp, ep, k, max_per, off, pos, rows, st), "k_locate");
  launches += 3;
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  // ---- keys and sort
  LAUNCH("k_occ_keys", k_occ_keys, grid, block, st, pos, (uint64_t)rows, off, k, d_rec, n, n_groups, has_map, map, f, ws.keys(), ws.vals(),
         grp);
  launches++;
  const unsigned long long *pl_in = nullptr;
  if (f.wide) {
    HIP_TRY(ws.sort(rows, f.pb + kOccLenBits, st), "radix sort");
    launches += 3 * (uint64_t)ws.passes;
    LAUNCH("k_occ_regroup", k_occ_regroup, grid, block, st, ws.keys(), ws.vals(), grp, (uint64_t)rows, pos, ws.free_keys(), ws.free_vals());
    launches++;
    ws.swap();
    HIP_TRY(ws.sort(rows, gb, st), "radix sort");
    launches += 3 * (uint64_t)ws.passes;
    pl_in = pos;
  } else {
    HIP_TRY(ws.sort(rows, f.pb + f.lb + gb, st), "radix sort");
    launches += 3 * (uint64_t)ws.passes;
  }
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  // ---- select: G in the free value buffer; PL in the free key buffer
  uint32_t *G = ws.free_vals();
  unsigned long long *PL = ws.free_keys();
  LAUNCH("k_occ_spread", k_occ_spread, grid, block, st, ws.keys(), ws.vals(), pl_in, (uint64_t)rows, f, G, PL);
  LAUNCH("k_occ_heads", k_occ_heads, grid, block, st, G, PL, (uint64_t)rows, (uint32_t)n_groups, mode == FMX_OCC_ALL ? 0 : 1, flag);
  launches += 2;
  const uint32_t *len_dev = nullptr;
  if (mode == FMX_OCC_DISJOINT) {
    HIP_TRY(ws.scan().sum(flag, rows, false, st), "scan");
    LAUNCH("k_occ_pick", k_occ_pick, grid, block, st, G, PL, flag, (uint64_t)rows, cG, cPL);
    uint32_t *m_dev = reinterpret_cast<uint32_t *>(bad) + 1;         // the size of the compacted set stays on the device
    HIP_TRY(hipMemcpyAsync(m_dev, flag + (rows - 1), 4, hipMemcpyDeviceToDevice, st), "D2D");
    LAUNCH("k_occ_next", k_occ_next, grid, block, st, cG, cPL, m_dev, ja, mark);
    int rounds = 1;
    while ((1ull << rounds) < rows + 1) rounds++;
    for (int r = 0; r < rounds; r++) {
      hipLaunchKernelGGL(k_occ_round, grid, block, 0, st, m_dev, ja, jb, mark);
      std::swap(ja, jb);
    }
    HIP_TRY(hipGetLastError(), "k_occ_round");
    LAUNCH("k_occ_marks", k_occ_marks, grid, block, st, m_dev, mark, (uint64_t)rows, flag);
    launches += 6 + (uint64_t)rounds;
    G = cG;
    PL = cPL;
    len_dev = m_dev;
  }
  HIP_TRY(ev.record(3, st), "hipEventRecord");
  // ---- compact
  HIP_TRY(ws.scan().sum(flag, rows, false, st), "scan");
  LAUNCH("k_occ_off", k_occ_off, dim3(flat_grid(n_groups + 1)), block, st, G, flag, (uint64_t)rows, len_dev, n_groups, d_out_off);
  if (cap) {
    LAUNCH("k_occ_emit", k_occ_emit, grid, block, st, G, PL, flag, (uint64_t)rows, len_dev, has_map, map, cap, d_out);
  }
  launches += 4;
  HIP_TRY(ev.record(4, st), "hipEventRecord");
  unsigned long long tot = 0;
  HIP_TRY(hipMemcpyAsync(&tot, d_out_off + n_groups, 8, hipMemcpyDeviceToHost, st), "D2H(total)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
  for (int i = 0; i < 4; i++) g_occ_last.phase_ms[i] = ev.ms(i, i + 1);
  done();
  *total = tot;
  return FMX_OK;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_occurrences_dev(const fmx_index *idx, const fmx_corpus *corpus, const void *d_rec, size_t k, size_t n_groups,
                        const fmx_occ_opts *opts, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  int rc = occ_args(d_rec, k, n_groups, opts, d_out_off, d_out, cap, n_out);
  if (rc || (rc = occ_handles(idx, corpus))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_occurrences_dev"))) return rc;
  uint64_t total = 0;
  if ((rc = occ_run(h, reinterpret_cast<const Corpus *>(corpus), static_cast<const fmx_result *>(d_rec), k, n_groups,
                    opts ? opts->mode : FMX_OCC_ALL, opts ? opts->max_per : 0, kOccLenBits, static_cast<unsigned long long *>(d_out_off),
                    static_cast<fmx_occurrence *>(d_out), cap, st, &total)))
    return rc;
  *n_out = (size_t)total;
  return total > cap ? csr_overflow("occurrences", total, cap) : FMX_OK;
}

int fmx_occurrences(const fmx_index *idx, const fmx_corpus *corpus, const fmx_result *rec, size_t k, size_t n_groups,
                    const fmx_occ_opts *opts, uint64_t *out_off, fmx_occurrence *out, size_t cap, size_t *n_out) {
  int rc = occ_args(rec, k, n_groups, opts, out_off, out, cap, n_out);
  if (rc) return rc;
  uint32_t max_len = 0;
  for (size_t i = 0; i < k; i++) {
    if (rec[i].regex >= n_groups) return arg_fail("occurrences: a record's group is not below n_groups");
    if (rec[i].len > FMX_OCC_MAX_LEN) return arg_fail("occurrences: a record's len is above FMX_OCC_MAX_LEN (65535)");
    if (rec[i].sp > rec[i].ep) return arg_fail("occurrences: a record with sp > ep");
    max_len = std::max(max_len, rec[i].len);
  }
  if ((rc = occ_handles(idx, corpus))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  if ((rc = hc.open())) return rc;
  if ((rc = device_room(24 * (uint64_t)k + 8 * ((uint64_t)n_groups + 1) + 32 * (uint64_t)cap + 4096, "fmx_occurrences"))) return rc;
  fmx_result *d_rec = nullptr;
  unsigned long long *d_off = nullptr;
  fmx_occurrence *d_out = nullptr;
  DEV_ALLOC(hc.mem, d_rec, sizeof(fmx_result) * (uint64_t)k, "occurrence records");
  DEV_ALLOC(hc.mem, d_off, 8 * ((uint64_t)n_groups + 1), "occurrence offsets");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_occurrence) * (uint64_t)cap, "occurrences");
  if (k) HIP_TRY(hipMemcpyAsync(d_rec, rec, sizeof(fmx_result) * (uint64_t)k, hipMemcpyHostToDevice, hc.own.s), "H2D(records)");
  uint64_t total = 0;
  if ((rc = occ_run(h, reinterpret_cast<const Corpus *>(corpus), d_rec, k, n_groups, opts ? opts->mode : FMX_OCC_ALL,
                    opts ? opts->max_per : 0, bits_for(max_len), d_off, d_out, cap, hc.own.s, &total)))
    return rc;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("occurrences", total, cap);
  return hc.download_csr(out_off, d_off, n_groups, out, d_out, total, sizeof(fmx_occurrence));
}

int fmx_occurrences_last(double *locate_ms, double *sort_ms, double *select_ms, double *compact_ms, uint64_t *rows) {
  if (locate_ms) *locate_ms = g_occ_last.phase_ms[0];
  if (sort_ms) *sort_ms = g_occ_last.phase_ms[1];
  if (select_ms) *select_ms = g_occ_last.phase_ms[2];
  if (compact_ms) *compact_ms = g_occ_last.phase_ms[3];
  if (rows) *rows = g_occ_last.rows;
  return FMX_OK;
}

}  // extern "C"
