// fmx_lines.hip -- lines: the map from a text position to its line, and occurrence lists reduced to the distinct lines that
// hold them (fmx.h: fmx_lines_batch, fmx_occurrence_lines).  The table is derived from the index alone:
//
//   rows    : the buckets [cf(c), cf(c) + counts(c)) of the break bytes c -- the occurrences of the one-byte strings
//   locate  : launch_locate_intervals (fmx_locate.hip) for their SA values
//   keys    : k_lines_keys    pos = n - 2 - SA (a value outside the text raises a flag and sorts last)
//   sort    : SortSpace (fmx_order.h) over the bits n needs
//   table   : k_lines_pack    brk[j] as u32 (a repeated position raises the flag); k_lines_dir  dir[i] = the breaks before
//                             position i << S, a lower bound per directory entry
//   lookup  : k_lines_lookup  p -> dir[p >> S], dir[(p >> S) + 1], a lower bound among at most 2^S entries of brk
//             k_lines_spans   L -> brk[L - 1] + 1, brk[L]
//   reduce  : k_ol_lines      every record's group (a search in the CSR offsets) and line; a pos outside the text raises a flag
//             k_ol_heads      1 where (group, line) differs from the record before; a scan (fmx_order.h) over the flags
//             k_ol_pick       head t's record index side by side; k_ol_emit one fmx_line_hit per head, n_hits from the next
//                             head's index; k_ol_off  out_off[g] = the heads before the group's first record
// No atomics anywhere: the same input gives the same bytes on every run.  Positions are u32 in the table (n < 2^32).
#include <fmx.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "fmx_corpus_dev.h"
#include "fmx_order.h"
#include "fmx_lines_dev.h"

namespace fmx {

constexpr int kLinThreads = 256;
constexpr uint32_t kLinNone = 0xffffffffu;           // a record without a line
constexpr uint64_t kLinMaxK = 1ull << 26;            // occurrence records and groups per call
static_assert(sizeof(fmx_line_hit) == 48 && sizeof(fmx_occurrence) == 32, "record sizes are ABI");

__global__ __launch_bounds__(kLinThreads) void k_lines_keys(const unsigned long long *__restrict__ sa, uint64_t m, uint64_t n,
                                                            unsigned long long sentinel, unsigned long long *__restrict__ key,
                                                            uint32_t *__restrict__ val, uint32_t *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const uint64_t s = sa[j];
    unsigned long long p = sentinel;
    if (s + 2 <= n) p = n - 2 - s;
    else *bad = 1u;
    key[j] = p;
    val[j] = (uint32_t)j;
  }
}

__global__ __launch_bounds__(kLinThreads) void k_lines_pack(const unsigned long long *__restrict__ key, uint64_t m, uint64_t len,
                                                            uint32_t *__restrict__ brk, uint32_t *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const unsigned long long p = key[j];
    if (p >= len || (j && key[j - 1] >= p)) *bad = 1u;
    brk[j] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(kLinThreads) void k_lines_dir(const uint32_t *__restrict__ brk, uint64_t m, uint64_t entries,
                                                           uint32_t shift, uint32_t *__restrict__ dir) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < entries; i += stride)
    dir[i] = (uint32_t)lower_bound(brk, 0, m, i << shift);
}

__global__ __launch_bounds__(kLinThreads) void k_lines_lookup(LinesDev L, const unsigned long long *__restrict__ pos, uint64_t k,
                                                              unsigned long long *__restrict__ line,
                                                              unsigned long long *__restrict__ start,
                                                              unsigned long long *__restrict__ end) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < k; q += stride) {
    const uint64_t p = pos[q];
    unsigned long long l = ~0ull, s = ~0ull, e = ~0ull;
    if (p < L.len) {
      l = lin_line(L, p);
      s = lin_start(L, l);
      e = lin_end(L, l);
    }
    if (line) line[q] = l;
    if (start) start[q] = s;
    if (end) end[q] = e;
  }
}

__global__ __launch_bounds__(kLinThreads) void k_lines_spans(LinesDev L, const unsigned long long *__restrict__ line, uint64_t k,
                                                             unsigned long long *__restrict__ start,
                                                             unsigned long long *__restrict__ end) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < k; q += stride) {
    const uint64_t l = line[q];
    const bool ok = l <= L.n_brk;
    if (start) start[q] = ok ? lin_start(L, l) : ~0ull;
    if (end) end[q] = ok ? lin_end(L, l) : ~0ull;
  }
}

// record i's group, from the CSR offsets, and the line of its pos; a record outside every group or the text: no line, the flag
__global__ __launch_bounds__(kLinThreads) void k_ol_lines(LinesDev L, const unsigned long long *__restrict__ occ_off, uint64_t n_groups,
                                                          const fmx_occurrence *__restrict__ occ, uint64_t n_occ,
                                                          uint32_t *__restrict__ grp, uint32_t *__restrict__ line,
                                                          uint32_t *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += stride) {
    const uint64_t u = upper_bound(occ_off, 0, n_groups + 1, i), p = occ[i].pos;
    uint32_t g = kLinNone, l = kLinNone;
    if (u >= 1 && u <= n_groups && p < L.len) {
      g = (uint32_t)(u - 1);
      l = (uint32_t)lin_line(L, p);
    } else {
      *bad = 1u;
    }
    grp[i] = g;
    line[i] = l;
  }
}

__global__ __launch_bounds__(kLinThreads) void k_ol_heads(const uint32_t *__restrict__ grp, const uint32_t *__restrict__ line,
                                                          uint64_t n_occ, uint32_t *__restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += stride)
    flag[i] = grp[i] != kLinNone && (i == 0 || grp[i - 1] != grp[i] || line[i - 1] != line[i]) ? 1u : 0u;
}

// hidx[t] = the record index of head t: incl = the inclusive sum of the flags
__global__ __launch_bounds__(kLinThreads) void k_ol_pick(const uint32_t *__restrict__ incl, uint64_t n_occ, uint32_t *__restrict__ hidx) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += stride) {
    const uint32_t c = incl[i];
    if (c != (i ? incl[i - 1] : 0u)) hidx[c - 1] = (uint32_t)i;
  }
}

// one record per head; the heads number incl[n_occ - 1], the first min(that, cap) are written
__global__ __launch_bounds__(kLinThreads) void k_ol_emit(LinesDev L, const unsigned long long *__restrict__ occ_off,
                                                         const uint32_t *__restrict__ grp, const uint32_t *__restrict__ line,
                                                         const uint32_t *__restrict__ incl, const uint32_t *__restrict__ hidx,
                                                         uint64_t n_occ, int has_map, CoMap m, uint64_t cap,
                                                         fmx_line_hit *__restrict__ out) {
  const uint64_t total = incl[n_occ - 1], lim = total < cap ? total : cap;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < lim; t += stride) {
    const uint64_t i = hidx[t], next = t + 1 < total ? (uint64_t)hidx[t + 1] : n_occ;
    const uint32_t g = grp[i];
    fmx_line_hit o = lin_record(L, line[i], has_map, m);
    o.group = g;
    o.n_hits = (uint32_t)(next - i);
    o.first = (uint32_t)(i - occ_off[g]);
    out[t] = o;
  }
}

// out_off[g] = the heads among the records before group g's first, g = 0 .. n_groups
__global__ __launch_bounds__(kLinThreads) void k_ol_off(const unsigned long long *__restrict__ occ_off, uint64_t n_groups,
                                                        const uint32_t *__restrict__ incl, uint64_t n_occ,
                                                        unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= n_groups; g += stride) {
    uint64_t j = n_occ ? occ_off[g] : 0;
    j = j < n_occ ? j : n_occ;
    out_off[g] = j ? incl[j - 1] : 0u;
  }
}

namespace {

struct LinesInfo {
  double locate_ms = 0, sort_ms = 0, lookup_ms = 0, compact_ms = 0;
};
thread_local LinesInfo g_lines_last;

void add_launches(const Index *h, uint64_t launches) {
  std::lock_guard<std::mutex> lk(h->mu);
  h->launches += launches;
}

// What the arguments alone decide about a break set; the set comes back ascending.
int lines_set_args(const uint8_t *breaks, size_t n_breaks, uint8_t set[4], uint32_t *n_set) {
  if (!breaks || !n_breaks) {
    set[0] = 10;
    *n_set = 1;
    return FMX_OK;
  }
  if (n_breaks > 4) return arg_fail("lines: a break set holds at most 4 bytes");
  for (size_t i = 0; i < n_breaks; i++) {
    if (breaks[i] == 0) return arg_fail("lines: byte 0 cannot be a break (it is not in the text)");
    for (size_t j = 0; j < i; j++)
      if (breaks[j] == breaks[i]) return arg_fail("lines: a break byte is repeated");
    set[i] = breaks[i];
  }
  std::sort(set, set + n_breaks);
  *n_set = (uint32_t)n_breaks;
  return FMX_OK;
}

// The table for `set` into h->lin, in place of one for another set; the locate samples are built.
int lines_table(const Index *h, const uint8_t *set, uint32_t n_set, hipStream_t st, DevMem &mem) {
  int rc;
  const uint64_t n = h->n, len = n - 1;
  const uint32_t shift = (uint32_t)h->policy.lines_shift.load(std::memory_order_relaxed);
  unsigned long long sp[4] = {0, 0, 0, 0}, ep[4] = {0, 0, 0, 0};
  uint64_t m = 0;
  for (uint32_t i = 0; i < n_set; i++) {
    sp[i] = h->cf[set[i]];
    ep[i] = sp[i] + (uint64_t)h->counts[set[i]];
    m += ep[i] - sp[i];
  }
  if (m > len) {
    set_error("lines: the break bytes' counts exceed the text -- not the BWT of one text");
    return FMX_ERR_FORMAT;
  }
  const uint64_t entries = (len >> shift) + 2, keep = 4 * std::max<uint64_t>(m, 1) + 4 * entries;
  // the table itself; where there are breaks, their SA values and the sort's workspace
  if ((rc = device_room(keep + (m ? 8 * m + SortSpace::bytes(m) : 0) + 8192, "the line table"))) return rc;
  Events<4> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  uint32_t *brk = nullptr, *dir = nullptr, *bad = nullptr;
  DEV_ALLOC(mem, brk, 4 * std::max<uint64_t>(m, 1), "line table");
  DEV_ALLOC(mem, dir, 4 * entries, "line table");
  DEV_ALLOC(mem, bad, 16, "line table");
  HIP_TRY(hipMemsetAsync(bad, 0, 16, st), "hipMemsetAsync");
  uint64_t launches = 0;
  uint32_t bad_h = 0;
  if (m) {
    unsigned long long *d_iv = nullptr, *off = nullptr, *sa = nullptr;
    SortSpace ws;
    DEV_ALLOC(mem, d_iv, 64, "line table");
    DEV_ALLOC(mem, off, 64, "line table");
    DEV_ALLOC(mem, sa, 8 * m, "line table");
    if ((rc = ws.alloc(mem, m, "line table"))) return rc;
    HIP_TRY(hipMemcpyAsync(d_iv, sp, 32, hipMemcpyHostToDevice, st), "H2D(intervals)");
    HIP_TRY(hipMemcpyAsync(d_iv + 4, ep, 32, hipMemcpyHostToDevice, st), "H2D(intervals)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");       // sp and ep are this frame's
    const dim3 grid(flat_grid(m)), block(kLinThreads);
    HIP_TRY(ev.record(0, st), "hipEventRecord");
    HIP_TRY(launch_locate_intervals(h, d_iv, d_iv + 4, n_set, 0, off, sa, m, st), "k_locate");
    HIP_TRY(ev.record(1, st), "hipEventRecord");
    const int pb = bits_for(n);
    LAUNCH("k_lines_keys", k_lines_keys, grid, block, st, sa, m, n, (1ull << pb) - 1, ws.keys(), ws.vals(), bad);
    HIP_TRY(ws.sort(m, pb, st), "radix sort");
    LAUNCH("k_lines_pack", k_lines_pack, grid, block, st, ws.keys(), m, len, brk, bad);
    HIP_TRY(ev.record(2, st), "hipEventRecord");
    launches += 5 + 3 * (uint64_t)ws.passes;
  } else {
    for (int i = 0; i < 3; i++) HIP_TRY(ev.record(i, st), "hipEventRecord");
  }
  LAUNCH("k_lines_dir", k_lines_dir, dim3(flat_grid(entries)), dim3(kLinThreads), st, brk, m, entries, shift, dir);
  HIP_TRY(ev.record(3, st), "hipEventRecord");
  launches++;
  HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st), "D2H(flag)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");         // the temporaries go when this returns
  add_launches(h, launches);
  if (bad_h) {
    set_error("lines: a break's position lies outside the text or repeats -- not the BWT of one text");
    return FMX_ERR_FORMAT;
  }
  g_lines_last.locate_ms = ev.ms(0, 1);
  g_lines_last.sort_ms = ev.ms(1, 3);
  h->lin.free_locked();                                    // a table for another set
  mem.keep(brk);
  mem.keep(dir);
  h->lin.brk = brk;
  h->lin.dir = dir;
  h->lin.n_brk = m;
  h->lin.shift = shift;
  std::copy(set, set + n_set, h->lin.set);
  h->lin.n_set = n_set;
  h->lin.bytes = keep;
  return FMX_OK;
}

// The table for `set` (ascending) on `st`, under lin.mu: nothing to do when the handle has it for that set, rebuilt when it
// has it for another.  Allocates, synchronises `st`, frees its temporaries on every path.
int lines_build(const Index *h, const uint8_t *set, uint32_t n_set, hipStream_t st) {
  if (const int rc = lines_check(h)) return rc;
  return build_locked(
      h->lin, st, "the line table is built by fmx_prepare(FMX_PREPARE_LINES), fmx_lines_prepare or a first lines call outside a stream capture",
      [&](DevMem &mem) { return lines_table(h, set, n_set, st, mem); },
      [&] { return h->lin.ready && h->lin.n_set == n_set && std::equal(set, set + n_set, h->lin.set); },
      [&] { return ensure_built(h, h->loc, locate_prepare, st); });      // the table is made from the locate samples
}

}  // namespace

// A table for a call that needs one: the handle's, or {10} / {10, 1} built on `st` (a stream of the handle's when null).
// With a corpus the set must hold byte 1.
int lines_ensure(const Index *h, bool with_corpus, hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(h->lin.mu);
    if (h->lin.ready) {
      if (with_corpus && !std::count(h->lin.set, h->lin.set + h->lin.n_set, (uint8_t)1))
        return arg_fail("lines: the line table's break set lacks byte 1, the corpus separator: fmx_lines_prepare with {10, 1}");
      return FMX_OK;
    }
  }
  const uint8_t plain[1] = {10}, stream[2] = {1, 10};
  const uint8_t *set = with_corpus ? stream : plain;
  const uint32_t n_set = with_corpus ? 2 : 1;
  if (st) return lines_build(h, set, n_set, st);
  CtxLease lease(h);
  if (!lease.c) return FMX_ERR_HIP;
  return lines_build(h, set, n_set, lease.c->stream);
}

namespace {

hipError_t lookup_enqueue(const Index *h, const void *d_pos, uint64_t k, void *d_line, void *d_start, void *d_end, hipStream_t st) {
  if (!k) return hipSuccess;
  hipLaunchKernelGGL(k_lines_lookup, dim3(flat_grid(k)), dim3(kLinThreads), 0, st, lines_dev(h),
                     static_cast<const unsigned long long *>(d_pos), k, static_cast<unsigned long long *>(d_line),
                     static_cast<unsigned long long *>(d_start), static_cast<unsigned long long *>(d_end));
  return hipGetLastError();
}

hipError_t spans_enqueue(const Index *h, const void *d_line, uint64_t k, void *d_start, void *d_end, hipStream_t st) {
  if (!k) return hipSuccess;
  hipLaunchKernelGGL(k_lines_spans, dim3(flat_grid(k)), dim3(kLinThreads), 0, st, lines_dev(h),
                     static_cast<const unsigned long long *>(d_line), k, static_cast<unsigned long long *>(d_start),
                     static_cast<unsigned long long *>(d_end));
  return hipGetLastError();
}

// The host forms of the two lookups: k u64 in, up to three arrays of k u64 out.
int lookup_host(const Index *h, bool spans, const uint64_t *in, size_t k, uint64_t *o0, uint64_t *o1, uint64_t *o2) {
  int rc = use_device(h);
  if (rc || (rc = lines_ensure(h, false, nullptr))) return rc;
  g_lines_last.lookup_ms = 0;
  if (!k) return FMX_OK;
  if ((rc = device_room(32 * (uint64_t)k + 4096, spans ? "fmx_line_spans" : "fmx_lines_batch"))) return rc;
  HostCall hc;
  if ((rc = hc.open())) return rc;
  Events<2> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  unsigned long long *d_in = nullptr, *d0 = nullptr, *d1 = nullptr, *d2 = nullptr;
  DEV_ALLOC(hc.mem, d_in, 8 * (uint64_t)k, "lines");
  if (o0) DEV_ALLOC(hc.mem, d0, 8 * (uint64_t)k, "lines");
  if (o1) DEV_ALLOC(hc.mem, d1, 8 * (uint64_t)k, "lines");
  if (o2) DEV_ALLOC(hc.mem, d2, 8 * (uint64_t)k, "lines");
  HIP_TRY(hipMemcpyAsync(d_in, in, 8 * (uint64_t)k, hipMemcpyHostToDevice, hc.own.s), "H2D(lines)");
  HIP_TRY(ev.record(0, hc.own.s), "hipEventRecord");
  if (spans) HIP_TRY(spans_enqueue(h, d_in, k, d0, d1, hc.own.s), "k_lines_spans");
  else HIP_TRY(lookup_enqueue(h, d_in, k, d0, d1, d2, hc.own.s), "k_lines_lookup");
  HIP_TRY(ev.record(1, hc.own.s), "hipEventRecord");
  if ((rc = hc.download(o0, d0, 8 * (uint64_t)k, "D2H(lines)")) || (rc = hc.download(o1, d1, 8 * (uint64_t)k, "D2H(lines)")) ||
      (rc = hc.download(o2, d2, 8 * (uint64_t)k, "D2H(lines)")) || (rc = hc.sync()))
    return rc;
  g_lines_last.lookup_ms = ev.ms(0, 1);
  add_launches(h, 1);
  return FMX_OK;
}

// What the arguments alone decide (both forms of the occurrence lines), before a handle is looked at.
int ol_args(const void *occ_off, const void *occ, size_t n_occ, size_t n_groups, const void *out_off, const void *out, size_t cap,
            const size_t *n_out) {
  if (!occ_off || !out_off || !n_out) return arg_fail("occurrence lines: occ_off, out_off or n_out is null");
  if (n_groups == 0 || (uint64_t)n_groups > kLinMaxK) return arg_fail("occurrence lines: n_groups must be 1 .. 2^26");
  if ((uint64_t)n_occ > kLinMaxK) return arg_fail("occurrence lines: at most 2^26 records per call");
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("occurrence lines: cap must be below 2^32");
  if (n_occ && !occ) return arg_fail("occurrence lines: the records are null");
  if (cap && !out) return arg_fail("occurrence lines: out is null");
  return FMX_OK;
}

int ol_handles(const fmx_index *idx, const fmx_corpus *corpus) {
  if (!idx) return arg_fail("occurrence lines: the handle is null");
  const Index *h = H(idx);
  const int rc = lines_check(h);
  if (rc) return rc;
  if (corpus) {
    const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
    if (h->n != c->stream_len + 1) return arg_fail("occurrence lines: the index is not the index of this corpus (n != stream length + 1)");
    if (h->device != c->device) return arg_fail("occurrence lines: the index and the corpus live on different devices");
  }
  return FMX_OK;
}

// The whole reduction on `st`: d_occ_off, d_occ, d_out_off and d_out in device memory.  Allocates, synchronises `st`, frees
// its temporaries on every path; *total = the lines found.
int ol_run(const Index *h, const Corpus *c, const unsigned long long *d_occ_off, const fmx_occurrence *d_occ, uint64_t n_occ,
           uint64_t n_groups, unsigned long long *d_out_off, fmx_line_hit *d_out, uint64_t cap, hipStream_t st, uint64_t *total) {
  g_lines_last.lookup_ms = g_lines_last.compact_ms = 0;
  int rc = lines_ensure(h, c != nullptr, st);
  if (rc) return rc;
  const dim3 block(kLinThreads);
  if (!n_occ) {
    LAUNCH("k_ol_off", k_ol_off, dim3(flat_grid(n_groups + 1)), block, st, d_occ_off, n_groups, nullptr, 0ull, d_out_off);
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    add_launches(h, 1);
    *total = 0;
    return FMX_OK;
  }
  if ((rc = device_room(16 * n_occ + ScanSpace::bytes(n_occ) + 4096, "fmx_occurrence_lines"))) return rc;
  const CoMap map = c ? c->map() : CoMap{nullptr, nullptr, nullptr, 0, 0, 0};
  const LinesDev L = lines_dev(h);
  Events<3> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  uint32_t *grp = nullptr, *line = nullptr, *flag = nullptr, *hidx = nullptr, *bad = nullptr;
  ScanSpace scan;
  DEV_ALLOC(mem, grp, 4 * n_occ, "occurrence lines");
  DEV_ALLOC(mem, line, 4 * n_occ, "occurrence lines");
  DEV_ALLOC(mem, flag, 4 * n_occ, "occurrence lines");
  DEV_ALLOC(mem, hidx, 4 * n_occ, "occurrence lines");
  if ((rc = scan.alloc(mem, n_occ, "occurrence lines"))) return rc;
  DEV_ALLOC(mem, bad, 16, "occurrence lines");
  const dim3 grid(flat_grid(n_occ));
  HIP_TRY(hipMemsetAsync(bad, 0, 16, st), "hipMemsetAsync");
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  LAUNCH("k_ol_lines", k_ol_lines, grid, block, st, L, d_occ_off, n_groups, d_occ, n_occ, grp, line, bad);
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  uint32_t bad_h = 0;
  HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st), "D2H(flag)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (bad_h) {
    add_launches(h, 1);
    return arg_fail("occurrence lines: a record with pos >= n - 1, or offsets that do not cover the records");
  }
  LAUNCH("k_ol_heads", k_ol_heads, grid, block, st, grp, line, n_occ, flag);
  HIP_TRY(scan.sum(flag, n_occ, false, st), "scan");
  LAUNCH("k_ol_off", k_ol_off, dim3(flat_grid(n_groups + 1)), block, st, d_occ_off, n_groups, flag, n_occ, d_out_off);
  if (cap) {
    LAUNCH("k_ol_pick", k_ol_pick, grid, block, st, flag, n_occ, hidx);
    LAUNCH("k_ol_emit", k_ol_emit, dim3(flat_grid(std::min(n_occ, cap))), block, st, L, d_occ_off, grp, line, flag, hidx, n_occ, c ? 1 : 0,
           map, cap, d_out);
  }
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  uint32_t tot = 0;
  HIP_TRY(hipMemcpyAsync(&tot, flag + (n_occ - 1), 4, hipMemcpyDeviceToHost, st), "D2H(total)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
  g_lines_last.lookup_ms = ev.ms(0, 1);
  g_lines_last.compact_ms = ev.ms(1, 2);
  add_launches(h, 7);
  *total = tot;
  return FMX_OK;
}

}  // namespace

int lines_check(const Index *h) {
  const int rc = locate_check(h);
  if (rc) return rc;
  if (h->n >= (1ull << 32)) {
    set_error("lines: indexes of 2^32 rows and more are not supported (positions are 32 bits in the line table)");
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

int lines_prepare(const Index *h, hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(h->lin.mu);
    if (h->lin.ready) return FMX_OK;
  }
  const uint8_t set[1] = {10};
  return lines_build(h, set, 1, st);
}

}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_lines_prepare(const fmx_index *idx, const uint8_t *breaks, size_t n_breaks) {
  uint8_t set[4];
  uint32_t n_set = 0;
  int rc = lines_set_args(breaks, n_breaks, set, &n_set);
  if (rc) return rc;
  if (!idx) return arg_fail("lines: the handle is null");
  const Index *h = H(idx);
  if ((rc = lines_check(h)) || (rc = use_device(h))) return rc;
  CtxLease lease(h);
  if (!lease.c) return FMX_ERR_HIP;
  return lines_build(h, set, n_set, lease.c->stream);
}

int fmx_lines_info(const fmx_index *idx, uint64_t *n_breaks_found, uint8_t set[4], uint32_t *n_set, uint32_t *shift, uint64_t *bytes,
                   double *build_ms) {
  if (!idx) return arg_fail("null argument");
  const Index *h = H(idx);
  std::lock_guard<std::mutex> lk(h->lin.mu);
  if (n_breaks_found) *n_breaks_found = h->lin.ready ? h->lin.n_brk : 0;
  if (set) {
    for (int i = 0; i < 4; i++) set[i] = h->lin.ready && (uint32_t)i < h->lin.n_set ? h->lin.set[i] : 0;
    if (!h->lin.ready) set[0] = 10;
  }
  if (n_set) *n_set = h->lin.ready ? h->lin.n_set : 1;
  if (shift) *shift = h->lin.ready ? h->lin.shift : (uint32_t)h->policy.lines_shift.load(std::memory_order_relaxed);
  if (bytes) *bytes = h->lin.ready ? h->lin.bytes : 0;
  if (build_ms) *build_ms = h->lin.ready ? h->lin.build_ms : 0.0;
  return FMX_OK;
}

int fmx_lines_batch(const fmx_index *idx, const uint64_t *pos, size_t k, uint64_t *line, uint64_t *start, uint64_t *end) {
  if (!idx) return arg_fail("lines: the handle is null");
  if (k && !pos) return arg_fail("lines: null argument (pos)");
  const Index *h = H(idx);
  const int rc = lines_check(h);
  if (rc) return rc;
  return lookup_host(h, false, pos, k, line, start, end);
}

int fmx_lines_batch_dev(const fmx_index *idx, const void *d_pos, size_t k, void *d_line, void *d_start, void *d_end, void *stream) {
  if (!idx) return arg_fail("lines: the handle is null");
  if (k && !d_pos) return arg_fail("lines: null argument (d_pos)");
  const Index *h = H(idx);
  int rc = lines_check(h);
  if (rc || !k) return rc;
  if ((rc = use_device(h)) || (rc = lines_ensure(h, false, (hipStream_t)stream))) return rc;
  HIP_TRY(lookup_enqueue(h, d_pos, k, d_line, d_start, d_end, (hipStream_t)stream), "k_lines_lookup");
  return FMX_OK;
}

int fmx_line_spans(const fmx_index *idx, const uint64_t *line, size_t k, uint64_t *start, uint64_t *end) {
  if (!idx) return arg_fail("lines: the handle is null");
  if (k && !line) return arg_fail("lines: null argument (line)");
  const Index *h = H(idx);
  const int rc = lines_check(h);
  if (rc) return rc;
  return lookup_host(h, true, line, k, start, end, nullptr);
}

int fmx_line_spans_dev(const fmx_index *idx, const void *d_line, size_t k, void *d_start, void *d_end, void *stream) {
  if (!idx) return arg_fail("lines: the handle is null");
  if (k && !d_line) return arg_fail("lines: null argument (d_line)");
  const Index *h = H(idx);
  int rc = lines_check(h);
  if (rc || !k) return rc;
  if ((rc = use_device(h)) || (rc = lines_ensure(h, false, (hipStream_t)stream))) return rc;
  HIP_TRY(spans_enqueue(h, d_line, k, d_start, d_end, (hipStream_t)stream), "k_lines_spans");
  return FMX_OK;
}

int fmx_occurrence_lines_dev(const fmx_index *idx, const fmx_corpus *corpus, const void *d_occ_off, const void *d_occ, size_t n_occ,
                             size_t n_groups, void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  int rc = ol_args(d_occ_off, d_occ, n_occ, n_groups, d_out_off, d_out, cap, n_out);
  if (rc || (rc = ol_handles(idx, corpus))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_occurrence_lines_dev"))) return rc;
  uint64_t total = 0;
  if ((rc = ol_run(h, reinterpret_cast<const Corpus *>(corpus), static_cast<const unsigned long long *>(d_occ_off),
                   static_cast<const fmx_occurrence *>(d_occ), n_occ, n_groups, static_cast<unsigned long long *>(d_out_off),
                   static_cast<fmx_line_hit *>(d_out), cap, st, &total)))
    return rc;
  *n_out = (size_t)total;
  return total > cap ? csr_overflow("occurrence lines", total, cap) : FMX_OK;
}

int fmx_occurrence_lines(const fmx_index *idx, const fmx_corpus *corpus, const uint64_t *occ_off, const fmx_occurrence *occ,
                         size_t n_groups, uint64_t *out_off, fmx_line_hit *out, size_t cap, size_t *n_out) {
  if (!occ_off) return arg_fail("occurrence lines: occ_off, out_off or n_out is null");
  if (n_groups == 0 || (uint64_t)n_groups > kLinMaxK) return arg_fail("occurrence lines: n_groups must be 1 .. 2^26");
  if (occ_off[0] != 0 || !offsets_monotonic(occ_off, 0, n_groups)) return arg_fail("occurrence lines: occ_off must begin at 0 and be non-decreasing");
  const uint64_t n_occ = occ_off[n_groups];
  int rc = ol_args(occ_off, occ, n_occ, n_groups, out_off, out, cap, n_out);
  if (rc || (rc = ol_handles(idx, corpus))) return rc;
  const Index *h = H(idx);
  for (uint64_t i = 0; i < n_occ; i++)
    if (occ[i].pos >= h->n - 1) return arg_fail("occurrence lines: a record's pos is not below n - 1");
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  if ((rc = hc.open())) return rc;
  if ((rc = device_room(32 * n_occ + 16 * ((uint64_t)n_groups + 1) + 48 * (uint64_t)cap + 4096, "fmx_occurrence_lines"))) return rc;
  unsigned long long *d_in_off = nullptr, *d_off = nullptr;
  fmx_occurrence *d_occ = nullptr;
  fmx_line_hit *d_out = nullptr;
  DEV_ALLOC(hc.mem, d_in_off, 8 * ((uint64_t)n_groups + 1), "occurrence offsets");
  DEV_ALLOC(hc.mem, d_off, 8 * ((uint64_t)n_groups + 1), "line offsets");
  DEV_ALLOC(hc.mem, d_occ, sizeof(fmx_occurrence) * n_occ, "occurrence records");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_line_hit) * (uint64_t)cap, "line hits");
  HIP_TRY(hipMemcpyAsync(d_in_off, occ_off, 8 * ((uint64_t)n_groups + 1), hipMemcpyHostToDevice, hc.own.s), "H2D(offsets)");
  if (n_occ) HIP_TRY(hipMemcpyAsync(d_occ, occ, sizeof(fmx_occurrence) * n_occ, hipMemcpyHostToDevice, hc.own.s), "H2D(records)");
  uint64_t total = 0;
  if ((rc = ol_run(h, reinterpret_cast<const Corpus *>(corpus), d_in_off, d_occ, n_occ, n_groups, d_off, d_out, cap, hc.own.s, &total)))
    return rc;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("occurrence lines", total, cap);
  return hc.download_csr(out_off, d_off, n_groups, out, d_out, total, sizeof(fmx_line_hit));
}

int fmx_lines_last(double *locate_ms, double *sort_ms, double *lookup_ms, double *compact_ms) {
  if (locate_ms) *locate_ms = g_lines_last.locate_ms;
  if (sort_ms) *sort_ms = g_lines_last.sort_ms;
  if (lookup_ms) *lookup_ms = g_lines_last.lookup_ms;
  if (compact_ms) *compact_ms = g_lines_last.compact_ms;
  return FMX_OK;
}

}  // extern "C"
