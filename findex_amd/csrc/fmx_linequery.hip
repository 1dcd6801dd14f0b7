// fmx_linequery.hip -- line queries: all-of, none-of, near and inverted matches over line-hit lists (fmx.h: fmx_line_query;
// DESIGN.md §24).  The input is what fmx_occurrence_lines leaves: per group one fmx_line_hit per distinct line, ascending by
// the key doc << 32 | line_no.  A query is an anchor -- a group, or every real line of the text -- and terms (group, window,
// NOT); its result is the anchor's records that satisfy every term, in order.
//
//   keys   : k_lq_keys   every hit's key into a dense u64[n_hits] (the searches never stride through 48-byte records); a key
//                        that does not ascend within its group raises a flag
//   flags  : k_lq_flags  one lane per candidate: its query (a search in the candidate offsets), its key (the anchor's, or from
//                        the line table with the realness test), per term a lower bound of (d, max(1, i - w)) in the term's
//                        key range compared with (d, i + w); with "lq_narrow" on a wave whose lanes share a query narrows
//                        the range first by the bounds of its first and last lane (off by default: it measured slower)
//   scan   : ScanSpace (fmx_order.h) over the flags
//   emit   : k_lq_emit   one record per kept candidate: the anchor's with `group` = the query, or lin_record's from the table
//   offsets: k_lq_off    out_off[q] = the inclusive sum in front of the query's first candidate
// No atomics decide an order: the same input gives the same bytes on every run.
#include <fmx.h>

#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "fmx_corpus_dev.h"
#include "fmx_order.h"
#include "fmx_lines_dev.h"

namespace fmx {

constexpr int kLqThreads = 256;
constexpr uint64_t kLqMaxK = 1ull << 26;             // hit records and groups per call
constexpr uint64_t kLqMaxQueries = 1ull << 16;
constexpr uint64_t kLqMaxTerms = 64;                 // per query
constexpr uint32_t kLqProbeCounter = 12;             // the word of a counter slot the probes are summed in (free: fmx_device.h)
static_assert(sizeof(fmx_line_term) == 16 && sizeof(fmx_line_hit) == 48, "record sizes are ABI");

struct LqTables {                                    // the query tables, one upload
  const unsigned long long *cand_off, *q_off;        // [n_queries + 1] each
  const uint32_t *anchor;                            // [n_queries]
  const fmx_line_term *terms;
  uint64_t n_queries;
};

__device__ __forceinline__ unsigned long long lq_key(uint32_t doc, uint64_t line_no) {
  return (unsigned long long)doc << 32 | (line_no & 0xffffffffull);
}

// keys[i] of every record; a line_no outside 1 .. 2^32 - 1 or a key not above its predecessor's in the same group: the flag
__global__ __launch_bounds__(kLqThreads) void k_lq_keys(const unsigned long long *__restrict__ hit_off, uint64_t n_groups,
                                                        const fmx_line_hit *__restrict__ hits, uint64_t n_hits,
                                                        unsigned long long *__restrict__ keys, uint32_t *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_hits; i += stride) {
    const uint64_t ln = hits[i].line_no;
    const unsigned long long k = lq_key(hits[i].doc, ln);
    bool ok = ln >= 1 && ln < (1ull << 32);
    if (i) {
      const uint64_t u = upper_bound(hit_off, 0, n_groups + 1, i);      // hit_off[u - 1] <= i: the group's first record, or not
      if (hit_off[u - 1] != i && lq_key(hits[i - 1].doc, hits[i - 1].line_no) >= k) ok = false;
    }
    if (!ok) *bad = 1u;
    keys[i] = k;
  }
}

// first index in [lo, hi) whose key is >= v, counting the keys read
__device__ __forceinline__ uint64_t lq_lower(const unsigned long long *__restrict__ keys, uint64_t lo, uint64_t hi,
                                             unsigned long long v, uint32_t &probes) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    probes++;
    if (keys[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the two ends of a term's window around the key (d, i): (d, max(1, i - w)) and (d, min(i + w, 2^32 - 1))
__device__ __forceinline__ void lq_window(unsigned long long key, uint32_t w, unsigned long long &klo, unsigned long long &khi) {
  const uint64_t i = key & 0xffffffffull, top = key & ~0xffffffffull;
  const uint64_t lo = i > w ? i - w : 1, hi = i + w > 0xffffffffull ? 0xffffffffull : i + w;
  klo = top | lo;
  khi = top | hi;
}

// The key of candidate j of an all-lines query: global line j of the table.  real: not the empty piece behind a final break
// (without a corpus) or in front of a document's separator (with one).  Keys ascend with j whether real or not.
__device__ __forceinline__ unsigned long long lq_line_key(const LinesDev &L, int has_map, const CoMap &m, uint64_t j, bool &real) {
  const uint64_t s = lin_start(L, j);
  if (!has_map) {
    real = s != L.len;
    return lq_key(0xffffffffu, j + 1);
  }
  if (s >= m.stream_len) {
    real = false;
    return ~0ull;
  }
  const uint64_t d = upper_bound(m.doc_start, 0, m.n_docs, s) - 1;       // doc_start[0] = 0 <= s
  real = s + 1 != (uint64_t)m.doc_start[d + 1];
  return lq_key((uint32_t)d, j - lin_line(L, m.doc_start[d]) + 1);
}

// flag[c] = 1 where candidate c is real and satisfies every term of its query.  Every lane of a wave runs every trip (the
// lanes past the end redo the last candidate and write nothing), so the wave-wide steps are convergent.
__global__ __launch_bounds__(kLqThreads) void k_lq_flags(LinesDev L, int has_map, CoMap m,
                                                         const unsigned long long *__restrict__ hit_off,
                                                         const unsigned long long *__restrict__ keys, LqTables T, uint64_t n_cand,
                                                         int narrow, uint32_t *__restrict__ flag,
                                                         unsigned long long *__restrict__ mine) {
  uint32_t probes = 0;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kLqThreads; c0 < n_cand; c0 += (uint64_t)gridDim.x * kLqThreads) {
    const uint64_t c = c0 + threadIdx.x, cc = c < n_cand ? c : n_cand - 1;
    const uint64_t q = upper_bound(T.cand_off, 0, T.n_queries + 1, cc) - 1;      // cand_off[0] = 0 <= cc < cand_off[n_queries]
    const uint64_t j = cc - T.cand_off[q];
    const uint32_t a = T.anchor[q];
    bool real = true;
    const unsigned long long key = a == FMX_LQ_ALL_LINES ? lq_line_key(L, has_map, m, j, real) : keys[hit_off[a] + j];
    const uint64_t t0 = T.q_off[q], t1 = T.q_off[q + 1];
    bool ok = real;
    const uint64_t q_first = __shfl(q, 0, 64);
    if (narrow && __all(q == q_first)) {
      // one query for the whole wave: its candidates' keys ascend with the lane, so every lane's bound lies between those
      // of lane 0 and lane 63
      const bool lead = lane == 0 || lane == 63;
      for (uint64_t t = t0; t < t1; t++) {
        if (!__any(ok)) break;
        const fmx_line_term tm = T.terms[t];
        const uint64_t lo = hit_off[tm.group], hi = hit_off[tm.group + 1];
        unsigned long long klo, khi;
        lq_window(key, tm.window, klo, khi);
        uint64_t p = lead ? lq_lower(keys, lo, hi, klo, probes) : 0;
        const uint64_t p_first = __shfl(p, 0, 64), p_last = __shfl(p, 63, 64);
        if (ok && !lead) p = lq_lower(keys, p_first, p_last, klo, probes);
        if (ok) {
          bool found = false;
          if (p < hi) {
            probes++;
            found = keys[p] <= khi;
          }
          ok = found != ((tm.flags & FMX_LQ_NOT) != 0);
        }
      }
    } else {
      for (uint64_t t = t0; t < t1 && ok; t++) {
        const fmx_line_term tm = T.terms[t];
        const uint64_t lo = hit_off[tm.group], hi = hit_off[tm.group + 1];
        unsigned long long klo, khi;
        lq_window(key, tm.window, klo, khi);
        const uint64_t p = lq_lower(keys, lo, hi, klo, probes);
        bool found = false;
        if (p < hi) {
          probes++;
          found = keys[p] <= khi;
        }
        ok = found != ((tm.flags & FMX_LQ_NOT) != 0);
      }
    }
    if (c < n_cand) flag[c] = ok ? 1u : 0u;
  }
  const unsigned long long sum = wave_sum(probes);
  if (lane == 0 && sum) atomicAdd(mine + (size_t)(blockIdx.x % kCounterSlots) * kCounterStride + kLqProbeCounter, sum);
}

// the probes of all counter slots into the call's line (one workgroup)
__global__ __launch_bounds__(kLqThreads) void k_lq_sum(const unsigned long long *__restrict__ mine, unsigned long long *__restrict__ line) {
  unsigned long long v = 0;
  for (uint32_t sl = threadIdx.x; sl < kCounterSlots; sl += kLqThreads) v += mine[(size_t)sl * kCounterStride + kLqProbeCounter];
  v = wave_sum(v);
  if ((threadIdx.x & 63u) == 0 && v) atomicAdd(line + kLineSteps, v);
}

// one record per kept candidate; the kept number incl[n_cand - 1], the first min(that, cap) are written
__global__ __launch_bounds__(kLqThreads) void k_lq_emit(LinesDev L, int has_map, CoMap m,
                                                        const unsigned long long *__restrict__ hit_off,
                                                        const fmx_line_hit *__restrict__ hits, LqTables T,
                                                        const uint32_t *__restrict__ incl, uint64_t n_cand, uint64_t cap,
                                                        fmx_line_hit *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cand; c += stride) {
    const uint32_t after = incl[c], before = c ? incl[c - 1] : 0u;
    if (after == before || (uint64_t)before >= cap) continue;
    const uint64_t q = upper_bound(T.cand_off, 0, T.n_queries + 1, c) - 1, j = c - T.cand_off[q];
    const uint32_t a = T.anchor[q];
    fmx_line_hit o;
    if (a == FMX_LQ_ALL_LINES) o = lin_record(L, j, has_map, m);
    else o = hits[hit_off[a] + j];
    o.group = (uint32_t)q;
    out[before] = o;
  }
}

// out_off[q] = the kept candidates before query q's first, q = 0 .. n_queries
__global__ __launch_bounds__(kLqThreads) void k_lq_off(LqTables T, const uint32_t *__restrict__ incl, uint64_t n_cand,
                                                       unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= T.n_queries; q += stride) {
    uint64_t j = n_cand ? T.cand_off[q] : 0;
    j = j < n_cand ? j : n_cand;
    out_off[q] = j ? incl[j - 1] : 0u;
  }
}

namespace {

struct LqInfo {
  double keys_ms = 0, flags_ms = 0, emit_ms = 0;
  uint64_t candidates = 0, probes = 0;
};
thread_local LqInfo g_lq_last;
std::atomic<int> g_lq_narrow{0};             // "lq_narrow": off by default (the plain search measured faster)

// What the arguments alone decide (both forms), before a handle is looked at.
int lq_args(const void *hit_off, const void *hits, size_t n_hits, size_t n_groups, const uint64_t *q_off, const uint32_t *anchor,
            const fmx_line_term *terms, size_t n_queries, const void *out_off, const void *out, size_t cap, const size_t *n_out) {
  if (!hit_off || !out_off || !n_out || !q_off || !anchor) return arg_fail("line query: hit_off, out_off, n_out, q_off or anchor is null");
  if (n_groups == 0 || (uint64_t)n_groups > kLqMaxK) return arg_fail("line query: n_groups must be 1 .. 2^26");
  if (n_queries == 0 || (uint64_t)n_queries > kLqMaxQueries) return arg_fail("line query: n_queries must be 1 .. 2^16");
  if (q_off[0] != 0 || !offsets_monotonic(q_off, 0, n_queries)) return arg_fail("line query: q_off must begin at 0 and be non-decreasing");
  for (size_t q = 0; q < n_queries; q++)
    if (q_off[q + 1] - q_off[q] > kLqMaxTerms) return arg_fail("line query: at most 64 terms in one query");
  const uint64_t n_terms = q_off[n_queries];
  if (n_terms && !terms) return arg_fail("line query: terms is null while there are some");
  for (size_t q = 0; q < n_queries; q++)
    if (anchor[q] != FMX_LQ_ALL_LINES && anchor[q] >= n_groups) return arg_fail("line query: an anchor names no group (>= n_groups)");
  for (uint64_t t = 0; t < n_terms; t++) {
    if (terms[t].group >= n_groups) return arg_fail("line query: a term names no group (>= n_groups)");
    if ((terms[t].flags & ~FMX_LQ_NOT) || terms[t].reserved) return arg_fail("line query: a term's flags hold unknown bits, or its reserved field is not 0");
  }
  if ((uint64_t)cap >= (1ull << 32)) return arg_fail("line query: cap must be below 2^32");
  if ((uint64_t)n_hits > kLqMaxK) return arg_fail("line query: at most 2^26 hit records per call");
  if (n_hits && !hits) return arg_fail("line query: the records are null");
  if (cap && !out) return arg_fail("line query: out is null");
  return FMX_OK;
}

int lq_handles(const fmx_index *idx, const fmx_corpus *corpus) {
  if (!idx) return arg_fail("line query: the handle is null");
  const Index *h = H(idx);
  if (corpus) {
    const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
    if (h->n != c->stream_len + 1) return arg_fail("line query: the index is not the index of this corpus (n != stream length + 1)");
    if (h->device != c->device) return arg_fail("line query: the index and the corpus live on different devices");
  }
  return FMX_OK;
}

void add_launches(const Index *h, uint64_t launches) {
  std::lock_guard<std::mutex> lk(h->mu);
  h->launches += launches;
}

// The whole evaluation on `st`: d_hit_off, d_hits, d_out_off and d_out in device memory, hit_off the same offsets on the host,
// the query arrays on the host.  Allocates, synchronises `st`, frees its temporaries on every path; *total = the records kept.
int lq_run(const Index *h, const Corpus *c, const uint64_t *hit_off, const unsigned long long *d_hit_off, const fmx_line_hit *d_hits,
           uint64_t n_hits, uint64_t n_groups, const uint64_t *q_off, const uint32_t *anchor, const fmx_line_term *terms,
           uint64_t n_queries, unsigned long long *d_out_off, fmx_line_hit *d_out, uint64_t cap, hipStream_t st, uint64_t *total) {
  g_lq_last = LqInfo{};
  int rc;
  bool all_lines = false;
  for (uint64_t q = 0; q < n_queries; q++) all_lines |= anchor[q] == FMX_LQ_ALL_LINES;
  if (all_lines && ((rc = lines_check(h)) || (rc = lines_ensure(h, c != nullptr, st)))) return rc;
  const LinesDev L = all_lines ? lines_dev(h) : LinesDev{nullptr, nullptr, 0, h->n - 1, 0};
  // the candidates: known here, before anything of their size is allocated
  const uint64_t n_terms = q_off[n_queries], words = n_queries + 1;
  std::vector<unsigned long long> tab(2 * words + (n_queries + 1) / 2 + 2 * n_terms);
  unsigned long long *cand_off = tab.data(), *qo = cand_off + words;
  uint32_t *an = reinterpret_cast<uint32_t *>(qo + words);
  fmx_line_term *tm = reinterpret_cast<fmx_line_term *>(qo + words + (n_queries + 1) / 2);
  uint64_t n_cand = 0;
  for (uint64_t q = 0; q < n_queries; q++) {
    cand_off[q] = n_cand;
    n_cand += anchor[q] == FMX_LQ_ALL_LINES ? L.n_brk + 1 : hit_off[anchor[q] + 1] - hit_off[anchor[q]];
    if (n_cand >= (1ull << 32)) {
      set_error("line query: the candidates of all queries together must be below 2^32");
      return FMX_ERR_OVERFLOW;
    }
    qo[q] = q_off[q];
    an[q] = anchor[q];
  }
  cand_off[n_queries] = n_cand;
  qo[n_queries] = n_terms;
  if (n_terms) std::memcpy(tm, terms, sizeof(fmx_line_term) * n_terms);
  const uint64_t tab_bytes = 8 * (uint64_t)tab.size();
  // 8 bytes per hit, 4 per candidate, the scan's block totals, the query tables
  if ((rc = device_room(8 * n_hits + 4 * n_cand + ScanSpace::bytes(n_cand) + tab_bytes + kMeteredBytes + 4096, "fmx_line_query"))) return rc;
  const CoMap map = c ? c->map() : CoMap{nullptr, nullptr, nullptr, 0, 0, 0};
  Events<5> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  Metered own;
  unsigned long long *d_tab = nullptr, *keys = nullptr;
  uint32_t *flag = nullptr, *bad = nullptr;
  ScanSpace scan;
  DEV_ALLOC(mem, d_tab, tab_bytes, "line query");
  DEV_ALLOC(mem, keys, 8 * n_hits, "line query");
  DEV_ALLOC(mem, flag, 4 * n_cand, "line query");
  if ((rc = scan.alloc(mem, n_cand, "line query"))) return rc;
  DEV_ALLOC(mem, bad, 16, "line query");
  if ((rc = own.alloc(mem, "line query")) || (rc = own.zero(st))) return rc;
  HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, st), "H2D(queries)");
  HIP_TRY(hipMemsetAsync(bad, 0, 16, st), "hipMemsetAsync");
  const LqTables T{d_tab, d_tab + words, reinterpret_cast<const uint32_t *>(d_tab + 2 * words),
                   reinterpret_cast<const fmx_line_term *>(d_tab + 2 * words + (n_queries + 1) / 2), n_queries};
  const dim3 block(kLqThreads);
  uint64_t launches = 0;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if (n_hits) {
    LAUNCH("k_lq_keys", k_lq_keys, dim3(flat_grid(n_hits)), block, st, d_hit_off, n_groups, d_hits, n_hits, keys, bad);
    launches++;
  }
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  uint32_t bad_h = 0;
  HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st), "D2H(flag)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (bad_h) {
    add_launches(h, launches);
    return arg_fail("line query: keys (doc, line_no) that do not ascend strictly inside a group, or a line_no outside 1 .. 2^32 - 1");
  }
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  if (n_cand) {
    LAUNCH("k_lq_flags", k_lq_flags, dim3(flat_grid(n_cand)), block, st, L, c ? 1 : 0, map, d_hit_off, keys, T, n_cand,
           g_lq_narrow.load(std::memory_order_relaxed), flag, own.mine);
    HIP_TRY(ev.record(3, st), "hipEventRecord");
    HIP_TRY(scan.sum(flag, n_cand, false, st), "scan");
    if (cap) {
      LAUNCH("k_lq_emit", k_lq_emit, dim3(flat_grid(n_cand)), block, st, L, c ? 1 : 0, map, d_hit_off, d_hits, T, flag, n_cand, cap, d_out);
    }
    launches += 5;
  } else {
    HIP_TRY(ev.record(3, st), "hipEventRecord");
  }
  LAUNCH("k_lq_off", k_lq_off, dim3(flat_grid(n_queries + 1)), block, st, T, flag, n_cand, d_out_off);
  HIP_TRY(ev.record(4, st), "hipEventRecord");
  LAUNCH("k_lq_sum", k_lq_sum, dim3(1), block, st, own.mine, own.line);
  uint32_t tot = 0;
  if (n_cand) HIP_TRY(hipMemcpyAsync(&tot, flag + (n_cand - 1), 4, hipMemcpyDeviceToHost, st), "D2H(total)");
  MeterCounts cnt;
  if ((rc = own.finish(h, st, launches + 2, &cnt))) return rc;       // synchronises: the temporaries go when this returns
  g_lq_last.keys_ms = ev.ms(0, 1);
  g_lq_last.flags_ms = ev.ms(2, 3);
  g_lq_last.emit_ms = ev.ms(3, 4);
  g_lq_last.candidates = n_cand;
  g_lq_last.probes = cnt.steps;
  *total = tot;
  return FMX_OK;
}

}  // namespace

int lq_config(const char *key, const char *value, const char **why) {
  if (std::strcmp(key, "lq_narrow") != 0) return 1;
  if (std::strcmp(value, "on") == 0) g_lq_narrow.store(1, std::memory_order_relaxed);
  else if (std::strcmp(value, "off") == 0) g_lq_narrow.store(0, std::memory_order_relaxed);
  else {
    *why = "lq_narrow must be on or off";
    return 2;
  }
  return 0;
}

}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_line_query_dev(const fmx_index *idx, const fmx_corpus *corpus, const void *d_hit_off, const void *d_hits, size_t n_hits,
                       size_t n_groups, const uint64_t *q_off, const uint32_t *anchor, const fmx_line_term *terms, size_t n_queries,
                       void *d_out_off, void *d_out, size_t cap, size_t *n_out, void *stream) {
  int rc = lq_args(d_hit_off, d_hits, n_hits, n_groups, q_off, anchor, terms, n_queries, d_out_off, d_out, cap, n_out);
  if (rc || (rc = lq_handles(idx, corpus))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "fmx_line_query_dev"))) return rc;
  // the anchor sizes are hit_off differences: the offsets come down
  std::vector<uint64_t> hit_off(n_groups + 1);
  HIP_TRY(hipMemcpyAsync(hit_off.data(), d_hit_off, 8 * ((uint64_t)n_groups + 1), hipMemcpyDeviceToHost, st), "D2H(offsets)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (hit_off[0] != 0 || !offsets_monotonic(hit_off.data(), 0, n_groups) || hit_off[n_groups] != n_hits)
    return arg_fail("line query: hit_off must begin at 0, be non-decreasing and end at n_hits");
  uint64_t total = 0;
  if ((rc = lq_run(h, reinterpret_cast<const Corpus *>(corpus), hit_off.data(), static_cast<const unsigned long long *>(d_hit_off),
                   static_cast<const fmx_line_hit *>(d_hits), n_hits, n_groups, q_off, anchor, terms, n_queries,
                   static_cast<unsigned long long *>(d_out_off), static_cast<fmx_line_hit *>(d_out), cap, st, &total)))
    return rc;
  *n_out = (size_t)total;
  return total > cap ? csr_overflow("line query", total, cap) : FMX_OK;
}

int fmx_line_query(const fmx_index *idx, const fmx_corpus *corpus, const uint64_t *hit_off, const fmx_line_hit *hits, size_t n_groups,
                   const uint64_t *q_off, const uint32_t *anchor, const fmx_line_term *terms, size_t n_queries, uint64_t *out_off,
                   fmx_line_hit *out, size_t cap, size_t *n_out) {
  if (!hit_off) return arg_fail("line query: hit_off, out_off, n_out, q_off or anchor is null");
  if (n_groups == 0 || (uint64_t)n_groups > kLqMaxK) return arg_fail("line query: n_groups must be 1 .. 2^26");
  if (hit_off[0] != 0 || !offsets_monotonic(hit_off, 0, n_groups)) return arg_fail("line query: hit_off must begin at 0 and be non-decreasing");
  const uint64_t n_hits = hit_off[n_groups];
  int rc = lq_args(hit_off, hits, n_hits, n_groups, q_off, anchor, terms, n_queries, out_off, out, cap, n_out);
  if (rc) return rc;
  for (size_t g = 0; g < n_groups; g++)
    for (uint64_t i = hit_off[g]; i < hit_off[g + 1]; i++) {
      const uint64_t ln = hits[i].line_no;
      const bool first = i == hit_off[g];
      if (ln < 1 || ln >= (1ull << 32) ||
          (!first && ((uint64_t)hits[i - 1].doc << 32 | hits[i - 1].line_no) >= ((uint64_t)hits[i].doc << 32 | ln)))
        return arg_fail("line query: keys (doc, line_no) that do not ascend strictly inside a group, or a line_no outside 1 .. 2^32 - 1");
    }
  if ((rc = lq_handles(idx, corpus))) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h))) return rc;
  HostCall hc;
  if ((rc = hc.open())) return rc;
  if ((rc = device_room(48 * n_hits + 16 * ((uint64_t)n_groups + 1) + 8 * ((uint64_t)n_queries + 1) + 48 * (uint64_t)cap + 4096, "fmx_line_query")))
    return rc;
  unsigned long long *d_in_off = nullptr, *d_off = nullptr;
  fmx_line_hit *d_hits = nullptr, *d_out = nullptr;
  DEV_ALLOC(hc.mem, d_in_off, 8 * ((uint64_t)n_groups + 1), "hit offsets");
  DEV_ALLOC(hc.mem, d_off, 8 * ((uint64_t)n_queries + 1), "query offsets");
  DEV_ALLOC(hc.mem, d_hits, sizeof(fmx_line_hit) * n_hits, "hit records");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_line_hit) * (uint64_t)cap, "line hits");
  HIP_TRY(hipMemcpyAsync(d_in_off, hit_off, 8 * ((uint64_t)n_groups + 1), hipMemcpyHostToDevice, hc.own.s), "H2D(offsets)");
  if (n_hits) HIP_TRY(hipMemcpyAsync(d_hits, hits, sizeof(fmx_line_hit) * n_hits, hipMemcpyHostToDevice, hc.own.s), "H2D(records)");
  uint64_t total = 0;
  if ((rc = lq_run(h, reinterpret_cast<const Corpus *>(corpus), hit_off, d_in_off, d_hits, n_hits, n_groups, q_off, anchor, terms,
                   n_queries, d_off, d_out, cap, hc.own.s, &total)))
    return rc;
  *n_out = (size_t)total;
  if (total > cap) return csr_overflow("line query", total, cap);
  return hc.download_csr(out_off, d_off, n_queries, out, d_out, total, sizeof(fmx_line_hit));
}

int fmx_line_query_last(double *keys_ms, double *flags_ms, double *emit_ms, uint64_t *candidates, uint64_t *probes) {
  if (keys_ms) *keys_ms = g_lq_last.keys_ms;
  if (flags_ms) *flags_ms = g_lq_last.flags_ms;
  if (emit_ms) *emit_ms = g_lq_last.emit_ms;
  if (candidates) *candidates = g_lq_last.candidates;
  if (probes) *probes = g_lq_last.probes;
  return FMX_OK;
}

}  // extern "C"
