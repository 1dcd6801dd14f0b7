// fmx_passages.hip -- passages: the best window and the per-term counts of every ranked hit (include/fmx.h).
//
//   hit table : k_psg_hit_keys writes query << doc_bits | document with the hit's index as value; one radix sort; the shared
//               head flags and their sum say whether a (query, document) pair stands there twice (FMX_ERR_ARG).
//   locate    : the listing's first step (corpus_locate_count), then the rows themselves.
//   filter    : k_psg_keys, one lane per located row: row -> interval -> slot -> query, the document of the row's LAST byte
//               (the ranking's rule), a lower bound for (query, document) in the sorted hit keys.  A row of a document
//               that is no hit of its query -- nearly all of them -- is dropped here; the others get the key hit <<
//               (slot_bits + pos_bits) | slot in query << pos_bits | f in the place of their SA.  Flags, their sum,
//               k_psg_compact: the second sort is sized to the survivors.
//   window    : launch_csr_off cuts the sorted keys into the hits' segments.  k_psg_window: one wave64 per hit, four waves a
//               workgroup.  The first lanes find the slots' runs inside the segment (lower bounds; at most 65 bounds, in
//               LDS): their differences are the tf row.  Then the lanes stride over the segment's occurrences as window
//               starts; for every slot one lower bound for f >= a in the slot's run and one comparison of its end against
//               a + window (the first f >= a has the smallest end of its run, so it decides), the weights added in slot
//               order (fmx_passage_math.h: no FMA).  The wave's best comes from a shuffle reduction over psg_before, a
//               total order; lane 0 maps the window's ends through the corpus map and writes the record.  No atomic anywhere.
#include <fmx.h>

#include <cmath>
#include <string>
#include <vector>

#include "fmx_corpus_dev.h"
#include "fmx_order.h"
#include "fmx_passage_math.h"

namespace fmx {

constexpr int kPsgThreads = 256;
constexpr int kPsgWaves = kPsgThreads / 64;

// key[h] = query of h << doc_bits | hit_doc[h], val[h] = h
__global__ __launch_bounds__(kPsgThreads) void k_psg_hit_keys(const unsigned long long *__restrict__ hit_off, uint64_t n_queries,
                                                              const uint32_t *__restrict__ hit_doc, uint64_t n_hits, int doc_bits,
                                                              unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    const uint64_t q = upper_bound(hit_off, 0, n_queries + 1, h) - 1;      // hit_off[0] = 0 <= h < hit_off[n_queries]
    key[h] = psg_hit_key(q, hit_doc[h], doc_bits);
    val[h] = (uint32_t)h;
  }
}

struct PsgKeys {
  const uint32_t *doc_start;
  uint64_t n_docs, stream_len;
  const unsigned long long *loc_off, *set_off, *q_off;
  uint64_t k, n_terms, n_queries;
  const uint32_t *term_len;
  const unsigned long long *hkey;
  const uint32_t *hval;
  uint64_t n_hits;
  int doc_bits;
  PsgBits bits;
};

// pos[j]: the SA of located row j in, its occurrence key out; flag[j] = 1 where the row is an occurrence of a hit
__global__ __launch_bounds__(kPsgThreads) void k_psg_keys(PsgKeys a, unsigned long long *__restrict__ pos, uint64_t rows,
                                                          uint32_t *__restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const uint64_t sa = pos[j];
    unsigned long long key = 0;
    uint32_t keep = 0;
    if (sa < a.stream_len) {
      const uint64_t e = a.stream_len - 1 - sa;
      const uint64_t d = upper_bound(a.doc_start, 0, a.n_docs, e) - 1;   // doc_start[0] = 0 <= e: co_map's document
      const uint64_t i = upper_bound(a.loc_off, 0, a.k + 1, j) - 1;
      const uint64_t slot = a.set_off ? upper_bound(a.set_off, 0, a.n_terms + 1, i) - 1 : i;
      const uint64_t q = upper_bound(a.q_off, 0, a.n_queries + 1, slot) - 1;
      const uint64_t hk = psg_hit_key(q, d, a.doc_bits);
      const uint64_t x = lower_bound(a.hkey, 0, a.n_hits, hk);
      if (x < a.n_hits && a.hkey[x] == hk) {
        const uint64_t len = a.term_len[slot];
        if (e - a.doc_start[d] + 1 >= len) {                            // f >= doc_start[d]
          keep = 1;
          key = psg_key(a.hval[x], slot - a.q_off[q], e + 1 - len, a.bits);
        }
      }
    }
    pos[j] = key;
    flag[j] = keep;
  }
}

// incl = the inclusive sum of the flags: the kept keys, in row order
__global__ __launch_bounds__(kPsgThreads) void k_psg_compact(const unsigned long long *__restrict__ key,
                                                             const uint32_t *__restrict__ incl, uint64_t rows,
                                                             unsigned long long *__restrict__ okey, uint32_t *__restrict__ oval) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const uint32_t c = incl[j];
    if (c == (j ? incl[j - 1] : 0u)) continue;
    okey[c - 1] = key[j];
    oval[c - 1] = c - 1;
  }
}

struct PsgWin {
  const unsigned long long *key, *seg_off, *hit_off, *q_off;
  const uint32_t *term_len;
  const double *w;                                  // nullptr: 1.0 each
  CoMap m;
  uint64_t n_queries, n_hits, cap, stride, window;
  PsgBits bits;
  fmx_passage *out;
  uint32_t *out_tf;
};

__global__ __launch_bounds__(kPsgThreads) void k_psg_window(PsgWin p) {
  __shared__ uint32_t s_bnd[kPsgWaves][kRankMaxSlots + 1];          // where the slots' runs begin in the sorted keys
  __shared__ double s_w[kPsgWaves][kRankMaxSlots];
  __shared__ uint32_t s_len[kPsgWaves][kRankMaxSlots];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t todo = p.n_hits < p.cap ? p.n_hits : p.cap;        // nothing is written for a hit past the capacity
  // the trip count is the workgroup's: every wave meets every barrier
  for (uint64_t h0 = (uint64_t)blockIdx.x * kPsgWaves; h0 < todo; h0 += (uint64_t)gridDim.x * kPsgWaves) {
    const uint64_t h = h0 + wave;
    const bool active = h < todo;
    uint64_t lo = 0, hi = 0, ns = 0;
    if (active) {
      const uint64_t q = upper_bound(p.hit_off, 0, p.n_queries + 1, h) - 1;
      const uint64_t base = p.q_off[q];
      ns = p.q_off[q + 1] - base;
      lo = p.seg_off[h];
      hi = p.seg_off[h + 1];
      for (uint64_t j = lane; j <= ns; j += 64)
        s_bnd[wave][j] = (uint32_t)(j == ns ? hi : lower_bound(p.key, lo, hi, psg_key(h, j, 0, p.bits)));
      if (lane < ns) {
        s_w[wave][lane] = p.w ? p.w[base + lane] : 1.0;
        s_len[wave][lane] = p.term_len[base + lane];
      }
    }
    __syncthreads();
    if (active) {
      for (uint64_t j = lane; j < p.stride; j += 64) p.out_tf[h * p.stride + j] = j < ns ? s_bnd[wave][j + 1] - s_bnd[wave][j] : 0u;
      PsgBest best{0.0, 0, 0, 0};
      for (uint64_t i = lo + lane; i < hi; i += 64) {
        const uint64_t a = psg_key_pos(p.key[i], p.bits), end = a + p.window;
        PsgBest cur{0.0, a, 0, 1};
        for (uint32_t s = 0; s < (uint32_t)ns; s++) {
          const uint64_t r1 = s_bnd[wave][s + 1];
          const uint64_t x = lower_bound(p.key, s_bnd[wave][s], r1, psg_key(h, s, a, p.bits));
          if (x < r1 && psg_key_pos(p.key[x], p.bits) + s_len[wave][s] <= end) psg_cover(cur, s, s_w[wave][s]);
        }
        if (psg_before(cur, best)) best = cur;
      }
      for (int off = 32; off > 0; off >>= 1) {
        PsgBest o;
        o.value = __shfl_xor(best.value, off);
        o.a = __shfl_xor((unsigned long long)best.a, off);
        o.mask = __shfl_xor((unsigned long long)best.mask, off);
        o.valid = __shfl_xor(best.valid, off);
        if (psg_before(o, best)) best = o;
      }
      if (lane == 0) {
        fmx_passage rec{0, 0, 0.0, 0u, 0u};
        uint32_t d;
        uint64_t eo, ra, rb;
        if (best.valid && co_map(p.m, best.a, d, eo, ra)) {
          const uint64_t sep = (uint64_t)p.m.doc_start[d + 1] - 1;  // the separator of d: never part of a passage
          const uint64_t b = best.a + p.window < sep ? best.a + p.window : sep;
          uint32_t d2;
          rec.raw_off = ra;
          rec.mask = best.mask;
          rec.value = best.value;
          rec.raw_len = b > best.a && co_map(p.m, b - 1, d2, eo, rb) ? (uint32_t)(rb + 1 - ra) : 0u;
          rec.n_occ = (uint32_t)(hi - lo);
        }
        p.out[h] = rec;
      }
    }
    __syncthreads();                                                // the next round overwrites the bounds
  }
}

// ---------------------------------------------------------------- host side
namespace {

struct PsgLast {
  double ms[4] = {0.0, 0.0, 0.0, 0.0};              // locate, filter, sort, window
  uint64_t rows = 0, occ = 0, hits = 0;
};
thread_local PsgLast g_psg_last;

// What needs no handle: the parameters, the shapes of set_off / q_off / hit_off, term_len and the weights.
// *max_slots: the longest query's slots; *n_hits = hit_off[n_queries].
int psg_check(const fmx_passage_params *p, const uint64_t *set_off, size_t n_iv, size_t n_terms, const uint32_t *term_len,
              const uint64_t *q_off, size_t n_queries, const uint64_t *hit_off, const double *weights, uint64_t *max_slots,
              uint64_t *n_hits) {
  if (p->window < 1 || p->window > 0xffffffffull) return arg_fail("passages: window must be 1 .. 2^32 - 1");
  if (p->flags != 0 || p->reserved != 0) return arg_fail("passages: flags and reserved must be 0");
  if ((uint64_t)n_queries >= 0xffffffffull) return arg_fail("passages: too many queries");
  if ((uint64_t)n_terms >= 0xffffffffull) return arg_fail("passages: too many slots");
  int rc;
  if ((rc = rank_check_tables("passages", q_off, n_queries, n_terms, weights, max_slots))) return rc;
  if (set_off) {
    if ((rc = rank_check_sets("passages", set_off, n_terms, n_iv))) return rc;
  } else if (n_iv != n_terms) {
    return arg_fail("passages: without set_off a slot is an interval (n_iv == n_terms)");
  }
  if (hit_off[0] != 0 || !offsets_monotonic(hit_off, 0, n_queries)) return arg_fail("passages: hit_off must start at 0 and never decrease");
  if (hit_off[n_queries] >= 0xffffffffull) return arg_fail("passages: too many hits");
  for (size_t t = 0; t < n_terms; t++)
    if (term_len[t] < 1) return arg_fail("passages: term_len must be >= 1");
  *n_hits = hit_off[n_queries];
  return FMX_OK;
}

int psg_check_docs(const uint64_t *hit_off, size_t n_queries, const uint32_t *hit_doc, uint64_t n_docs) {
  for (size_t q = 0; q < n_queries; q++)
    for (uint64_t h = hit_off[q]; h < hit_off[q + 1]; h++)
      if (hit_doc[h] >= n_docs) {
        set_error("passages: hit " + std::to_string(h) + " (query " + std::to_string(q) + ", document " + std::to_string(hit_doc[h]) +
                  "): the corpus has " + std::to_string(n_docs) + " documents");
        return FMX_ERR_ARG;
      }
  return FMX_OK;
}

// all zeros for the first `m` hits: what a call without occurrences leaves
int psg_zero(fmx_passage *d_out, uint32_t *d_out_tf, uint64_t m, uint64_t stride, hipStream_t st) {
  if (m) HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(fmx_passage) * m, st), "hipMemset(passages)");
  if (m * stride) HIP_TRY(hipMemsetAsync(d_out_tf, 0, 4 * m * stride, st), "hipMemset(tf)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  return FMX_OK;
}

// The call itself, every array in device memory; the caller has made the checks (psg_check, psg_check_docs) on host copies.
int psg_core(const Corpus *c, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
             const unsigned long long *d_set_off, size_t n_terms, const uint32_t *d_term_len, const unsigned long long *d_q_off,
             size_t n_queries, const unsigned long long *d_hit_off, const uint32_t *d_hit_doc, uint64_t n_hits, uint64_t max_slots,
             const double *d_weights, const fmx_passage_params &prm, fmx_passage *d_out, uint32_t *d_out_tf, size_t cap,
             hipStream_t st) {
  g_psg_last = PsgLast{};
  g_psg_last.hits = n_hits;
  const uint64_t todo = std::min<uint64_t>(n_hits, cap);
  if (todo == 0) return FMX_OK;
  const PsgBits bits = psg_bits(n_hits, max_slots, c->stream_len);
  if (bits.total() > 64) {
    set_error("passages: the bits of " + std::to_string(n_hits) + " hits, " + std::to_string(max_slots) + " slots per query and a stream of " +
              std::to_string(c->stream_len) + " bytes must fit a 64-bit key (" + std::to_string(bits.total()) + " > 64)");
    return FMX_ERR_UNSUPPORTED;
  }
  const int doc_bits = bits_for(c->n_docs), q_bits = bits_for(n_queries);
  int rc;
  Events<5> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  // ---- the hit table
  if ((rc = device_room(SortSpace::bytes(n_hits) + 8192, "passages"))) return rc;
  SortSpace hs;
  if ((rc = hs.alloc(mem, n_hits, "passages"))) return rc;
  LAUNCH("k_psg_hit_keys", k_psg_hit_keys, dim3(flat_grid(n_hits)), dim3(kPsgThreads), st, d_hit_off, (uint64_t)n_queries, d_hit_doc, n_hits,
         doc_bits, hs.keys(), hs.vals());
  HIP_TRY(hs.sort(n_hits, q_bits + doc_bits, st), "radix sort");
  uint32_t *head = reinterpret_cast<uint32_t *>(hs.free_keys());    // the free key buffer holds the head flags
  HIP_TRY(launch_heads(hs.keys(), n_hits, head, st), "k_heads");
  HIP_TRY(hs.scan().sum(head, n_hits, false, st), "scan");
  uint32_t distinct = 0;
  HIP_TRY(hipMemcpyAsync(&distinct, head + (n_hits - 1), 4, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (distinct != n_hits) {
    std::vector<unsigned long long> hk(n_hits);
    HIP_TRY(hipMemcpyAsync(hk.data(), hs.keys(), 8 * n_hits, hipMemcpyDeviceToHost, st), "D2H(hit keys)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    for (uint64_t i = 1; i < n_hits; i++)
      if (hk[i] == hk[i - 1]) {
        set_error("passages: document " + std::to_string(hk[i] & ((1ull << doc_bits) - 1)) + " is a hit of query " +
                  std::to_string(hk[i] >> doc_bits) + " twice");
        return FMX_ERR_ARG;
      }
    return arg_fail("passages: a (query, document) pair twice");
  }
  // ---- locate
  unsigned long long *loc_off = nullptr, *pos = nullptr;
  uint64_t rows = 0;
  if ((rc = corpus_locate_count(idx, d_sp, d_ep, n_iv, prm.max_per, st, "passages", mem, &loc_off, &rows))) return rc;
  g_psg_last.rows = rows;
  if (rows == 0) return psg_zero(d_out, d_out_tf, todo, max_slots, st);
  if ((rc = device_room(12 * rows + ScanSpace::bytes(rows) + 8192, "passages"))) return rc;
  uint32_t *flag = nullptr;
  ScanSpace fscan;
  DEV_ALLOC(mem, pos, 8 * rows, "passages");
  DEV_ALLOC(mem, flag, 4 * rows, "passages");
  if ((rc = fscan.alloc(mem, rows, "passages"))) return rc;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if ((rc = fmx_locate_intervals_dev(idx, d_sp, d_ep, n_iv, prm.max_per, loc_off, pos, rows, st))) return rc;
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  // ---- filter and key
  const PsgKeys ka{c->d_doc_start, c->n_docs, c->stream_len, loc_off, d_set_off, d_q_off, (uint64_t)n_iv, (uint64_t)n_terms,
                   (uint64_t)n_queries, d_term_len, hs.keys(), hs.vals(), n_hits, doc_bits, bits};
  LAUNCH("k_psg_keys", k_psg_keys, dim3(flat_grid(rows, 8192)), dim3(kPsgThreads), st, ka, pos, rows, flag);
  HIP_TRY(fscan.sum(flag, rows, false, st), "scan");
  uint32_t n_occ = 0;
  HIP_TRY(hipMemcpyAsync(&n_occ, flag + (rows - 1), 4, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  g_psg_last.occ = n_occ;
  if (n_occ == 0) {
    g_psg_last.ms[0] = ev.ms(0, 1);
    return psg_zero(d_out, d_out_tf, todo, max_slots, st);
  }
  if ((rc = device_room(SortSpace::bytes(n_occ) + 8 * (n_hits + 1) + 8192, "passages"))) return rc;
  SortSpace os;
  unsigned long long *seg_off = nullptr;
  if ((rc = os.alloc(mem, n_occ, "passages"))) return rc;
  DEV_ALLOC(mem, seg_off, 8 * (n_hits + 1), "passages");
  LAUNCH("k_psg_compact", k_psg_compact, dim3(flat_grid(rows, 8192)), dim3(kPsgThreads), st, pos, flag, rows, os.keys(), os.vals());
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(os.sort(n_occ, bits.total(), st), "radix sort");
  HIP_TRY(ev.record(3, st), "hipEventRecord");
  // ---- segments and windows
  HIP_TRY(launch_csr_off(os.keys(), n_occ, n_hits, bits.hit_shift(), seg_off, st), "k_csr_off");
  const PsgWin wa{os.keys(), seg_off, d_hit_off, d_q_off, d_term_len, d_weights, c->map(), (uint64_t)n_queries, n_hits, (uint64_t)cap,
                  max_slots, prm.window, bits, d_out, d_out_tf};
  uint32_t grid = 1;
  HIP_TRY(resident_grid<k_psg_window>(H(idx), kPsgThreads, todo, kPsgWaves, &grid), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
  LAUNCH("k_psg_window", k_psg_window, dim3(grid), dim3(kPsgThreads), st, wa);
  HIP_TRY(ev.record(4, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
  for (int i = 0; i < 4; i++) g_psg_last.ms[i] = ev.ms(i, i + 1);
  return FMX_OK;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_corpus_passages_last(double *locate_ms, double *filter_ms, double *sort_ms, double *window_ms, uint64_t *rows,
                             uint64_t *occurrences, uint64_t *hits) {
  const PsgLast &l = g_psg_last;
  if (locate_ms) *locate_ms = l.ms[0];
  if (filter_ms) *filter_ms = l.ms[1];
  if (sort_ms) *sort_ms = l.ms[2];
  if (window_ms) *window_ms = l.ms[3];
  if (rows) *rows = l.rows;
  if (occurrences) *occurrences = l.occ;
  if (hits) *hits = l.hits;
  return FMX_OK;
}

int fmx_corpus_passages_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
                            const void *d_set_off, size_t n_terms, const void *d_term_len, const void *d_q_off,
                            size_t n_queries, const void *d_hit_off, const void *d_hit_doc, const void *d_weights,
                            const fmx_passage_params *params, void *d_out, void *d_out_tf, size_t cap, uint32_t *out_stride,
                            void *stream) {
  if (!corpus || !idx || !params || !d_q_off || !d_hit_off || !out_stride || (n_iv && (!d_sp || !d_ep)) || (n_terms && !d_term_len) ||
      (cap && (!d_out || !d_out_tf)))
    return arg_fail("null argument");
  if ((uint64_t)n_queries >= 0xffffffffull) return arg_fail("passages: too many queries");
  if ((uint64_t)n_terms >= 0xffffffffull) return arg_fail("passages: too many slots");
  const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = corpus_index_check(c, idx, n_iv, st, "passages"))) return rc;
  // the tables the checks read, on the host
  const uint64_t nt = n_terms, nq = n_queries;
  std::vector<uint64_t> set_off(d_set_off ? nt + 1 : 0), q_off(nq + 1), hit_off(nq + 1);
  std::vector<uint32_t> term_len(nt);
  std::vector<double> weights(d_weights ? nt : 0);
  if (d_set_off) HIP_TRY(hipMemcpyAsync(set_off.data(), d_set_off, 8 * (nt + 1), hipMemcpyDeviceToHost, st), "D2H(set_off)");
  HIP_TRY(hipMemcpyAsync(q_off.data(), d_q_off, 8 * (nq + 1), hipMemcpyDeviceToHost, st), "D2H(q_off)");
  HIP_TRY(hipMemcpyAsync(hit_off.data(), d_hit_off, 8 * (nq + 1), hipMemcpyDeviceToHost, st), "D2H(hit_off)");
  if (nt) HIP_TRY(hipMemcpyAsync(term_len.data(), d_term_len, 4 * nt, hipMemcpyDeviceToHost, st), "D2H(term_len)");
  if (d_weights && nt) HIP_TRY(hipMemcpyAsync(weights.data(), d_weights, 8 * nt, hipMemcpyDeviceToHost, st), "D2H(weights)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  uint64_t max_slots = 0, n_hits = 0;
  if ((rc = psg_check(params, d_set_off ? set_off.data() : nullptr, n_iv, n_terms, term_len.data(), q_off.data(), n_queries, hit_off.data(),
                      d_weights ? weights.data() : nullptr, &max_slots, &n_hits)))
    return rc;
  *out_stride = (uint32_t)max_slots;
  if (n_hits && !d_hit_doc) return arg_fail("null argument");
  std::vector<uint32_t> hit_doc(n_hits);
  if (n_hits) {
    HIP_TRY(hipMemcpyAsync(hit_doc.data(), d_hit_doc, 4 * n_hits, hipMemcpyDeviceToHost, st), "D2H(hit_doc)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  }
  if ((rc = psg_check_docs(hit_off.data(), n_queries, hit_doc.data(), c->n_docs))) return rc;
  if ((rc = psg_core(c, idx, d_sp, d_ep, n_iv, static_cast<const unsigned long long *>(d_set_off), n_terms,
                     static_cast<const uint32_t *>(d_term_len), static_cast<const unsigned long long *>(d_q_off), n_queries,
                     static_cast<const unsigned long long *>(d_hit_off), static_cast<const uint32_t *>(d_hit_doc), n_hits, max_slots,
                     static_cast<const double *>(d_weights), *params, static_cast<fmx_passage *>(d_out), static_cast<uint32_t *>(d_out_tf),
                     cap, st)))
    return rc;
  if (n_hits > cap) return csr_overflow("corpus_passages", n_hits, cap);
  return FMX_OK;
}

int fmx_corpus_passages(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_iv,
                        const uint64_t *set_off, size_t n_terms, const uint32_t *term_len, const uint64_t *q_off, size_t n_queries,
                        const uint64_t *hit_off, const uint32_t *hit_doc, const double *weights, const fmx_passage_params *params,
                        fmx_passage *out, uint32_t *out_tf, size_t cap, uint32_t *out_stride) {
  if (!corpus || !idx || !params || !q_off || !hit_off || !out_stride || (n_iv && (!sp || !ep)) || (n_terms && !term_len) ||
      (cap && (!out || !out_tf)))
    return arg_fail("null argument");
  int rc;
  uint64_t max_slots = 0, n_hits = 0;
  if ((rc = psg_check(params, set_off, n_iv, n_terms, term_len, q_off, n_queries, hit_off, weights, &max_slots, &n_hits))) return rc;
  if (n_hits && !hit_doc) return arg_fail("null argument");
  // everything above is decided before a handle or the device is touched
  *out_stride = (uint32_t)max_slots;
  const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
  uint64_t n = 0;
  if ((rc = fmx_n(idx, &n))) return rc;
  for (size_t t = 0; t < n_iv; t++)
    if (sp[t] > n || ep[t] > n) return arg_fail("interval out of range (sp, ep <= n)");
  HostCall hc;
  if ((rc = hc.open())) return rc;
  if ((rc = corpus_index_check(c, idx, n_iv, hc.own.s, "passages"))) return rc;
  if ((rc = psg_check_docs(hit_off, n_queries, hit_doc, c->n_docs))) return rc;
  const uint64_t nt = n_terms, nq = n_queries, ni = n_iv, m = std::min<uint64_t>(n_hits, cap);
  if ((rc = device_room(16 * ni + 8 * (nt + 1) + 12 * nt + 16 * (nq + 1) + 4 * n_hits + (32 + 4 * max_slots) * m + 8192, "passages"))) return rc;
  unsigned long long *d_sp = nullptr, *d_ep = nullptr, *d_set_off = nullptr, *d_q_off = nullptr, *d_hit_off = nullptr;
  uint32_t *d_term_len = nullptr, *d_hit_doc = nullptr, *d_tf = nullptr;
  double *d_w = nullptr;
  fmx_passage *d_out = nullptr;
  hipStream_t st = hc.own.s;
  DEV_ALLOC(hc.mem, d_sp, 8 * ni, "passages");
  DEV_ALLOC(hc.mem, d_ep, 8 * ni, "passages");
  DEV_ALLOC(hc.mem, d_term_len, 4 * nt, "passages");
  DEV_ALLOC(hc.mem, d_q_off, 8 * (nq + 1), "passages");
  DEV_ALLOC(hc.mem, d_hit_off, 8 * (nq + 1), "passages");
  DEV_ALLOC(hc.mem, d_hit_doc, 4 * n_hits, "passages");
  DEV_ALLOC(hc.mem, d_out, sizeof(fmx_passage) * m, "passages");
  DEV_ALLOC(hc.mem, d_tf, 4 * max_slots * m, "passages");
  if (set_off) {
    DEV_ALLOC(hc.mem, d_set_off, 8 * (nt + 1), "passages");
    HIP_TRY(hipMemcpyAsync(d_set_off, set_off, 8 * (nt + 1), hipMemcpyHostToDevice, st), "H2D(set_off)");
  }
  if (weights) {
    DEV_ALLOC(hc.mem, d_w, 8 * nt, "passages");
    if (nt) HIP_TRY(hipMemcpyAsync(d_w, weights, 8 * nt, hipMemcpyHostToDevice, st), "H2D(weights)");
  }
  if (ni) {
    HIP_TRY(hipMemcpyAsync(d_sp, sp, 8 * ni, hipMemcpyHostToDevice, st), "H2D(sp)");
    HIP_TRY(hipMemcpyAsync(d_ep, ep, 8 * ni, hipMemcpyHostToDevice, st), "H2D(ep)");
  }
  if (nt) HIP_TRY(hipMemcpyAsync(d_term_len, term_len, 4 * nt, hipMemcpyHostToDevice, st), "H2D(term_len)");
  HIP_TRY(hipMemcpyAsync(d_q_off, q_off, 8 * (nq + 1), hipMemcpyHostToDevice, st), "H2D(q_off)");
  HIP_TRY(hipMemcpyAsync(d_hit_off, hit_off, 8 * (nq + 1), hipMemcpyHostToDevice, st), "H2D(hit_off)");
  if (n_hits) HIP_TRY(hipMemcpyAsync(d_hit_doc, hit_doc, 4 * n_hits, hipMemcpyHostToDevice, st), "H2D(hit_doc)");
  if ((rc = psg_core(c, idx, d_sp, d_ep, n_iv, d_set_off, n_terms, d_term_len, d_q_off, n_queries, d_hit_off, d_hit_doc, n_hits, max_slots,
                     weights ? d_w : nullptr, *params, d_out, d_tf, cap, st)))
    return rc;
  if (m) {
    if ((rc = hc.download(out, d_out, sizeof(fmx_passage) * m, "D2H(passages)"))) return rc;
    if (max_slots && (rc = hc.download(out_tf, d_tf, 4 * max_slots * m, "D2H(tf)"))) return rc;
  }
  if ((rc = hc.sync())) return rc;
  if (n_hits > cap) return csr_overflow("corpus_passages", n_hits, cap);
  return FMX_OK;
}

}  // extern "C"
