// fmx_rank.hip -- ranked retrieval: the top-K documents of multi-term queries by BM25 (include/fmx.h).
//
//   postings   : the document listing's pipeline (fmx_corpus_dev.h, corpus_doc_keys) with the LAST byte of an occurrence as
//                its position (pat_len = 1), so terms of any lengths share one call: rows -> SA -> document -> the sorted keys
//                slot << doc_bits | doc, heads, their sum.  k_rank_df: df[t] = the distinct real documents of slot t, a
//                difference of two head counts.  The host reads df back, computes the weights and uploads them.
//   candidates : k_rank_postings writes one (key, value) per posting: query << (doc_bits + slot_bits) | doc << slot_bits |
//                slot in query, and the posting's index (its tf lies there); a posting without a document gets query =
//                n_queries and sorts behind all.  A second, much smaller radix sort.  k_rank_score: one lane per (query,
//                document) head walks its run (at most 64 postings, in slot order) and adds the terms up in that order
//                (fmx_rank_math.h: no FMA); under FMX_RANK_ALL a run shorter than the query is no candidate.  Flags, a
//                scan, k_rank_compact: per query a segment of (score key, doc), documents ascending.  No atomic decides an order.
//   selection  : k_rank_select, one workgroup per query.  A segment of at most 1024 candidates goes to LDS as it is; a
//                longer one goes through a radix select on the 64-bit score key, most significant byte first (LDS
//                histogram, counts only), which leaves a threshold, the keys above it and the first of its ties in segment
//                order (ballots and wave sums, never an atomic).  Then one bitonic sort in LDS by (key descending, doc
//                ascending) of at most 1024 pairs, and the scores go out as doubles again.
#include <fmx.h>

#include <cmath>
#include <string>
#include <vector>

#include "fmx_corpus_dev.h"
#include "fmx_order.h"
#include "fmx_rank_math.h"

namespace fmx {

constexpr int kRkThreads = 256;
constexpr uint32_t kRkLds = kRankMaxTop;            // pairs one workgroup holds and sorts
constexpr uint32_t kRkNoDoc = 0xffffffffu;          // the padding's document: behind every real one

// df[t] = the distinct documents of slot t, the "no document" key (doc == n_docs, last of its slot) not counted;
// df[n_terms] = all postings, that one included
__global__ __launch_bounds__(kRkThreads) void k_rank_df(const unsigned long long *__restrict__ key, uint64_t rows,
                                                        const uint32_t *__restrict__ incl, uint64_t n_terms, int doc_bits,
                                                        uint64_t n_docs, uint32_t *__restrict__ df) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_terms; t += stride) {
    if (t == n_terms) {
      df[t] = incl[rows - 1];
      continue;
    }
    const uint64_t lo = lower_bound(key, 0, rows, t << doc_bits);
    const uint64_t hi = lower_bound(key, lo, rows, (t << doc_bits) | n_docs);
    df[t] = (hi ? incl[hi - 1] : 0u) - (lo ? incl[lo - 1] : 0u);
  }
}

// One (candidate key, posting index) per head of the sorted row keys, and the posting's tf
__global__ __launch_bounds__(kRkThreads) void k_rank_postings(const unsigned long long *__restrict__ key, uint64_t rows,
                                                              const uint32_t *__restrict__ incl, int doc_bits, uint64_t n_docs,
                                                              const unsigned long long *__restrict__ q_off, uint64_t n_queries,
                                                              int slot_bits, unsigned long long *__restrict__ ckey,
                                                              uint32_t *__restrict__ cval, uint32_t *__restrict__ tf) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const int q_shift = doc_bits + slot_bits;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const unsigned long long kj = key[j];
    if (j && key[j - 1] == kj) continue;
    const uint64_t p = (uint64_t)incl[j] - 1;
    const uint64_t slot = kj >> doc_bits, d = kj & ((1ull << doc_bits) - 1);
    tf[p] = (uint32_t)(upper_bound(key, j, rows, kj) - j);
    const uint64_t q = upper_bound(q_off, 0, n_queries + 1, slot) - 1;      // q_off[0] = 0 <= slot < q_off[n_queries]
    ckey[p] = d >= n_docs ? (unsigned long long)n_queries << q_shift
                          : ((unsigned long long)q << q_shift) | ((unsigned long long)d << slot_bits) | (slot - q_off[q]);
    cval[p] = (uint32_t)p;
  }
}

struct RankScore {
  const uint32_t *doc_start, *doc_esc;
  const unsigned long long *q_off;
  const double *w;
  const uint32_t *tf;
  uint64_t n_queries;
  double avglen, k1, b;
  int doc_bits, slot_bits, all;
};

// flag[i] = 1 and skey[i] = the score's key where sorted posting i heads a (query, document) run that is a candidate
__global__ __launch_bounds__(kRkThreads) void k_rank_score(const unsigned long long *__restrict__ ckey,
                                                           const uint32_t *__restrict__ cval, uint64_t n_post, RankScore a,
                                                           uint32_t *__restrict__ flag, unsigned long long *__restrict__ skey) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const int q_shift = a.doc_bits + a.slot_bits;
  const unsigned long long slot_mask = (1ull << a.slot_bits) - 1, doc_mask = (1ull << a.doc_bits) - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_post; i += stride) {
    const unsigned long long k = ckey[i], run = k >> a.slot_bits;
    const uint64_t q = k >> q_shift;
    uint32_t f = 0;
    if (q < a.n_queries && (i == 0 || (ckey[i - 1] >> a.slot_bits) != run)) {
      const uint64_t d = run & doc_mask;
      const uint64_t len = (uint64_t)(a.doc_start[d + 1] - a.doc_start[d] - 1u) - (uint64_t)(a.doc_esc[d + 1] - a.doc_esc[d]);
      const double nd = rank_norm(len, a.avglen, a.k1, a.b);
      const uint64_t base = a.q_off[q], slots = a.q_off[q + 1] - base;
      double acc = 0.0;
      uint64_t seen = 0;
      for (uint64_t x = i; x < n_post && (ckey[x] >> a.slot_bits) == run; x++) {
        acc = rank_add(acc, rank_term(a.w[base + (ckey[x] & slot_mask)], a.tf[cval[x]], a.k1, nd));
        seen++;
      }
      if (!a.all || seen == slots) {
        f = 1;
        skey[i] = rank_key(acc);
      }
    }
    flag[i] = f;
  }
}

// incl = the inclusive sum of flag: the candidates in sorted order, (score key, doc)
__global__ __launch_bounds__(kRkThreads) void k_rank_compact(const unsigned long long *__restrict__ ckey,
                                                             const unsigned long long *__restrict__ skey,
                                                             const uint32_t *__restrict__ incl, uint64_t n_post, int doc_bits,
                                                             int slot_bits, unsigned long long *__restrict__ cand_key,
                                                             uint32_t *__restrict__ cand_doc) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_post; i += stride) {
    const uint32_t c = incl[i];
    if (c == (i ? incl[i - 1] : 0u)) continue;
    cand_key[c - 1] = skey[i];
    cand_doc[c - 1] = (uint32_t)((ckey[i] >> slot_bits) & ((1ull << doc_bits) - 1));
  }
}

// cand_off[q] = the candidates of the queries before q, q = 0 .. n_queries
__global__ __launch_bounds__(kRkThreads) void k_rank_cand_off(const unsigned long long *__restrict__ ckey,
                                                              const uint32_t *__restrict__ incl, uint64_t n_post,
                                                              uint64_t n_queries, int q_shift, uint32_t *__restrict__ cand_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n_queries; q += stride) {
    const uint64_t lb = lower_bound(ckey, 0, n_post, q << q_shift);         // (n_queries << q_shift fits: bits_for holds it)
    cand_off[q] = lb ? incl[lb - 1] : 0u;
  }
}

// sel[q] = min(top, candidates of q); sel[n_queries] = 0: its exclusive sum is where a query's results go
__global__ __launch_bounds__(kRkThreads) void k_rank_sel_count(const uint32_t *__restrict__ cand_off, uint64_t n_queries,
                                                               uint32_t top, uint32_t *__restrict__ sel) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= n_queries; q += stride) {
    const uint32_t c = q < n_queries ? cand_off[q + 1] - cand_off[q] : 0u;
    sel[q] = c < top ? c : top;
  }
}

// (key, doc) a stands before b: the larger score first, equal scores by document ascending
__device__ __forceinline__ bool rk_before(unsigned long long ka, uint32_t da, unsigned long long kb, uint32_t db) {
  return ka > kb || (ka == kb && da < db);
}

__global__ __launch_bounds__(kRkThreads) void k_rank_select(const unsigned long long *__restrict__ cand_key,
                                                            const uint32_t *__restrict__ cand_doc,
                                                            const uint32_t *__restrict__ cand_off,
                                                            const uint32_t *__restrict__ sel_off, uint64_t n_queries,
                                                            uint32_t top, uint64_t cap, unsigned long long *__restrict__ out_off,
                                                            uint32_t *__restrict__ out_doc, double *__restrict__ out_score) {
  __shared__ unsigned long long sk[kRkLds];
  __shared__ uint32_t sd[kRkLds];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[2][kRkThreads / 64];
  __shared__ unsigned long long s_prefix;
  __shared__ uint32_t s_need, s_done;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1;
  for (uint64_t q = blockIdx.x; q <= n_queries; q += gridDim.x) {           // every branch on q, C, m is uniform over the workgroup
    if (tid == 0) out_off[q] = sel_off[q];
    if (q == n_queries) continue;
    const uint64_t a = cand_off[q], C = (uint64_t)cand_off[q + 1] - a;
    const uint64_t o0 = sel_off[q];
    const uint32_t m = sel_off[q + 1] - sel_off[q];
    if (m == 0) continue;
    uint32_t cnt;
    if (C <= kRkLds) {
      for (uint64_t i = tid; i < C; i += kRkThreads) {
        sk[i] = cand_key[a + i];
        sd[i] = cand_doc[a + i];
      }
      cnt = (uint32_t)C;
    } else {
      // radix select: after a pass the keys that match `prefix` down to bit `shift` hold the threshold, and `need` of them
      // are still to be taken
      unsigned long long prefix = 0;
      uint32_t need = top;
      int shift = 56;
      for (;;) {
        hist[tid] = 0;
        __syncthreads();
        const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        for (uint64_t i = tid; i < C; i += kRkThreads) {
          const unsigned long long k = cand_key[a + i];
          if ((k & himask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          uint32_t above = 0, bin = 255;
          while (bin > 0 && above + hist[bin] < need) above += hist[bin--];
          s_prefix = prefix | ((unsigned long long)bin << shift);
          s_need = need - above;
          s_done = hist[bin] <= need - above ? 1u : 0u;             // every key of the bin is taken: nothing left to decide
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
        const bool done = s_done != 0 || shift == 0;
        __syncthreads();
        if (done) break;
        shift -= 8;
      }
      // the keys above the threshold, and the first `need` of its ties in segment order (ascending document)
      const unsigned long long pp = prefix >> shift;
      uint32_t taken = 0, ties = 0;
      for (uint64_t base = 0; base < C; base += kRkThreads) {
        const uint64_t i = base + tid;
        const bool valid = i < C;
        const unsigned long long k = valid ? cand_key[a + i] : 0ull;
        const uint32_t d = valid ? cand_doc[a + i] : 0u;
        const unsigned long long kk = k >> shift;
        const bool tie = valid && kk == pp;
        const unsigned long long bt = __ballot(tie);
        if (lane == 0) wsum[0][wave] = (uint32_t)__popcll(bt);
        __syncthreads();
        uint32_t trank = ties + (uint32_t)__popcll(bt & lt), tsum = 0;
        for (uint32_t w = 0; w < kRkThreads / 64; w++) {
          if (w < wave) trank += wsum[0][w];
          tsum += wsum[0][w];
        }
        const bool take = (valid && kk > pp) || (tie && trank < need);
        const unsigned long long bk = __ballot(take);
        if (lane == 0) wsum[1][wave] = (uint32_t)__popcll(bk);
        __syncthreads();
        uint32_t pos = taken + (uint32_t)__popcll(bk & lt), ksum = 0;
        for (uint32_t w = 0; w < kRkThreads / 64; w++) {
          if (w < wave) pos += wsum[1][w];
          ksum += wsum[1][w];
        }
        if (take && pos < kRkLds) {
          sk[pos] = k;
          sd[pos] = d;
        }
        ties += tsum;
        taken += ksum;
        __syncthreads();
      }
      cnt = taken < kRkLds ? taken : kRkLds;                        // == top
    }
    uint32_t M = 1;
    while (M < cnt) M <<= 1;
    for (uint32_t i = cnt + tid; i < M; i += kRkThreads) {          // the padding sorts behind every candidate
      sk[i] = 0ull;
      sd[i] = kRkNoDoc;
    }
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= M; k2 <<= 1) {
      for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
        for (uint32_t i = tid; i < M; i += kRkThreads) {
          const uint32_t l = i ^ j;
          if (l > i) {
            const unsigned long long ki = sk[i], kl = sk[l];
            const uint32_t di = sd[i], dl = sd[l];
            const bool swap = (i & k2) == 0 ? rk_before(kl, dl, ki, di) : rk_before(ki, di, kl, dl);
            if (swap) {
              sk[i] = kl;
              sd[i] = dl;
              sk[l] = ki;
              sd[l] = di;
            }
          }
        }
        __syncthreads();
      }
    }
    for (uint32_t r = tid; r < m; r += kRkThreads) {
      const uint64_t o = o0 + r;
      if (o < cap) {
        out_doc[o] = sd[r];
        out_score[o] = rank_unkey(sk[r]);
      }
    }
    __syncthreads();                                                // the next query overwrites the pairs
  }
}

// ---------------------------------------------------------------- host side
// The shapes of a call's term slots, for the ranking and the passages alike (fmx_corpus_dev.h): `noun` heads the messages
int rank_check_tables(const char *noun, const uint64_t *q_off, size_t n_queries, size_t n_terms, const double *weights,
                      uint64_t *max_slots) {
  const auto fail = [noun](const char *what) { return arg_fail((std::string(noun) + what).c_str()); };
  if (q_off[0] != 0 || !offsets_monotonic(q_off, 0, n_queries) || q_off[n_queries] != n_terms)
    return fail(": q_off must start at 0, never decrease and end at n_terms");
  uint64_t longest = 0;
  for (size_t q = 0; q < n_queries; q++) longest = std::max<uint64_t>(longest, q_off[q + 1] - q_off[q]);
  if (longest > kRankMaxSlots) return fail(": at most 64 term slots per query");
  if (weights)
    for (size_t t = 0; t < n_terms; t++)
      if (!std::isfinite(weights[t])) return fail(": the weights must be finite");
  *max_slots = longest;
  return FMX_OK;
}

int rank_check_sets(const char *noun, const uint64_t *set_off, size_t n_terms, size_t n_iv) {
  if (set_off[0] != 0 || !offsets_monotonic(set_off, 0, n_terms) || set_off[n_terms] != n_iv)
    return arg_fail((std::string(noun) + ": set_off must start at 0, never decrease and end at n_iv").c_str());
  return FMX_OK;
}

namespace {

struct RankLast {
  double ms[4] = {0.0, 0.0, 0.0, 0.0};              // locate, postings, score, select
  uint64_t rows = 0, postings = 0, candidates = 0;
};
thread_local RankLast g_rank_last;

int rank_check_params(const fmx_rank_params *p) {
  if (p->top < 1 || p->top > kRankMaxTop) return arg_fail("ranking: top must be 1 .. 1024");
  if (!std::isfinite(p->k1) || p->k1 < 0.0) return arg_fail("ranking: k1 must be finite and >= 0");
  if (!std::isfinite(p->b) || p->b < 0.0 || p->b > 1.0) return arg_fail("ranking: b must be in 0 .. 1");
  if (p->flags & ~FMX_RANK_ALL) return arg_fail("ranking: unknown flag");
  return FMX_OK;
}

// The call itself.  q_off and (when given) the weights are there twice: on the device for the kernels, on the host for
// the checks, which the caller has made (rank_check_tables).  d_weights == nullptr: the default weights from df.
// d_set_off != nullptr: n_iv intervals in n_terms slots (fmx_corpus_rank_sets); else n_iv == n_terms, a slot is an interval.
int rank_core(const Corpus *c, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
              const unsigned long long *d_set_off, size_t n_terms, const unsigned long long *d_q_off, size_t n_queries,
              uint64_t max_slots, const fmx_rank_params &prm,
              const double *d_weights, unsigned long long *d_out_off, uint32_t *d_out_doc, double *d_out_score, size_t cap,
              uint32_t *d_out_df, double *d_out_weight, hipStream_t st) {
  g_rank_last = RankLast{};
  const int doc_bits = bits_for(c->n_docs), slot_bits = bits_for(max_slots), q_bits = bits_for(n_queries);
  if (q_bits + doc_bits + slot_bits > 64) {
    set_error("ranking: the bits of " + std::to_string(n_queries) + " queries, " + std::to_string(c->n_docs) + " documents and " +
              std::to_string(max_slots) + " slots per query must fit a 64-bit key (" + std::to_string(q_bits + doc_bits + slot_bits) + " > 64)");
    return FMX_ERR_UNSUPPORTED;
  }
  int rc;
  Events<5> ev;
  Events<3> ev2;
  HIP_TRY(ev.create(), "hipEventCreate");
  HIP_TRY(ev2.create(), "hipEventCreate");
  DevMem mem;
  DocKeys dk;
  if ((rc = corpus_doc_keys(c, idx, d_sp, d_ep, n_iv, 1, prm.max_per, st, "ranking", mem, ev, dk, d_set_off, n_terms))) return rc;
  const uint64_t rows = dk.rows;
  // df, and with it the posting count, to the host: the weights are computed there
  if ((rc = device_room(12 * ((uint64_t)n_terms + 1) + 4096, "a ranking"))) return rc;
  uint32_t *d_df = nullptr;
  double *d_w = nullptr;
  DEV_ALLOC(mem, d_df, 4 * ((uint64_t)n_terms + 1), "rank");
  std::vector<uint32_t> df(n_terms + 1, 0u);
  if (rows) {
    LAUNCH("k_rank_df", k_rank_df, dim3(flat_grid(n_terms + 1)), dim3(kRkThreads), st, dk.ws.keys(), rows, dk.incl, (uint64_t)n_terms,
           doc_bits, c->n_docs, d_df);
    HIP_TRY(hipMemcpyAsync(df.data(), d_df, 4 * ((uint64_t)n_terms + 1), hipMemcpyDeviceToHost, st), "D2H(df)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  } else {
    HIP_TRY(hipMemsetAsync(d_df, 0, 4 * ((uint64_t)n_terms + 1), st), "hipMemset(df)");
  }
  const double *w = d_weights;
  if (!w) {
    DEV_ALLOC(mem, d_w, 8 * (uint64_t)n_terms, "rank");
    std::vector<double> hw(n_terms);
    for (size_t t = 0; t < n_terms; t++) hw[t] = rank_weight(c->n_docs, df[t]);
    if (n_terms) HIP_TRY(hipMemcpyAsync(d_w, hw.data(), 8 * (uint64_t)n_terms, hipMemcpyHostToDevice, st), "H2D(weights)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");       // hw goes when this block ends
    w = d_w;
  }
  if (d_out_df && n_terms) HIP_TRY(hipMemcpyAsync(d_out_df, d_df, 4 * (uint64_t)n_terms, hipMemcpyDeviceToDevice, st), "D2D(df)");
  if (d_out_weight && n_terms) HIP_TRY(hipMemcpyAsync(d_out_weight, w, 8 * (uint64_t)n_terms, hipMemcpyDeviceToDevice, st), "D2D(weights)");
  if (rows == 0) {
    HIP_TRY(hipMemsetAsync(d_out_off, 0, 8 * ((uint64_t)n_queries + 1), st), "hipMemset(out_off)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return FMX_OK;
  }
  const uint64_t n_post = df[n_terms];
  const uint64_t need = SortSpace::bytes(n_post) + 24 * n_post + 8 * ((uint64_t)n_queries + 2) + ScanSpace::bytes(n_queries + 1) + 8192;
  if ((rc = device_room(need, "a ranking"))) return rc;
  SortSpace ws;
  ScanSpace qscan;
  uint32_t *tf = nullptr, *cand_doc = nullptr, *cand_off = nullptr, *sel = nullptr;
  unsigned long long *skey = nullptr, *cand_key = nullptr;
  if ((rc = ws.alloc(mem, n_post, "rank")) || (rc = qscan.alloc(mem, n_queries + 1, "rank"))) return rc;
  DEV_ALLOC(mem, tf, 4 * n_post, "rank");
  DEV_ALLOC(mem, skey, 8 * n_post, "rank");
  DEV_ALLOC(mem, cand_key, 8 * n_post, "rank");
  DEV_ALLOC(mem, cand_doc, 4 * n_post, "rank");
  DEV_ALLOC(mem, cand_off, 4 * ((uint64_t)n_queries + 1), "rank");
  DEV_ALLOC(mem, sel, 4 * ((uint64_t)n_queries + 1), "rank");
  LAUNCH("k_rank_postings", k_rank_postings, dim3(flat_grid(rows, 8192)), dim3(kRkThreads), st, dk.ws.keys(), rows, dk.incl, doc_bits,
         c->n_docs, d_q_off, (uint64_t)n_queries, slot_bits, ws.keys(), ws.vals(), tf);
  HIP_TRY(ev2.record(0, st), "hipEventRecord");
  HIP_TRY(ws.sort(n_post, q_bits + doc_bits + slot_bits, st), "radix sort");
  RankScore sc{c->d_doc_start, c->d_doc_esc, d_q_off, w, tf, (uint64_t)n_queries,
               (double)(c->stream_len - c->n_docs - c->n_esc) / (double)c->n_docs, prm.k1, prm.b, doc_bits, slot_bits,
               (prm.flags & FMX_RANK_ALL) ? 1 : 0};
  uint32_t *flag = reinterpret_cast<uint32_t *>(ws.free_keys());    // the free key buffer holds the candidate flags
  LAUNCH("k_rank_score", k_rank_score, dim3(flat_grid(n_post, 8192)), dim3(kRkThreads), st, ws.keys(), ws.vals(), n_post, sc, flag, skey);
  HIP_TRY(ws.scan().sum(flag, n_post, false, st), "scan");
  LAUNCH("k_rank_compact", k_rank_compact, dim3(flat_grid(n_post, 8192)), dim3(kRkThreads), st, ws.keys(), skey, flag, n_post, doc_bits,
         slot_bits, cand_key, cand_doc);
  LAUNCH("k_rank_cand_off", k_rank_cand_off, dim3(flat_grid(n_queries + 1)), dim3(kRkThreads), st, ws.keys(), flag, n_post,
         (uint64_t)n_queries, doc_bits + slot_bits, cand_off);
  LAUNCH("k_rank_sel_count", k_rank_sel_count, dim3(flat_grid(n_queries + 1)), dim3(kRkThreads), st, cand_off, (uint64_t)n_queries,
         prm.top, sel);
  HIP_TRY(qscan.sum(sel, n_queries + 1, true, st), "scan");
  HIP_TRY(ev2.record(1, st), "hipEventRecord");
  const int cus = std::max(H(idx)->cu_count, 1);
  const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)n_queries + 1, (uint64_t)cus * 8);
  LAUNCH("k_rank_select", k_rank_select, dim3(grid), dim3(kRkThreads), st, cand_key, cand_doc, cand_off, sel, (uint64_t)n_queries, prm.top,
         (uint64_t)cap, d_out_off, d_out_doc, d_out_score);
  HIP_TRY(ev2.record(2, st), "hipEventRecord");
  uint32_t n_cand = 0;
  HIP_TRY(hipMemcpyAsync(&n_cand, cand_off + n_queries, 4, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
  float ms = 0;
  g_rank_last.ms[0] = ev.ms(0, 1);
  g_rank_last.ms[1] = hipEventElapsedTime(&ms, ev.ev[1], ev2.ev[0]) == hipSuccess ? ms : 0.0;
  g_rank_last.ms[2] = ev2.ms(0, 1);
  g_rank_last.ms[3] = ev2.ms(1, 2);
  g_rank_last.rows = rows;
  g_rank_last.postings = n_post;
  g_rank_last.candidates = n_cand;
  return FMX_OK;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_corpus_rank_last(double *locate_ms, double *postings_ms, double *score_ms, double *select_ms, uint64_t *rows,
                         uint64_t *postings, uint64_t *candidates) {
  const RankLast &l = g_rank_last;
  if (locate_ms) *locate_ms = l.ms[0];
  if (postings_ms) *postings_ms = l.ms[1];
  if (score_ms) *score_ms = l.ms[2];
  if (select_ms) *select_ms = l.ms[3];
  if (rows) *rows = l.rows;
  if (postings) *postings = l.postings;
  if (candidates) *candidates = l.candidates;
  return FMX_OK;
}

// both device forms: d_set_off == nullptr is fmx_corpus_rank_dev (n_iv == n_terms)
static int rank_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
                    const void *d_set_off, size_t n_terms, const void *d_q_off, size_t n_queries, const fmx_rank_params *params,
                    const void *d_weights, void *d_out_off, void *d_out_doc, void *d_out_score, size_t cap, void *d_out_df,
                    void *d_out_weight, void *stream) {
  if (!corpus || !idx || !params || !d_q_off || !d_out_off || (n_iv && (!d_sp || !d_ep)) || (cap && (!d_out_doc || !d_out_score)))
    return arg_fail("null argument");
  int rc = rank_check_params(params);
  if (rc) return rc;
  if ((uint64_t)n_queries >= 0xffffffffull) return arg_fail("ranking: too many queries");
  if ((uint64_t)n_terms >= 0xffffffffull) return arg_fail("ranking: too many slots");
  const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = corpus_index_check(c, idx, n_iv, st, "ranking"))) return rc;
  // the tables the checks read, on the host
  if (d_set_off) {
    std::vector<uint64_t> set_off(n_terms + 1);
    HIP_TRY(hipMemcpyAsync(set_off.data(), d_set_off, 8 * ((uint64_t)n_terms + 1), hipMemcpyDeviceToHost, st), "D2H(set_off)");
    HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if ((rc = rank_check_sets("ranking", set_off.data(), n_terms, n_iv))) return rc;
  }
  std::vector<uint64_t> q_off(n_queries + 1);
  std::vector<double> weights(d_weights ? n_terms : 0);
  HIP_TRY(hipMemcpyAsync(q_off.data(), d_q_off, 8 * ((uint64_t)n_queries + 1), hipMemcpyDeviceToHost, st), "D2H(q_off)");
  if (d_weights && n_terms) HIP_TRY(hipMemcpyAsync(weights.data(), d_weights, 8 * (uint64_t)n_terms, hipMemcpyDeviceToHost, st), "D2H(weights)");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  uint64_t max_slots = 0;
  if ((rc = rank_check_tables("ranking", q_off.data(), n_queries, n_terms, d_weights ? weights.data() : nullptr, &max_slots))) return rc;
  return rank_core(c, idx, d_sp, d_ep, n_iv, static_cast<const unsigned long long *>(d_set_off), n_terms,
                   static_cast<const unsigned long long *>(d_q_off), n_queries, max_slots, *params,
                   static_cast<const double *>(d_weights), static_cast<unsigned long long *>(d_out_off),
                   static_cast<uint32_t *>(d_out_doc), static_cast<double *>(d_out_score), cap, static_cast<uint32_t *>(d_out_df),
                   static_cast<double *>(d_out_weight), st);
}

int fmx_corpus_rank_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_terms,
                        const void *d_q_off, size_t n_queries, const fmx_rank_params *params, const void *d_weights,
                        void *d_out_off, void *d_out_doc, void *d_out_score, size_t cap, void *d_out_df, void *d_out_weight,
                        void *stream) {
  return rank_dev(corpus, idx, d_sp, d_ep, n_terms, nullptr, n_terms, d_q_off, n_queries, params, d_weights, d_out_off, d_out_doc,
                  d_out_score, cap, d_out_df, d_out_weight, stream);
}

int fmx_corpus_rank_sets_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t n_iv,
                             const void *d_set_off, size_t n_terms, const void *d_q_off, size_t n_queries,
                             const fmx_rank_params *params, const void *d_weights, void *d_out_off, void *d_out_doc,
                             void *d_out_score, size_t cap, void *d_out_df, void *d_out_weight, void *stream) {
  if (!d_set_off) return arg_fail("null argument");
  return rank_dev(corpus, idx, d_sp, d_ep, n_iv, d_set_off, n_terms, d_q_off, n_queries, params, d_weights, d_out_off, d_out_doc,
                  d_out_score, cap, d_out_df, d_out_weight, stream);
}

// both host forms: set_off == nullptr is fmx_corpus_rank (n_iv == n_terms)
static int rank_host(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_iv,
                     const uint64_t *set_off, size_t n_terms, const uint64_t *q_off, size_t n_queries, const fmx_rank_params *params,
                     const double *weights, uint64_t *out_off, uint32_t *out_doc, double *out_score, size_t cap, uint32_t *out_df,
                     double *out_weight) {
  if (!corpus || !idx || !params || !q_off || !out_off || (n_iv && (!sp || !ep)) || (cap && (!out_doc || !out_score)))
    return arg_fail("null argument");
  int rc = rank_check_params(params);
  if (rc) return rc;
  if ((uint64_t)n_queries >= 0xffffffffull) return arg_fail("ranking: too many queries");
  uint64_t max_slots = 0;
  if ((rc = rank_check_tables("ranking", q_off, n_queries, n_terms, weights, &max_slots))) return rc;
  if (set_off && (rc = rank_check_sets("ranking", set_off, n_terms, n_iv))) return rc;
  // everything above is decided before a handle or the device is touched
  const Corpus *c = reinterpret_cast<const Corpus *>(corpus);
  uint64_t n = 0;
  if ((rc = fmx_n(idx, &n))) return rc;
  for (size_t t = 0; t < n_iv; t++)
    if (sp[t] > n || ep[t] > n) return arg_fail("interval out of range (sp, ep <= n)");
  HostCall hc;
  if ((rc = hc.open())) return rc;
  if ((rc = corpus_index_check(c, idx, n_iv, hc.own.s, "ranking"))) return rc;
  const uint64_t nt = n_terms, nq = n_queries, ni = n_iv;
  if ((rc = device_room(16 * ni + 28 * nt + 8 * (nq + 1) + 8 * (nq + 1) + 12 * (uint64_t)cap + 8192, "a ranking"))) return rc;
  unsigned long long *d_sp = nullptr, *d_ep = nullptr, *d_q_off = nullptr, *d_off = nullptr, *d_set_off = nullptr;
  double *d_w = nullptr, *d_score = nullptr, *d_ow = nullptr;
  uint32_t *d_doc = nullptr, *d_df = nullptr;
  DEV_ALLOC(hc.mem, d_sp, 8 * ni, "rank");
  DEV_ALLOC(hc.mem, d_ep, 8 * ni, "rank");
  if (set_off) {
    DEV_ALLOC(hc.mem, d_set_off, 8 * (nt + 1), "rank");
    HIP_TRY(hipMemcpyAsync(d_set_off, set_off, 8 * (nt + 1), hipMemcpyHostToDevice, hc.own.s), "H2D(set_off)");
  }
  DEV_ALLOC(hc.mem, d_q_off, 8 * (nq + 1), "rank");
  DEV_ALLOC(hc.mem, d_off, 8 * (nq + 1), "rank");
  DEV_ALLOC(hc.mem, d_doc, 4 * (uint64_t)cap, "rank");
  DEV_ALLOC(hc.mem, d_score, 8 * (uint64_t)cap, "rank");
  DEV_ALLOC(hc.mem, d_df, 4 * nt, "rank");
  DEV_ALLOC(hc.mem, d_ow, 8 * nt, "rank");
  if (weights) DEV_ALLOC(hc.mem, d_w, 8 * nt, "rank");
  if (ni) {
    HIP_TRY(hipMemcpyAsync(d_sp, sp, 8 * ni, hipMemcpyHostToDevice, hc.own.s), "H2D(sp)");
    HIP_TRY(hipMemcpyAsync(d_ep, ep, 8 * ni, hipMemcpyHostToDevice, hc.own.s), "H2D(ep)");
  }
  if (nt && weights) HIP_TRY(hipMemcpyAsync(d_w, weights, 8 * nt, hipMemcpyHostToDevice, hc.own.s), "H2D(weights)");
  HIP_TRY(hipMemcpyAsync(d_q_off, q_off, 8 * (nq + 1), hipMemcpyHostToDevice, hc.own.s), "H2D(q_off)");
  if ((rc = rank_core(c, idx, d_sp, d_ep, n_iv, d_set_off, n_terms, d_q_off, n_queries, max_slots, *params, weights ? d_w : nullptr,
                      d_off, d_doc, d_score, cap, d_df, d_ow, hc.own.s)))
    return rc;
  if (nt) {
    if ((rc = hc.download(out_df, d_df, 4 * nt, "D2H(df)")) || (rc = hc.download(out_weight, d_ow, 8 * nt, "D2H(weights)"))) return rc;
  }
  if ((rc = hc.download(out_off, d_off, 8 * (nq + 1), "D2H(offsets)")) || (rc = hc.sync())) return rc;
  const uint64_t total = out_off[nq], m = std::min<uint64_t>(total, cap);
  if (m) {
    if ((rc = hc.download(out_doc, d_doc, 4 * m, "D2H(doc)")) || (rc = hc.download(out_score, d_score, 8 * m, "D2H(score)")) ||
        (rc = hc.sync()))
      return rc;
  }
  if (total > cap) return csr_overflow("corpus_rank", total, cap);
  return FMX_OK;
}

int fmx_corpus_rank(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_terms,
                    const uint64_t *q_off, size_t n_queries, const fmx_rank_params *params, const double *weights,
                    uint64_t *out_off, uint32_t *out_doc, double *out_score, size_t cap, uint32_t *out_df, double *out_weight) {
  return rank_host(corpus, idx, sp, ep, n_terms, nullptr, n_terms, q_off, n_queries, params, weights, out_off, out_doc, out_score, cap,
                   out_df, out_weight);
}

int fmx_corpus_rank_sets(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t n_iv,
                         const uint64_t *set_off, size_t n_terms, const uint64_t *q_off, size_t n_queries,
                         const fmx_rank_params *params, const double *weights, uint64_t *out_off, uint32_t *out_doc,
                         double *out_score, size_t cap, uint32_t *out_df, double *out_weight) {
  if (!set_off) return arg_fail("null argument");
  return rank_host(corpus, idx, sp, ep, n_iv, set_off, n_terms, q_off, n_queries, params, weights, out_off, out_doc, out_score, cap,
                   out_df, out_weight);
}

}  // extern "C"
