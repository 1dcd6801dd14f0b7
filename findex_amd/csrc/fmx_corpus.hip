// fmx_corpus.hip -- a directory of files as ONE indexed stream, and the way back from a stream position to (file, offset).
//
// The reference's IndexerApp indexes a directory through DirBWTReader (bwtreader.scala:17-173): every file's bytes with
// three values escaped (raw 0 -> '\' '0', raw 1 -> '\' '1', raw 255 -> '\' 'f', :144-155; the backslash itself is not
// escaped), one separator byte 1 after every file (:133-137), and BWTMerger2.merge over that one stream.  Walking the
// tree and dropping binary files is host work (findex_amd/corpus.py); this unit does the rest on the device:
//
//   stream build : raw bytes of all documents back to back + their end offsets -> the escaped stream, doc_start[] (each
//                  document's first stream position, entry n_docs = the stream length) and esc_pos[] (the stream position
//                  of every escape's backslash, ascending).
//                  k_corpus_count : per tile of kCoTile raw bytes the number of escapes, and the first document whose end
//                                   lies at or behind the tile's first byte (a search in the end offsets).
//                  scan           : the exclusive sum of the escape counts (fmx_order.h, ScanSpace).
//                  k_corpus_emit  : a raw byte i goes to stream position i + #escapes before i + #documents ended at or
//                                   before i.  The escapes before i = the tile's scanned count + the lanes' counts scanned
//                                   over the wave and the block; the documents = a search per lane, then comparisons with
//                                   the next end.  The tile's output is staged in LDS and leaves in 16-byte stores.  A
//                                   raw-derived byte is never 1, so the stage starts as all separators and the bytes are
//                                   put on top: what stays is exactly the separators, any number of empty documents included.
//                  No atomics anywhere: the same input gives the same bytes on every run.
//   position map : k_corpus_map, two binary searches per position (doc_start, esc_pos); the escapes before each document's
//                  start are kept per document (k_corpus_doc_esc), so a document's own escapes are a difference.
//   doc listing  : rows of k intervals -> SA (fmx_locate_intervals_dev) -> text offsets -> documents (k_corpus_list_keys)
//                  -> radix sort of interval << bits | doc (fmx_order.h, SortSpace) -> heads, scan, compact.  Everything up
//                  to the scan is corpus_doc_keys (fmx_corpus_dev.h), which the ranking (fmx_rank.hip) calls too.
//
// Positions are u32 on the device (a stream has at most 2^32 - 2 bytes, the suffix sort's limit) and u64 at the ABI.
#include <fmx.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "fmx_corpus_dev.h"
#include "fmx_order.h"

namespace fmx {

constexpr int kCoThreads = 256;
constexpr uint32_t kCoTile = 4096;                   // raw bytes per tile: 16 per lane
constexpr uint32_t kCoStage = 3 * kCoTile;           // bytes of a tile's output staged at once (2 per raw byte + separators)
constexpr uint64_t kCoMaxStream = 0xfffffffeull;     // the suffix sort's limit (fmx_bwt_from_text)
constexpr uint32_t kCoPad = 0x61616161u;             // what a lane's bytes past the end of the raw text read as: no escape

__device__ __forceinline__ bool co_esc(uint32_t c) { return ((c + 1u) & 255u) <= 2u; }      // 0, 1, 255
__device__ __forceinline__ uint32_t co_letter(uint32_t c) { return c == 255u ? 'f' : '0' + c; }

// A lane's 16 raw bytes from `base` on: one 16-byte load where the text and the pointer allow it.  Returns how many are real.
__device__ __forceinline__ uint32_t co_load16(const uint8_t *__restrict__ raw, uint64_t base, uint64_t raw_len, int aligned,
                                              uint4 &v) {
  if (aligned && base + 16 <= raw_len) {
    v = *reinterpret_cast<const uint4 *>(raw + base);
    return 16;
  }
  uint32_t w[4] = {kCoPad, kCoPad, kCoPad, kCoPad};
  const uint32_t nb = base < raw_len ? (raw_len - base < 16 ? (uint32_t)(raw_len - base) : 16u) : 0u;
#pragma unroll
  for (int j = 0; j < 16; j++)
    if ((uint32_t)j < nb) w[j >> 2] = (w[j >> 2] & ~(255u << (8 * (j & 3)))) | ((uint32_t)raw[base + j] << (8 * (j & 3)));
  v = make_uint4(w[0], w[1], w[2], w[3]);
  return nb;
}

__device__ __forceinline__ uint32_t co_count16(const uint4 &v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) c += co_esc((w[j >> 2] >> (8 * (j & 3))) & 255u) ? 1u : 0u;
  return c;
}

// esc_cnt[t] = escapes in tile t (esc_cnt[ntiles] = 0: the scan leaves the total there); tile_doc[t] = the first document
// whose end offset is >= the tile's first byte.
__global__ __launch_bounds__(kCoThreads) void k_corpus_count(const uint8_t *__restrict__ raw, uint64_t raw_len, int aligned,
                                                             const unsigned long long *__restrict__ ends, uint64_t n_docs,
                                                             uint64_t ntiles, uint32_t *__restrict__ esc_cnt,
                                                             uint32_t *__restrict__ tile_doc) {
  __shared__ uint32_t ws[kCoThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t a = t * kCoTile;
    uint4 v;
    (void)co_load16(raw, a + (uint64_t)tid * 16, raw_len, aligned, v);
    uint32_t c = co_count16(v);
    for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0) ws[wave] = c;
    __syncthreads();
    if (tid == 0) {
      esc_cnt[t] = ws[0] + ws[1] + ws[2] + ws[3];
      tile_doc[t] = (uint32_t)lower_bound(ends, 0, n_docs, a);
      if (t == ntiles - 1) esc_cnt[ntiles] = 0;
    }
    __syncthreads();
  }
}

// esc_base: the exclusive sum of esc_cnt.  Tile t owns the separators of the documents tile_doc[t] .. tile_doc[t + 1] - 1
// (the last tile: all the rest, those that end where the raw text ends included).
__global__ __launch_bounds__(kCoThreads) void k_corpus_emit(const uint8_t *__restrict__ raw, uint64_t raw_len, int aligned,
                                                            const unsigned long long *__restrict__ ends, uint64_t n_docs,
                                                            uint64_t ntiles, const uint32_t *__restrict__ esc_base,
                                                            const uint32_t *__restrict__ tile_doc, uint8_t *__restrict__ out,
                                                            uint32_t *__restrict__ doc_start, uint32_t *__restrict__ esc_pos) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kCoStage + 16];
  __shared__ __attribute__((aligned(16))) uint8_t rawt[kCoTile];
  __shared__ uint32_t pre[kCoThreads + 1];
  __shared__ uint32_t wsum[kCoThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t a = t * kCoTile, b = a + kCoTile < raw_len ? a + kCoTile : raw_len;
    const uint64_t d_lo = tile_doc[t], d_hi = t + 1 == ntiles ? n_docs : (uint64_t)tile_doc[t + 1];
    const uint64_t base = a + (uint64_t)tid * 16;
    uint4 v;
    const uint32_t nb = co_load16(raw, base, raw_len, aligned, v);
    *reinterpret_cast<uint4 *>(rawt + tid * 16) = v;
    const uint32_t mine = co_count16(v);
    uint32_t incl = mine;                             // the lane's escapes, scanned over the wave, then over the block
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(incl, off);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0;
    for (int w = 0; w < kCoThreads / 64; w++) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    pre[tid] = before;
    if (tid == 0) pre[kCoThreads] = total;
    const uint32_t ebase = esc_base[t];
    const uint64_t out_base = a + ebase + d_lo;       // the stream position of the tile's first output byte
    const uint64_t tile_out = (b - a) + total + (d_hi - d_lo);
    // the lane's bytes: place in the tile's output = bytes and escapes before it + documents ended at or before it
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    uint32_t lp[16];
    {
      uint64_t d = nb ? upper_bound(ends, d_lo, d_hi, base) : d_hi;
      uint64_t next_end = d < d_hi ? (uint64_t)ends[d] : ~0ull;
      uint32_t run = (uint32_t)(base - a) + before, ne = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        lp[j] = 0;
        if ((uint32_t)j < nb) {
          const uint64_t i = base + j;
          if (next_end <= i) {
            d = upper_bound(ends, d, d_hi, i);
            next_end = d < d_hi ? (uint64_t)ends[d] : ~0ull;
          }
          const uint32_t c = (w4[j >> 2] >> (8 * (j & 3))) & 255u;
          lp[j] = run + (uint32_t)(d - d_lo);
          if (co_esc(c)) {
            esc_pos[(uint64_t)ebase + before + ne] = (uint32_t)(out_base + lp[j]);
            ne++;
            run++;
          }
          run++;
        }
      }
    }
    __syncthreads();                                  // rawt, pre
    // where the tile's documents start: one past each separator = end + escapes before the end + documents before + 1
    for (uint64_t d = d_lo + tid; d < d_hi; d += kCoThreads) {
      const uint64_t e = ends[d];
      const uint32_t r = (uint32_t)(e - a), u = r >> 4;
      uint32_t c = pre[u];
      for (uint32_t q = u * 16; q < r; q++) c += co_esc(rawt[q]) ? 1u : 0u;
      doc_start[d + 1] = (uint32_t)(e + ebase + c + d + 1);
    }
    if (t == 0 && tid == 0) doc_start[0] = 0;
    const uint32_t mis = (uint32_t)(out_base & 15u);  // stage[mis + x] is output byte x of the window: 16-byte stores line up
    for (uint64_t w0 = 0; w0 < tile_out; w0 += kCoStage) {
      const uint32_t wl = tile_out - w0 < kCoStage ? (uint32_t)(tile_out - w0) : kCoStage;
      for (uint32_t x = tid * 16; x < kCoStage + 16; x += kCoThreads * 16)
        *reinterpret_cast<uint4 *>(stage + x) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if ((uint32_t)j < nb) {
          const uint32_t c = (w4[j >> 2] >> (8 * (j & 3))) & 255u;
          const bool esc = co_esc(c);
          const uint64_t p0 = lp[j], p1 = p0 + 1;
          if (p0 >= w0 && p0 < w0 + wl) stage[mis + (uint32_t)(p0 - w0)] = esc ? (uint8_t)'\\' : (uint8_t)c;
          if (esc && p1 >= w0 && p1 < w0 + wl) stage[mis + (uint32_t)(p1 - w0)] = (uint8_t)co_letter(c);
        }
      }
      __syncthreads();
      uint8_t *g = out + (out_base + w0 - mis);
      for (uint32_t x = tid * 16; x < mis + wl; x += kCoThreads * 16) {
        if (x >= mis && x + 16 <= mis + wl) {
          *reinterpret_cast<uint4 *>(g + x) = *reinterpret_cast<const uint4 *>(stage + x);
        } else {
          for (uint32_t q = x; q < x + 16; q++)
            if (q >= mis && q < mis + wl) g[q] = stage[q];
        }
      }
      __syncthreads();
    }
  }
}

// doc_esc[d] = escapes in front of document d's first byte (d = n_docs: all of them)
__global__ __launch_bounds__(kCoThreads) void k_corpus_doc_esc(const uint32_t *__restrict__ doc_start, uint64_t n_docs,
                                                               const uint32_t *__restrict__ esc_pos, uint64_t n_esc,
                                                               uint32_t *__restrict__ doc_esc) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += stride)
    doc_esc[d] = (uint32_t)lower_bound(esc_pos, 0, n_esc, doc_start[d]);
}

__global__ __launch_bounds__(kCoThreads) void k_corpus_map(CoMap m, const unsigned long long *__restrict__ pos, uint64_t k,
                                                           uint32_t *__restrict__ doc, unsigned long long *__restrict__ esc_off,
                                                           unsigned long long *__restrict__ raw_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < k; q += stride) {
    uint32_t d = 0xffffffffu;
    uint64_t eo = ~0ull, ro = ~0ull;
    (void)co_map(m, pos[q], d, eo, ro);
    doc[q] = d;
    esc_off[q] = eo;
    raw_off[q] = ro;
  }
}

// ---- document listing.  sa[j] = SA of the j-th located row (off[] says which interval it belongs to); a pattern of
// pat_len stream bytes found at SA begins at stream position stream_len - pat_len - SA (fmx.h, locate).  A position that
// is no stream position sorts behind every document, as document n_docs, and is listed as UINT32_MAX.
__global__ __launch_bounds__(kCoThreads) void k_corpus_list_keys(CoMap m, const unsigned long long *__restrict__ sa, uint64_t rows,
                                                                 const unsigned long long *__restrict__ off, uint64_t k,
                                                                 uint64_t pat_len, int doc_bits,
                                                                 const unsigned long long *__restrict__ set_off, uint64_t n_slots,
                                                                 unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    uint64_t i = upper_bound(off, 0, k + 1, j) - 1;
    if (set_off) i = upper_bound(set_off, 0, n_slots + 1, i) - 1;      // the slot that holds interval i (set_off[0] = 0 <= i)
    const uint64_t s = sa[j];
    uint32_t d = (uint32_t)m.n_docs;
    uint64_t eo, ro;
    if (pat_len <= m.stream_len && s <= m.stream_len - pat_len) {
      uint32_t dd;
      if (co_map(m, m.stream_len - pat_len - s, dd, eo, ro)) d = dd;
    }
    key[j] = ((unsigned long long)i << doc_bits) | d;
    val[j] = (uint32_t)j;
  }
}

// incl = the inclusive sum of head.  out_off[i] = distinct (interval, document) pairs of the intervals before i
__global__ __launch_bounds__(kCoThreads) void k_corpus_list_off(const unsigned long long *__restrict__ key, uint64_t rows,
                                                                const uint32_t *__restrict__ incl, uint64_t k, int doc_bits,
                                                                unsigned long long *__restrict__ out_off) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= k; i += stride) {
    const uint64_t j = lower_bound(key, 0, rows, i << doc_bits);
    out_off[i] = j ? incl[j - 1] : 0u;
  }
}

__global__ __launch_bounds__(kCoThreads) void k_corpus_list_emit(const unsigned long long *__restrict__ key, uint64_t rows,
                                                                 const uint32_t *__restrict__ incl, int doc_bits, uint64_t n_docs,
                                                                 uint64_t cap, uint32_t *__restrict__ out_doc,
                                                                 uint32_t *__restrict__ out_cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const unsigned long long kj = key[j];
    if (j && key[j - 1] == kj) continue;
    const uint64_t slot = (uint64_t)incl[j] - 1;
    if (slot >= cap) continue;
    const uint64_t d = kj & ((1ull << doc_bits) - 1);
    out_doc[slot] = d >= n_docs ? 0xffffffffu : (uint32_t)d;
    out_cnt[slot] = (uint32_t)(upper_bound(key, j, rows, kj) - j);
  }
}

// ---------------------------------------------------------------- host side
namespace {

int co_arg(const char *msg) {
  set_error(msg);
  return FMX_ERR_ARG;
}

unsigned co_grid(uint64_t m) {
  const uint64_t b = (m + kCoThreads - 1) / kCoThreads;
  return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

int co_check_ends(const uint64_t *ends, uint64_t n_docs, uint64_t raw_len) {
  if (n_docs < 1) return co_arg("a corpus has at least one document");
  if (!ends) return co_arg("null argument");
  if (n_docs >= 0xffffffffull || raw_len > kCoMaxStream || raw_len + n_docs > kCoMaxStream) {
    set_error("corpus of " + std::to_string(raw_len) + " bytes in " + std::to_string(n_docs) +
              " documents: the stream takes at most 2^32 - 2 bytes (the suffix sort's limit)");
    return FMX_ERR_UNSUPPORTED;
  }
  uint64_t prev = 0;
  for (uint64_t d = 0; d < n_docs; d++) {
    if (ends[d] < prev) return co_arg("the documents' end offsets must not decrease");
    prev = ends[d];
  }
  if (prev != raw_len) return co_arg("the last document must end where the raw bytes end");
  return FMX_OK;
}

// The map's own tables from doc_start / esc_pos in device memory: takes ownership on success.
int co_finish(Corpus *c, hipStream_t st) {
  LAUNCH("k_corpus_doc_esc", k_corpus_doc_esc, dim3(co_grid(c->n_docs + 1)), dim3(kCoThreads), st, c->d_doc_start, c->n_docs, c->d_esc_pos,
         c->n_esc, c->d_doc_esc);
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  return FMX_OK;
}

// d_raw[raw_len] (device) + ends (host) -> a corpus.  `extra`: device bytes the caller holds beside (the raw text of the host form).
int co_build(const uint8_t *d_raw, uint64_t raw_len, const uint64_t *ends, uint64_t n_docs, int device, hipStream_t st,
             Corpus **out) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t ntiles = std::max<uint64_t>(1, (raw_len + kCoTile - 1) / kCoTile);
  const uint64_t tmp = 8 * n_docs + 4 * (ntiles + 1) + 4 * ntiles + ScanSpace::bytes(ntiles + 1);
  // the stream is raw_len + n_docs + escapes bytes: what is known before the count pass is checked now, the rest after it
  int rc = device_room(tmp + raw_len + n_docs + 8 * (n_docs + 1) + 4096, "the corpus stream");
  if (rc) return rc;
  DevMem mem;
  unsigned long long *d_ends = nullptr;
  uint32_t *esc_cnt = nullptr, *tile_doc = nullptr;
  ScanSpace scan;
  DEV_ALLOC(mem, d_ends, 8 * n_docs, "corpus");
  DEV_ALLOC(mem, esc_cnt, 4 * (ntiles + 1), "corpus");
  DEV_ALLOC(mem, tile_doc, 4 * ntiles, "corpus");
  if ((rc = scan.alloc(mem, ntiles + 1, "corpus"))) return rc;
  HIP_TRY(hipMemcpyAsync(d_ends, ends, 8 * n_docs, hipMemcpyHostToDevice, st), "H2D(ends)");
  const int aligned = (reinterpret_cast<uintptr_t>(d_raw) & 15u) == 0 ? 1 : 0;
  const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 4096);
  LAUNCH("k_corpus_count", k_corpus_count, dim3(grid), dim3(kCoThreads), st, d_raw, raw_len, aligned, d_ends, n_docs, ntiles, esc_cnt,
         tile_doc);
  HIP_TRY(scan.sum(esc_cnt, ntiles + 1, true, st), "scan");
  uint32_t n_esc = 0;
  HIP_TRY(hipMemcpyAsync(&n_esc, esc_cnt + ntiles, 4, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  const uint64_t stream_len = raw_len + n_esc + n_docs;
  if (stream_len > kCoMaxStream) {
    set_error("the corpus stream would be " + std::to_string(stream_len) + " bytes: at most 2^32 - 2 (the suffix sort's limit)");
    return FMX_ERR_UNSUPPORTED;
  }
  if ((rc = device_room(stream_len + 8 * (n_docs + 1) + 4 * (uint64_t)n_esc + 4096, "the corpus stream"))) return rc;
  std::unique_ptr<Corpus> c(new Corpus);
  c->device = device;
  c->n_docs = n_docs;
  c->stream_len = stream_len;
  c->n_esc = n_esc;
  hipError_t e = hipMalloc((void **)&c->d_stream, stream_len);
  if (e == hipSuccess) e = hipMalloc((void **)&c->d_doc_start, 4 * (n_docs + 1));
  if (e == hipSuccess) e = hipMalloc((void **)&c->d_doc_esc, 4 * (n_docs + 1));
  if (e == hipSuccess) e = hipMalloc((void **)&c->d_esc_pos, 4 * std::max<uint64_t>(n_esc, 1));
  if (e != hipSuccess) {
    set_error(std::string("hipMalloc(corpus): ") + hipGetErrorString(e));
    return FMX_ERR_NOMEM;
  }
  LAUNCH("k_corpus_emit", k_corpus_emit, dim3(grid), dim3(kCoThreads), st, d_raw, raw_len, aligned, d_ends, n_docs, ntiles, esc_cnt,
         tile_doc, c->d_stream, c->d_doc_start, c->d_esc_pos);
  if ((rc = co_finish(c.get(), st))) return rc;
  c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = c.release();
  return FMX_OK;
}

inline Corpus *C(fmx_corpus *p) { return reinterpret_cast<Corpus *>(p); }
inline const Corpus *C(const fmx_corpus *p) { return reinterpret_cast<const Corpus *>(p); }

int co_use(const Corpus *c) {
  HIP_TRY(hipSetDevice(c->device), "hipSetDevice");
  return FMX_OK;
}

}  // namespace

int corpus_index_check(const Corpus *c, const fmx_index *idx, size_t k, hipStream_t st, const char *noun) {
  uint64_t n = 0;
  int dev = -1, rc;
  if ((rc = fmx_n(idx, &n)) || (rc = fmx_device(idx, &dev))) return rc;
  if (n != c->stream_len + 1) return co_arg("the index is not the index of this corpus (n != stream length + 1)");
  if (dev != c->device) return co_arg("the index and the corpus live on different devices");
  if ((uint64_t)k >= 0xffffffffull) return co_arg("too many intervals");
  if ((rc = co_use(c))) return rc;
  return not_capturing(st, (std::string("a ") + noun).c_str());
}

int corpus_locate_count(const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, uint64_t max_per, hipStream_t st,
                        const char *noun, DevMem &mem, unsigned long long **loc_off, uint64_t *n_rows) {
  int rc;
  if ((rc = device_room(8 * ((uint64_t)k + 1) + 4096, std::string("a ") + noun))) return rc;
  DEV_ALLOC(mem, *loc_off, 8 * ((uint64_t)k + 1), "corpus");
  // the row counts first (no positions: cap 0), then room for exactly that many
  if ((rc = fmx_locate_intervals_dev(idx, d_sp, d_ep, k, max_per, *loc_off, nullptr, 0, st))) return rc;
  unsigned long long rows = 0;
  HIP_TRY(hipMemcpyAsync(&rows, *loc_off + k, 8, hipMemcpyDeviceToHost, st), "D2H");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rows >= 0xffffffffull) {
    set_error(std::string(noun) + " of " + std::to_string(rows) + " rows: at most 2^32 - 2 per call (use max_per)");
    return FMX_ERR_UNSUPPORTED;
  }
  *n_rows = rows;
  return FMX_OK;
}

int corpus_doc_keys(const Corpus *c, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, uint64_t pat_len,
                    uint64_t max_per, hipStream_t st, const char *noun, DevMem &mem, Events<5> &ev, DocKeys &out,
                    const unsigned long long *d_set_off, uint64_t n_slots) {
  const std::string what = std::string("a ") + noun;
  int rc;
  uint64_t rows = 0;
  if ((rc = corpus_locate_count(idx, d_sp, d_ep, k, max_per, st, noun, mem, &out.loc_off, &rows))) return rc;
  out.doc_bits = bits_for(c->n_docs);                               // documents 0 .. n_docs (n_docs: no document) fit
  out.rows = rows;
  if (rows == 0) return FMX_OK;
  const int k_bits = bits_for(d_set_off ? n_slots : (uint64_t)k);
  if ((rc = device_room(8 * rows + SortSpace::bytes(rows) + 8192, what))) return rc;
  unsigned long long *pos = nullptr;
  SortSpace &ws = out.ws;
  DEV_ALLOC(mem, pos, 8 * rows, "corpus");
  if ((rc = ws.alloc(mem, rows, "corpus"))) return rc;
  HIP_TRY(ev.record(0, st), "hipEventRecord");
  if ((rc = fmx_locate_intervals_dev(idx, d_sp, d_ep, k, max_per, out.loc_off, pos, rows, st))) return rc;
  HIP_TRY(ev.record(1, st), "hipEventRecord");
  LAUNCH("k_corpus_list_keys", k_corpus_list_keys, dim3(co_grid(rows)), dim3(kCoThreads), st, c->map(), pos, (uint64_t)rows, out.loc_off,
         (uint64_t)k, pat_len, out.doc_bits, d_set_off, n_slots, ws.keys(), ws.vals());
  HIP_TRY(ev.record(2, st), "hipEventRecord");
  HIP_TRY(ws.sort(rows, out.doc_bits + k_bits, st), "radix sort");
  HIP_TRY(ev.record(3, st), "hipEventRecord");
  uint32_t *head = reinterpret_cast<uint32_t *>(ws.free_keys());    // the free key buffer holds the head flags
  HIP_TRY(launch_heads(ws.keys(), rows, head, st), "k_corpus_list_heads");
  HIP_TRY(ws.scan().sum(head, rows, false, st), "scan");
  out.incl = head;
  return FMX_OK;
}

}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_corpus_build_dev(const void *d_raw, uint64_t raw_len, const uint64_t *doc_ends, uint64_t n_docs, int device,
                         void *stream, fmx_corpus **out) {
  if (!out) return co_arg("out is null");
  *out = nullptr;
  if (raw_len && !d_raw) return co_arg("null argument");
  int rc = co_check_ends(doc_ends, n_docs, raw_len);
  if (rc) return rc;
  if ((rc = use_device_index(device))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "a corpus build"))) return rc;
  Corpus *c = nullptr;
  if ((rc = co_build(static_cast<const uint8_t *>(d_raw), raw_len, doc_ends, n_docs, device, st, &c))) return rc;
  *out = reinterpret_cast<fmx_corpus *>(c);
  return FMX_OK;
}

int fmx_corpus_build(const uint8_t *raw, uint64_t raw_len, const uint64_t *doc_ends, uint64_t n_docs, int device,
                     fmx_corpus **out) {
  if (!out) return co_arg("out is null");
  *out = nullptr;
  if (raw_len && !raw) return co_arg("null argument");
  int rc = co_check_ends(doc_ends, n_docs, raw_len);
  if (rc) return rc;
  if ((rc = use_device_index(device))) return rc;
  if ((rc = device_room(2 * raw_len + 9 * n_docs + 4096, "the corpus stream"))) return rc;
  DevMem mem;
  StreamGuard own;
  HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
  uint8_t *d_raw = nullptr;
  DEV_ALLOC(mem, d_raw, raw_len, "corpus");
  if (raw_len) HIP_TRY(hipMemcpyAsync(d_raw, raw, raw_len, hipMemcpyHostToDevice, own.s), "H2D(raw)");
  Corpus *c = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = co_build(d_raw, raw_len, doc_ends, n_docs, device, own.s, &c))) return rc;
  c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = reinterpret_cast<fmx_corpus *>(c);
  return FMX_OK;
}

int fmx_corpus_free(fmx_corpus *corpus) {
  if (!corpus) return FMX_OK;
  Corpus *c = C(corpus);
  (void)hipSetDevice(c->device);
  delete c;
  return FMX_OK;
}

int fmx_corpus_info(const fmx_corpus *corpus, uint64_t *n_docs, uint64_t *stream_len, uint64_t *n_esc, uint64_t *bytes,
                    double *build_ms, uint32_t *tile_bytes) {
  const Corpus *c = C(corpus);
  if (n_docs) *n_docs = c ? c->n_docs : 0;
  if (stream_len) *stream_len = c ? c->stream_len : 0;
  if (n_esc) *n_esc = c ? c->n_esc : 0;
  if (bytes) *bytes = c ? c->bytes() : 0;
  if (build_ms) *build_ms = c ? c->build_ms : 0.0;
  if (tile_bytes) *tile_bytes = kCoTile;
  return FMX_OK;
}

int fmx_corpus_stream_dev(const fmx_corpus *corpus, const void **d_stream, uint64_t *stream_len) {
  if (!corpus || !d_stream) return co_arg("null argument");
  const Corpus *c = C(corpus);
  if (!c->d_stream) return co_arg("the corpus holds no stream (dropped, or made from tables)");
  *d_stream = c->d_stream;
  if (stream_len) *stream_len = c->stream_len;
  return FMX_OK;
}

int fmx_corpus_stream(const fmx_corpus *corpus, uint8_t *out, uint64_t cap) {
  if (!corpus || !out) return co_arg("null argument");
  const Corpus *c = C(corpus);
  if (!c->d_stream) return co_arg("the corpus holds no stream (dropped, or made from tables)");
  if (cap < c->stream_len) {
    set_error("corpus stream: " + std::to_string(c->stream_len) + " bytes, room for " + std::to_string(cap));
    return FMX_ERR_OVERFLOW;
  }
  int rc = co_use(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, c->d_stream, c->stream_len, hipMemcpyDeviceToHost), "D2H(stream)");
  return FMX_OK;
}

int fmx_corpus_drop_stream(fmx_corpus *corpus) {
  if (!corpus) return co_arg("null argument");
  Corpus *c = C(corpus);
  if (c->d_stream) {
    (void)hipSetDevice(c->device);
    (void)hipFree(c->d_stream);
    c->d_stream = nullptr;
  }
  return FMX_OK;
}

int fmx_corpus_open_index(const fmx_corpus *corpus, void *stream, fmx_index **out) {
  if (!out) return co_arg("out is null");
  *out = nullptr;
  if (!corpus) return co_arg("null argument");
  const Corpus *c = C(corpus);
  if (!c->d_stream) return co_arg("the corpus holds no stream (dropped, or made from tables)");
  int rc = co_use(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "index construction"))) return rc;
  const uint64_t n = c->stream_len + 1;
  if ((rc = device_room(sufsort_peak_bytes(c->stream_len, false) + n, "the index of the corpus stream"))) return rc;
  DevMem mem;
  uint8_t *d_bwt = nullptr;
  DEV_ALLOC(mem, d_bwt, n, "corpus");
  uint64_t eof = 0;
  int64_t counts[256];
  if ((rc = fmx_bwt_from_text_dev(c->d_stream, c->stream_len, d_bwt, nullptr, &eof, counts, c->device, stream))) return rc;
  return fmx_open_dev(d_bwt, n, eof, counts, c->device, stream, out);
}

int fmx_corpus_tables(const fmx_corpus *corpus, uint64_t *doc_start, uint64_t *raw_len, uint64_t *esc_pos) {
  if (!corpus) return co_arg("null argument");
  const Corpus *c = C(corpus);
  int rc = co_use(c);
  if (rc) return rc;
  std::vector<uint32_t> ds(c->n_docs + 1), de(c->n_docs + 1);
  HIP_TRY(hipMemcpy(ds.data(), c->d_doc_start, 4 * (c->n_docs + 1), hipMemcpyDeviceToHost), "D2H(doc_start)");
  HIP_TRY(hipMemcpy(de.data(), c->d_doc_esc, 4 * (c->n_docs + 1), hipMemcpyDeviceToHost), "D2H(doc_esc)");
  for (uint64_t d = 0; d <= c->n_docs; d++) {
    if (doc_start) doc_start[d] = ds[d];
    if (raw_len && d < c->n_docs) raw_len[d] = (uint64_t)(ds[d + 1] - ds[d] - 1) - (de[d + 1] - de[d]);
  }
  if (esc_pos && c->n_esc) {
    std::vector<uint32_t> ep(c->n_esc);
    HIP_TRY(hipMemcpy(ep.data(), c->d_esc_pos, 4 * c->n_esc, hipMemcpyDeviceToHost), "D2H(esc_pos)");
    for (uint64_t i = 0; i < c->n_esc; i++) esc_pos[i] = ep[i];
  }
  return FMX_OK;
}

int fmx_corpus_from_tables(const uint64_t *doc_start, const uint64_t *raw_len, const uint64_t *esc_pos, uint64_t n_docs,
                           uint64_t n_esc, int device, fmx_corpus **out) {
  if (!out) return co_arg("out is null");
  *out = nullptr;
  if (!doc_start || !raw_len || (n_esc && !esc_pos)) return co_arg("null argument");
  if (n_docs < 1) return co_arg("a corpus has at least one document");
  auto bad = [](const std::string &m) { set_error("corpus tables: " + m); return (int)FMX_ERR_FORMAT; };
  if (n_docs >= 0xffffffffull) return bad("too many documents");
  if (doc_start[0] != 0) return bad("doc_start[0] is not 0");
  if (doc_start[n_docs] > kCoMaxStream || n_esc > doc_start[n_docs]) return bad("the stream is longer than 2^32 - 2 bytes, or has more escapes than bytes");
  std::vector<uint32_t> ds(n_docs + 1), ep(std::max<uint64_t>(n_esc, 1));
  for (uint64_t i = 0; i < n_esc; i++) {
    if ((i && esc_pos[i] < esc_pos[i - 1] + 2) || esc_pos[i] + 2 >= doc_start[n_docs]) return bad("esc_pos is not ascending inside the stream");
    ep[i] = (uint32_t)esc_pos[i];
  }
  uint64_t e = 0;
  for (uint64_t d = 0; d < n_docs; d++) {
    if (doc_start[d + 1] <= doc_start[d]) return bad("doc_start is not strictly increasing");
    uint64_t in_doc = 0;
    while (e < n_esc && esc_pos[e] < doc_start[d + 1]) {
      if (esc_pos[e] + 2 >= doc_start[d + 1]) return bad("an escape runs into a separator");
      e++;
      in_doc++;
    }
    if (raw_len[d] != doc_start[d + 1] - doc_start[d] - 1 - in_doc) return bad("raw_len of document " + std::to_string(d) + " disagrees with doc_start and esc_pos");
    ds[d] = (uint32_t)doc_start[d];
  }
  ds[n_docs] = (uint32_t)doc_start[n_docs];
  int rc = use_device_index(device);
  if (rc) return rc;
  if ((rc = device_room(8 * (n_docs + 1) + 4 * n_esc + 4096, "the corpus map"))) return rc;
  std::unique_ptr<Corpus> c(new Corpus);
  c->device = device;
  c->n_docs = n_docs;
  c->n_esc = n_esc;
  c->stream_len = doc_start[n_docs];
  hipError_t he = hipMalloc((void **)&c->d_doc_start, 4 * (n_docs + 1));
  if (he == hipSuccess) he = hipMalloc((void **)&c->d_doc_esc, 4 * (n_docs + 1));
  if (he == hipSuccess) he = hipMalloc((void **)&c->d_esc_pos, 4 * ep.size());
  if (he != hipSuccess) {
    set_error(std::string("hipMalloc(corpus): ") + hipGetErrorString(he));
    return FMX_ERR_NOMEM;
  }
  HIP_TRY(hipMemcpy(c->d_doc_start, ds.data(), 4 * ds.size(), hipMemcpyHostToDevice), "H2D(doc_start)");
  HIP_TRY(hipMemcpy(c->d_esc_pos, ep.data(), 4 * ep.size(), hipMemcpyHostToDevice), "H2D(esc_pos)");
  if ((rc = co_finish(c.get(), nullptr))) return rc;
  *out = reinterpret_cast<fmx_corpus *>(c.release());
  return FMX_OK;
}

int fmx_corpus_map_dev(const fmx_corpus *corpus, const void *d_pos, size_t k, void *d_doc, void *d_esc_off, void *d_raw_off,
                       void *stream) {
  if (!corpus || (k && (!d_pos || !d_doc || !d_esc_off || !d_raw_off))) return co_arg("null argument");
  const Corpus *c = C(corpus);
  int rc = co_use(c);
  if (rc || !k) return rc;
  LAUNCH("k_corpus_map", k_corpus_map, dim3(co_grid(k)), dim3(kCoThreads), (hipStream_t)stream, c->map(),
         static_cast<const unsigned long long *>(d_pos), (uint64_t)k, static_cast<uint32_t *>(d_doc),
         static_cast<unsigned long long *>(d_esc_off), static_cast<unsigned long long *>(d_raw_off));
  return FMX_OK;
}

int fmx_corpus_map(const fmx_corpus *corpus, const uint64_t *pos, size_t k, uint32_t *doc, uint64_t *esc_off, uint64_t *raw_off) {
  if (!corpus || (k && (!pos || !doc || !esc_off || !raw_off))) return co_arg("null argument");
  const Corpus *c = C(corpus);
  int rc = co_use(c);
  if (rc || !k) return rc;
  if ((rc = device_room(28 * (uint64_t)k + 4096, "a corpus map call"))) return rc;
  DevMem mem;
  unsigned long long *d_pos = nullptr, *d_eo = nullptr, *d_ro = nullptr;
  uint32_t *d_doc = nullptr;
  DEV_ALLOC(mem, d_pos, 8 * k, "corpus");
  DEV_ALLOC(mem, d_eo, 8 * k, "corpus");
  DEV_ALLOC(mem, d_ro, 8 * k, "corpus");
  DEV_ALLOC(mem, d_doc, 4 * k, "corpus");
  HIP_TRY(hipMemcpy(d_pos, pos, 8 * k, hipMemcpyHostToDevice), "H2D(pos)");
  if ((rc = fmx_corpus_map_dev(corpus, d_pos, k, d_doc, d_eo, d_ro, nullptr))) return rc;
  HIP_TRY(hipMemcpy(doc, d_doc, 4 * k, hipMemcpyDeviceToHost), "D2H(doc)");
  HIP_TRY(hipMemcpy(esc_off, d_eo, 8 * k, hipMemcpyDeviceToHost), "D2H(esc_off)");
  HIP_TRY(hipMemcpy(raw_off, d_ro, 8 * k, hipMemcpyDeviceToHost), "D2H(raw_off)");
  return FMX_OK;
}

static thread_local double g_list_phases[4] = {0.0, 0.0, 0.0, 0.0};

int fmx_corpus_doc_list_phases(double *locate_ms, double *map_ms, double *sort_ms, double *compact_ms) {
  if (locate_ms) *locate_ms = g_list_phases[0];
  if (map_ms) *map_ms = g_list_phases[1];
  if (sort_ms) *sort_ms = g_list_phases[2];
  if (compact_ms) *compact_ms = g_list_phases[3];
  return FMX_OK;
}

int fmx_corpus_doc_list_dev(const fmx_corpus *corpus, const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k,
                            uint64_t pat_len, uint64_t max_per, void *d_out_off, void *d_out_doc, void *d_out_cnt, size_t cap,
                            void *stream) {
  if (!corpus || !idx || !d_out_off || (k && (!d_sp || !d_ep)) || (cap && (!d_out_doc || !d_out_cnt))) return co_arg("null argument");
  const Corpus *c = C(corpus);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = corpus_index_check(c, idx, k, st, "document listing"))) return rc;
  Events<5> ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  DevMem mem;
  DocKeys dk;
  if ((rc = corpus_doc_keys(c, idx, d_sp, d_ep, k, pat_len, max_per, st, "document listing", mem, ev, dk))) return rc;
  const uint64_t rows = dk.rows;
  if (rows == 0) {
    LAUNCH("k_corpus_list_off", k_corpus_list_off, dim3(co_grid(k + 1)), dim3(kCoThreads), st, nullptr, 0ull, nullptr, (uint64_t)k,
           dk.doc_bits, static_cast<unsigned long long *>(d_out_off));
    for (double &p : g_list_phases) p = 0.0;
    return FMX_OK;
  }
  const unsigned long long *key = dk.ws.keys();
  LAUNCH("k_corpus_list_off", k_corpus_list_off, dim3(co_grid(k + 1)), dim3(kCoThreads), st, key, (uint64_t)rows, dk.incl, (uint64_t)k,
         dk.doc_bits, static_cast<unsigned long long *>(d_out_off));
  if (cap) {
    LAUNCH("k_corpus_list_emit", k_corpus_list_emit, dim3(co_grid(rows)), dim3(kCoThreads), st, key, (uint64_t)rows, dk.incl, dk.doc_bits,
           c->n_docs, (uint64_t)cap, static_cast<uint32_t *>(d_out_doc), static_cast<uint32_t *>(d_out_cnt));
  }
  HIP_TRY(ev.record(4, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");        // the temporaries go when this returns
  for (int i = 0; i < 4; i++) g_list_phases[i] = ev.ms(i, i + 1);
  return FMX_OK;
}

int fmx_corpus_doc_list(const fmx_corpus *corpus, const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t k,
                        uint64_t pat_len, uint64_t max_per, uint64_t *out_off, uint32_t *out_doc, uint32_t *out_cnt, size_t cap) {
  if (!corpus || !idx || !out_off || (k && (!sp || !ep)) || (cap && (!out_doc || !out_cnt))) return co_arg("null argument");
  const Corpus *c = C(corpus);
  uint64_t n = 0;
  int rc = fmx_n(idx, &n);
  if (rc) return rc;
  for (size_t i = 0; i < k; i++)
    if (sp[i] > n || ep[i] > n) return co_arg("interval out of range (sp, ep <= n)");
  if ((rc = co_use(c))) return rc;
  if ((rc = device_room(24 * (uint64_t)k + 8 * (uint64_t)cap + 8192, "a document listing"))) return rc;
  DevMem mem;
  StreamGuard own;
  HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
  unsigned long long *d_sp = nullptr, *d_ep = nullptr, *d_off = nullptr;
  uint32_t *d_doc = nullptr, *d_cnt = nullptr;
  DEV_ALLOC(mem, d_sp, 8 * k, "corpus");
  DEV_ALLOC(mem, d_ep, 8 * k, "corpus");
  DEV_ALLOC(mem, d_off, 8 * (k + 1), "corpus");
  DEV_ALLOC(mem, d_doc, 4 * cap, "corpus");
  DEV_ALLOC(mem, d_cnt, 4 * cap, "corpus");
  if (k) {
    HIP_TRY(hipMemcpyAsync(d_sp, sp, 8 * k, hipMemcpyHostToDevice, own.s), "H2D(sp)");
    HIP_TRY(hipMemcpyAsync(d_ep, ep, 8 * k, hipMemcpyHostToDevice, own.s), "H2D(ep)");
  }
  if ((rc = fmx_corpus_doc_list_dev(corpus, idx, d_sp, d_ep, k, pat_len, max_per, d_off, d_doc, d_cnt, cap, own.s))) return rc;
  HIP_TRY(hipMemcpyAsync(out_off, d_off, 8 * (k + 1), hipMemcpyDeviceToHost, own.s), "D2H(off)");
  HIP_TRY(hipStreamSynchronize(own.s), "hipStreamSynchronize");
  const uint64_t total = out_off[k], m = std::min<uint64_t>(total, cap);
  if (m) {
    HIP_TRY(hipMemcpyAsync(out_doc, d_doc, 4 * m, hipMemcpyDeviceToHost, own.s), "D2H(doc)");
    HIP_TRY(hipMemcpyAsync(out_cnt, d_cnt, 4 * m, hipMemcpyDeviceToHost, own.s), "D2H(cnt)");
    HIP_TRY(hipStreamSynchronize(own.s), "hipStreamSynchronize");
  }
  if (total > cap) {
    set_error("corpus_doc_list: " + std::to_string(total) + " (interval, document) pairs, room for " + std::to_string(cap));
    return FMX_ERR_OVERFLOW;
  }
  return FMX_OK;
}

int fmx_corpus_escape(const uint8_t *in, size_t len, uint8_t *out, size_t cap, size_t *out_len) {
  if ((len && !in) || !out_len || (cap && !out)) return co_arg("null argument");
  size_t need = len;
  for (size_t i = 0; i < len; i++) need += in[i] <= 1 || in[i] == 255 ? 1 : 0;
  *out_len = need;
  if (need > cap) {
    set_error("corpus_escape: " + std::to_string(need) + " bytes, room for " + std::to_string(cap));
    return FMX_ERR_OVERFLOW;
  }
  size_t o = 0;
  for (size_t i = 0; i < len; i++) {
    const uint8_t ch = in[i];
    if (ch <= 1 || ch == 255) {
      out[o++] = '\\';
      out[o++] = ch == 255 ? 'f' : (uint8_t)('0' + ch);
    } else {
      out[o++] = ch;
    }
  }
  return FMX_OK;
}

}  // extern "C"
