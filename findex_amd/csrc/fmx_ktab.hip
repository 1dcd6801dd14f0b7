// fmx_ktab.hip -- the k-mer jump table: the first K backward steps of a search as ONE lookup.
//
// SuffixAlgo.search (findex.scala:15-31) starts every pattern from (0, n) and its first steps depend on nothing but
// the pattern's last characters: the interval after K steps is a function of the K-mer.  The reference's kernels
// already answer step 0 from C[] alone; this generalises that shortcut (the "ftab" of short-read aligners):
//     T[code] = (sp, ep, steps) after consuming the K symbols of `code`, most significant digit first,
// with symbols numbered densely over the ones that occur in the BWT (sigma' of them) and
// code = ((d0 * sigma' + d1) * sigma' + ...) + d(K-1), d0 = the pattern's LAST character.  A K-mer that does not occur
// keeps what the reference's loop holds when it stops -- the (sp, ep) of the first empty step and the number of
// steps taken -- so a miss returns the reference's values and counts the reference's steps.
//
// K is the largest with sigma'^K <= n / 8 (longer K-mers mostly do not occur) and a table of at most 16 GiB and a
// quarter of the free HBM: K = 4 at C3 (n = 2^32, sigma = 128: 4 GiB beside a 77 GiB dictionary), 12 at C2
// (n = 2^28, sigma = 4: 268 MB), 5 at C4 (sigma = 28).  Built on the device at the first search, level by level
// with the rank primitive (sigma'^K steps: ~10 ms at C3); every level is kept (the smaller ones cost 1/sigma' more)
// because the regex frontier steps through them one character at a time.
#include "fmx_device.h"
#include "fmx_host.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>

namespace fmx {

constexpr int kKtThreads = 256;

// level j+1 from level j: entry (code, c) = step(T_j[code], symbol c); one lane group per new entry.  full != 0 (level K+1's
// insertion points, build_kext): every step is taken, also on an empty interval -- (sp, ep) = the images of 0 and n.
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kKtThreads) void k_ktab_level(DevIndex ix, const uint4 *__restrict__ prev, uint4 *__restrict__ next,
                                                            uint64_t n_prev, uint32_t sigma, uint32_t level,
                                                            const uint8_t *__restrict__ sym_of /* [sigma] */, uint32_t full) {
  __shared__ uint64_t s_cf[256];
  __shared__ uint16_t s_slot[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) { s_cf[c] = ix.cf[c]; s_slot[c] = ix.slot[c]; }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t total = n_prev * sigma;
  const uint64_t ngroups = (uint64_t)gridDim.x * (kKtThreads / G);
  for (uint64_t e = ((uint64_t)blockIdx.x * kKtThreads + threadIdx.x) / G; e < total; e += ngroups) {
    const uint64_t code = e / sigma;
    const uint32_t c = sym_of[e % sigma];
    uint64_t sp, ep;
    uint32_t steps;
    if (level == 0) { sp = 0; ep = ix.n; steps = 0; }
    else {
      const uint4 p = prev[code];
      sp = (((uint64_t)p.y << 32) | p.x) & ((1ull << 56) - 1);
      steps = p.y >> 24;
      ep = ((uint64_t)p.w << 32) | p.z;
    }
    if (sp < ep || full) {              // still alive: one more step of the reference's loop
      backward_step<WIDE, LAYOUT>(ix, c, s_slot[c], s_cf[c], lc, sp, ep);
      steps++;
    }
    if (lc.t == 0)
      next[e] = make_uint4((uint32_t)sp, (uint32_t)(sp >> 32) | (steps << 24), (uint32_t)ep, (uint32_t)(ep >> 32));
  }
}

// ---- level K+1 (build_kext).  A search's first K+1 steps consume Y = its last K+1 characters; the rows whose suffix starts
// with Y are the sub-range of Z's interval I_Z (Z = the first K characters of Y, in text order) whose (K+1)-th character is
// y (Y's last, the search's first): the rows are sorted, so those characters do not decrease across I_Z, and
//     Y's interval = [sp_Z + #(characters < y), sp_Z + #(characters <= y)).
// E[code of Z] holds that list (the same code as T's: Z's last character is the most significant digit), 32 bytes:
//   bytes 0..4  sp_Z, the images of row 0 under Z's steps -- Z's insertion point, defined whether Z occurs or not;
//   byte 5      |I_Z| when it is at most kExtCap, else 0xFF: the list is in the overflow array;
//   bytes 6..31 the characters, the row of suffix sp_Z first; unused bytes 0xFF (never below a character, and counted
//               as "<= y" only when y = 255: then the count is |I_Z|);
//   overflow:   bytes 6..10 the list's offset in the overflow array in 16-byte units, bytes 11..15 |I_Z|; the list is
//               padded with 0xFF to a multiple of 16 bytes.
// The (K+1)-th character of the suffix of row q is F[r], r the row K steps of LF behind q (q = LF^K r): the bucket of r.
// An index where some list is longer than kExtMaxList (a text: its common words' k-mers hold millions of rows) gets no level
// K+1: a lookup counts its list 32 bytes per round trip, so the lists it may meet are held to two rounds.
constexpr uint32_t kExtCap = 26, kExtMaxList = 64;

// E's headers: the last of K full steps (k_ktab_level, full = 1, gave the levels before it); an overflowing entry draws its
// list's place from units[0] (16-byte units), units[1] = the longest list
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kKtThreads) void k_kext_head(DevIndex ix, const uint4 *__restrict__ prev, uint4 *__restrict__ ext,
                                                           uint64_t n_prev, uint32_t sigma, const uint8_t *__restrict__ sym_of,
                                                           unsigned long long *__restrict__ units) {
  __shared__ uint64_t s_cf[256];
  __shared__ uint16_t s_slot[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) { s_cf[c] = ix.cf[c]; s_slot[c] = ix.slot[c]; }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t total = n_prev * sigma;
  const uint64_t ngroups = (uint64_t)gridDim.x * (kKtThreads / G);
  for (uint64_t e = ((uint64_t)blockIdx.x * kKtThreads + threadIdx.x) / G; e < total; e += ngroups) {
    const uint32_t c = sym_of[e % sigma];
    uint64_t sp = 0, ep = ix.n;
    if (prev) {
      const uint4 p = prev[e / sigma];
      sp = (((uint64_t)p.y << 32) | p.x) & ((1ull << 56) - 1);
      ep = ((uint64_t)p.w << 32) | p.z;
    }
    backward_step<WIDE, LAYOUT>(ix, c, s_slot[c], s_cf[c], lc, sp, ep);
    if (lc.t == 0) {
      const uint64_t cnt = ep - sp;
      uint4 lo = make_uint4((uint32_t)sp, ((uint32_t)(sp >> 32) & 0xFFu) | ((uint32_t)cnt << 8) | 0xFFFF0000u, ~0u, ~0u);
      if (cnt > kExtCap) {
        const uint64_t off = atomicAdd(units, (unsigned long long)((cnt + 15) / 16));
        atomicMax(units + 1, (unsigned long long)cnt);
        lo = make_uint4((uint32_t)sp, ((uint32_t)(sp >> 32) & 0xFFu) | 0xFF00u | ((uint32_t)off << 16),
                        ((uint32_t)(off >> 16) & 0xFFFFFFu) | ((uint32_t)cnt << 24), (uint32_t)(cnt >> 8));
      }
      ext[2 * e] = lo;
      ext[2 * e + 1] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
  }
}

// E's characters: per row r the K steps of LF from it -- Z's code and q = LF^K r -- and F[r] into Z's list at q - sp_Z.
// Rows whose K characters are not all in the table's alphabet (the end-of-text symbol, 0) belong to no entry.
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kKtThreads) void k_kext_fill(DevIndex ix, const uint4 *__restrict__ ext, uint8_t *__restrict__ extb,
                                                           uint8_t *__restrict__ ovf, const uint8_t *__restrict__ dense,
                                                           uint32_t sigma, uint32_t K) {
  __shared__ uint64_t s_cf[256];
  __shared__ uint16_t s_slot[256];
  __shared__ uint8_t s_dense[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) { s_cf[c] = ix.cf[c]; s_slot[c] = ix.slot[c]; s_dense[c] = dense[c]; }
  __syncthreads();
  constexpr int G = Lay<LAYOUT>::G;
  const LaneConst lc = lane_const<G>();
  const uint64_t ngroups = (uint64_t)gridDim.x * (kKtThreads / G);
  for (uint64_t r0 = ((uint64_t)blockIdx.x * kKtThreads + threadIdx.x) / G; r0 < ix.n; r0 += ngroups) {
    uint64_t r = r0, code = 0;
    bool ok = true;
    for (uint32_t s = 0; s < K && ok; s++) {      // (group-uniform: every lane of the group walks the same row)
      const uint32_t c = r == ix.eof ? 0u : ix.bwt[r];
      const uint32_t d = s_dense[c];
      ok = d != 0xFFu;
      if (ok) {
        code = code * sigma + d;
        r = s_cf[c] + rank_excl<WIDE, LAYOUT>(ix, c, s_slot[c], r, lc);
      }
    }
    if (!ok || lc.t != 0) continue;
    uint32_t f = 0;                                // F[r0]: the largest symbol whose bucket starts at or below r0 (C[] does not decrease)
    for (uint32_t step = 128; step; step >>= 1)
      if (s_cf[f + step] <= r0) f += step;
    const uint4 hd = ext[2 * code];
    const uint64_t sp = hd.x | ((uint64_t)(hd.y & 0xFFu) << 32);
    const uint64_t slot = r - sp;
    if (((hd.y >> 8) & 0xFFu) != 0xFFu) {
      extb[32 * code + 6 + slot] = (uint8_t)f;
    } else {
      const uint64_t off = (hd.y >> 16) | ((uint64_t)(hd.z & 0xFFFFFFu) << 16);
      ovf[16 * off + slot] = (uint8_t)f;
    }
  }
}

// Level K+1 of the table whose K levels are built, for KE = the K a search uses (a multiple of four, fmx_search.hip plan_of).
// It serves the kernels with a row jump table of pairs (k_search4<.., KX>) and is built where they will run ("auto": a
// one-hot index for which "jump_pairs" asks for pairs, when the 32-byte entries, the 8 n bytes of the three-step table and
// the 32 n bytes of the pairs all fit beside each other and the margins -- it never takes the pairs' place), or whenever it
// fits ("on").  Leaves the record's kt.ext null when it is not built; a failure is no error (the kernels without the level serve).
static void build_kext(const Index *h, hipStream_t st, uint32_t KE, const uint8_t *d_sym, const uint8_t *d_dense) {
  const int mode = h->policy.ktab_ext.load(std::memory_order_relaxed);
  if (mode == 0 || KE == 0 || h->layout != kLayoutOneHot || h->block_mode || h->n > (1ull << 32)) return;      // (the kernels that use it are not WIDE)
  const uint32_t sigma = h->nslots;
  uint64_t codes = 1;
  for (uint32_t j = 0; j < KE; j++) codes *= sigma;
  const uint64_t ext_bytes = codes * 32, ovf_reserve = std::max<uint64_t>(ext_bytes / 32, 64ull << 20);
  if (ext_bytes > (16ull << 30)) return;
  if (mode < 0) {
    const int pcfg = h->policy.jump_pairs.load(std::memory_order_relaxed);
    const bool pairs = (pcfg < 0 ? h->n >= (1ull << 30) : pcfg != 0) && (h->policy.jump_mode.load(std::memory_order_relaxed) & 6) == 6;
    if (!pairs || ext_bytes + ovf_reserve + 40 * h->n + (8ull << 30) > table_room(h, 0)) return;
  } else if (ext_bytes + ovf_reserve > table_room(h, 1ull << 30)) {
    return;
  }
  uint64_t tmp_entries = 0;
  for (uint64_t j = 1, c = sigma; j < KE; j++, c *= sigma) tmp_entries += c;      // levels 1 .. KE-1, every step taken
  DevMem mem;
  void *d_ext = nullptr, *d_ovf = nullptr, *d_tmp = nullptr;
  uint64_t ovf_bytes = 0;
  const hipError_t built = [&]() -> hipError_t {
    hipError_t e = table_malloc(h, mem, &d_ext, ext_bytes);
    if (e != hipSuccess || (e = mem.get(&d_tmp, std::max<uint64_t>(tmp_entries, 1) * 16 + 256)) != hipSuccess) return e;
    void *d_units = static_cast<uint8_t *>(d_tmp) + std::max<uint64_t>(tmp_entries, 1) * 16;
    if ((e = hipMemsetAsync(d_units, 0, 16, st)) != hipSuccess) return e;
    uint64_t off = 0, n_prev = 1;
    const uint4 *prev = nullptr;
    for (uint32_t lv = 0; lv + 1 < KE; lv++) {
      uint4 *next = static_cast<uint4 *>(d_tmp) + off;
      const uint64_t n_next = n_prev * sigma;
#define CALL(W, L) k_ktab_level<W, L><<<row_walk_grid(h, n_next, kKtThreads), kKtThreads, 0, st>>>(h->dev, prev, next, n_prev, sigma, lv, d_sym, 1u)
      FMX_LAYOUT_DISPATCH(h, CALL);
#undef CALL
      if ((e = hipGetLastError()) != hipSuccess) return e;
      prev = next;
      off += n_next;
      n_prev = n_next;
    }
#define CALL(W, L) k_kext_head<W, L><<<row_walk_grid(h, codes, kKtThreads), kKtThreads, 0, st>>>(h->dev, prev, static_cast<uint4 *>(d_ext), n_prev, sigma, d_sym, static_cast<unsigned long long *>(d_units))
    FMX_LAYOUT_DISPATCH(h, CALL);
#undef CALL
    if ((e = hipGetLastError()) != hipSuccess) return e;
    unsigned long long units[2] = {0, 0};
    if ((e = hipMemcpyAsync(units, d_units, 16, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (units[1] > kExtMaxList) return hipErrorNotSupported;      // (not an error: no level)
    ovf_bytes = std::max<uint64_t>(units[0], 1) * 16;
    if (ovf_bytes > table_room(h, mode < 0 ? 40 * h->n + (8ull << 30) : (1ull << 30))) return hipErrorOutOfMemory;      // (a skewed text)
    if ((e = table_malloc(h, mem, &d_ovf, ovf_bytes)) != hipSuccess || (e = hipMemsetAsync(d_ovf, 0xFF, ovf_bytes, st)) != hipSuccess) return e;
#define CALL(W, L) k_kext_fill<W, L><<<row_walk_grid(h, h->n, kKtThreads), kKtThreads, 0, st>>>(h->dev, static_cast<const uint4 *>(d_ext), static_cast<uint8_t *>(d_ext), static_cast<uint8_t *>(d_ovf), d_dense, sigma, KE)
    FMX_LAYOUT_DISPATCH(h, CALL);
#undef CALL
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(st);
  }();
  if (built != hipSuccess) { (void)hipGetLastError(); return; }
  Derived<KmerTable> &t = h->kmer;
  mem.free_now(d_tmp);
  mem.keep(d_ext);
  mem.keep(d_ovf);
  t.ext = d_ext;
  t.ovf = d_ovf;
  t.kt.ext = static_cast<const uint4 *>(d_ext);
  t.kt.ovf = static_cast<const uint4 *>(d_ovf);
  t.kt.ext_k = KE;
  table_publish(h, t, ext_bytes + ovf_bytes, ext_bytes + ovf_bytes + tmp_entries * 16);
}

// The body of ktab_get, under kmer.mu: chooses K, allocates and fills the levels, then level K+1.
static hipError_t build_ktab(const Index *h, hipStream_t st) {
  Derived<KmerTable> &t = h->kmer;
  const uint32_t sigma = h->nslots;
  static const int forced = getenv("FMX_KTAB") ? atoi(getenv("FMX_KTAB")) : -1;      // 0 = off, k > 0 = exactly k levels
  if (sigma < 2 || forced == 0 || !h->policy.ktab.load(std::memory_order_relaxed)) return hipSuccess;
  size_t free_b = 0, total_b = 0;
  hipError_t e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) return e;
  // at most 16 GiB, a quarter of the free HBM, and a quarter of what the handle's budget leaves (the row tables want the rest)
  const uint64_t room = table_room(h, 0);
  const uint64_t share = std::max<uint64_t>(room / 4, std::min<uint64_t>(room, 64ull << 20));
  const uint64_t max_bytes = std::min<uint64_t>(std::min<uint64_t>(16ull << 30, free_b / 4), share);
  uint32_t k = 0;
  uint64_t entries = 1, all = 0;
  for (;;) {
    const uint64_t nxt = entries * sigma;
    if (k >= 16 || nxt > h->n / 8 || nxt > (1ull << 32) || (all + nxt) * 16 > max_bytes) break;
    if (forced > 0 && k >= (uint32_t)forced) break;
    entries = nxt;
    all += nxt;
    k++;
  }
  if (forced > 0)       // a test may ask for more levels than the size rule gives (tiny indexes)
    while (k < (uint32_t)forced && k < 16 && (all + entries * sigma) * 16 <= max_bytes) { entries *= sigma; all += entries; k++; }
  if (k == 0) return hipSuccess;
  uint8_t dense[256], sym_of[256];
  for (int c = 0; c < 256; c++) {
    dense[c] = 0xFF;
    if (h->slot[c] < kSlotEof) { dense[c] = (uint8_t)h->slot[c]; sym_of[h->slot[c]] = (uint8_t)c; }    // slots number the present symbols densely
  }
  DevMem mem;
  void *d_all = nullptr, *d_dense = nullptr, *d_sym = nullptr, *d_levels = nullptr;
  if ((e = table_malloc(h, mem, &d_all, all * 16)) != hipSuccess || (e = mem.get(&d_dense, 256)) != hipSuccess ||
      (e = mem.get(&d_sym, 256)) != hipSuccess ||
      (e = hipMemcpyAsync(d_dense, dense, 256, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(d_sym, sym_of, 256, hipMemcpyHostToDevice, st)) != hipSuccess)
    return e;
  uint64_t off = 0, n_prev = 1;
  const uint4 *prev = nullptr;
  for (uint32_t lv = 0; lv < k; lv++) {
    uint4 *next = static_cast<uint4 *>(d_all) + off;
    const uint64_t n_next = n_prev * sigma;
#define CALL(W, L) k_ktab_level<W, L><<<row_walk_grid(h, n_next, kKtThreads), kKtThreads, 0, st>>>(h->dev, prev, next, n_prev, sigma, lv, (const uint8_t *)d_sym, 0u)
    FMX_LAYOUT_DISPATCH(h, CALL);
#undef CALL
    if ((e = hipGetLastError()) != hipSuccess) return e;
    t.kt.level[lv] = next;
    prev = next;
    off += n_next;
    n_prev = n_next;
  }
  if ((e = mem.get(&d_levels, sizeof t.kt.level)) != hipSuccess ||
      (e = hipMemcpyAsync(d_levels, t.kt.level, sizeof t.kt.level, hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess)      // `dense` / `sym_of` go out of scope
    return e;
  for (void *p : {d_all, d_dense, d_levels}) mem.keep(p);
  t.all = d_all;
  t.dense = d_dense;
  t.levels = d_levels;
  t.kt.level_dev = static_cast<const uint4 *const *>(d_levels);
  t.kt.k = k;
  t.kt.tab = t.kt.level[k - 1];
  t.kt.dense = static_cast<const uint8_t *>(d_dense);
  table_publish(h, t, all * 16 + 256, all * 16 + 256);
  // level K+1 over the K-mers of the level a search uses (plan_of: 12, 8 or 4); d_sym goes with `mem` (build_kext has
  // synchronised the stream)
  build_kext(h, st, k >= 12 ? 12u : k >= 8 ? 8u : k >= 4 ? 4u : 0u, static_cast<const uint8_t *>(d_sym), static_cast<const uint8_t *>(d_dense));
  return hipSuccess;
}

// The table of a handle (k == 0: none, or not yet: the search walks its first steps on the rank dictionary), built on first
// use.  A build that fails (out of memory for the table, usually) is no table: every step on the rank dictionary is always
// correct, and the failure must not stick to the handle -- or to the HIP runtime's last-error slot.
hipError_t ktab_get(const Index *h, hipStream_t st, KTab *out, bool build) {
  return table_get(h, h->kmer, build, true, [&] { return build_ktab(h, st); }, [&] {
    *out = h->kmer.kt;
    out->sigma = h->nslots;
  });
}

}  // namespace fmx
