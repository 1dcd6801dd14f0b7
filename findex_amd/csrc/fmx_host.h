// fmx_host.h -- host-side handle and the launch entry points shared by the .hip/.cpp units.
#pragma once
#include <fmx.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fmx_device.h"
#include "fmx_hostpar.h"
#include "fmx_order_math.h"

namespace fmx {

// What one host-pointer call needs on the device side: a stream, two events and grow-only scratch buffers.
// A handle keeps a few of them between calls (fmx_api.cpp, class Call), so that a call costs copies and
// launches only -- creating them afresh took longer than a small batch's kernel.
struct CallCtx {
  static constexpr int kBufs = 8;
  hipStream_t stream = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  void *buf[kBufs] = {nullptr};
  size_t cap[kBufs] = {0};
  std::vector<hipEvent_t> chunk_ev;   // per-chunk events of the pipelined batch search (created on first use)
  void *pin = nullptr;            // pinned host staging for small calls (operands packed into one copy each way)
  size_t pin_cap = 0;
  size_t total() const { size_t t = 0; for (size_t c : cap) t += c; return t; }
};

// The k-mer jump table of an index (fmx_ktab.hip): level[j] holds the intervals of all (j+1)-mers, tab = the last.
struct KTab {
  const uint4 *tab = nullptr;
  const uint4 *level[16] = {nullptr};
  const uint4 *const *level_dev = nullptr;   // the same 16 pointers in device memory (kernels that pick a level at run time
                                             // stage them in LDS: indexing the by-value array would go through scratch)
  const uint8_t *dense = nullptr;   // [256] byte -> dense symbol id, 0xFF for bytes without a bit-vector
  uint32_t k = 0, sigma = 0;
  // the regex frontier's row table (fmx_jump.hip, row1_get): per row BWT'[r] << 40 | LF r, or nullptr
  const unsigned long long *row1 = nullptr;
  // level ext_k + 1 (fmx_ktab.hip, build_kext; nullptr: none): per ext_k-mer Z a 32-byte entry -- Z's insertion point, its
  // row count and the (ext_k + 1)-th characters of its rows -- and the overflow lists of the entries that hold more than 26
  const uint4 *ext = nullptr, *ovf = nullptr;
  uint32_t ext_k = 0;
};

// Host-resident rank dictionary of a (block-sized) index, for ONE dependent chain of rank queries (fmx_hostrank.cpp):
// per 256 positions one record = the running count of every symbol that occurs (nslots x u32), then the 256 BWT' bytes --
// a query touches its symbol's count and the bytes behind it, neighbours in memory.
struct HostRank {
  std::vector<uint8_t> blob;        // (n / 256 + 1) records of `stride` bytes
  size_t stride = 0;                // nslots * 4 + 256
};

// What a handle may build beside its rank dictionary, and when (round 5: per handle -- until round 4 these were process-global
// atomics in fmx_jump.hip, so two handles in one JVM could not differ).  fmx_config_set sets the DEFAULTS a handle takes at
// open; fmx_index_config_set changes one handle's own copy afterwards (a table that exists stays until fmx_drop_tables).
struct TablePolicy {
  std::atomic<int> ktab{1};                    // the k-mer jump table: 1 auto, 0 off
  std::atomic<int> ktab_ext{-1};               // its level K+1 (fmx_ktab.hip): -1 auto (where the row jump table is built as pairs), 0 off, 1 whenever it fits
  std::atomic<int> jump_mode{7};               // bit 0: row table (R1), bit 1: row jump table (J), bit 2: three-step row table (R3)
  std::atomic<int> jump_pairs{-1};             // -1 auto (indexes of 2^30 rows and more, when 32 n bytes fit), 0 never, 1 whenever they fit
  std::atomic<int> search_lanes{-1};           // -1 auto (pairs of lanes from k >= CUs x 512 patterns), 0 quads, 1 pairs of lanes where they can
  std::atomic<int> jump_chars{9};
  std::atomic<long long> tables_after{-1};     // patterns before a search builds tables; -1 auto
  // the BUDGET: device bytes all derived tables of this handle (k-mer, row, row jump, select) may hold together
  std::atomic<uint64_t> budget_bytes{~0ull};   // ~0: none (what fits beside the margins)
  std::atomic<uint32_t> budget_ppb{0};         // != 0: a fraction (billionths) of the HBM that is free when a table is decided, the handle's own tables counted as free
  std::atomic<int> locate_sample{32};          // "locate_sample": the rate s of the locate samples (rows with SA % s == 0), 1 .. 4096
  std::atomic<int> extract_sample{32};         // "extract_sample": the rate s of the inverse-SA samples (the row of every SA value j s), 1 .. 4096
  std::atomic<int> lines_shift{6};             // "lines_shift": the line table's directory step 2^S (fmx_lines.hip), 4 .. 16
  TablePolicy() = default;
  TablePolicy(const TablePolicy &o) { *this = o; }
  TablePolicy &operator=(const TablePolicy &o) {
    ktab.store(o.ktab.load()); ktab_ext.store(o.ktab_ext.load()); jump_mode.store(o.jump_mode.load()); jump_pairs.store(o.jump_pairs.load());
    search_lanes.store(o.search_lanes.load());
    jump_chars.store(o.jump_chars.load()); tables_after.store(o.tables_after.load());
    budget_bytes.store(o.budget_bytes.load()); budget_ppb.store(o.budget_ppb.load());
    locate_sample.store(o.locate_sample.load());
    extract_sample.store(o.extract_sample.load());
    lines_shift.store(o.lines_shift.load());
    return *this;
  }
};
TablePolicy &default_policy();          // fmx_jump.hip: what fmx_config_set writes and fmx_open* copies
// One policy key = value into `p`: 0 ok, 1 unknown key (not a table key), 2 bad value (*why says which values there are)
int policy_set(TablePolicy &p, const char *key, const char *value, const char **why);

// A structure a handle derives from its index at first use and keeps until fmx_drop_tables: the lock its build and its drop
// take, and what every *_info call reports.  Derived<F> adds the feature's own fields F; free_locked is the one place that
// frees F's buffers, and it puts every field back to its default (the info calls report 0 while `ready` is false).
struct Side {
  std::mutex mu;
  bool ready = false;
  uint64_t bytes = 0;                           // device bytes held (the budgeted tables: the bytes fmx_stats reports for them)
  double build_ms = 0.0;                        // host time of the build (the budgeted tables keep theirs in Index::tables_ms)
  bool decided() { std::lock_guard<std::mutex> lk(mu); return ready; }      // `ready`, for a caller that only asks
};
template <class F>
struct Derived : Side, F {
  void free_locked() {                          // under mu
    F::free_buffers();
    static_cast<F &>(*this) = F{};
    ready = false;
    bytes = 0;
    build_ms = 0.0;
  }
  void drop() {
    std::lock_guard<std::mutex> lk(mu);
    free_locked();
  }
};
struct LocateSamples {                          // the sampled suffix array
  void *marks = nullptr;                        // one-hot rank blocks over the rows: bit r set <=> SA[r] % rate == 0
  void *samples = nullptr;                      // SA of the marked rows in row order: u32, or u64 when wide
  uint32_t rate = 0;
  bool wide = false;
  void free_buffers() { (void)hipFree(marks); (void)hipFree(samples); }
};
struct LcpArray {                               // u32[n]
  void *lcp = nullptr;
  uint32_t max = 0;                             // the largest entry, the first row that holds it, the sum of all entries
  uint64_t max_row = 0, sum = 0;
  void free_buffers() { (void)hipFree(lcp); }
};
struct ExtractSamples {                         // the inverse-SA samples for extraction by text position
  void *isa = nullptr;                          // isa[j] = the row with SA == j * rate, j = 0 .. (n - 1) / rate: u32, or u64 when wide
  uint32_t rate = 0;
  bool wide = false;
  void free_buffers() { (void)hipFree(isa); }
};
struct LineTable {
  void *brk = nullptr;                          // u32[max(n_brk, 1)]: the positions of the break bytes, ascending
  void *dir = nullptr;                          // u32[((n - 1) >> shift) + 2]: dir[i] = the breaks before position i << shift
  uint64_t n_brk = 0;
  uint32_t shift = 0;
  uint8_t set[4] = {0, 0, 0, 0};                // the break set, ascending
  uint32_t n_set = 0;
  void free_buffers() { (void)hipFree(brk); (void)hipFree(dir); }
};

// The five tables under the handle's table budget (TablePolicy::budget_*), records of the same shape.  For them `ready` means
// DECIDED, not built: a table that is switched off, does not fit the budget or failed to build is decided and holds nothing,
// and the question is not asked again until a drop (the four structures above are asked for again at every call until they
// are built).  table_get builds them, table_publish counts them, table_drop frees them (below).
struct KmerTable {                              // fmx_ktab.hip
  KTab kt;                                      // what the kernels see (sigma is filled in when it is copied out)
  void *all = nullptr, *dense = nullptr, *levels = nullptr;      // the levels in one allocation, KTab::dense, KTab::level_dev
  void *ext = nullptr, *ovf = nullptr;          // level K+1 and its overflow lists (KTab::ext, ::ovf)
  void free_buffers() { for (void *p : {all, dense, levels, ext, ovf}) if (p) (void)hipFree(p); }
};
struct JumpTable {                              // fmx_jump.hip: the row jump table J
  void *tab = nullptr;
  bool pairs = false;                           // the table holds pairs J[r] | J[LF^jc r] (32 bytes per row): up to 2 jc steps per request
  uint32_t chars = 0;                           // characters (backward steps) one entry stands for: 8 .. 11
  void free_buffers() { if (tab) (void)hipFree(tab); }
};
struct RowWords {                               // fmx_jump.hip: one 8-byte word per row (R1, R3)
  void *words = nullptr;
  void free_buffers() { if (words) (void)hipFree(words); }
};
struct SelectDir {                              // fmx_select.hip: the select directory for Psi
  void *dir = nullptr, *off = nullptr, *shift = nullptr;
  void free_buffers() { for (void *p : {dir, off, shift}) if (p) (void)hipFree(p); }
};
// The row jump table as a search sees it: copied under the record's lock, as KTab is
struct JumpView {
  const uint4 *tab = nullptr;                   // nullptr: the handle has none
  bool pairs = false;
  uint32_t chars = 0;
};

struct Index {
  uint64_t serial = 0;          // unique per open in this process: what a resident regex batch remembers of its index
  int device = 0;
  int cu_count = 256;
  uint64_t n = 0, eof = 0, nblocks = 0;
  uint32_t nslots = 0;
  int64_t counts[256] = {0};
  uint64_t cf[256] = {0};
  uint16_t slot[256] = {0};
  // device memory owned by the handle
  // NaiveBWTSearcher form (fmx_open_block, findex.scala:459-506): bucket starts come from the caller, symbol 0 is an
  // ordinary (absent) symbol, and the block's first byte decides one quirk (build_index)
  bool block_mode = false;
  int64_t block_bs[256] = {0};
  int block_first = -1;         // BWT byte at position 0 (-1: position 0 is the skipped row)
  int block_skipped = -1;       // BWT byte at the skipped row rk0
  uint32_t layout = 0;          // kLayoutOneHot | kLayoutBytes
  void *d_bv = nullptr;
  void *d_chk = nullptr;        // bytes layout: checkpoints
  void *d_sup = nullptr;        // bytes layout: superblock counts
  void *d_bwt = nullptr;
  void *d_cf = nullptr;
  void *d_slot = nullptr;
  unsigned long long *d_counters = nullptr;   // kCounterSlots slots of kCounterStride counters (fmx_device.h)
  DevIndex dev{};
  uint64_t index_bytes = 0;
  double build_ms = 0.0;
  // host-call bookkeeping
  mutable std::mutex mu;
  mutable std::vector<CallCtx *> ctx_pool;      // idle call contexts (guarded by mu)
  // the tables of the budget, each decided at first use: the k-mer jump table (at a search, or by fmx_prepare), the row jump
  // table J and the three-step row table R3 = (BWT'[r], BWT'[LF r], BWT'[LF^2 r]; LF^3 r) (at the first literal search that
  // finds them due), the regex frontier's row table R1 = (BWT'[r], LF r) (at the first regex match) and the select directory
  // (at the first Psi / nextSubstr call).  LOCK ORDER: jump.mu before row3.mu (J is built from R3, inside J's build); no other
  // two of these locks are ever held together, and none is held while Index::mu is taken.
  mutable Derived<KmerTable> kmer;
  mutable Derived<JumpTable> jump;
  mutable Derived<RowWords> row1, row3;
  mutable Derived<SelectDir> sel;
  mutable std::atomic<double> tables_ms{0.0};   // host time spent deciding and building the five (TableSpan)
  // when the derived tables are built (fmx_jump.hip, tables_due): patterns searched so far, fmx_prepare seen
  // ticket areas of the literal search kernel (fmx_device.h, kTixAreas): which stream owns which.  A launch draws its last
  // batches from the area of the stream it is enqueued on; launches on ONE stream follow each other, so an area serves one
  // launch at a time.  Streams beyond the areas (and streams being captured) get none: their launches stride statically.
  mutable std::mutex tix_mu;
  mutable void *tix_owner[16] = {};
  mutable bool tix_used[16] = {};
  mutable std::atomic<uint64_t> patterns_seen{0};
  mutable std::atomic<uint32_t> search_residency{0};     // fmx_stats.search_residency
  // fmx_prepare has been asked for the k-mer table / the row tables: searches use them (and build what a drop took away)
  // whatever the pattern count says.  One flag per table (one shared flag made prepare(KTAB) build 40 n bytes
  // of row tables inside the next search).
  mutable std::atomic<bool> prepared_ktab{false}, prepared_rows{false};
  mutable TablePolicy policy;                                   // this handle's own (copied from the defaults at open)
  mutable std::atomic<uint64_t> tables_held{0};                 // device bytes of all derived tables right now (what the budget counts)
  mutable std::atomic<uint64_t> tables_alloc_us{0};             // of tables_ms: microseconds spent inside hipMalloc for the tables (the driver wiping memory somebody released: profiles/r05_alloc.md)
  mutable std::atomic<uint64_t> hbm_free_after_tables{0};       // hipMemGetInfo's free bytes right after the last table build (0: none built)
  mutable std::atomic<uint64_t> peak_table_build_bytes{0};      // most device memory a table build held at once (table + its scratch)
  // what is built at first use outside the table budget (the search tables never see it): by fmx_prepare(FMX_PREPARE_LOCATE |
  // _LCP | _EXTRACT | _LINES), fmx_lines_prepare or the first call that needs it
  mutable Derived<LocateSamples> loc;           // fmx_locate.hip
  mutable Derived<LcpArray> lcp;                // fmx_lcp.hip
  mutable Derived<ExtractSamples> ext;          // fmx_extract.hip
  mutable Derived<LineTable> lin;               // fmx_lines.hip
  mutable uint64_t launches = 0;
  mutable double last_kernel_ms = 0.0;
  // the handle's host thread for the one-process-several-GPUs entry points (made at the first such call; fmx_hostpar.h)
  mutable std::unique_ptr<Worker> worker;
  // host-side rank dictionary (fmx_occ_host / fmx_calc_gaps_chain), built at first use
  mutable std::mutex hr_mu;
  mutable std::unique_ptr<HostRank> hr;
};

Worker *worker_of(const Index *h);     // fmx_api.cpp

void set_error(const std::string &msg);
// Borrow / return one of the handle's call contexts (stream + events created on first use).  ctx_acquire
// returns nullptr and records the error when the stream or events cannot be created.
CallCtx *ctx_acquire(const Index *h);
void ctx_release(const Index *h, CallCtx *c);
hipError_t ctx_scratch(CallCtx *c, int i, size_t bytes, void **out);   // grow-only device scratch buffer i
struct CtxLease {            // scope guard around ctx_acquire / ctx_release
  const Index *h;
  CallCtx *c;
  explicit CtxLease(const Index *hh) : h(hh), c(ctx_acquire(hh)) {}
  ~CtxLease() { if (c) ctx_release(h, c); }
  CtxLease(const CtxLease &) = delete;
  CtxLease &operator=(const CtxLease &) = delete;
};
// The derived tables are built when they have a chance to pay: by fmx_prepare, or at the search that brings the patterns a
// handle has been asked for to `threshold` (fmx_config_set("tables_after", ..)); `build` = false only looks.
bool tables_due(const Index *h, uint64_t k, bool small_table);      // fmx_jump.hip: counts k, then decides
void note_table_build(const Index *h, uint64_t bytes_held);
// Room for one more derived table of this handle: min(free HBM - margin, what the handle's budget leaves); 0 when hipMemGetInfo fails.
uint64_t table_room(const Index *h, uint64_t margin);
void tables_account(const Index *h, int64_t delta);                 // a table of |delta| bytes was built (+) or freed (-)
struct DevMem;
hipError_t table_malloc(const Index *h, DevMem &mem, void **p, size_t bytes);      // mem.get for a derived table, its time added to tables_alloc_us
// A budgeted table is there: `bytes` more on its record and on the handle's count, `peak_bytes` = what its build held at once
void table_publish(const Index *h, Side &t, uint64_t bytes, uint64_t peak_bytes);
// The host time of a table build, for Index::tables_ms.  Builds nest (J's contains R3's): only a thread's outermost span adds.
struct TableSpan {
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  TableSpan();
  ~TableSpan();
  TableSpan(const TableSpan &) = delete;
  void add_to(const Index *h) const;
};
template <class F>
void table_drop_locked(const Index *h, Derived<F> &t) {             // under t.mu: undecided again, nothing held
  tables_account(h, -(int64_t)t.bytes);
  t.free_locked();
}
template <class F>
void table_drop(const Index *h, Derived<F> &t) {
  std::lock_guard<std::mutex> lk(t.mu);
  table_drop_locked(h, t);
}
// The one way to a budgeted table: under its lock, `body` decides and builds it unless it is decided or the caller only looks
// (`build` false), then `out` copies what the caller needs.  body allocates from a DevMem of its own, keeps what it fills
// the record with and calls table_publish last.  A body that fails leaves the record empty; `optional`: that is "no table,
// no error" -- decided, the HIP last-error slot cleared -- else the error comes back and the next call asks again.
template <class F, class Body, class Out>
hipError_t table_get(const Index *h, Derived<F> &t, bool build, bool optional, Body body, Out out) {
  std::lock_guard<std::mutex> lk(t.mu);
  if (!t.ready && build) {
    const TableSpan span;
    const hipError_t e = body();
    if (e != hipSuccess) {
      table_drop_locked(h, t);
      if (!optional) return e;
      (void)hipGetLastError();
    }
    span.add_to(h);
    t.ready = true;
  }
  out();
  return hipSuccess;
}
// Grid of a table build whose lane groups (8 lanes in the bytes layout, 4 in the one-hot) each walk from one of `items` rows
inline int row_walk_grid(const Index *h, uint64_t items, int threads) {
  const uint64_t per_wg = (uint64_t)threads / (h->layout == kLayoutBytes ? 8 : 4);
  return (int)std::min<uint64_t>((items + per_wg - 1) / per_wg, (uint64_t)h->cu_count * 8);
}
// What fmx_stats reports of the five tables, each read under its own lock (fmx_jump.hip)
struct TablesSnapshot {
  uint64_t kmer_held = 0, jump_held = 0, row1_held = 0, row3_held = 0, sel_held = 0;      // the records' bytes
  uint32_t kmer_k = 0, jump_jc = 0;
};
TablesSnapshot tables_snapshot(const Index *h);
hipError_t ktab_get(const Index *h, hipStream_t st, KTab *out, bool build = true);     // fmx_ktab.hip
hipError_t select_prepare(const Index *h, hipStream_t st);          // fmx_select.hip: builds the select directory now
hipError_t jump_get(const Index *h, hipStream_t st, JumpView *out, bool build = true);   // fmx_jump.hip (tab == nullptr: the handle has none)
hipError_t row1_get(const Index *h, hipStream_t st, const unsigned long long **out, bool build = true);   // fmx_jump.hip (nullptr: none)
hipError_t row3_get(const Index *h, hipStream_t st, const unsigned long long **out, bool build = true);   // fmx_jump.hip (nullptr: none)
// fmx_jump.hip: frees the budgeted tables `what` names (FMX_PREPARE_KTAB | _JUMP | _FRONTIER; fmx_close adds _SELECT)
int drop_tables(Index *h, unsigned what);

// fmx_locate.hip: the locate samples.  locate_prepare builds them under loc.mu (allocates, synchronises `st`; an FMX_*
// status with its message); launch_locate* need them built.  locate_write_sa: every row's SA as big-endian u32 into
// d_sa_be (n < 2^32), the handle's own samples untouched; locate_write_sa_bytes: the device bytes that takes, d_sa_be included.
int locate_check(const Index *h);               // FMX_ERR_UNSUPPORTED for handles locate cannot serve
int locate_prepare(const Index *h, hipStream_t st);
int locate_write_sa(const Index *h, hipStream_t st, uint32_t *d_sa_be);
uint64_t locate_write_sa_bytes(const Index *h);
hipError_t launch_locate(const Index *h, const void *d_rows, uint64_t k, void *d_out, hipStream_t st);
hipError_t launch_locate_intervals(const Index *h, const void *d_sp, const void *d_ep, uint64_t k, uint64_t max_per,
                                   void *d_off, void *d_pos, uint64_t cap, hipStream_t st);
// the inversion with s and a native-endian SA as outputs (n < 2^32): d_sa[row] = SA[row], d_s[v] = s[v] for v < n - 1 and
// the sentinel 0 at d_s[n - 1]; locate_invert_text_bytes: the device bytes of its temporaries (the outputs not counted).
int locate_invert_text(const Index *h, hipStream_t st, uint32_t *d_sa, uint8_t *d_s);
uint64_t locate_invert_text_bytes(const Index *h);

// pass 2 of the inversion alone (fmx_extract.hip): d_tmp[v / rate] = the row with SA == v for every v % rate == 0, d_tmp of
// (n - 1) / rate + 1 entries given by the caller; locate_invert_rows_bytes: the device bytes of its temporaries (d_tmp not
// counted).  Synchronises `st`; the handle's own samples are untouched.
int locate_invert_rows(const Index *h, hipStream_t st, uint32_t rate, uint64_t *d_tmp);
uint64_t locate_invert_rows_bytes(const Index *h);

// fmx_extract.hip: text by position from inverse-SA samples, its entry points included.  extract_prepare builds
// the samples under ext.mu (allocates, synchronises `st`; an FMX_* status with its message).
int extract_check(const Index *h);              // FMX_ERR_UNSUPPORTED for handles extraction cannot serve (those of locate)
int extract_prepare(const Index *h, hipStream_t st);

// fmx_lines.hip: the line table.  lines_prepare builds it for the set {10} under lin.mu unless one exists
// (allocates, synchronises `st`; an FMX_* status with its message); its entry points are in the unit.
int lines_check(const Index *h);                // FMX_ERR_UNSUPPORTED for handles the line table cannot serve (locate's, n >= 2^32)
int lines_prepare(const Index *h, hipStream_t st);
// a table for a call that needs one: the handle's, or {10} / {10, 1} (with a corpus) built on `st` (a stream of the handle's
// when null); FMX_ERR_ARG for a table that lacks byte 1 combined with a corpus
int lines_ensure(const Index *h, bool with_corpus, hipStream_t st);

// fmx_linequery.hip: the query algebra over line-hit lists, its entry points included.  lq_config: the
// process-wide key "lq_narrow" = on | off (default off); 0 ok, 1 not this unit's key, 2 bad value (*why says which values there are)
int lq_config(const char *key, const char *value, const char **why);

// fmx_lcp.hip: the LCP array.  lcp_core: LCP[n] of s from s and its suffix array, all in device memory;
// d_s is s itself (lcp_text_bytes(n) bytes: s, the sentinel 0 last, and zero padding); allocates 4 n bytes, synchronises `st`, returns an FMX_*
// status with its message.  max / first row of the max / sum of the array come back through the pointers (may be null).
struct LcpInfo {
  uint32_t max = 0;
  uint64_t max_row = 0, sum = 0;
  float phase_ms[3] = {0, 0, 0};                // k_lcp_phi, k_lcp_plcp, k_lcp_gather: device events
};
uint64_t lcp_core_bytes(uint64_t n);            // device bytes lcp_core allocates
uint64_t lcp_text_bytes(uint64_t n);            // device bytes of s with the padding the comparisons read
int lcp_core(const uint8_t *d_s, uint64_t n, const uint32_t *d_sa, uint32_t *d_lcp, int cu_count, hipStream_t st, LcpInfo *info);
void lcp_reverse_text(const uint8_t *d_text, uint64_t len, uint8_t *d_s, int cu_count, hipStream_t st);   // s = reverse(text) + 0
int lcp_check(const Index *h);                  // FMX_ERR_UNSUPPORTED for handles that have no LCP array
int lcp_prepare(const Index *h, hipStream_t st);   // builds the handle's array under lcp.mu (allocates, synchronises `st`)
hipError_t launch_lcp_gather(const Index *h, const void *d_rows, uint64_t k, void *d_out, hipStream_t st);

// fmx_approx.hip and fmx_mstat.hip (§16) hold their entry points themselves.

// fmx_search.hip: the residency census of the k_search4 instantiation this handle's full-size searches use now, taken with
// calibration launches on `st` (synchronises it): fmx_prepare's last step, never a _dev call's.
hipError_t search_calibrate(const Index *h, hipStream_t st);
bool force_superblocks();                       // fmx_config_set("checkpoints", "superblock"): the bytes layout's >= 2^32-count form
int layout_preference();                        // -1 auto, else kLayoutOneHot / kLayoutBytes (fmx_config_set)
int hip_fail(hipError_t e, const char *what);   // records the message, returns FMX_ERR_HIP

// ---- host helpers every unit shares
#define HIP_TRY(call, what)                                   \
  do {                                                        \
    const hipError_t e__ = (call);                            \
    if (e__ != hipSuccess) return ::fmx::hip_fail(e__, what); \
  } while (0)
// One kernel launch on `st` (no dynamic LDS) and its error check
#define LAUNCH(what, kernel, grid, block, st, ...)                    \
  do {                                                                \
    hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);      \
    HIP_TRY(hipGetLastError(), what);                                 \
  } while (0)

struct DevMem {                 // the hipMalloc'ed temporaries of one call; freed on every return path
  std::vector<void *> ps;
  DevMem() = default;
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { for (void *p : ps) (void)hipFree(p); }
  hipError_t get(void **out, size_t bytes) {
    *out = nullptr;
    const hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e == hipSuccess) ps.push_back(*out);
    return e;
  }
  template <class T>
  hipError_t alloc(T **out, size_t count) { return get(reinterpret_cast<void **>(out), count * sizeof(T)); }
  void keep(const void *p) {                    // p outlives the call: it is the caller's now
    const auto it = std::find(ps.begin(), ps.end(), p);
    if (it != ps.end()) ps.erase(it);
  }
  void free_now(void *p) { keep(p); (void)hipFree(p); }      // a temporary that goes before the call ends
  int take(void **out, size_t bytes, const char *what) {     // get, or "hipMalloc(<what>): .." and FMX_ERR_NOMEM
    const hipError_t e = get(out, bytes);
    if (e == hipSuccess) return FMX_OK;
    set_error(std::string("hipMalloc(") + what + "): " + hipGetErrorString(e));
    return FMX_ERR_NOMEM;
  }
};
// p = `bytes` of device memory from the bag `mem`, or "hipMalloc(<what>): .." and FMX_ERR_NOMEM
#define DEV_ALLOC(mem, p, bytes, what)                                           \
  do {                                                                           \
    if (const int rc__ = (mem).take((void **)&(p), (bytes), what)) return rc__;  \
  } while (0)

struct StreamGuard {            // a stream the call made for itself
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};

template <int N>
struct Events {                 // the N timing events of one call; destroyed on every return path
  hipEvent_t ev[N] = {};
  Events() = default;
  Events(const Events &) = delete;
  Events &operator=(const Events &) = delete;
  ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t create() {
    for (hipEvent_t &e : ev) {
      const hipError_t r = hipEventCreate(&e);
      if (r != hipSuccess) return r;
    }
    return hipSuccess;
  }
  hipError_t record(int i, hipStream_t st) { return hipEventRecord(ev[i], st); }
  hipError_t elapsed(int i, int j, float *ms) const { return hipEventElapsedTime(ms, ev[i], ev[j]); }
  float ms(int i, int j) const {               // 0 when the runtime has no answer
    float m = 0;
    (void)elapsed(i, j, &m);
    return m;
  }
};

// A call's own counters: kernels add to `mine`, private counter slots, and to `line`; fold adds the slots to the
// handle's and sums counter `steps_counter` and the requests into the line; finish copies the line back, synchronises `st`
// and adds `launches` to the handle's.  Both buffers belong to the caller's bag, which places its event records itself.
struct MeterCounts {
  uint64_t hits = 0, steps = 0, requests = 0;
};
struct Metered {
  unsigned long long *line = nullptr, *mine = nullptr;
  int alloc(DevMem &mem, const char *what);
  int zero(hipStream_t st);
  int fold(const Index *h, uint32_t steps_counter, hipStream_t st);
  int finish(const Index *h, hipStream_t st, uint64_t launches, MeterCounts *out);
};
constexpr uint64_t kMeteredBytes = kCounterBytes + 8 * kLineWords;      // what alloc takes

// Grid of a kernel whose workgroups loop over the work: what is resident on the device at once, at most one workgroup per
// `per_block` items.  The occupancy query is made once per kernel.
template <auto Kernel>
hipError_t resident_grid(const Index *h, int threads, uint64_t work, uint64_t per_block, uint32_t *grid) {
  static std::atomic<int> cached{0};
  int per_cu = cached.load(std::memory_order_relaxed);
  if (per_cu <= 0) {
    const hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, threads, 0);
    if (he != hipSuccess) return he;
    per_cu = std::max(per_cu, 1);
    cached.store(per_cu, std::memory_order_relaxed);
  }
  const uint64_t resident = (uint64_t)per_cu * (uint64_t)std::max(h->cu_count, 1);
  *grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident, (work + per_block - 1) / per_block));
  return hipSuccess;
}
// Grid of a 256-thread kernel that strides over `items`
inline uint32_t flat_grid(uint64_t items, uint32_t cap = 4096) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, cap));
}

// fmx_api.cpp.  use_device_index: a device there is, `device` names one, hipSetDevice.  no_capture: FMX_ERR_HIP with `text`
// when `st` is being captured; not_capturing: the same with "<what> allocates and synchronises: not under a stream capture".
// device_room: FMX_ERR_NOMEM with "<what> <verb> <need> bytes of device memory, <free> are free" when `need` exceeds the
// free device memory.  ensure_built: `prepare` (which takes side.mu itself and looks again) on `st`, or on a stream of the
// handle's when st is null, unless the side is ready.
int arg_fail(const char *msg);                  // records the message, returns FMX_ERR_ARG
int use_device(const Index *h);
int use_device_index(int device);
int no_capture(hipStream_t st, const char *text);
int not_capturing(hipStream_t st, const char *what);
int device_room(uint64_t need, const std::string &what, const char *verb = "needs");
int ensure_built(const Index *h, Side &side, int (*prepare)(const Index *, hipStream_t), hipStream_t st);
// The build of a derived structure under its lock: nothing when `ready` says it is there; not under a stream capture
// (`capture_text` is the feature's refusal); `first`, what the build needs built before it (its time is not the structure's);
// then `body`, which checks the room, allocates from `mem` (what it keeps it takes out of the bag), builds and, as its last
// step, fills the record; then the build time and the ready flag, and only then the temporaries go.
template <class Body, class Ready, class First>
int build_locked(Side &side, hipStream_t st, const char *capture_text, Body body, Ready ready, First first) {
  std::lock_guard<std::mutex> lk(side.mu);
  if (ready()) return FMX_OK;
  int rc = no_capture(st, capture_text);
  if (rc || (rc = first())) return rc;
  DevMem mem;
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = body(mem))) return rc;
  side.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  side.ready = true;
  return FMX_OK;
}
template <class Body>
int build_locked(Side &side, hipStream_t st, const char *capture_text, Body body) {      // unless side.ready; nothing first
  return build_locked(side, st, capture_text, body, [&] { return side.ready; }, [] { return (int)FMX_OK; });
}
bool offsets_monotonic(const uint64_t *off, size_t a, size_t b);      // off[a] <= off[a+1] <= .. <= off[b]
inline Index *H(fmx_index *p) { return reinterpret_cast<Index *>(p); }
inline const Index *H(const fmx_index *p) { return reinterpret_cast<const Index *>(p); }

// The device side of one host-pointer call of a metered feature: its temporaries and a non-blocking stream of its own.
struct HostCall {
  DevMem mem;
  StreamGuard own;
  int open() { HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate"); return FMX_OK; }
  // `bytes` of pat and the k + 1 offsets into the bag, then a synchronise.  rebase: the offsets travel less off[0] (pat is the
  // caller's pointer already advanced), and an empty batch copies nothing; otherwise off[0] == 0 and an empty batch gets one
  // zero offset.  The labels are those of DEV_ALLOC.
  int upload(const char *pat_what, const void *pat, uint64_t bytes, const char *off_what, const uint64_t *off, size_t k,
             bool rebase, void **d_pat, uint64_t **d_off);
  int download(void *dst, const void *src, uint64_t bytes, const char *what) {      // enqueues; dst == nullptr: nothing
    if (dst) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, own.s), what);
    return FMX_OK;
  }
  int sync() { HIP_TRY(hipStreamSynchronize(own.s), "hipStreamSynchronize"); return FMX_OK; }
  // a CSR result: k + 1 offsets and `total` records of `rec` bytes, then a synchronise
  int download_csr(uint64_t *out_off, const void *d_out_off, size_t k, void *out, const void *d_out, uint64_t total, size_t rec) {
    int rc;
    if ((rc = download(out_off, d_out_off, 8 * ((uint64_t)k + 1), "D2H(offsets)"))) return rc;
    if (total && (rc = download(out, d_out, rec * total, "D2H(hits)"))) return rc;
    return sync();
  }
};
// "<prefix>: <total> hits, room for <cap>" and FMX_ERR_OVERFLOW
int csr_overflow(const char *prefix, uint64_t total, size_t cap);

// fmx_build.hip
int build_index(Index *h, hipStream_t st, const int64_t *given_counts);   // returns an FMX_* status

// fmx_sufsort.hip: index construction from text (fmx_bwt_from_text*, fmx_open_text); arguments checked by the caller,
// `extra` = device bytes the caller still allocates, counted in the free-memory check.  Synchronises `st`.
uint64_t sufsort_peak_bytes(uint64_t len, bool sa_given);
int sufsort_bwt(const void *d_text, uint64_t len, void *d_bwt, void *d_sa_or_null, uint64_t *eof, int64_t counts[256],
                hipStream_t st, uint64_t extra);

// The scan, the radix sort and the shared order kernels: fmx_order.h (bits_for and the workspace sizes: fmx_order_math.h).

// fmx_kernels.hip (launch_psi, launch_next_substr: fmx_select.hip)
hipError_t launch_occ(const Index *h, const void *d_c, const void *d_i, void *d_out, uint64_t k, hipStream_t st);
hipError_t launch_prev_range(const Index *h, const void *d_sp, const void *d_ep, const void *d_c, void *d_sp1,
                             void *d_ep1, uint64_t k, hipStream_t st);
hipError_t launch_search(const Index *h, const void *d_pat, const void *d_off, void *d_sp, void *d_ep, uint64_t k,
                         hipStream_t st, uint32_t fixed_len = 0,       // d_off == nullptr: k patterns of fixed_len bytes each
                         uint64_t pack_cap = ~0ull,                    // != ~0: the 8-byte form into d_sp (escape list of pack_cap), d_ep scratch
                         uint32_t flags = 0);                          // kSearchMissNone: fmx.h, FMX_SEARCH_MISS_NONE
constexpr uint32_t kSearchMissNone = 1u;
// the 8-byte form of a batch's intervals (fmx.h: fmx_pack_intervals_dev); in place when d_packed == d_sp
hipError_t launch_pack_intervals(const Index *h, const void *d_sp, const void *d_ep, uint64_t k, uint64_t escape_cap,
                                 void *d_packed, hipStream_t st);
hipError_t launch_unpack_intervals(const Index *h, const void *d_packed, uint64_t k, uint64_t escape_cap, void *d_sp,
                                   void *d_ep, hipStream_t st);
// fmx_config_set("validate", "1"): is d_off[0..k] non-decreasing?  Synchronises the stream.
hipError_t check_offsets(const Index *h, const void *d_off, uint64_t k, hipStream_t st, bool *ok);
hipError_t launch_lf_walk(const Index *h, const void *d_rows, uint64_t k, uint32_t len, void *d_out, void *d_end,
                          hipStream_t st);
hipError_t launch_fm_fill(const Index *h, void *d_fm, hipStream_t st);
hipError_t launch_psi(const Index *h, const void *d_rows, void *d_out, uint64_t k, hipStream_t st);
hipError_t launch_next_substr(const Index *h, const void *d_sps, uint64_t k, uint32_t len, void *d_out,
                              void *d_out_len, hipStream_t st);

// fmx_refmatch.hip
struct RefTables;
}  // namespace fmx
struct fmx_result;
namespace fmx {
int regex_match_reference(const Index *h, const RefTables &rt, size_t k, uint32_t max_fanout, uint32_t max_branching,
                          uint32_t max_iterations, fmx_result *out, size_t cap, size_t *n_out,
                          uint32_t *per_regex_count, uint32_t *front_left);

}  // namespace fmx
