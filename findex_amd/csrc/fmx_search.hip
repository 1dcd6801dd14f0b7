// fmx_search.hip -- K3's host side: which instantiation of k_search4 (fmx_search4.h) a literal search launches, and how.
//
// A search first prepares the handle's tables (search_tables), then computes the form of the kernel they select (plan_of,
// select_plan: plain functions of the handle and the batch size) and launches that form's entry of the list of
// instantiations that exist (kForms, from FMX_SEARCH4_LIST) with a grid sized by the residency census.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "fmx_host.h"
#include "fmx_search4.h"

namespace fmx {

hipError_t launch_search_v1(const Index *h, const void *d_pat, PatOff po, void *d_sp, void *d_ep, uint64_t k,
                            hipStream_t st);

// The search's own diagnostic switches, read once: FMX_SEARCH_WGS=n, fewer resident workgroups per CU (an experiment on how
// throughput follows the chains in flight), and FMX_TRACE, every census and launch on stderr.
struct SearchKnobs {
  int wgs;        // 0: as many as are resident
  bool trace;
};
static const SearchKnobs &knobs() {
  static const SearchKnobs v = [] {
    const char *w = getenv("FMX_SEARCH_WGS");
    return SearchKnobs{w ? std::max(1, atoi(w)) : 0, getenv("FMX_TRACE") != nullptr};
  }();
  return v;
}

// What the occupancy query says is an upper bound: on this chip a kernel with 81..96 scalar registers gets one
// workgroup per CU fewer than it answers (MI355X_MICROARCH.md, "Residency"; there is no API for the scalar register
// count), and the surplus workgroups run as a second generation behind the first -- C5's bytes-layout kernel: 8 asked
// for, 7 resident, a launch of 0.205 ms instead of 0.170.  So every instantiation of k_search4 is calibrated by a
// CENSUS on the device it runs on: a calibration launch of the full grid (one empty pattern; every workgroup spins
// 60 us) leaves each workgroup's begin and end times behind the counters (fmx_device.h); the host counts the workgroups
// that began before the first one ended and divides by the CUs.  A census taken while other work held part of the
// device counts late workgroups that waited for THAT: only an answer of the query's number or up to two below it is
// believed, and only when two launches in a row give it (at most four are made).
// Round 4 took the readings inside fmx_search_batch_dev -- a 64 KB copy and a stream synchronisation on the CALLER's
// stream in the 2nd to 6th full-size call, against the header's promise that _dev entry points only enqueue work
// (ADVICE r4).  Now search_calibrate does it: called by fmx_prepare, and by the search that builds
// a handle's tables at its threshold (that call allocates and synchronises anyway, and says so); no other call reads
// anything back.  An instantiation that was never calibrated keeps the query's answer.
struct Residency {
  std::atomic<int> admitted{0};            // workgroups per CU that were resident at once; 0 = not measured yet
  std::mutex mu;                           // one calibration at a time per instantiation and device
};
constexpr uint32_t kCalibSpin = 6000;      // 60 us
static int census_read(const Index *h, int grid, int api, hipStream_t st) {
  std::vector<unsigned long long> t(2 * (size_t)kCensusBlocks + 2);
  if (hipMemcpyAsync(t.data(), h->d_counters + (size_t)kCounterSlots * kCounterStride, kCensusBytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (t[2 * (size_t)kCensusBlocks] != (unsigned long long)grid) return 0;      // the last launch to write here was not the calibration (another stream's search)
  const int nb = std::min<int>(grid, (int)kCensusBlocks);
  unsigned long long first_begin = ~0ull, first_end = ~0ull;
  for (int i = 0; i < nb; i++) {
    if (!t[2 * i] || t[2 * i + 1] < t[2 * i]) return 0;      // overwritten half-way by another launch
    first_begin = std::min(first_begin, t[2 * i]);
    first_end = std::min(first_end, t[2 * i + 1]);
  }
  if (first_end < first_begin + kCalibSpin / 2) return 0;
  int resident = 0;
  for (int i = 0; i < nb; i++) resident += t[2 * i] < first_end ? 1 : 0;
  const int got = resident / std::max(1, h->cu_count);
  return (got >= api - 2 && got >= 1) ? std::min(api, got) : 0;      // fewer: the device was not this launch's alone
}

// The ticket area (1 .. kTixAreas; 0: none) of the stream a search is enqueued on: k_search4, "The last rounds are DRAWN".
static uint32_t ticket_area(const Index *h, hipStream_t st) {
  if (st == hipStreamPerThread) return 0u;      // ONE handle value, a stream per host thread: launches "on it" may run side by side
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return 0u; }
  if (cs != hipStreamCaptureStatusNone) return 0u;      // a graph may be replayed on any stream, beside anything
  static_assert(sizeof(h->tix_owner) / sizeof(h->tix_owner[0]) == kTixAreas, "one owner per ticket area");
  std::lock_guard<std::mutex> lk(h->tix_mu);
  uint32_t free_at = 0;
  for (uint32_t i = 0; i < kTixAreas; i++) {
    if (h->tix_used[i] && h->tix_owner[i] == (void *)st) return i + 1u;
    if (!h->tix_used[i] && !free_at) free_at = i + 1u;
  }
  if (free_at) { h->tix_used[free_at - 1u] = true; h->tix_owner[free_at - 1u] = (void *)st; }
  return free_at;
}

// full rounds of batches that are drawn with the partial last one: 2 by measurement -- C5 0.318-0.320 / 0.314-0.316 /
// 0.315-0.316 ms, C3text 0.425 / 0.423 / 0.435 ms with 1 / 2 / 4: every drawn batch starts cold; again with the shorter
// ramp (profiles/ends_c3_ab.md): C3 0.1092 / 0.1104 / 0.1124 ms with 2 / 3 / 4
constexpr uint32_t kPoolRounds = 2;

// ---------------------------------------------------------------- which instantiation
// The handle's tables as a search finds them.
struct SearchTables {
  KTab kt;
  JumpView jt;                                     // the row jump table
  const unsigned long long *r3 = nullptr;          // the three-step row table
  const unsigned long long *r1 = nullptr;          // the frontier's row table (asked for only where there is neither of the two)
};

// The row tables are built by fmx_prepare or by the search that brings the handle's patterns to the threshold (fmx_jump.hip,
// tables_due); until then -- a per-call adapter's single queries -- every step is walked on the dictionary.  The search that
// finds them due builds them (it allocates and synchronises, fmx.h says so) and calibrates the kernels they select right
// away: later calls only enqueue.  cal: search_calibrate's call -- nothing is built.
static hipError_t search_tables(const Index *h, uint32_t k, hipStream_t st, bool cal, SearchTables *t) {
  hipError_t e = ktab_get(h, st, &t->kt, !cal && tables_due(h, k, true));
  if (e != hipSuccess) return e;
  bool built_now = false;
  const bool due = !cal && tables_due(h, k, false);
  if (due) built_now = !h->jump.decided();
  if ((e = jump_get(h, st, &t->jt, due)) != hipSuccess) return e;
  if (built_now) {
    const unsigned long long *r3b = nullptr;
    (void)row3_get(h, st, &r3b, true);
    if ((e = search_calibrate(h, st)) != hipSuccess) return e;
  }
  // beside the jump table, the three-step table serves the steps no aligned jump covers; without it, the three-step table or,
  // where the handle has that one already, the regex frontier's row table
  const unsigned long long *have1 = nullptr;
  if (!t->jt.tab) (void)row1_get(h, st, &have1, false);      // (only looks)
  if (!have1 && (e = row3_get(h, st, &t->r3, due)) != hipSuccess) return e;
  if (!t->jt.tab && !t->r3 && (e = row1_get(h, st, &t->r1, due)) != hipSuccess) return e;
  return hipSuccess;
}

// The template arguments of one k_search4 instantiation.
struct SearchPlan {
  bool wide;
  uint32_t layout, kt, jt, rw;
  bool r3t, g2, kx;
  bool operator==(const SearchPlan &o) const {
    return wide == o.wide && layout == o.layout && kt == o.kt && jt == o.jt && rw == o.rw && r3t == o.r3t && g2 == o.g2 && kx == o.kx;
  }
};

// With a row jump table the lane groups finish the one-row part themselves, eight steps per lookup, in lockstep (C3: 0.240 ms;
// handing it to k_search_rows: 0.248 ms -- both run at ~37 G requests/s, and the hand-over costs two more launches: C2 0.129 ->
// 0.155 ms).  Without one (it does not fit: C5, n = 2^34) a table of a third of the size serves it with one lane per pattern:
// the three-step row table, or the regex frontier's one-step row table where the handle has that one already (C5: 49 -> 75 G
// rank queries/s with R1).  g2: a pair of lanes per pattern instead of a quad (only where can_pair_lanes).
static SearchPlan plan_of(const Index *h, const SearchTables &t, bool g2) {
  SearchPlan p{h->layout == kLayoutBytes || h->n > (1ull << 32), h->layout, 0u, 0u, 0u, false, false, false};      // (FMX_LAYOUT_DISPATCH)
  // the search uses the k-mer table's levels in steps of four characters (all levels are kept: fmx_ktab.hip)
  p.kt = t.kt.k >= 12 ? 12u : t.kt.k >= 8 ? 8u : t.kt.k >= 4 ? 4u : 0u;
  if (t.jt.tab) {
    p.jt = t.jt.pairs ? 2u : 1u;      // (pairs are built from the three-step table: it is there)
    p.r3t = t.r3 != nullptr;
    p.g2 = g2;
    // level KT + 1 of the k-mer table (fmx_ktab.hip, build_kext) serves the kernels with pairs of row jump entries; "ktab_ext" =
    // "off" on the handle switches it off for its searches (the level stays until fmx_drop_tables)
    p.kx = t.kt.ext && t.kt.ext_k == p.kt && p.jt == 2u && p.r3t && !p.wide && h->policy.ktab_ext.load(std::memory_order_relaxed) != 0;
  } else {
    p.rw = t.r3 ? 3u : t.r1 ? 1u : 0u;
  }
  return p;
}

// Pairs of lanes serve the one-hot layout with a row jump table (single entries or pairs of them) and the three-step table.
static bool can_pair_lanes(const Index *h, const SearchTables &t) {
  return h->layout == kLayoutOneHot && t.jt.tab && t.r3 && h->policy.search_lanes.load(std::memory_order_relaxed) != 0;
}

// Large batches on the one-hot layout: a PAIR of lanes per pattern, 32 patterns per wave (k_search4<.., G2>) -- half the
// lockstep batches per wave; a batch that does not give every CU four workgroups of pairs keeps the quads, which spread it over
// twice the workgroups (C3 by batch size, pairs / quads: 125 k 0.0296 / 0.0335 ms, 250 k 0.0484 / 0.0493, 500 k 0.0751 /
// 0.0744, 1 M 0.127 / 0.133, 4 M 0.482 / 0.499).  "search_lanes" = "pairs" / "quads": whenever they can / never.
static SearchPlan select_plan(const Index *h, const SearchTables &t, uint64_t k) {
  const int lanes = h->policy.search_lanes.load(std::memory_order_relaxed);
  return plan_of(h, t, can_pair_lanes(h, t) && (lanes == 1 || k >= (uint64_t)h->cu_count * 512));
}

// The list of what exists, and per entry and device what its census found.
struct SearchForm {
  SearchPlan plan;
  void (*launch)(const Search4Args &, int, hipStream_t);
  int (*occupancy)();
#ifdef FMX_SEARCHLOG
  int (*searchlog)(void *, size_t);
#define FMX_SEARCHLOG_FN_(...) , &search4_searchlog<__VA_ARGS__>
#else
#define FMX_SEARCHLOG_FN_(...)
#endif
};
#define FMX_FORM_(W, L, KT, JT, RW, R3T, G2, KX)                                                                            \
  {{W, L, KT, JT, RW, R3T, G2, KX}, &search4_launch<W, L, KT, JT, RW, R3T, G2, KX>, &search4_occupancy<W, L, KT, JT, RW, R3T, G2, KX> \
   FMX_SEARCHLOG_FN_(W, L, KT, JT, RW, R3T, G2, KX)},
static const SearchForm kForms[] = {FMX_SEARCH4_LIST(FMX_FORM_)};
#undef FMX_FORM_
#undef FMX_SEARCHLOG_FN_
constexpr size_t kNumForms = sizeof(kForms) / sizeof(kForms[0]);
struct FormState {
  std::atomic<int> api{0};      // resident workgroups per CU by the occupancy query, 1 .. 8; 0 = not asked yet
  Residency res[16];            // by device
};
static FormState g_forms[kNumForms];
#ifdef FMX_SEARCHLOG
static std::atomic<const SearchForm *> g_last_form{nullptr};
#endif

// The entry of plan p (nullptr: no such instantiation -- a selection that does not match the list is a programming error).
static const SearchForm *find_form(const SearchPlan &p) {
  for (const SearchForm &f : kForms)
    if (f.plan == p) return &f;
  fprintf(stderr, "[fmx] no k_search4<%d,%u,%u,%u,%u,%d,%d,%d> in FMX_SEARCH4_LIST\n", (int)p.wide, p.layout, p.kt, p.jt, p.rw, (int)p.r3t, (int)p.g2, (int)p.kx);
  return nullptr;
}

// Resident workgroups per CU for an instantiation: the grid is sized to what is resident so that every group starts at once
// and the static batch striding stays balanced.
static int form_api(const SearchForm &f) {
  FormState &fs = g_forms[&f - kForms];
  int api = fs.api.load(std::memory_order_relaxed);
  if (!api) {
    api = std::min(8, std::max(1, f.occupancy()));
    fs.api.store(api, std::memory_order_relaxed);
  }
  return api;
}

// The kernel's arguments for the tables t; a search's own pattern, output and flags are filled in by the caller.
static Search4Args form_args(const Index *h, const SearchPlan &p, const SearchTables &t) {
  Search4Args a{};
  a.ix = h->dev;
  a.ktab = p.kt ? t.kt.level[p.kt - 1] : nullptr;
  a.kdense = t.kt.dense;
  a.ksigma = t.kt.sigma;
  a.kext = p.kx ? t.kt.ext : nullptr;
  a.kovf = p.kx ? t.kt.ovf : nullptr;
  a.jtab = t.jt.tab;
  a.jc = t.jt.chars;
  a.r3tab = p.rw == 1u ? t.r1 : (p.r3t || p.rw == 3u) ? t.r3 : nullptr;      // (the one-step table is passed in the same argument)
  a.counters = h->d_counters;
  return a;
}

// The residency census of one instantiation on h's device, once (see Residency above).
static hipError_t calibrate_form(const Index *h, const SearchPlan &p, const SearchTables &t, hipStream_t st) {
  const SearchForm *f = find_form(p);
  if (!f) return hipErrorInvalidValue;
  const int api = form_api(*f);
  const int forced = knobs().wgs ? std::min(knobs().wgs, api) : 0;
  Residency &rs = g_forms[f - kForms].res[(unsigned)h->device & 15u];
  std::lock_guard<std::mutex> lk(rs.mu);
  if (!forced && !rs.admitted.load() && h->cu_count * api <= (int)kCensusBlocks) {
    // scratch behind the census entries: two zero words (the offsets of one empty pattern) and the two output words
    unsigned long long *scr = h->d_counters + (kCounterBytes + kCensusBytes) / 8;
    const int grid = h->cu_count * api;
    { const hipError_t e0 = hipMemsetAsync(scr, 0, kCalibScratchBytes, st); if (e0 != hipSuccess) return e0; }      // (the offsets MUST be zeros: the kernel reads pat[off])
    Search4Args a = form_args(h, p, t);
    a.pat = (const uint8_t *)h->d_bwt;
    a.po = PatOff{(const uint64_t *)scr, 0ull};
    a.sp_out = (uint64_t *)(scr + 2);
    a.ep_out = (uint64_t *)(scr + 3);
    a.k = 1u;
    a.pk_cap = ~0ull;
    a.spin = kCalibSpin;
    int last = 0, got = 0;
    for (int attempt = 0; attempt < 4 && !rs.admitted.load(); attempt++) {
      f->launch(a, grid, st);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      got = census_read(h, grid, api, st);
      if (knobs().trace) fprintf(stderr, "[fmx] k_search4<%d,%u,%u,%d,%u,%d,%d,%d> census: %d of the %d workgroups per CU the occupancy query allows were resident\n",
                                 (int)p.wide, p.layout, p.kt, (int)p.jt, p.rw, (int)p.r3t, (int)p.g2, (int)p.kx, got, api);
      if (got && got == last) rs.admitted.store(got);
      last = got;
    }
    if (!rs.admitted.load()) rs.admitted.store(-1);      // no two agreeing readings (a shared device): the query's answer stands, and is not asked again
  }
  const int m = rs.admitted.load();
  h->search_residency.store(forced ? ((uint32_t)forced | 0x100u) : ((uint32_t)(m > 0 ? m : api) | (m > 0 ? 0x100u : 0u)));
  return hipSuccess;
}

// ONE launch in every configuration (round 5: the kernels without a row jump table used to be followed by k_search_rows and
// k_search_defer); the 8-byte form, where asked for, is written by the kernel itself.
static hipError_t launch_form(const Index *h, const SearchPlan &p, const SearchTables &t, const uint8_t *pat, const PatOff off,
                              uint64_t *sp, uint64_t *ep, uint32_t k, hipStream_t st, uint64_t pk_cap, uint32_t flags) {
  const SearchForm *f = find_form(p);
  if (!f) return hipErrorInvalidValue;
  const int api = form_api(*f);
  const int forced = knobs().wgs ? std::min(knobs().wgs, api) : 0;
  const int measured = std::max(0, g_forms[f - kForms].res[(unsigned)h->device & 15u].admitted.load());
  const int per_cu = forced ? forced : (measured ? measured : api);
  const uint32_t G = p.g2 ? 2u : p.layout == kLayoutBytes ? 8u : 4u;      // lanes per pattern (Lay<LAYOUT>::G)
  const uint64_t per_wg = kSThreads / G;
  const uint64_t want = ((uint64_t)k + per_wg - 1) / per_wg;
  const uint64_t cap = (uint64_t)h->cu_count * per_cu;
  const int grid = (int)(want < cap ? (want ? want : 1) : cap);
  h->search_residency.store((uint32_t)per_cu | ((forced || measured) ? 0x100u : 0u));
  const uint32_t area = ticket_area(h, st);
  if (knobs().trace) {      // (what the kernel will make of it: k_search4, "The last rounds are DRAWN")
    const uint64_t Pw = 64u / G, nbatch = ((uint64_t)k + Pw - 1) / Pw, nw = (uint64_t)grid * (kSThreads / 64), rounds = nbatch / nw;
    const bool pooled = (p.g2 || p.rw != 0u) && area && rounds >= kPoolRounds + 2u;
    fprintf(stderr, "[fmx] k_search4<%d,%u,%u,%d,%u,%d,%d,%d>: %llu batches over %llu waves, the last %llu drawn from ticket area %u\n", (int)p.wide, p.layout, p.kt,
            (int)p.jt, p.rw, (int)p.r3t, (int)p.g2, (int)p.kx, (unsigned long long)nbatch, (unsigned long long)nw,
            (unsigned long long)(pooled ? nbatch - (rounds - kPoolRounds) * nw : 0), pooled ? area : 0u);
  }
  Search4Args a = form_args(h, p, t);
  a.pat = pat;
  a.po = off;
  a.sp_out = sp;
  a.ep_out = ep;
  a.k = k;
  a.pk_cap = pk_cap;
  a.spin = (area << 16) | (kPoolRounds << 24) | ((flags & kSearchMissNone) ? 0x80000000u : 0u);
  f->launch(a, grid, st);
#ifdef FMX_SEARCHLOG
  g_last_form.store(f);
#endif
  return hipGetLastError();
}

// One launch per call: no scratch, nothing to own per stream, so concurrent calls on one handle need no lock.
// d_off == nullptr: a batch of k patterns of fixed_len bytes each, one behind the other (fmx_search_opts.fixed_len).
// pack_cap != ~0: the intervals in the 8-byte form (fmx.h) with room for pack_cap escape entries -- d_sp receives the
// packed words (its first k words double as the kernels' sp array where a set of kernels cannot pack by itself), d_ep is
// scratch.
hipError_t launch_search(const Index *h, const void *d_pat, const void *d_off, void *d_sp, void *d_ep, uint64_t k,
                         hipStream_t st, uint32_t fixed_len, uint64_t pack_cap, uint32_t flags) {
  if (pack_cap != ~0ull) {       // the count of wide intervals (word k): zero before anything appends to the list
    const hipError_t e0 = hipMemsetAsync(static_cast<unsigned long long *>(d_sp) + k, 0, 8, st);
    if (e0 != hipSuccess) return e0;
  }
  if (!k) return hipSuccess;
  const PatOff po{d_off ? (const uint64_t *)d_off : (const uint64_t *)h->d_cf, d_off ? 0ull : (uint64_t)fixed_len};
  if (k > 0xFFFFFFF0ull) {       // (k_search4 counts patterns in 32 bits)
    hipError_t e1 = launch_search_v1(h, d_pat, po, d_sp, d_ep, k, st);
    if (e1 == hipSuccess && pack_cap != ~0ull) e1 = launch_pack_intervals(h, d_sp, d_ep, k, pack_cap, d_sp, st);
    return e1;
  }
  SearchTables t;
  const hipError_t e = search_tables(h, (uint32_t)k, st, false, &t);
  if (e != hipSuccess) return e;
  return launch_form(h, select_plan(h, t, k), t, (const uint8_t *)d_pat, po, (uint64_t *)d_sp, (uint64_t *)d_ep, (uint32_t)k, st, pack_cap, flags);
}

// The residency census of the k_search4 instantiations this handle's tables select now (see Residency above): which one a
// search takes depends on its size, so both the pairs of lanes (first) and the quads are calibrated where there are both.
hipError_t search_calibrate(const Index *h, hipStream_t st) {
  SearchTables t;
  hipError_t e = search_tables(h, 1u, st, true, &t);
  if (e != hipSuccess) return e;
  if (can_pair_lanes(h, t) && (e = calibrate_form(h, plan_of(h, t, true), t, st)) != hipSuccess) return e;
  return calibrate_form(h, plan_of(h, t, false), t, st);
}

}  // namespace fmx

#ifdef FMX_SEARCHLOG
// the log of the last k_search4 launch (each unit that instantiates it keeps its own: the one of the last launch's entry)
extern "C" int fmx_debug_searchlog(void *out, size_t bytes) {
  const fmx::SearchForm *f = fmx::g_last_form.load();
  return f ? f->searchlog(out, bytes) : -1;
}
#endif
