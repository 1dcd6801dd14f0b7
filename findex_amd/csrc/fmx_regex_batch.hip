// fmx_regex_batch.hip -- the regex frontier's host side: a batch of compiled regexes made resident on a device
// (regex_batch_create), the match call that drives the kernels of fmx_frontier.hip over it (regex_batch_match), the
// same for several GPUs in one process, and the regex C ABI: fmx_regex_compile and its relatives, the
// fmx_regex_batch_* / fmx_regex_match_batch entry points.
#include <fmx.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fmx_frontier.h"
#include "fmx_hostpar.h"
#include "fmx_regex.h"

namespace fmx {

// ---- Environment knobs of the regex frontier's host side: diagnostics, A/B runs and tests, none needed in
// production.  Read once per process.
struct FrontierKnobs {
  bool trace;              // FMX_TRACE: host-side timings of a call on stderr
  // FMX_FRONTIER_TAG_LIMIT: the bound on the queue's generation tags at which the queue is zeroed (count_tags); a test
  // makes the tags wrap within a few calls
  uint32_t tag_limit;
  // FMX_FRONTIER_CHAIN: launches per chain on the full grid.  One: a batch like C4 is done by one, and a second launch
  // that finds nothing costs ~8 us with its advance kernel (0.4170 -> 0.4109 ms per call); a search that needs more
  // pays a host look per launch
  uint32_t chain;
  // FMX_FRONTIER_ROUNDS: rounds a wave works at most in one launch (what it still holds then goes to the queue): the
  // bound that makes every wave end.  C4 is done in one launch of ~50 rounds per wave (the longest wave: 113);
  // measured 64 / 96 / 128 / 256: 0.565 / 0.548 / 0.527 / 0.534 ms
  uint32_t rounds;
  // FMX_FRONTIER_WGS: workgroups per CU in the full grid: what is resident at once (FMX_FWAVES waves per SIMD) -- a
  // launch lasts as long as the search does, so a second generation of workgroups would find nothing (measured 3 / 4
  // / 6: 0.567 / 0.712 / 0.664 ms)
  int wgs;
  // FMX_FRONTIER_CHAIN_SMALL, FMX_FRONTIER_ROUNDS_SMALL: the same for the small grid.  Its chain is short: a launch
  // that finds nothing to do still costs ~3 us.  The small grid serves a single regex or the thin end of a batch: there
  // a search is a few elements that grow into a tree, and what spreads it over the waves is the hand-over at the end
  // of a launch -- short launches, more of them (a[ab]*c on 2 M rows: 302 us per call with 128-round launches, 250
  // with 32; a 24-character literal: 87 / 95 us)
  uint32_t chain_small, rounds_small;
  // FMX_FRONTIER_PRERESET=0: a call resets its batch by launch instead of finding it left ready by the call before
  // (RegexBatch::pre_ok); the only way a test can run the reset-by-launch form over many calls
  bool prereset;
  // FMX_FRONTIER_DEEP: steps past ceil(log_sigma n) at which an element counts as deep.  Without effect now: the value
  // still travels to FrontierCtl::deep_len, but the express pool that read it is gone
  int deep_extra;
  bool export_direct;      // FMX_EXPORT_DIRECT=0: device-resident results are grouped in the batch's own buffer, then copied (A/B runs)
  bool balance;            // FMX_FRONTIER_BALANCE=0: a batch's start elements stay in regex order (A/B runs)
};
static int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}
static FrontierKnobs read_knobs() {
  FrontierKnobs k;
  k.trace = getenv("FMX_TRACE") != nullptr;
  k.tag_limit = (uint32_t)std::max(1, env_int("FMX_FRONTIER_TAG_LIMIT", (int)kTagLimit));
  k.chain = (uint32_t)std::max(1, env_int("FMX_FRONTIER_CHAIN", 1));
  k.rounds = (uint32_t)std::max(1, env_int("FMX_FRONTIER_ROUNDS", 128));
  k.wgs = std::max(1, env_int("FMX_FRONTIER_WGS", FMX_FWAVES));
  k.chain_small = (uint32_t)std::max(1, env_int("FMX_FRONTIER_CHAIN_SMALL", 2));
  k.rounds_small = (uint32_t)std::max(1, env_int("FMX_FRONTIER_ROUNDS_SMALL", 32));
  k.prereset = env_int("FMX_FRONTIER_PRERESET", 1) != 0;
  k.deep_extra = env_int("FMX_FRONTIER_DEEP", 2);
  k.export_direct = env_int("FMX_EXPORT_DIRECT", 1) != 0;
  k.balance = env_int("FMX_FRONTIER_BALANCE", 1) != 0;
  return k;
}
static const FrontierKnobs &knobs() {
  static const FrontierKnobs k = read_knobs();
  return k;
}

// Copies go through the caller's own (non-blocking) stream and wait for it: a plain hipMemcpy runs on the legacy
// stream, which implicitly waits for every blocking stream -- an error while a caller captures a graph in another host thread.
static hipError_t copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

// Expected number of frontier elements a regex makes on an index of n rows over sigma symbols whose BWT looks random:
// an element at depth d (characters matched so far) holds an interval of about n / sigma^d rows; its step survives
// with probability min(1, rows / sigma), and a surviving element pushes its follows.  Summed over depths until the
// expectation has died away.  Used to deal the start elements to the waves so that every wave gets about the same
// amount of work (a starred class next to the regex's end is a few hundred elements, one next to its beginning a
// handful), and to cut a batch into slices for several GPUs.
static double frontier_work_estimate(const Regex &re, double n, double sigma, std::vector<double> &cur, std::vector<double> &nxt) {
  const size_t ns = re.st_c.size();
  if (!ns || re.firsts.empty()) return 1.0;
  cur.assign(ns, 0.0);
  for (int32_t f : re.firsts) cur[(size_t)f] += 1.0;
  double work = 0.0, rows = n;
  if (sigma < 2.0) sigma = 2.0;
  for (int depth = 0; depth < 48; depth++) {
    const double p = std::min(1.0, rows / sigma);      // the step at this depth survives
    rows = std::max(1.0, rows / sigma);
    nxt.assign(ns, 0.0);
    double level = 0.0, alive = 0.0;
    for (size_t s = 0; s < ns; s++) {
      const double c = cur[s];
      if (c == 0.0) continue;
      level += c;
      if (re.last_stops && re.st_last[s]) continue;
      const double live = c * p;
      for (int32_t j = re.fol_off[s]; j < re.fol_off[s + 1]; j++) { nxt[(size_t)re.fol[j]] += live; alive += live; }
    }
    work += level;
    if (alive < 1e-3) break;
    if (work > 1e9) break;
    cur.swap(nxt);
  }
  return work;
}

// The order of a batch's start elements.  Element i belongs to slice i % kSub (StartSrc), and a launch hands slice s's entries to the waves s, s + kSub, s + 2 kSub .. in contiguous chunks
// (frontier_pass): which wave gets element i is a function of i, the element count and the number of waves.  The
// elements are sorted by expected work and dealt to the waves in serpentine passes (heaviest first), so the waves'
// totals come out even; the element order itself carries no meaning (results are grouped by regex afterwards).
static void balanced_start_order(const std::vector<double> &work, size_t waves, std::vector<uint32_t> &perm /* position -> element */) {
  const size_t count = work.size();
  perm.resize(count);
  std::vector<uint32_t> by_work(count);
  for (size_t i = 0; i < count; i++) by_work[i] = (uint32_t)i;
  std::stable_sort(by_work.begin(), by_work.end(), [&](uint32_t a, uint32_t b) { return work[a] > work[b]; });
  if (waves < kSub) waves = kSub;
  std::vector<std::vector<uint32_t>> pos(waves);
  for (size_t i = 0; i < count; i++) {
    const size_t s = i % kSub, j = i / kSub;
    const size_t cnt_s = count > s ? (count - s + kSub - 1) / kSub : 0;
    const size_t class_waves = (waves - s + kSub - 1) / kSub;
    const size_t chunk = (cnt_s + class_waves - 1) / class_waves;
    size_t w = s + kSub * (chunk ? j / chunk : 0);
    if (w >= waves) w = s;
    pos[w].push_back((uint32_t)i);
  }
  size_t next = 0;
  for (size_t pass = 0; next < count; pass++) {
    for (size_t q = 0; q < waves; q++) {
      const size_t w = (pass & 1u) ? waves - 1 - q : q;
      if (pass < pos[w].size()) perm[pos[w][pass]] = by_work[next++];
    }
  }
}

int regex_batch_create(const Index *h, const Regex *const *res, size_t k, RegexBatch **out) {
  // Sizes first (per regex, then one prefix sum), then every regex fills its own stretch of the pre-sized arrays:
  // both passes run on all host cores (100 k regexes: 1.3 M states, 2 M follows).
  std::vector<size_t> st_base(k + 1, 0), fol_base(k + 1, 0), first_base(k + 1, 0);
  std::atomic<int> not_retree{0}, too_many{0};
  parallel_for(k, 1024, [&](size_t a, size_t b) {
    for (size_t r = a; r < b; r++) {
      const Regex &re = *res[r];
      size_t nf = 0;
      for (size_t s = 0; s < re.st_c.size(); s++)
        if (!(re.last_stops && re.st_last[s])) {
          const size_t cnt = (size_t)(re.fol_off[s + 1] - re.fol_off[s]);
          if (cnt > kMaxFollows) too_many.store(1);
          nf += cnt;
        }
      st_base[r + 1] = re.st_c.size();
      fol_base[r + 1] = nf;
      first_base[r + 1] = re.firsts.size();
      if (re.engine != 0) not_retree.store(1);
    }
  });
  if (too_many.load()) { set_error("a state has more than 65535 follows"); return FMX_ERR_UNSUPPORTED; }
  for (size_t r = 0; r < k; r++) { st_base[r + 1] += st_base[r]; fol_base[r + 1] += fol_base[r]; first_base[r + 1] += first_base[r]; }
  const size_t n_states = st_base[k], n_fol = fol_base[k], n_first = first_base[k];
  if (n_states >= (1ull << 32) || n_fol >= (1ull << 32)) { set_error("regex batch too large (2^32 states or follows)"); return FMX_ERR_UNSUPPORTED; }
  const bool all_retree = not_retree.load() == 0;
  std::vector<StateRec> recs(n_states);
  std::vector<uint32_t> fol(n_fol), q_state(n_first), st_num(n_states), first_off(k + 1, 0), start_final;
  std::vector<uint8_t> fol_c(n_fol);
  std::vector<uint32_t> fanout(k, 1);
  std::vector<double> elem_work(n_first, 1.0);
  const double est_n = (double)h->n, est_sigma = (double)std::max<uint32_t>(h->nslots, 2u);
  parallel_for(k, 1024, [&](size_t ra, size_t rb) {
    std::vector<double> dp_a, dp_b;
    for (size_t r = ra; r < rb; r++) {
      const Regex &re = *res[r];
      const size_t base = st_base[r];
      if (!re.firsts.empty()) {
        const double w = frontier_work_estimate(re, est_n, est_sigma, dp_a, dp_b) / (double)re.firsts.size();
        for (size_t f = 0; f < re.firsts.size(); f++) elem_work[first_base[r] + f] = w;
      }
      size_t fo = fol_base[r], qo = first_base[r];
      uint32_t max_fanout = 1;
      for (size_t s = 0; s < re.st_c.size(); s++) {
        StateRec &rec = recs[base + s];
        rec.fol_off = (uint32_t)fo;
        // ReTree: `if (q.state.isLast) ret ::= ... else pqFront ++= follows` -- last states do not expand
        if (!(re.last_stops && re.st_last[s]))
          for (int32_t j = re.fol_off[s]; j < re.fol_off[s + 1]; j++) {
            fol_c[fo] = re.st_c[(size_t)re.fol[j]];
            fol[fo++] = (uint32_t)base + (uint32_t)re.fol[j];
          }
        const uint32_t cnt = (uint32_t)fo - rec.fol_off;
        rec.cnt_c_emit = cnt | ((uint32_t)re.st_c[s] << 16) | ((uint32_t)(re.st_last[s] ? 1 : 0) << 24);
        rec.regex = (uint32_t)r;
        rec.fc = 0;
        for (uint32_t j = 0; j < kInlineFollows; j++) {
          rec.f[j] = j < cnt ? fol[rec.fol_off + j] : 0u;
          if (j < cnt) rec.fc |= (uint32_t)fol_c[rec.fol_off + j] << (8 * j);
        }
        st_num[base + s] = (uint32_t)re.st_num[s];
        max_fanout = std::max(max_fanout, cnt);
      }
      // literal stretches (fmx_nfa.h): chain lengths from the regex's last state backwards, then the bytes
      {
        const size_t ns = re.st_c.size();
        auto single = [&](size_t s) {
          const StateRec &rec = recs[base + s];
          return rec_cnt(rec) == 1 && !rec_emit(rec) && s + 1 < ns && rec.f[0] == (uint32_t)(base + s + 1);
        };
        uint32_t next_chain = 0;
        for (size_t s = ns; s-- > 0;) {
          const uint32_t chain = single(s) ? std::min<uint32_t>(kMaxChain, 1 + next_chain) : 0;
          next_chain = chain;
          if (!chain) continue;
          StateRec &rec = recs[base + s];
          rec.cnt_c_emit |= chain << 25;
          uint8_t rr[kMaxChain] = {0};
          for (uint32_t j = 0; j < chain; j++) rr[chain - 1 - j] = re.st_c[s + 1 + j];
          std::memcpy(&rec.f[1], rr, kMaxChain);
        }
      }
      for (int32_t f : re.firsts) q_state[qo++] = (uint32_t)base + (uint32_t)f;
      first_off[r + 1] = (uint32_t)qo;
      fanout[r] = std::max<uint32_t>(max_fanout, (uint32_t)re.firsts.size());
    }
  });
  uint32_t max_fanout = 1;
  for (size_t r = 0; r < k; r++) {
    max_fanout = std::max(max_fanout, fanout[r]);
    if (res[r]->start_is_final) start_final.push_back((uint32_t)r);
  }
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  CtxLease lease(h);
  if (!lease.c) return FMX_ERR_HIP;
  hipStream_t st = lease.c->stream;
  std::unique_ptr<RegexBatch> b(new RegexBatch());
  b->device = h->device;
  b->k = k;
  b->index_serial = h->serial;
  b->n_first = q_state.size();
  b->n_states = n_states;
  b->n_fol = n_fol;
  b->start_final = start_final;
  b->max_fanout = max_fanout;
  b->all_retree = all_retree;
  StateRec *d_st = nullptr;
  uint32_t *d_fol = nullptr;
  uint8_t *d_fol_c = nullptr;
  HIP_TRY(b->mem.alloc(&d_st, recs.size()), "hipMalloc");
  HIP_TRY(b->mem.alloc(&d_fol, fol.size()), "hipMalloc");
  HIP_TRY(b->mem.alloc(&d_fol_c, fol_c.size() + 4), "hipMalloc");
  if (!fol_c.empty()) HIP_TRY(copy_sync(d_fol_c, fol_c.data(), fol_c.size(), hipMemcpyHostToDevice, st), "H2D");
  HIP_TRY(b->mem.alloc(&b->d_first_state, q_state.size()), "hipMalloc");
  if (!recs.empty()) HIP_TRY(copy_sync(d_st, recs.data(), recs.size() * sizeof(StateRec), hipMemcpyHostToDevice, st), "H2D");
  if (!fol.empty()) HIP_TRY(copy_sync(d_fol, fol.data(), fol.size() * 4, hipMemcpyHostToDevice, st), "H2D");
  if (!q_state.empty()) HIP_TRY(copy_sync(b->d_first_state, q_state.data(), q_state.size() * 4, hipMemcpyHostToDevice, st), "H2D");
  {   // the frontier kernel's start elements, in the order that balances the waves (the full grid's wave count)
    std::vector<uint32_t> perm, q_perm(q_state.size());
    if (knobs().balance && !q_state.empty()) {
      balanced_start_order(elem_work, (size_t)std::max(1, h->cu_count * FMX_FWAVES * 4 / kFWaves) * kFWaves, perm);
      for (size_t i = 0; i < q_state.size(); i++) q_perm[i] = q_state[perm[i]];
    } else {
      q_perm = q_state;
    }
    // element i belongs to slice i % kSub, position i / kSub (what balanced_start_order assumed)
    b->start_cap = (q_perm.size() + kSub - 1) / kSub;
    std::vector<unsigned long long> elem((size_t)b->start_cap * kSub, 0ull);
    for (size_t i = 0; i < q_perm.size(); i++)
      elem[(i % kSub) * b->start_cap + i / kSub] = (unsigned long long)q_perm[i] | ((unsigned long long)rec_c(recs[q_perm[i]]) << 40);
    HIP_TRY(b->mem.alloc(&b->d_start_elem, elem.size()), "hipMalloc");
    if (!elem.empty()) HIP_TRY(copy_sync(b->d_start_elem, elem.data(), elem.size() * 8, hipMemcpyHostToDevice, st), "H2D");
  }
  if (all_retree) {
    HIP_TRY(b->mem.alloc(&b->d_st_num, st_num.size()), "hipMalloc");
    HIP_TRY(b->mem.alloc(&b->d_first_off, first_off.size()), "hipMalloc");
    if (!st_num.empty()) HIP_TRY(copy_sync(b->d_st_num, st_num.data(), st_num.size() * 4, hipMemcpyHostToDevice, st), "H2D");
    HIP_TRY(copy_sync(b->d_first_off, first_off.data(), first_off.size() * 4, hipMemcpyHostToDevice, st), "H2D");
    // the reference-order kernel's push records (fmx_nfa.h)
    std::vector<FolRec> fr(fol.size()), qr(q_state.size());
    auto rec_of = [&](uint32_t sid) { return FolRec{recs[sid].fc, recs[sid].fol_off, recs[sid].cnt_c_emit & 0x01FFFFFFu, st_num[sid]}; };
    parallel_for(fol.size(), 1 << 16, [&](size_t a, size_t e) { for (size_t i = a; i < e; i++) fr[i] = rec_of(fol[i]); });
    for (size_t i = 0; i < q_state.size(); i++) qr[i] = rec_of(q_state[i]);
    uint32_t mx = 0;
    for (uint32_t v : st_num) mx = std::max(mx, v);
    b->max_num = mx;
    HIP_TRY(b->mem.alloc(&b->d_fol_rec, fr.size()), "hipMalloc");
    HIP_TRY(b->mem.alloc(&b->d_first_rec, qr.size()), "hipMalloc");
    if (!fr.empty()) HIP_TRY(copy_sync(b->d_fol_rec, fr.data(), fr.size() * sizeof(FolRec), hipMemcpyHostToDevice, st), "H2D");
    if (!qr.empty()) HIP_TRY(copy_sync(b->d_first_rec, qr.data(), qr.size() * sizeof(FolRec), hipMemcpyHostToDevice, st), "H2D");
  }
  b->nfa = NfaTables{d_st, d_fol, d_fol_c};
  *out = b.release();
  return FMX_OK;
}

// ---- the match call

struct CallTrace {       // FMX_TRACE: host-side timings of a call on stderr
  std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  void mark(const char *what) const {
    if (knobs().trace) fprintf(stderr, "[fmx] regex_batch_match %-18s +%.3f ms\n", what,
                               std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  }
};

static int ok_or_truncated(bool truncated) {
  if (!truncated) return FMX_OK;
  set_error("some matches run past max_steps: results hold every match of length <= max_steps");
  return FMX_TRUNCATED;
}

// slices: each holds its share of max_frontier plus a quarter of headroom (appends rotate over the slices,
// so they fill evenly, not exactly); the result segments get 4x their share
static uint64_t sub_cap_of(uint64_t qcap) { return (qcap + kSub - 1) / kSub + qcap / (4 * kSub) + 1024; }
static uint64_t seg_cap_of(size_t rcap) { return (uint64_t)rcap / 16 + 1024; }

// The batch's scratch: the queue, the result buffers and the counters, kept from call to call while the limits fit.
static int ensure_scratch(RegexBatch *b, uint64_t qcap, size_t cap) {
  const size_t rcap = cap ? cap : 1;
  if (b->scratch && b->qcap == qcap && b->rcap >= rcap) return FMX_OK;
  b->scratch.reset(new DevMem());
  b->qcap = 0;
  if (!b->h_tot) HIP_TRY(hipHostMalloc((void **)&b->h_tot, sizeof(GroupTotals), hipHostMallocDefault), "hipHostMalloc(totals)");
  if (!b->h_sum) HIP_TRY(hipHostMalloc((void **)&b->h_sum, sizeof(FrontierSummary), hipHostMallocDefault), "hipHostMalloc(summary)");
  if (!b->h_args) HIP_TRY(hipHostMalloc((void **)&b->h_args, sizeof(CallArgs), hipHostMallocDefault), "hipHostMalloc(export)");
  for (unsigned long long **g : {&b->fq.g0, &b->fq.g1, &b->fq.g2}) {
    HIP_TRY(b->scratch->alloc(g, 2 * kSub * sub_cap_of(qcap)), "hipMalloc(queue)");
  }
  HIP_TRY(b->scratch->alloc(&b->d_res, rcap), "hipMalloc(results)");
  HIP_TRY(b->scratch->alloc(&b->d_res_seg, kSub * seg_cap_of(rcap)), "hipMalloc(result slices)");
  HIP_TRY(b->scratch->alloc(&b->d_ctl, 1), "hipMalloc(ctl)");
  b->tag_bound = ~0u;                // new memory: zeroed before it is used (tag 0 = never written)
  {   // counts, fill cursors and the big-group list in one block
    uint32_t *blk = nullptr;
    HIP_TRY(b->scratch->alloc(&blk, 3 * (b->k + 1) + (sizeof(BigGroups) + 3) / 4), "hipMalloc(result counts)");
    b->d_rcnt2[0] = blk;
    b->d_rcnt2[1] = blk + 2 * (b->k + 1);
    b->d_rcnt = blk;
    b->rc_sel = 0;
    b->pre_ok = false;
    b->d_rfill = blk + (b->k + 1);
    b->d_big = reinterpret_cast<BigGroups *>(blk + 3 * (b->k + 1));
  }
  HIP_TRY(b->scratch->alloc(&b->d_rstart, b->k + 1), "hipMalloc(result offsets)");
  HIP_TRY(b->scratch->alloc(&b->d_rpart, (b->k + 1) / kScanChunk + 2), "hipMalloc(scan parts)");
  b->qcap = qcap;
  b->rcap = rcap;
  return FMX_OK;
}

// ---- The queue's generation tags.  INVARIANT: b->tag_bound >= the largest generation tag any buffer can hold.
// Tags are 16 bits wide and wrap at 65535; long before a tag can come round to a value that an old entry still carries
// -- when the bound reaches FrontierKnobs::tag_limit -- the queue and the tags are zeroed (a 100 MB memset every few
// tens of thousands of calls).  A buffer's tag advances by at most one in each of three places:
//   * the reset launch that begins a call (k_frontier_reset with CallArgs::fresh; not launched under pre_now, when
//     the advance was the pre-reset of the call before and was counted there);
//   * every launch of a chain (k_frontier_advance rewinds a buffer that has been emptied);
//   * the pre-reset of a call that leaves the batch ready (k_res_sort's last workgroup, behind the chain that ends
//     the search).
// count_tags adds all three for one chain, and it does so before the chain is enqueued, so that no return path, an
// error's included, leaves an advance uncounted.  Under pre_next it counts the pre-reset behind every chain although
// only a call's last chain does one: over-counting only brings the zeroing forward, under-counting lets a tag wrap.
static void count_tags(RegexBatch *b, const CallPlan &p, const ChainShape &shape, bool first_chain) {
  b->tag_bound += (first_chain && !p.pre_now ? 1u : 0u) + shape.launches + (p.pre_next ? 1u : 0u);
}
static int zero_queue_if_due(RegexBatch *b, hipStream_t st) {
  if (b->tag_bound < knobs().tag_limit) return FMX_OK;
  for (unsigned long long *g : {b->fq.g0, b->fq.g1, b->fq.g2})
    HIP_TRY(hipMemsetAsync(g, 0, 2 * kSub * sub_cap_of(b->qcap) * 8, st), "hipMemset(queue)");
  HIP_TRY(hipMemsetAsync(b->d_ctl, 0, sizeof(FrontierCtl), st), "hipMemset(ctl)");
  b->tag_bound = 0;
  b->pre_ok = false;                 // (whatever the last call left ready is gone: this call resets by launch)
  return FMX_OK;
}

// page-locked caller buffers are written by the device itself (k_res_export, the last launch of the grouping)
static bool pinned(const void *p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

// Fills in the call's plan (p.kt is there already) and its page-locked arguments.
static void plan_call(const Index *h, RegexBatch *b, uint32_t max_steps, fmx_result *out, size_t cap, uint32_t *per_regex_count, bool dev, CallPlan &p) {
  const FrontierKnobs &kn = knobs();
  p.max_len = max_steps;
  p.sub_cap = sub_cap_of(b->qcap);
  // a function of the ALLOCATED size: the result slices keep theirs when a later call passes a smaller cap
  p.seg_cap = seg_cap_of(b->rcap);
  p.full = ChainShape{std::max(1, h->cu_count * kn.wgs * 4 / kFWaves), kn.chain, kn.rounds};      // wgs counts 256-thread units
  p.small = ChainShape{std::max(1, 256 / kFWaves), kn.chain_small, kn.rounds_small};              // 256 waves
  p.ss = StartSrc{b->d_start_elem, b->start_cap, p.kt.k ? 0 : h->n};
  // ceil(log_sigma n) steps narrow an interval to a single row (no kernel reads deep_len now: FrontierCtl)
  const double sig = (double)std::max<uint32_t>(h->nslots, 2u);
  p.deep_len = (uint32_t)std::max(1.0, std::ceil(std::log((double)h->n + 1.0) / std::log(sig)) + kn.deep_extra);
  p.pre_next = kn.prereset;
  if (p.pre_next && b->pre_ok) b->rc_sel ^= 1u;          // the array the last call's scan zeroed
  if (!p.pre_next) b->rc_sel = 0;
  b->d_rcnt = b->d_rcnt2[b->rc_sel];
  p.pre_now = p.pre_next && b->pre_ok && b->pre_max_len == max_steps && b->pre_deep == p.deep_len && b->pre_count == b->n_first &&
              b->pre_ss.elem == p.ss.elem && b->pre_ss.cap == p.ss.cap && b->pre_ss.ep == p.ss.ep;
  b->pre_ok = false;                         // until this call has ended normally
  p.export_out = cap && (dev || (pinned(out) && pinned(out + (cap - 1))));
  p.export_per = per_regex_count && b->k && (dev || (pinned(per_regex_count) && pinned(per_regex_count + (b->k - 1))));
  p.direct = dev && p.export_out && kn.export_direct;
  CallArgs &a = *b->h_args;
  a.out = p.export_out ? out : nullptr;
  a.cap = cap;
  a.per = p.export_per ? per_regex_count : nullptr;
  a.max_len = max_steps;
  a.fresh = 1;
  a.direct = p.direct ? 1u : 0u;
  a.deep_len = p.deep_len;
}

// The call's chains: each is enqueued with the grouping behind it, then the host looks at the summary; a search that
// is not over goes on with the next chain, on the small grid when what is queued fits its lanes.
static int run_chains(const Index *h, RegexBatch *b, const CallPlan &p, CallCtx *c, const CallTrace &tr, FrontierSummary &sum) {
  hipStream_t st = c->stream;
  const uint64_t small_total = (uint64_t)p.small.grid * kFThreads;     // elements the small grid's workgroups hold at once
  uint64_t total = b->n_first;               // elements queued for the next launch
  uint64_t launches = 1;
  uint32_t pass = 0;
  do {
    const ChainShape &shape = total <= small_total ? p.small : p.full;
    count_tags(b, p, shape, b->h_args->fresh != 0);
    HIP_TRY(enqueue_chain(h, b, p, shape, st), "k_frontier chain");
    HIP_TRY(enqueue_group(b, p, st), "result grouping kernels");
    HIP_TRY(hipEventRecord(c->ev_b, st), "hipEventRecord");
    launches += 2 * shape.launches + (p.direct ? 3 : 4);
    HIP_TRY(hipStreamSynchronize(st), "sync(passes)");
    b->h_args->fresh = 0;              // further chains of this call continue the search
    sum = *b->h_sum;
    pass += shape.launches;
    if (sum.overflow & 4ull) { set_error("frontier work queue: an appended entry never became readable"); return FMX_ERR_HIP; }
    if (sum.overflow & 1ull) { set_error("frontier work queue overflow (raise fmx_limits.max_frontier)"); return FMX_ERR_OVERFLOW; }
    total = sum.left;
    if (knobs().trace)
      fprintf(stderr, "[fmx] frontier after launch %u: queue %llu, results %llu, overflow %llu\n", pass,
              (unsigned long long)total, (unsigned long long)sum.results, sum.overflow);
  } while (total != 0);
  if (p.pre_next && sum.overflow == 0) {     // the device saw the same (left == 0, no overflow) and left the batch ready: k_res_sort
    b->pre_ok = true;
    b->pre_max_len = p.max_len;
    b->pre_deep = p.deep_len;
    b->pre_count = b->n_first;
    b->pre_ss = p.ss;
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev_a, c->ev_b);
  tr.mark("passes done");
  std::lock_guard<std::mutex> lk(h->mu);
  h->last_kernel_ms = ms;
  h->launches += launches;
  return FMX_OK;
}

static bool by_key(const fmx_result &a, const fmx_result &b) {
  if (a.len != b.len) return a.len < b.len;
  if (a.sp != b.sp) return a.sp < b.sp;
  return a.ep < b.ep;
}

// Canonical order (regex, len, sp, ep) of the `nres` results in `out`, of which the last `extra` are the host's own.
// The device delivered the frontier's results grouped by regex, every group of up to kMidGroup results ordered and
// the few larger ones listed; per_regex_count (host memory, may be null) is filled in unless the device wrote it.
static int order_on_host(RegexBatch *b, hipStream_t st, const CallTrace &tr, fmx_result *out, size_t nres, size_t extra, uint32_t *per_regex_count, bool per_done) {
  const uint32_t nbig = b->h_tot->n_big;
  if (!extra && nbig <= kBigMax) {
    if (nbig) {
      std::vector<uint32_t> ent(2 * (size_t)nbig);
      HIP_TRY(copy_sync(ent.data(), b->d_big->ent, ent.size() * 4, hipMemcpyDeviceToHost, st), "D2H(big groups)");
      size_t tot_big = 0;
      for (uint32_t g = 0; g < nbig; g++) {
        if (ent[2 * g + 1]) std::sort(out + ent[2 * g], out + ent[2 * g] + ent[2 * g + 1], by_key);
        tot_big += ent[2 * g + 1];
      }
      if (knobs().trace) fprintf(stderr, "[fmx] %u large result groups (%zu results) ordered on the host\n", nbig, tot_big);
    }
    tr.mark("large groups");
    if (per_regex_count && nres && !per_done)
      HIP_TRY(copy_sync(per_regex_count, b->d_rcnt, b->k * 4, hipMemcpyDeviceToHost, st), "D2H(result counts)");
    return FMX_OK;
  }
  // host-made results to merge in (or too many large groups to list): bucket everything by regex id
  std::vector<uint32_t> cnt(b->k + 1, 0);
  for (size_t j = 0; j < nres; j++) cnt[out[j].regex]++;
  std::vector<uint32_t> start(b->k + 1, 0);
  for (size_t r = 0; r < b->k; r++) start[r + 1] = start[r] + cnt[r];
  std::vector<fmx_result> tmp(out, out + nres);
  std::vector<uint32_t> fill(start.begin(), start.end() - 1);
  for (size_t j = 0; j < nres; j++) out[fill[tmp[j].regex]++] = tmp[j];
  for (size_t r = 0; r < b->k; r++)
    if (cnt[r] > 1) std::sort(out + start[r], out + start[r + 1], by_key);
  if (per_regex_count)
    for (size_t r = 0; r < b->k; r++) per_regex_count[r] = cnt[r];
  return FMX_OK;
}

// What is left to do when the search is over: the results the device did not deliver itself are copied, the host adds
// those of final DFA start states (dfa.scala:270-273 with the start StatePoint(0,0,0,n)) and orders what the device
// left unordered.  With `dev` the results stay in HBM; the rare cases that need the host (groups of more than 1024
// results, host-made results) are staged through host memory and written back.
static int finish_results(const Index *h, RegexBatch *b, const CallPlan &p, hipStream_t st, const CallTrace &tr, const FrontierSummary &sum,
                          fmx_result *out, size_t cap, size_t *n_out, uint32_t *per_regex_count, bool dev) {
  const bool truncated = sum.truncated != 0;
  const size_t extra = b->start_final.size(), ndev = (size_t)sum.results, nres = ndev + extra;
  *n_out = nres;
  if ((sum.overflow & 2ull) || nres > cap) { set_error("result buffer too small"); return FMX_ERR_OVERFLOW; }
  fmx_result *const dev_out = out;
  uint32_t *const dev_per = per_regex_count;
  std::vector<fmx_result> stage_out;
  std::vector<uint32_t> stage_per;
  const bool staged = dev && (extra || b->h_tot->n_big);
  if (dev && !staged) {
    tr.mark("results on the device");
    return ok_or_truncated(truncated);
  }
  if (staged) {
    stage_out.resize(nres);
    out = stage_out.data();
    if (per_regex_count) { stage_per.assign(b->k, 0u); per_regex_count = stage_per.data(); }
  }
  if (ndev && (!p.export_out || staged))
    HIP_TRY(copy_sync(out, p.direct ? dev_out : b->d_res, ndev * sizeof(fmx_result), hipMemcpyDeviceToHost, st), "D2H(results)");
  tr.mark("results copied");
  for (size_t j = 0; j < extra; j++) {
    fmx_result &o = out[ndev + j];
    o.regex = b->start_final[j]; o.len = 0; o.sp = 0; o.ep = h->n;
  }
  if (nres) {
    const int rc = order_on_host(b, st, tr, out, nres, extra, per_regex_count, p.export_per && !staged);
    if (rc != FMX_OK) return rc;
  }
  if (staged) {
    HIP_TRY(copy_sync(dev_out, out, nres * sizeof(fmx_result), hipMemcpyHostToDevice, st), "H2D(results)");
    if (dev_per) HIP_TRY(copy_sync(dev_per, per_regex_count, b->k * 4, hipMemcpyHostToDevice, st), "H2D(result counts)");
  }
  tr.mark("results ordered");
  return ok_or_truncated(truncated);
}

// `dev`: out / per_regex_count are DEVICE pointers -- the results stay in HBM (fmx_regex_batch_match_dev).
int regex_batch_match(const Index *h, RegexBatch *b, const fmx_limits *lim, fmx_result *out, size_t cap,
                      size_t *n_out, uint32_t *per_regex_count, bool dev = false) {
  const CallTrace tr;
  const uint32_t max_steps = std::min<uint32_t>((lim && lim->max_steps) ? lim->max_steps : 4096u, kMaxLen);
  const uint64_t qcap = (lim && lim->max_frontier) ? lim->max_frontier : (1ull << 22);
  if (b->index_serial != h->serial) { set_error("regex batch was prepared for another index"); return FMX_ERR_ARG; }
  if (per_regex_count && !dev) std::fill(per_regex_count, per_regex_count + b->k, 0u);
  *n_out = 0;
  if (b->n_first == 0 && b->start_final.empty()) {
    if (per_regex_count && dev && b->k) {
      HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
      HIP_TRY(hipMemset(per_regex_count, 0, b->k * 4), "hipMemset(result counts)");
    }
    return FMX_OK;
  }
  if (b->n_first > qcap) { set_error("initial frontier exceeds max_frontier"); return FMX_ERR_OVERFLOW; }
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  int rc = ensure_scratch(b, qcap, cap);
  if (rc != FMX_OK) return rc;
  CtxLease lease(h);                 // stream and events from the handle's pool
  if (!lease.c) return FMX_ERR_HIP;
  hipStream_t st = lease.c->stream;
  CallPlan p{};
  HIP_TRY(ktab_get(h, st, &p.kt), "k-mer table");
  HIP_TRY(row1_get(h, st, &p.kt.row1), "row table");
  rc = zero_queue_if_due(b, st);
  if (rc != FMX_OK) return rc;
  tr.mark("setup");
  HIP_TRY(hipEventRecord(lease.c->ev_a, st), "hipEventRecord");
  plan_call(h, b, max_steps, out, cap, per_regex_count, dev, p);
  FrontierSummary sum{};
  rc = run_chains(h, b, p, lease.c, tr, sum);
  if (rc != FMX_OK) return rc;
  return finish_results(h, b, p, st, tr, sum, out, cap, n_out, per_regex_count, dev);
}

}  // namespace fmx

using namespace fmx;

extern "C" {

// ---- the compile side: a Regex behind the fmx_regex handle.  (Here, not in fmx_regex.cpp: these need set_error and
// parallel_for, and that file stays free of the library's other units so that a test can build it on its own.)
int fmx_regex_compile(const char *re, int line_only, fmx_regex **out) {
  if (!re || !out) { set_error("null argument"); return FMX_ERR_ARG; }
  *out = nullptr;
  try {
    Regex *r = new Regex(compile_regex(re, line_only != 0));
    *out = reinterpret_cast<fmx_regex *>(r);
    return FMX_OK;
  } catch (const RegexError &e) {
    set_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc &) {
    set_error("out of host memory");
    return FMX_ERR_NOMEM;
  }
}

// The batched front-end: REParser.re2post + ReTree.apply are independent per regex, so a batch is compiled on all the
// host cores the process may use (fmx_hostpar.h).  status[i] = FMX_OK / FMX_ERR_SYNTAX / FMX_ERR_MATCH as
// fmx_regex_compile would return for res[i]; out[i] = its handle or NULL.
int fmx_regex_compile_batch(const char *const *res, size_t k, int line_only, fmx_regex **out, int *status) {
  if ((k && (!res || !out))) { set_error("null argument"); return FMX_ERR_ARG; }
  for (size_t i = 0; i < k; i++) {
    out[i] = nullptr;
    if (!res[i]) { set_error("null regex string"); return FMX_ERR_ARG; }
  }
  std::atomic<size_t> first_bad{k};
  std::atomic<int> nomem{0};
  auto compile_range = [&](size_t a, size_t b) {
    for (size_t i = a; i < b; i++) {
      int rc = FMX_OK;
      try {
        out[i] = reinterpret_cast<fmx_regex *>(new Regex(compile_regex(res[i], line_only != 0)));
      } catch (const RegexError &e) {
        rc = e.code;
      } catch (...) {       // bad_alloc, length_error ..: nothing may leave a worker thread (std::terminate) or this extern "C" function
        rc = FMX_ERR_NOMEM;
        nomem.store(1);
      }
      if (status) status[i] = rc;
      if (rc != FMX_OK) {
        size_t cur = first_bad.load();
        while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
      }
    }
  };
  parallel_for(k, 256, compile_range);      // (starts as many threads as it can get and never throws: fmx_hostpar.cpp)
  if (nomem.load()) {
    for (size_t i = 0; i < k; i++) { delete reinterpret_cast<Regex *>(out[i]); out[i] = nullptr; }
    set_error("out of host memory");
    return FMX_ERR_NOMEM;
  }
  const size_t bad = first_bad.load();
  if (bad < k) {        // the first failure's message, as the one-regex entry point would have left it
    try { (void)compile_regex(res[bad], line_only != 0); } catch (const RegexError &e) { set_error(e.msg + " (regex " + std::to_string(bad) + " of the batch)"); } catch (...) {}
  }
  return FMX_OK;
}

int fmx_regex_free_batch(fmx_regex *const *res, size_t k) {
  if (k && !res) { set_error("null argument"); return FMX_ERR_ARG; }
  auto free_range = [&](size_t a, size_t b) {
    for (size_t i = a; i < b; i++) delete reinterpret_cast<Regex *>(res[i]);
  };
  parallel_for(k, 4096, free_range);
  return FMX_OK;
}

// REParser.createNFA (re2/re2.scala:264-334): `src` is a regex (parsed by re2post) or, with
// src_is_postfix, a postfix string for post2re (:188-205, '.' = concat) as the reference's tests use.
int fmx_nfa_compile(const char *src, int line_only, int src_is_postfix, fmx_regex **out) {
  if (!src || !out) { set_error("null argument"); return FMX_ERR_ARG; }
  *out = nullptr;
  try {
    const std::vector<PostPoint> post = src_is_postfix ? post2re(src) : re2post(src, line_only != 0);
    *out = reinterpret_cast<fmx_regex *>(new Regex(compile_thompson(post, src)));
    return FMX_OK;
  } catch (const RegexError &e) {
    set_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc &) {
    set_error("out of host memory");
    return FMX_ERR_NOMEM;
  }
}

int fmx_dfa_compile(const int32_t *moves, uint32_t nstates, uint32_t nchars, const uint8_t *finish, fmx_regex **out) {
  if (!out) { set_error("null argument"); return FMX_ERR_ARG; }
  *out = nullptr;
  try {
    *out = reinterpret_cast<fmx_regex *>(new Regex(compile_dfa(moves, nstates, nchars, finish)));
    return FMX_OK;
  } catch (const RegexError &e) {
    set_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc &) {
    set_error("out of host memory");
    return FMX_ERR_NOMEM;
  }
}

int fmx_regex_free(fmx_regex *re) {
  delete reinterpret_cast<Regex *>(re);
  return FMX_OK;
}

int fmx_regex_post_string(const char *re, int line_only, char *out, size_t cap) {
  if (!re || !out || !cap) { set_error("null argument"); return FMX_ERR_ARG; }
  try {
    std::string s = re2poststr(re, line_only != 0);
    if (s.size() + 1 > cap) { set_error("output buffer too small"); return FMX_ERR_OVERFLOW; }
    std::copy(s.begin(), s.end(), out);
    out[s.size()] = 0;
    return FMX_OK;
  } catch (const RegexError &e) {
    set_error(e.msg);
    return e.code;
  }
}

int fmx_regex_tables(const fmx_regex *re, uint32_t *n_states, uint8_t *st_c, int32_t *st_num, uint8_t *st_last,
                     int32_t *fol_off, uint32_t *n_follows, int32_t *fol, uint32_t *n_firsts, int32_t *firsts) {
  if (!re) { set_error("null argument"); return FMX_ERR_ARG; }
  const Regex *r = reinterpret_cast<const Regex *>(re);
  if (n_states) *n_states = (uint32_t)r->st_c.size();
  if (n_follows) *n_follows = (uint32_t)r->fol.size();
  if (n_firsts) *n_firsts = (uint32_t)r->firsts.size();
  if (st_c) std::copy(r->st_c.begin(), r->st_c.end(), st_c);
  if (st_num) std::copy(r->st_num.begin(), r->st_num.end(), st_num);
  if (st_last) std::copy(r->st_last.begin(), r->st_last.end(), st_last);
  if (fol_off) std::copy(r->fol_off.begin(), r->fol_off.end(), fol_off);
  if (fol) std::copy(r->fol.begin(), r->fol.end(), fol);
  if (firsts) std::copy(r->firsts.begin(), r->firsts.end(), firsts);
  return FMX_OK;
}

// ---- resident batches
int fmx_regex_batch_create(const fmx_index *idx, fmx_regex *const *res, size_t k, fmx_regex_batch **out) {
  if (!idx || !out || (k && !res)) { set_error("null argument"); return FMX_ERR_ARG; }
  *out = nullptr;
  for (size_t r = 0; r < k; r++)
    if (!res[r]) { set_error("null regex handle"); return FMX_ERR_ARG; }
  RegexBatch *b = nullptr;
  int rc = regex_batch_create(reinterpret_cast<const Index *>(idx), reinterpret_cast<const Regex *const *>(res), k, &b);
  if (rc == FMX_OK) *out = reinterpret_cast<fmx_regex_batch *>(b);
  return rc;
}

int fmx_regex_batch_info(const fmx_regex_batch *b, uint64_t *n_regexes, uint64_t *n_states, uint64_t *n_follows,
                         uint64_t *n_firsts) {
  if (!b) { set_error("null argument"); return FMX_ERR_ARG; }
  const RegexBatch *rb = reinterpret_cast<const RegexBatch *>(b);
  if (n_regexes) *n_regexes = rb->k;
  if (n_states) *n_states = rb->n_states;
  if (n_follows) *n_follows = rb->n_fol;
  if (n_firsts) *n_firsts = rb->n_first;
  return FMX_OK;
}

int fmx_regex_batch_free(fmx_regex_batch *b) {
  RegexBatch *rb = reinterpret_cast<RegexBatch *>(b);
  if (rb) { (void)hipSetDevice(rb->device); delete rb; }
  return FMX_OK;
}

int fmx_regex_batch_match(const fmx_index *idx, fmx_regex_batch *b, const fmx_limits *lim, fmx_result *out,
                          size_t cap, size_t *n_out, uint32_t *per_regex_count) {
  if (!idx || !b || !n_out || (cap && !out)) { set_error("null argument"); return FMX_ERR_ARG; }
  const Index *h = reinterpret_cast<const Index *>(idx);
  RegexBatch *rb = reinterpret_cast<RegexBatch *>(b);
  if (lim && lim->mode == FMX_MATCH_REFERENCE) {
    if (lim->max_branching == 0) { set_error("max_branching must be positive"); return FMX_ERR_ARG; }
    if (!rb->all_retree) {
      set_error("the reference-order mode replays ReTree._matchSA; Thompson and DFA handles use the frontier mode");
      return FMX_ERR_UNSUPPORTED;
    }
    if (rb->index_serial != h->serial) { set_error("regex batch was prepared for another index"); return FMX_ERR_ARG; }
    const RefTables rt{rb->nfa.st, rb->nfa.fol, rb->d_st_num, rb->d_first_off, rb->d_first_state, rb->d_fol_rec, rb->d_first_rec, rb->max_num};
    return regex_match_reference(h, rt, rb->k, rb->max_fanout, lim->max_branching, lim->max_iterations, out, cap, n_out,
                                 per_regex_count, nullptr);
  }
  if (lim && lim->mode != FMX_MATCH_FRONTIER) { set_error("unknown fmx_limits.mode"); return FMX_ERR_ARG; }
  return regex_batch_match(h, rb, lim, out, cap, n_out, per_regex_count);
}

int fmx_regex_batch_match_dev(const fmx_index *idx, fmx_regex_batch *b, const fmx_limits *lim, void *d_out, size_t cap,
                              size_t *n_out, void *d_per_regex_count) {
  if (!idx || !b || !n_out || (cap && !d_out)) { set_error("null argument"); return FMX_ERR_ARG; }
  if (lim && lim->mode != FMX_MATCH_FRONTIER) { set_error("the device-resident form runs the frontier mode"); return FMX_ERR_UNSUPPORTED; }
  return regex_batch_match(reinterpret_cast<const Index *>(idx), reinterpret_cast<RegexBatch *>(b), lim,
                           static_cast<fmx_result *>(d_out), cap, n_out, static_cast<uint32_t *>(d_per_regex_count), true);
}

// ---- one process, several GPUs: the batch is cut into contiguous slices of about equal ESTIMATED
// frontier work, slice r is made resident on idxs[r]'s device, slices are matched from one host thread each and
// their result lists -- each already in canonical order, regex ids ascending across slices -- are concatenated.
struct RegexBatchMulti {
  size_t k = 0;
  std::vector<const Index *> idx;
  std::vector<RegexBatch *> part;
  std::vector<size_t> cut;       // n_idx + 1 slice bounds
  // per-slice result buffers, kept between calls and never value-initialised (a fresh zeroed 100 MB vector per
  // slice and call cost 25 ms)
  struct PinnedFree { void operator()(fmx_result *p) const { if (p) (void)hipHostFree(p); } };
  std::vector<std::unique_ptr<fmx_result[], PinnedFree>> buf;      // page-locked: the device writes a slice's results itself
  std::vector<size_t> buf_cap;
  ~RegexBatchMulti() {
    for (size_t r = 0; r < part.size(); r++)
      if (part[r]) { (void)hipSetDevice(part[r]->device); delete part[r]; }
  }
};

// What a regex is expected to cost: its start elements, its states (each is stepped at least once per path through
// it) and its follow entries (every one is a push); a starred class shows up as many follows.
static double regex_work_estimate(const Regex &re, double n, double sigma) {
  std::vector<double> a, b;
  return frontier_work_estimate(re, n, sigma, a, b) + 4.0 * (double)re.firsts.size();
}

int fmx_regex_batch_create_multi(fmx_index *const *idxs, size_t n_idx, fmx_regex *const *res, size_t k,
                                 fmx_regex_batch_multi **out) {
  if (!idxs || !n_idx || !out || (k && !res)) { set_error("null argument"); return FMX_ERR_ARG; }
  *out = nullptr;
  for (size_t r = 0; r < n_idx; r++) {
    if (!idxs[r]) { set_error("null index handle"); return FMX_ERR_ARG; }
    const Index *a = reinterpret_cast<const Index *>(idxs[r]), *b0 = reinterpret_cast<const Index *>(idxs[0]);
    if (a->n != b0->n || a->eof != b0->eof) { set_error("the handles are not replicas of one index"); return FMX_ERR_ARG; }
  }
  for (size_t r = 0; r < k; r++)
    if (!res[r]) { set_error("null regex handle"); return FMX_ERR_ARG; }
  std::unique_ptr<RegexBatchMulti> m(new RegexBatchMulti());
  m->k = k;
  std::vector<double> cum(k + 1, 0.0);
  {
    const Index *h0 = reinterpret_cast<const Index *>(idxs[0]);
    std::vector<double> w(k, 0.0);
    parallel_for(k, 1024, [&](size_t a, size_t b) {
      for (size_t r = a; r < b; r++)
        w[r] = regex_work_estimate(*reinterpret_cast<const Regex *>(res[r]), (double)h0->n, (double)std::max<uint32_t>(h0->nslots, 2u));
    });
    for (size_t r = 0; r < k; r++) cum[r + 1] = cum[r] + w[r];
  }
  m->cut.assign(n_idx + 1, k);
  m->cut[0] = 0;
  for (size_t r = 1; r < n_idx; r++) {
    const double want = cum[k] * (double)r / (double)n_idx;
    size_t c = (size_t)(std::lower_bound(cum.begin(), cum.end(), want) - cum.begin());
    if (c > k) c = k;
    m->cut[r] = std::max(c, m->cut[r - 1]);
  }
  for (size_t r = 0; r < n_idx; r++) {
    m->idx.push_back(reinterpret_cast<const Index *>(idxs[r]));
    m->part.push_back(nullptr);
    const size_t a = m->cut[r], b = m->cut[r + 1];
    int rc = regex_batch_create(m->idx[r], reinterpret_cast<const Regex *const *>(res) + a, b - a, &m->part[r]);
    if (rc != FMX_OK) return rc;
  }
  *out = reinterpret_cast<fmx_regex_batch_multi *>(m.release());
  return FMX_OK;
}

int fmx_regex_batch_free_multi(fmx_regex_batch_multi *mb) {
  delete reinterpret_cast<RegexBatchMulti *>(mb);
  return FMX_OK;
}

int fmx_regex_batch_match_multi(fmx_regex_batch_multi *mb, const fmx_limits *lim, fmx_result *out, size_t cap,
                                size_t *n_out, uint32_t *per_regex_count) {
  if (!mb || !n_out || (cap && !out)) { set_error("null argument"); return FMX_ERR_ARG; }
  RegexBatchMulti *m = reinterpret_cast<RegexBatchMulti *>(mb);
  if (lim && lim->mode != FMX_MATCH_FRONTIER) { set_error("the multi-device form runs the frontier mode"); return FMX_ERR_UNSUPPORTED; }
  const size_t np = m->part.size();
  {   // one slice holds the whole batch (one handle, or every regex in one slice): no thread, no merge
    size_t only = np, busy = 0;
    for (size_t r = 0; r < np; r++)
      if (m->cut[r] != m->cut[r + 1]) { only = r; busy++; }
    if (busy == 1 && m->cut[only] == 0) return regex_batch_match(m->idx[only], m->part[only], lim, out, cap, n_out, per_regex_count);
  }
  m->buf.resize(np);
  m->buf_cap.resize(np, 0);
  for (size_t r = 0; r < np; r++)
    if (m->cut[r] != m->cut[r + 1] && m->buf_cap[r] < (cap ? cap : 1)) {
      void *p = nullptr;
      m->buf[r].reset();
      if (hipSetDevice(m->idx[r]->device) != hipSuccess || hipHostMalloc(&p, (cap ? cap : 1) * sizeof(fmx_result), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        set_error("out of page-locked host memory");
        return FMX_ERR_NOMEM;
      }
      m->buf[r].reset(static_cast<fmx_result *>(p));
      m->buf_cap[r] = cap ? cap : 1;
    }
  std::vector<size_t> cnt(np, 0);
  std::vector<int> rc(np, FMX_OK);
  std::vector<std::string> msg(np);
  std::vector<Worker *> busy;          // slice r runs on handle r's own host thread (kept with the handle)
  for (size_t r = 0; r < np; r++) {
    if (m->cut[r] == m->cut[r + 1]) continue;
    Worker *w = worker_of(m->idx[r]);
    w->submit([&, r]() {
      // every slice may fill the caller's whole capacity
      uint32_t *per = per_regex_count ? per_regex_count + m->cut[r] : nullptr;
      rc[r] = regex_batch_match(m->idx[r], m->part[r], lim, m->buf[r].get(), cap, &cnt[r], per);
      if (rc[r] != FMX_OK) msg[r] = fmx_last_error();
    });
    busy.push_back(w);
  }
  for (Worker *w : busy) w->wait();
  size_t total = 0;
  bool truncated = false;
  for (size_t r = 0; r < np; r++) {
    if (rc[r] == FMX_TRUNCATED) { truncated = true; msg[np - 1] = msg[r]; }
    else if (rc[r] != FMX_OK) { set_error(msg[r]); *n_out = cnt[r]; return rc[r]; }
    total += cnt[r];
  }
  *n_out = total;
  if (total > cap) { set_error("result buffer too small"); return FMX_ERR_OVERFLOW; }
  size_t at = 0;
  for (size_t r = 0; r < np; r++) {
    for (size_t j = 0; j < cnt[r]; j++) {
      out[at] = m->buf[r][j];
      out[at].regex += (uint32_t)m->cut[r];
      at++;
    }
  }
  if (truncated) { set_error("some matches run past max_steps: results hold every match of length <= max_steps"); return FMX_TRUNCATED; }
  return FMX_OK;
}

int fmx_regex_match_batch(const fmx_index *idx, fmx_regex *const *res, size_t k, const fmx_limits *lim,
                          fmx_result *out, size_t cap, size_t *n_out, uint32_t *per_regex_count) {
  if (!n_out) { set_error("null argument"); return FMX_ERR_ARG; }
  fmx_regex_batch *b = nullptr;
  int rc = fmx_regex_batch_create(idx, res, k, &b);
  if (rc != FMX_OK) return rc;
  rc = fmx_regex_batch_match(idx, b, lim, out, cap, n_out, per_regex_count);
  fmx_regex_batch_free(b);
  return rc;
}

}  // extern "C"
