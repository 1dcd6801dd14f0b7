// fmx_frontier.hip -- K5: Glushkov SA-interval frontier expansion for a batch of regexes.
//
// Reference: ReTree._matchSA, re2/retree.scala:618-653.  There one priority queue of
// StatePoint(len, sp, ep, state) is popped serially; each pop is one getPrevRange; a non-empty
// range either emits SAResult (isLast) or pushes one StatePoint per entry of state.follows.
// Every frontier element is independent of the others, so the order in which they are stepped does
// not change the result multiset (whenever the reference's maxBranching / maxIterations do not bind),
// and the device is free to choose the order that costs least memory traffic:
//
//   * A LANE holds an element in registers -- state, length, interval and the state's 32-byte record -- and
//     follows it: after a step that survives, the lane keeps the first follow for itself (same sp/ep, len + 1) and
//     goes on -- a literal stretch of a regex is walked like a literal pattern in k_search4, with no queue round
//     trip per character.  The state record carries the bytes of its first follows, so the next step's rank blocks
//     are requested together with the next state's record: one memory latency per step, not two.  All of an
//     element's bookkeeping runs once, in its lane (64 elements per wave).
//   * The rank queries themselves want a lane group (a quad in the one-hot layout, an octet in the bytes layout:
//     16 bytes of the block per lane, DPP reductions).  Each round hands the 64 intervals through a wave-private
//     exchange area in LDS to the lane groups in G sub-rounds of 64/G elements and takes the stepped intervals back
//     the same way.  A narrowed interval lies inside one block: one line per element, the rare second block in a
//     second trip.
//   * The other follows go to the wave's own POOL in LDS (256 entries, newest first out: depth-first, so the live
//     set stays small; a nearly empty pool is emptied oldest first); lanes whose element died take their next one
//     from there.
//   * What a wave cannot hold goes to a sliced work queue in HBM whose entries other waves may take DURING THE SAME
//     LAUNCH (tagged 8-byte granules, agent-scope stores and loads; below), and what was queued before a launch is
//     dealt out in fixed shares.  No wave ever waits for another: one that finds nothing ends, every wave ends
//     after at most `max_rounds` rounds (handing over what it still holds), and launches repeat until the queue is
//     empty.  A batch like C4 is one launch (round 1 ran one launch per match length: 64+ launches, every element
//     through HBM queues at every level; profiles/r02_c4_analysis.md has the history).
#include <algorithm>
#include <cstdint>

#include "fmx_frontier.h"

namespace fmx {

__host__ __device__ inline uint32_t next_tag(uint32_t t) { return t % 0xFFFFu + 1u; }

// Agent-scope relaxed accesses to words other workgroups write during the launch: global_load / global_store with
// sc1 (they bypass the CU's L1 and are written through; plain accesses could be served from a stale line).
typedef __attribute__((address_space(1))) unsigned long long gu64;
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) {
  return __hip_atomic_load((gu64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store((gu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exclusive prefix sum over the 64 lanes with DPP adds only (row shifts inside each row of 16, then the row
// totals carried over with row_bcast:15 / row_bcast:31): six VALU instructions, no LDS crossbar round trips
// (the __shfl_up form of round 1 cost seven dependent ds_bpermute per scan).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t x) {
  return x + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xF, ROW_MASK == 0xF);
}
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t &total) {
  uint32_t x = v;
  x = dpp_add<0x111, 0xF>(x);     // row_shr:1
  x = dpp_add<0x112, 0xF>(x);     // row_shr:2
  x = dpp_add<0x114, 0xF>(x);     // row_shr:4
  x = dpp_add<0x118, 0xF>(x);     // row_shr:8
  x = dpp_add<0x142, 0xA>(x);     // row_bcast:15 into rows 1 and 3
  x = dpp_add<0x143, 0xC>(x);     // row_bcast:31 into rows 2 and 3
  total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
  return x - v;
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
  return ((unsigned long long)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}

constexpr uint32_t kPoolSmall = 6;      // follow lists with up to this many pushed entries go through the pool
#ifdef FMX_WAVELOG
// Diagnostic build only (tools/wave_timeline.py): per launch and wave {start, first round, end, rounds} in the
// constant 100 MHz clock, so that the occupancy of the wave slots over a launch can be drawn.
constexpr uint32_t kLogPasses = 16, kLogWaves = 1u << 15;
__device__ unsigned long long g_wavelog[kLogPasses][kLogWaves][8];
// launch 0, per wave and round (first 128): elements held | pool entries << 8 | deepest held length << 20 | narrow << 28
__device__ unsigned int g_wavetrace[kLogWaves][128];
// with -DFMX_PHASELOG=<round>: cycles (s_memtime) a wave spends in the four phases of its rounds from that round on
// (take | stage + issue | wait + ranks | bookkeeping), rounds counted, in g_phaselog[wave][0..4] of launch 0
__device__ unsigned long long g_phaselog[kLogWaves][8];
#endif
__device__ __forceinline__ void pool_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One launch.  Every wave works until it finds nothing more to take (or its round budget ends): it takes entries
// from the queue, follows them, keeps what they branch into in its pool, and hands pool entries beyond kPoolKeep
// back to the queue, where waves that have run dry find them during the same launch.  No wave ever waits for
// another one: a wave that finds the queue empty a few polls in a row simply ends, and whatever is appended after
// that is the next launch's input.
#ifndef FMX_FBATCH
#define FMX_FBATCH 4
#endif
#ifndef FMX_TAKE_OLDEST
#define FMX_TAKE_OLDEST 32
#endif
constexpr uint32_t kTakeOldest = FMX_TAKE_OLDEST;   // pool sizes up to which idle lanes take the oldest entries
#ifndef FMX_POOL_KEEP
#define FMX_POOL_KEEP 192
#endif
#ifndef FMX_GRAB
#define FMX_GRAB 64
#endif
constexpr uint32_t kPoolKeep = FMX_POOL_KEEP;   // pool entries a wave keeps for itself; the older ones go to the queue
constexpr uint32_t kGrab = FMX_GRAB;            // entries taken from the queue at a time
#ifndef FMX_IDLE_LOOKS
#define FMX_IDLE_LOOKS 3
#endif
#ifndef FMX_NARROW
#define FMX_NARROW 1
#endif
#ifndef FMX_DEEP_PRIO
#define FMX_DEEP_PRIO 1
#endif

#ifndef FMX_DEEP_SLACK
#define FMX_DEEP_SLACK 4u
#endif
constexpr uint32_t kIdleLooks = FMX_IDLE_LOOKS; // looks that find nothing before a wave without work ends
constexpr uint32_t kTagSpins = 1u << 16;        // re-reads of a reserved entry before the wave gives up (an error)
constexpr uint32_t kPool64 = 256, kPool64Mask = kPool64 - 1;
struct Pool64 {          // 24 bytes per entry, 6 KiB per wave
  uint32_t state[kPool64];
  uint32_t meta[kPool64];
  uint64_t sp[kPool64];
  uint64_t ep[kPool64];
};
constexpr uint32_t kRes64 = 64;
struct ResStage64 {
  fmx_result r[kRes64];
};
struct Xchg {            // a round's intervals on their way to the lane groups and back, by element (= lane) number
  uint64_t sp[64];
  uint64_t ep[64];
  uint32_t key[64];      // slot | byte << 16, 0xFFFFFFFF: this element has no rank query this round
};
constexpr uint32_t kNoQuery = 0xFFFFFFFFu;
// A workgroup's MAILBOX: a wave with a long backlog leaves some of its oldest pool entries here for the three other
// waves of its workgroup, which look here first when they run dry -- the launch waits for its longest wave, and this
// shares a long backlog at the price of LDS accesses (handing over through the HBM queue costs more than it
// balances).  Guarded by a lock that one lane takes with an LDS compare-and-swap; the holder only copies entries.
// Every wave empties the mailbox before it ends, so nothing is left behind.
#ifndef FMX_MAIL
#define FMX_MAIL 80
#endif
#ifndef FMX_MAIL_KEEP
#define FMX_MAIL_KEEP 128
#endif
#ifndef FMX_MAIL_GIVE
#define FMX_MAIL_GIVE 32
#endif
constexpr uint32_t kMail = FMX_MAIL, kMailKeep = FMX_MAIL_KEEP, kMailGive = FMX_MAIL_GIVE;
struct Mailbox {
  uint32_t lock;           // 0 free, 1 held
  uint32_t n;              // entries held (a stack)
  uint32_t state[kMail ? kMail : 1];
  uint32_t meta[kMail ? kMail : 1];
  uint64_t sp[kMail ? kMail : 1];
  uint64_t ep[kMail ? kMail : 1];
};

template <bool WIDE, uint32_t LAYOUT>
__device__ __forceinline__ void frontier_pass(const DevIndex &ix, const KTab &kt, const NfaTables &nfa, const FlowQueue &fq, uint32_t j,
                                              uint32_t max_rounds, uint64_t sub_cap, fmx_result *__restrict__ res,
                                              uint64_t seg_cap, FrontierCtl *__restrict__ ctl, uint32_t *__restrict__ rcnt,
                                              unsigned long long *__restrict__ counters) {
  constexpr int G = Lay<LAYOUT>::G;
  constexpr uint32_t EPS = 64 / G;           // elements per sub-round
  constexpr int B = LAYOUT == kLayoutBytes ? 2 : FMX_FBATCH;     // sub-rounds whose lines are requested before any is consumed
#ifdef FMX_WAVELOG
  const unsigned long long wl_t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long wl_t1 = 0;
#endif
  const uint32_t lane = __lane_id();
  const uint32_t w = uni((blockIdx.x * kFThreads + threadIdx.x) >> 6);      // this wave (kept in scalar registers)
  // After a queue overflow entries are missing: later launches of the chain do nothing (the host reports it).
  if (ctl->left == 0 || (ctl->overflow & 1ull)) return;      // uniform over the grid
  // which buffer of a slice is written, and the buffers' tags, do not change during a launch
  __shared__ uint32_t s_wsel[kSub], s_tags[kSub];            // tags: tag[0] | tag[1] << 16
  if (threadIdx.x < kSub) {
    const SliceCtl &q = ctl->q[threadIdx.x];
    s_wsel[threadIdx.x] = q.wsel;
    s_tags[threadIdx.x] = q.tag[0] | (q.tag[1] << 16);
  }
  __shared__ Mailbox s_mail;
  __shared__ uint16_t s_slot[256];
  __shared__ Pool64 s_pool[kFThreads / 64];
  __shared__ ResStage64 s_res[kFThreads / 64];
  __shared__ Xchg s_xc[kFThreads / 64];
  __shared__ const uint4 *s_lvl[16];         // the k-mer table's levels (picked by an element's length at run time)
  for (int c = threadIdx.x; c < 256; c += blockDim.x) s_slot[c] = ix.slot[c];
  if (threadIdx.x == 0) { s_mail.lock = 0; s_mail.n = 0; }
  if (threadIdx.x < 16) s_lvl[threadIdx.x] = kt.k ? kt.level_dev[threadIdx.x] : nullptr;
  __syncthreads();
  Pool64 &pl = s_pool[threadIdx.x >> 6];
  ResStage64 &rs = s_res[threadIdx.x >> 6];
  Xchg &xc = s_xc[threadIdx.x >> 6];
  uint32_t rs_n = 0;                         // wave-uniform
  const LaneConst lc = lane_const<G>();
  const uint32_t grp = lane / G;             // this lane's group: it serves element r * EPS + grp in sub-round r
  const uint32_t max_len = ctl->max_len;
  uint32_t pb = 0, pn = 0, appends = 0, grabs = 0, rounds = 0, idle_looks = 0;     // wave-uniform
  // This wave's share of what the launch found queued: slice w % kSub's buffer that is not written now is dealt out
  // evenly to the waves of that class, one contiguous chunk each, read without atomics (nobody else touches it).
  const uint32_t nw = gridDim.x * (kFThreads / 64);
  const uint32_t sub = w % kSub, part = w / kSub;
  const uint32_t class_waves = (nw - sub + kSub - 1) / kSub;
  const uint32_t in_buf = 1u - s_wsel[sub];
  const uint64_t in_off = ((uint64_t)sub * 2 + in_buf) * sub_cap;
  uint64_t a_next, a_end;
  {
    const SliceCtl &q = ctl->q[sub];
    const uint64_t hd = q.head[in_buf], tl = q.tail[in_buf] < sub_cap ? q.tail[in_buf] : sub_cap;
    const uint64_t cnt = tl > hd ? tl - hd : 0, chunk = (cnt + class_waves - 1) / class_waves;
    a_next = hd + (uint64_t)part * chunk;
    a_end = a_next + chunk < tl ? a_next + chunk : tl;
    if (a_next > a_end) a_next = a_end;
    a_next = uni64(a_next);
    a_end = uni64(a_end);
  }
  bool prio_up = false;                      // wave-uniform: running at raised issue priority (FMX_DEEP_PRIO)
  bool have = false;                         // the element this lane holds
  uint32_t state = 0, meta = 0;
  uint64_t sp = 0, ep = 0;
  // the held element's state record; it stays while the element walks a literal stretch (meta bits 24..31)
  uint4 ra = make_uint4(0, 0, 0, 0);         // fol_off, cnt_c_emit, f[0], f[1]
  uint4 rb = make_uint4(0, 0, 0, 0);         // f[2], f[3], fc, regex
  uint32_t n_reqs = 0, n_recs = 0, n_ktl = 0, n_jl = 0, n_writes = 0, n_emits = 0, n_reads = 0, stepped = 0, trunc = 0;

  // room for `cnt` entries in some slice's write buffer: slice, buffer, tag and first index (wave-uniform)
  struct Slot { uint64_t first; uint32_t tag; unsigned long long at; };
  auto reserve = [&](uint32_t cnt) -> Slot {
    const uint32_t so = (w + appends++) % kSub;
    const uint32_t buf = s_wsel[so];
    Slot s;
    s.tag = (s_tags[so] >> (16u * buf)) & 0xFFFFu;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctl->q[so].tail[buf], (unsigned long long)cnt);
    s.at = __shfl(base, 0, 64);
    s.first = ((uint64_t)so * 2 + buf) * sub_cap;
    return s;
  };
  auto put = [&](const Slot &s, unsigned long long at, uint32_t st, uint32_t mt, uint64_t esp, uint64_t eep) {
    if (at < sub_cap) {
      const unsigned long long tg = (unsigned long long)s.tag << 48;
      const uint64_t i = s.first + at;
      st_agent(fq.g0 + i, tg | ((unsigned long long)((mt >> 16) & 0xFFu) << 40) | esp);
      st_agent(fq.g1 + i, tg | eep);
      st_agent(fq.g2 + i, tg | ((unsigned long long)(mt & 0xFFFFu) << 32) | st);
    } else {
      atomicOr(&ctl->overflow, 1ull);
    }
  };
  // the `cnt` oldest pool entries go to the queue
  auto spill = [&](uint32_t cnt) {
    if (!cnt) return;
    pool_sync();
    const Slot s = reserve(cnt);
    for (uint32_t i = lane; i < cnt; i += 64) {
      const uint32_t idx = (pb + i) & kPool64Mask;
      put(s, s.at + i, pl.state[idx], pl.meta[idx], pl.sp[idx], pl.ep[idx]);
    }
    pool_sync();
    pb = uni((pb + cnt) & kPool64Mask);
    pn = uni(pn - cnt);
    n_writes += cnt;
  };
  auto to_pool = [&](uint32_t cnt, unsigned long long e0, unsigned long long e1, unsigned long long e2) {
    if (lane < cnt) {
      const uint32_t idx = (pb + pn + lane) & kPool64Mask;
      pl.state[idx] = (uint32_t)e2;
      pl.meta[idx] = (uint32_t)((e2 >> 32) & 0xFFFFu) | ((uint32_t)((e0 >> 40) & 0xFFu) << 16);
      pl.sp[idx] = e0 & (kMaxRows - 1);
      pl.ep[idx] = e1 & (kMaxRows - 1);
    }
    pn = uni(pn + cnt);
    n_reads += cnt;
    pool_sync();
  };
  // The next entries of the wave's share enter the pool (wave-uniform).  They were written before this launch began.
  auto take_batch = [&]() -> bool {
    if (a_next >= a_end) return false;
    const uint64_t left = a_end - a_next;
    uint32_t room = kPool64 - 64u - pn;      // the push phase wants 64 free entries afterwards
    if (room > 64u) room = 64u;
    const uint32_t cnt = left < room ? (uint32_t)left : room;
    unsigned long long e0 = 0, e1 = 0, e2 = 0;
    if (lane < cnt) {
      if (j == 0 && ctl->fresh != 0) {                 // uniform over the grid: a call's first launch, its share is start elements
        const StartSrc ss = ctl->start;
        const unsigned long long se = ss.elem[(uint64_t)sub * ss.cap + a_next + lane];
        e0 = se & (0xFFull << 40);                       // the state's byte; sp = 0
        e1 = ss.ep;
        e2 = se & 0xFFFFFFFFull;                         // len = 0
      } else {
        const uint64_t i = in_off + a_next + lane;
        e0 = fq.g0[i]; e1 = fq.g1[i]; e2 = fq.g2[i];
      }
    }
    a_next += cnt;
    to_pool(cnt, e0, e1, e2);
    return true;
  };
  // A wave with nothing left looks for entries that other waves appended during THIS launch (wave-uniform; returns
  // how many it took): four slices per look, one round trip -- lanes 0..3 read the written buffer's tail and head of
  // one slice each -- then a compare-and-swap on the first head that has something below its tail, and the reserved
  // entries are re-read until they carry the buffer's tag (the wave that reserved them writes them at once).
  auto steal = [&]() -> uint32_t {
    const uint32_t s4 = (w + 4u * grabs++) & 63u;
    unsigned long long tail_w = 0, head_w = 0;
    if (lane < 4) {
      const uint32_t sl = (s4 + lane) & 63u;
      SliceCtl *const q = ctl->q + sl;
      const uint32_t ws = s_wsel[sl];
      tail_w = ld_agent(&q->tail[ws]);
      head_w = ld_agent(&q->head[ws]);
      if (tail_w > sub_cap) tail_w = sub_cap;          // appends past the capacity were dropped (overflow is flagged)
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(tail_w > head_w);
    if (!m) return 0;
    const uint32_t src = (uint32_t)__builtin_ctzll(m);
    const uint32_t s = (s4 + src) & 63u, ws = s_wsel[s];
    tail_w = __shfl(tail_w, (int)src, 64);
    head_w = __shfl(head_w, (int)src, 64);
    const uint32_t cnt = tail_w - head_w < kGrab ? (uint32_t)(tail_w - head_w) : kGrab;
    unsigned long long old = 0;
    if (lane == 0) old = atomicCAS(&ctl->q[s].head[ws], head_w, head_w + cnt);
    if (uni64(old) != head_w) return 0;                // another wave was faster
    const unsigned long long tag = (s_tags[s] >> (16u * ws)) & 0xFFFFu;
    const uint64_t i = ((uint64_t)s * 2 + ws) * sub_cap + head_w + lane;
    unsigned long long e0 = 0, e1 = 0, e2 = 0;
    bool ok = true;
    for (uint32_t spins = 0;; spins++) {
      if (lane < cnt) {
        e0 = ld_agent(fq.g0 + i); e1 = ld_agent(fq.g1 + i); e2 = ld_agent(fq.g2 + i);
        ok = (e0 >> 48) == tag && (e1 >> 48) == tag && (e2 >> 48) == tag;
      }
      if (!__builtin_amdgcn_ballot_w64(!ok)) break;
      if (spins >= kTagSpins) { atomicOr(&ctl->overflow, 4ull); return 0; }
      __builtin_amdgcn_s_sleep(2);
    }
    to_pool(cnt, e0, e1, e2);
    return cnt;
  };
  // staged results go to the result slices: one returning atomic per flush, not per round with a result
  auto flush_results = [&]() {
    if (!rs_n) return;
    pool_sync();
    const uint32_t so = (w + appends++) % kSub;
    unsigned long long rbase = 0;
    if (lane == 0) rbase = atomicAdd(&ctl->res_count[so].v, (unsigned long long)rs_n);
    rbase = __shfl(rbase, 0, 64);
    if (lane < rs_n) {
      const unsigned long long at = rbase + lane;
      if (at < seg_cap) { res[(uint64_t)so * seg_cap + at] = rs.r[lane]; atomicAdd(&rcnt[rs.r[lane].regex], 1u); }   // per-regex counts: the grouping starts from them
      else atomicOr(&ctl->overflow, 2ull);
    }
    pool_sync();
    n_emits += rs_n;
    rs_n = 0;
  };

  Mailbox &mb = s_mail;
  auto mail_lock = [&]() {
    if (lane == 0)
      while (atomicCAS(&mb.lock, 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };
  auto mail_unlock = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) atomicExch(&mb.lock, 0u);
  };
  // up to `room` mailbox entries enter the pool (wave-uniform; returns how many)
  auto mail_take = [&](uint32_t room) -> uint32_t {
    if (!kMail || !room) return 0;
    pool_sync();
    mail_lock();
    const uint32_t have_n = uni(*(volatile uint32_t *)&mb.n);
    const uint32_t cnt = have_n < room ? have_n : room;
    if (lane < cnt) {
      const uint32_t src = have_n - cnt + lane, idx = (pb + pn + lane) & kPool64Mask;
      pl.state[idx] = mb.state[src]; pl.meta[idx] = mb.meta[src]; pl.sp[idx] = mb.sp[src]; pl.ep[idx] = mb.ep[src];
    }
    if (lane == 0 && cnt) *(volatile uint32_t *)&mb.n = have_n - cnt;
    mail_unlock();
    pn = uni(pn + cnt);
    pool_sync();
    return cnt;
  };
  // up to kMailGive of the pool's oldest entries go to the mailbox (wave-uniform)
  auto mail_give = [&]() {
    pool_sync();
    mail_lock();
    const uint32_t have_n = uni(*(volatile uint32_t *)&mb.n);
    uint32_t cnt = kMail - have_n < kMailGive ? kMail - have_n : kMailGive;
    if (cnt > pn) cnt = pn;
    if (lane < cnt) {
      const uint32_t dst = have_n + lane, idx = (pb + lane) & kPool64Mask;
      mb.state[dst] = pl.state[idx]; mb.meta[dst] = pl.meta[idx]; mb.sp[dst] = pl.sp[idx]; mb.ep[dst] = pl.ep[idx];
    }
    if (lane == 0 && cnt) *(volatile uint32_t *)&mb.n = have_n + cnt;
    mail_unlock();
    pb = uni((pb + cnt) & kPool64Mask);
    pn = uni(pn - cnt);
    pool_sync();
  };
  auto mail_n = [&]() -> uint32_t { return kMail ? uni(*(volatile uint32_t *)&mb.n) : 0u; };

#ifdef FMX_WAVELOG
  wl_t1 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef FMX_PHASELOG
  unsigned long long ph_t = 0, ph0 = 0, ph1 = 0, ph2 = 0, ph3 = 0, ph_n = 0;
#define PH_MARK(acc) do { if (rounds >= FMX_PHASELOG) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - ph_t; ph_t = now_; } } while (0)
#else
#define PH_MARK(acc) do {} while (0)
#endif
  for (;;) {
#ifdef FMX_PHASELOG
    ph_t = __builtin_amdgcn_s_memtime();
#endif
    // ---- NARROW rounds.  A wave that holds no more elements than it has lane groups (the thin end of a launch: a
    // few chains of dependent steps, which are the launch's critical path) keeps them in the groups' first lanes and
    // steps each in its own group, like k_search4 does: the interval goes to the group's lanes by DPP, the ranks come
    // back the same way -- no exchange area, no LDS round trips around the memory latency.
    bool narrow = false;
#if FMX_NARROW
    {
      const unsigned long long havem = __builtin_amdgcn_ballot_w64(have);
      const uint32_t n_have = (uint32_t)__builtin_popcountll(havem);
      narrow = n_have + pn <= (uint32_t)(64 / G) && n_have + pn != 0u && a_next >= a_end;
      if (narrow) {
        constexpr unsigned long long kLeaders = G == 4 ? 0x1111111111111111ull : 0x0101010101010101ull;
        const unsigned long long stray = havem & ~kLeaders;       // elements held by other lanes go through the pool
        if (stray) {
          if (have && lc.t != 0u) {
            const uint32_t idx = (pb + pn + (uint32_t)__builtin_popcountll(stray & ((1ull << lane) - 1ull))) & kPool64Mask;
            pl.state[idx] = state; pl.meta[idx] = meta & 0x00FFFFFFu; pl.sp[idx] = sp; pl.ep[idx] = ep;   // the stretch context stays behind
            have = false;
          }
          pn = uni(pn + (uint32_t)__builtin_popcountll(stray));
          pool_sync();
        }
        const unsigned long long idle_l = ~__builtin_amdgcn_ballot_w64(have) & kLeaders;
        if (idle_l && pn) {
          const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle_l);
          const uint32_t take = n_idle < pn ? n_idle : pn;
          const uint32_t rank = (uint32_t)__builtin_popcountll(idle_l & ((1ull << lane) - 1ull));
          if (!have && lc.t == 0u && rank < take) {
            const uint32_t idx = (pb + rank) & kPool64Mask;       // a small pool: oldest first
            state = pl.state[idx]; meta = pl.meta[idx]; sp = pl.sp[idx]; ep = pl.ep[idx];
            have = true;
          }
          pb = uni((pb + take) & kPool64Mask);
          pn = uni(pn - take);
          pool_sync();
        }
      }
    }
#endif
    // ---- lanes without an element take the newest pool entries; a pool that cannot feed them is refilled from the
    // wave's share, and a wave with nothing left at all looks for entries appended during this launch
    if (!narrow) {
      const unsigned long long idle = __builtin_amdgcn_ballot_w64(!have);
      if (idle) {
        const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle);
        // what a sibling wave left for this one -- looked for only by a wave that cannot fill half its lanes (every look
        // is an LDS round trip on the round's critical path)
        if (pn < n_idle && n_idle > 32u && mail_n()) mail_take(64u);
        if (pn < n_idle && !take_batch() && pn == 0 && n_idle == 64u) steal();
        if (pn) {
          const uint32_t take = n_idle < pn ? n_idle : pn;
          const uint32_t rank = (uint32_t)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
          // A small pool is emptied from its OLD end: the oldest entries are the shallowest, i.e. the ones with the
          // longest way still to go, and a wave's last rounds are the launch's critical path.  A large pool is emptied
          // from its new end (depth first), which keeps it from growing.
          const bool oldest = pn <= kTakeOldest;
          if (!have && rank < take) {
            const uint32_t idx = (oldest ? pb + rank : pb + pn - 1 - rank) & kPool64Mask;
            state = pl.state[idx]; meta = pl.meta[idx]; sp = pl.sp[idx]; ep = pl.ep[idx];
            have = true;
          }
          if (oldest) pb = uni((pb + take) & kPool64Mask);
          pn = uni(pn - take);
          pool_sync();
        }
      }
    }
    if (!__builtin_amdgcn_ballot_w64(have)) {      // nothing held, pool empty, share used up, nothing found
      if (++idle_looks > kIdleLooks) break;
      for (uint32_t z = 0; z < (1u << (idle_looks < 3u ? idle_looks : 3u)); z++) __builtin_amdgcn_s_sleep(16);      // 1, 2, 4 .. x ~0.5 us: another wave may be about to hand work over
      continue;
    }
    idle_looks = 0;
#ifdef FMX_WAVELOG
    if (j == 0 && w < kLogWaves && rounds < 128u) {
      const uint32_t nh = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(have));
      uint32_t ml = have ? (meta & 0xFFFFu) : 0u;
      for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)ml, d, 64); ml = o > ml ? o : ml; }
      if (lane == 0) g_wavetrace[w][rounds] = nh | (pn << 8) | ((ml > 255u ? 255u : ml) << 20) | ((narrow ? 1u : 0u) << 28);
    }
#endif
#if FMX_DEEP_PRIO
    // A wave that holds an element which has advanced in (nearly) every round since the launch began is on the
    // launch's critical path -- a chain of dependent steps as long as the deepest match explored: it gets the SIMD's
    // issue slots ahead of its neighbours, whose backlog is throughput work.
    {
      const uint32_t floor_len = (rounds > 16u ? rounds : 16u);
      const bool deep_now = __builtin_amdgcn_ballot_w64(have && (meta & 0xFFFFu) + FMX_DEEP_SLACK >= floor_len) != 0ull;
      if (deep_now != prio_up) {
        if (deep_now) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(0);
        prio_up = deep_now;
      }
    }
#endif
    PH_MARK(ph0);
    // ---- every element's state record and its step's lines are requested together
    const uint32_t run = meta >> 24;          // > 0: inside a literal stretch whose bytes the held record carries
    const uint32_t c = (meta >> 16) & 0xFFu, len = meta & 0xFFFFu;
    const uint16_t slot = s_slot[c];
    const uint64_t cfc = ix.cf[c];            // C[c]: needed only when the ranks are back, so its load rides along
    if (have && run == 0) {
      const uint4 *rp = reinterpret_cast<const uint4 *>(nfa.st + state);
      ra = rp[0];
      rb = rp[1];
      n_recs++;
    }
    // An element shorter than the k-mer table's K carries its k-mer code instead of an interval (ep == 0 marks it,
    // sp = the code): its step is a lookup in the next level of the table.
    bool cm = have && kt.k != 0 && ep == 0;
    uint32_t ncode = 0;
    bool from_tab = false;
    uint4 ent = make_uint4(0, 0, 0, 0);
    if (cm) {
      if (slot < kSlotEof) {
        ncode = (uint32_t)sp * kt.sigma + slot;
        ent = s_lvl[len][ncode];
        from_tab = true;
        n_ktl++;
      } else if (slot == kSlotNone) {
        sp = 0; ep = 0;                                 // a byte that does not occur: the interval is empty
      } else {                                          // the EOF symbol: leave the table, step on the interval itself
        if (len == 0) { sp = 0; ep = ix.n; }
        else {
          const uint4 e0 = s_lvl[len - 1][sp];
          sp = (((uint64_t)e0.y << 32) | e0.x) & ((1ull << 56) - 1);
          ep = ((uint64_t)e0.w << 32) | e0.z;
        }
        cm = false;
      }
    }
    const bool ranked = have && !cm;
    // a rank query is needed unless the symbol is absent / EOF or the element is a start element ...
    const bool step_q = ranked && len != 0 && slot < kSlotEof;
    // ... or holds one row and the handle has a row table: [r, r + 1) steps to [LF r, LF r + 1) if the state's byte is
    // BWT'[r], to nothing otherwise -- one 8-byte load by the element's own lane, no lane group, no exchange slot
    const bool row_q = kt.row1 != nullptr && step_q && (ep - sp) == 1;
    unsigned long long r1e = 0;
    if (row_q) { r1e = kt.row1[sp]; n_jl++; }
    const bool query = step_q && !row_q;
    // The elements that have a query take the exchange slots 0, 1, 2 .. in lane order, so the lane groups serve
    // ceil(queries / (64/G)) sub-rounds, not all G: in a launch's thin end, and in rounds where most elements step
    // through the k-mer table, most sub-rounds have nothing to do and are skipped.
    const unsigned long long qmask = __builtin_amdgcn_ballot_w64(query);
    const uint32_t n_query = (uint32_t)__builtin_popcountll(qmask);
    const uint32_t xslot = (uint32_t)__builtin_popcountll(qmask & ((1ull << lane) - 1ull));      // this lane's slot, if it has a query
    uint64_t nsp = 0, nep = 0;                         // narrow rounds: the group's ranks
    if (narrow) {
      PH_MARK(ph1);
      // the first lane's interval and symbol to its whole group, then the step where the data is
      const uint32_t qk = group_bcast<G, 0>(query ? ((uint32_t)slot | (c << 16)) : kNoQuery);
      uint64_t gsp = group_bcast64<G, 0>(sp), gep = group_bcast64<G, 0>(ep);
      if (qk != kNoQuery) {
        const uint32_t rq = backward_step<WIDE, LAYOUT>(ix, qk >> 16, (uint16_t)(qk & 0xFFFFu), 0ull, lc, gsp, gep);
        if (lc.t == 0) n_reqs += rq;
        nsp = gsp;
        nep = gep;
      }
    } else {
    if (query) {
      xc.sp[xslot] = sp;
      xc.ep[xslot] = ep;
      xc.key[xslot] = (uint32_t)slot | (c << 16);
    }
    if (lane >= n_query) xc.key[lane] = kNoQuery;      // the slots behind the last query
    pool_sync();
    PH_MARK(ph1);
    if constexpr (LAYOUT == kLayoutBytes) {
      // Bytes layout: a rank query is the 128-position block (16 bytes per lane of the octet) plus its checkpoint.
      // As below, sp and ep of a narrowed interval lie in one block: one request pair per element, both ranks from
      // it, a second trip for the elements whose ep lies in the next block.
      constexpr uint32_t kTwo = 1u << 30, kPending = 1u << 31;
      constexpr int BB = 2;
      bool any_two = false;
#pragma unroll
      for (int r0 = 0; r0 < G; r0 += BB) {
        ByteRankReq q[BB];
        uint32_t key[BB], m[BB];      // m: ep's in-block offset | kTwo
#pragma unroll
        for (int b = 0; b < BB; b++) {
          const uint32_t e = (uint32_t)(r0 + b) * EPS + grp;
          key[b] = xc.key[e];
          m[b] = 0;
          q[b].w = make_uint4(0, 0, 0, 0); q[b].chk = 0; q[b].sup = 0; q[b].rem = 0;
          if (key[b] != kNoQuery) {
            const uint64_t esp = xc.sp[e], eep = xc.ep[e];
            q[b] = byte_rank_issue(ix, (uint16_t)(key[b] & 0xFFFFu), esp, lc);
            const bool two = (eep >> 7) != (esp >> 7);
            m[b] = ((uint32_t)eep & 127u) | (two ? kTwo : 0u);
            if (lc.t == 0) n_reqs += two ? 4u : 2u;
          }
        }
#pragma unroll
        for (int b = 0; b < BB; b++) {
          if (key[b] != kNoQuery) {
            const uint32_t e = (uint32_t)(r0 + b) * EPS + grp;
            const uint32_t ec = (key[b] >> 16) & 0xFFu;
            const bool two = (m[b] & kTwo) != 0;
            const uint64_t r1 = byte_rank_finish(q[b], ec, lc);
            q[b].rem = m[b] & 127u;
            const uint64_t r2 = byte_rank_finish(q[b], ec, lc);
            if (lc.t == 0) {
              xc.sp[e] = r1;
              if (two) xc.key[e] |= kPending;      // ep's own block is still to be read
              else xc.ep[e] = r2;
            }
            any_two |= two;
          }
        }
      }
      if (__builtin_amdgcn_ballot_w64(any_two)) {
        pool_sync();
#pragma unroll 1
        for (int r = 0; r < G; r++) {
          const uint32_t e = (uint32_t)r * EPS + grp;
          const uint32_t key = xc.key[e];
          if (key != kNoQuery && (key & kPending)) {
            const ByteRankReq q2 = byte_rank_issue(ix, (uint16_t)(key & 0xFFFFu), xc.ep[e], lc);
            const uint64_t r2 = byte_rank_finish(q2, (key >> 16) & 0xFFu, lc);
            if (lc.t == 0) xc.ep[e] = r2;
          }
        }
      }
    } else {
      // One-hot layout.  An interval that has been narrowed by a few steps lies inside one 448-position block, so the
      // common case is ONE line per element: B sub-rounds request their sp-block together (5 registers each: the
      // line and the two in-block boundaries), both ranks come from it, and the few elements whose ep falls into
      // another block are finished in a second trip afterwards (their ep stays in the exchange area meanwhile).
      constexpr uint32_t kTwo = 1u << 30, kActive = 1u << 31, kPending = 1u << 31;
      bool any_two = false;
#pragma unroll
      for (int r0 = 0; r0 < G; r0 += B) {
        uint4 w[B];
        uint32_t m[B];      // m1 | m2 << 9 | kTwo | kActive
#pragma unroll
        for (int b = 0; b < B; b++) {
          const uint32_t e = (uint32_t)(r0 + b) * EPS + grp;
          const uint32_t key = xc.key[e];
          m[b] = 0;
          w[b] = make_uint4(0, 0, 0, 0);
          if (key != kNoQuery) {
            const uint64_t esp = xc.sp[e], eep = xc.ep[e];
            uint32_t b1, m1, b2, m2;
            split448(esp, b1, m1);
            split448(eep, b2, m2);
            w[b] = load_line16(block_addr(ix, key & 0xFFFFu, b1, lc));
            m[b] = m1 | (m2 << 9) | kActive | (b2 != b1 ? kTwo : 0u);
            if (lc.t == 0) n_reqs += b2 != b1 ? 2u : 1u;
          }
        }
#pragma unroll
        for (int b = 0; b < B; b++) {
          if (m[b] & kActive) {
            const uint32_t e = (uint32_t)(r0 + b) * EPS + grp;
            const bool two = (m[b] & kTwo) != 0;
            const uint64_t r1 = rank_finish<WIDE>(w[b], m[b] & 0x1FFu, lc);
            const uint64_t r2 = rank_finish<WIDE>(w[b], (m[b] >> 9) & 0x1FFu, lc);
            if (lc.t == 0) {
              xc.sp[e] = r1;
              if (two) xc.key[e] |= kPending;      // ep's own block is still to be read
              else xc.ep[e] = r2;
            }
            any_two |= two;
          }
        }
      }
      if (__builtin_amdgcn_ballot_w64(any_two)) {
        pool_sync();
        uint4 w2[G];
        uint32_t m2s[G];
#pragma unroll
        for (int r = 0; r < G; r++) {
          const uint32_t e = (uint32_t)r * EPS + grp;
          const uint32_t key = xc.key[e];
          m2s[r] = 0xFFFFFFFFu;
          w2[r] = make_uint4(0, 0, 0, 0);
          if (key != kNoQuery && (key & kPending)) {
            uint32_t b2, m2;
            split448(xc.ep[e], b2, m2);
            w2[r] = load_line16(block_addr(ix, key & 0xFFFFu, b2, lc));
            m2s[r] = m2;
          }
        }
#pragma unroll
        for (int r = 0; r < G; r++) {
          if (m2s[r] != 0xFFFFFFFFu) {
            const uint64_t r2 = rank_finish<WIDE>(w2[r], m2s[r], lc);
            if (lc.t == 0) xc.ep[(uint32_t)r * EPS + grp] = r2;
          }
        }
      }
    }
    pool_sync();
    }      // !narrow
    PH_MARK(ph2);
    // the table entries are not needed before this point: keeps their loads in flight beside the rank lines'
    asm volatile("" : "+v"(ent.x), "+v"(ent.y), "+v"(ent.z), "+v"(ent.w));
    asm volatile("" : "+v"(r1e));
    if (have) {
      if (from_tab) {
        sp = (((uint64_t)ent.y << 32) | ent.x) & ((1ull << 56) - 1);
        ep = ((uint64_t)ent.w << 32) | ent.z;
      } else if (ranked) {
        if (len == 0) {       // every start element is (0, n): rank(c, 0) = 0, rank(c, n) = the symbol's count
          sp = cfc;
          ep = (c == 255u) ? ix.n : ix.cf[c + 1];
          if (slot == kSlotNone) ep = sp;
          else if (slot == kSlotEof) ep = sp + 1;
        } else if (slot >= kSlotEof) {                  // absent symbol, or the EOF symbol 0
          const uint64_t r1 = (slot == kSlotEof && sp > ix.eof) ? 1 : 0;
          const uint64_t r2 = (slot == kSlotEof && ep > ix.eof) ? 1 : 0;
          sp = cfc + r1;
          ep = cfc + r2;
        } else if (row_q) {
          sp = r1e & ((1ull << 40) - 1);
          ep = sp + (((uint32_t)(r1e >> 40) & 0xFFu) == c ? 1u : 0u);
        } else if (narrow) {
          sp = cfc + nsp;
          ep = cfc + nep;
        } else {
          sp = cfc + xc.sp[xslot];
          ep = cfc + xc.ep[xslot];
        }
      }
      stepped++;
    }
    const uint32_t cce = ra.y;
    uint32_t nf = 0, len1 = 0;
    bool emit = false;
    if (have && sp < ep) {                             // Some((sp1,ep1)), retree.scala:634
      emit = run == 0 && ((cce >> 24) & 1u) != 0;
      nf = run ? 1u : (cce & 0xFFFFu);
      len1 = len + 1;
      if (nf && len1 >= max_len) { nf = 0; trunc = 1; }
    }
    // what the element and its follows carry on: the code while they are still inside the table, else the interval
    const bool keep_code = from_tab && len1 < kt.k;
    const uint64_t ssp = keep_code ? (uint64_t)ncode : sp, sep = keep_code ? 0ull : ep;
    // ---- results are staged in LDS
    {
      const unsigned long long em = __builtin_amdgcn_ballot_w64(emit);
      if (em) {
        const uint32_t cnt = (uint32_t)__builtin_popcountll(em);
        if (rs_n + cnt > kRes64) flush_results();
        if (emit) {
          fmx_result r;
          r.regex = rb.w;
          r.len = len + 1;
          r.sp = sp;
          r.ep = ep;
          rs.r[rs_n + (uint32_t)__builtin_popcountll(em & ((1ull << lane) - 1ull))] = r;
        }
        rs_n = uni(rs_n + cnt);
      }
    }
    // ---- the first follow stays with the lane, the others go to the pool (short lists) or straight to the
    // output queue (a '.' has 253)
    const uint32_t npush = nf ? nf - 1 : 0u;
    {
      uint32_t nsmall = npush <= kPoolSmall ? npush : 0u;
      bool demoted = false;
      if (__builtin_amdgcn_ballot_w64(nsmall != 0)) {
        uint32_t small_total = 0;
        uint32_t my_off = wave_excl_scan(nsmall, small_total);
        if (small_total > 128u) {      // more than the pool can take in one round: lists of 3 and more go the long way
          demoted = nsmall > 2u;
          if (demoted) nsmall = 0;
          my_off = wave_excl_scan(nsmall, small_total);
        }
        if (pn + small_total + 64u > kPool64) {
          const uint32_t need = pn + small_total + 64u - kPool64;
          const uint32_t half = pn < 64u ? pn : 64u;
          const uint32_t out = need > half ? need : half;
          spill(out < pn ? out : pn);
        }
        for (uint32_t q = 0; q < nsmall; q++) {
          const uint32_t fj = q + 1;
          const uint32_t fst = fj < kInlineFollows ? (fj == 1 ? ra.w : (fj == 2 ? rb.x : rb.y)) : nfa.fol[ra.x + fj];
          const uint32_t fch = fj < kInlineFollows ? ((rb.z >> (8u * fj)) & 0xFFu) : (uint32_t)nfa.fol_c[ra.x + fj];
          const uint32_t idx = (pb + pn + my_off + q) & kPool64Mask;
          pl.state[idx] = fst;
          pl.meta[idx] = len1 | (fch << 16);
          pl.sp[idx] = ssp;
          pl.ep[idx] = sep;
        }
        pn = uni(pn + small_total);
        pool_sync();
        // what the wave cannot work off soon goes to the queue, oldest (shallowest) first: waves that ran dry take it
        if (pn > kPoolKeep) spill(pn - kPoolKeep / 2 < 64u ? pn - kPoolKeep / 2 : 64u);
        // a backlog is shared with the workgroup's other waves while the mailbox is nearly empty (nobody takes: it
        // fills once and stays)
        if (kMail && pn > kMailKeep && mail_n() <= kMail - kMailGive) mail_give();
      }
      unsigned long long big = __builtin_amdgcn_ballot_w64(npush > kPoolSmall || demoted);
      while (big) {                                     // one long list at a time, written by the whole wave
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const uint32_t nl = (uint32_t)__builtin_amdgcn_readlane((int)npush, src);
        const uint32_t fo = (uint32_t)__builtin_amdgcn_readlane((int)ra.x, src);
        const uint32_t l1 = (uint32_t)__builtin_amdgcn_readlane((int)len1, src);
        const uint64_t xsp = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(ssp >> 32), src) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)ssp, src);
        const uint64_t xep = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(sep >> 32), src) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)sep, src);
        const Slot sl = reserve(nl);
        for (uint32_t q = lane; q < nl; q += 64)
          put(sl, sl.at + q, nfa.fol[fo + q + 1], l1 | ((uint32_t)nfa.fol_c[fo + q + 1] << 16), xsp, xep);
        n_writes += nl;
      }
    }
    if (have) {
      if (nf) {
        sp = ssp;
        ep = sep;
        // on a literal stretch the next state is state + 1 and its byte comes from the held record:
        // rr[k - 1] with k = states of the stretch still ahead (the chain length when it was just entered)
        const uint32_t k = run ? run : (nf == 1 ? (cce >> 25) & 0xFu : 0u);
        if (k) {
          const uint32_t word = k <= 4u ? ra.w : (k <= 8u ? rb.x : rb.y);
          const uint32_t ch = (word >> (8u * ((k - 1u) & 3u))) & 0xFFu;
          state = run ? state + 1u : ra.z;
          meta = len1 | (ch << 16) | ((k - 1u) << 24);
        } else {
          state = ra.z;
          meta = len1 | ((rb.z & 0xFFu) << 16);
        }
      } else {
        have = false;
      }
    }
    PH_MARK(ph3);
#ifdef FMX_PHASELOG
    if (rounds >= FMX_PHASELOG) ph_n++;
#endif
    if (++rounds >= max_rounds) {
      // ---- out of rounds: everything this wave still holds goes to the output queue
      const unsigned long long held = __builtin_amdgcn_ballot_w64(have);
      if (held) {
        if (have) {
          const uint32_t idx = (pb + pn + (uint32_t)__builtin_popcountll(held & ((1ull << lane) - 1ull))) & kPool64Mask;
          pl.state[idx] = state; pl.meta[idx] = meta & 0x00FFFFFFu; pl.sp[idx] = sp; pl.ep[idx] = ep;   // the stretch context stays behind
        }
        pn = uni(pn + (uint32_t)__builtin_popcountll(held));
      }
      while (pn) spill(pn < 64u ? pn : 64u);
      while (take_batch()) spill(pn);        // carried over, not consumed here
      while (mail_n()) { mail_take(64u); spill(pn); }      // nothing stays in the mailbox when its waves are gone
      break;
    }
  }
  flush_results();
#ifdef FMX_PHASELOG
  if (lane == 0 && j == 0 && w < kLogWaves) { unsigned long long *e = g_phaselog[w]; e[0] = ph0; e[1] = ph1; e[2] = ph2; e[3] = ph3; e[4] = ph_n; }
#endif
#ifdef FMX_WAVELOG
  {
    const unsigned long long st_all = wave_sum((unsigned long long)stepped);
    if (lane == 0 && j < kLogPasses && w < kLogWaves) {
      unsigned long long *e = g_wavelog[j][w];
      e[0] = wl_t0; e[1] = wl_t1; e[2] = __builtin_amdgcn_s_memrealtime(); e[3] = rounds | (st_all << 32);
      e[4] = (unsigned long long)n_writes | ((unsigned long long)n_reads << 32);      // queue entries appended | read (lane 0's counts)
      e[5] = (unsigned long long)appends | ((unsigned long long)grabs << 32);         // reservations in the queue / result slices | looks for others' entries
    }
  }
#endif
  if (trunc) atomicOr(&ctl->truncated, 1ull);
  counters_add(counters, 2ull * stepped, stepped, 0);
  counters_add_frontier(counters, n_reqs, lane == 0 ? n_writes : 0u, lane == 0 ? n_emits : 0u, stepped,
                        lane == 0 ? n_reads : 0u, n_recs);
  {
    const unsigned long long lookups = wave_sum((unsigned long long)n_ktl);
    if (lane == 0 && lookups) atomicAdd(counters + (size_t)(blockIdx.x % kCounterSlots) * kCounterStride + 9, lookups);
    const unsigned long long rows = wave_sum((unsigned long long)n_jl);
    if (lane == 0 && rows) atomicAdd(counters + (size_t)(blockIdx.x % kCounterSlots) * kCounterStride + 11, rows);
  }
}

// 128 registers: 4 waves per SIMD = 256 elements in flight per SIMD.  `j` = the launch's number in its chain (diagnostics).
template <bool WIDE, uint32_t LAYOUT>
__global__ __launch_bounds__(kFThreads, FMX_FWAVES) void k_frontier(DevIndex ix, KTab kt, NfaTables nfa, FlowQueue fq, uint32_t j,
                                                            uint32_t max_rounds, uint64_t sub_cap,
                                                            fmx_result *__restrict__ res, uint64_t seg_cap,
                                                            FrontierCtl *__restrict__ ctl, uint32_t *__restrict__ rcnt,
                                                            unsigned long long *__restrict__ counters) {
  frontier_pass<WIDE, LAYOUT>(ix, kt, nfa, fq, j, max_rounds, sub_cap, res, seg_cap, ctl, rcnt, counters);
}

// where the grouping works: the batch's own result buffer, or straight in the caller's device memory
__device__ __forceinline__ fmx_result *group_out(const CallArgs *call, fmx_result *own, uint64_t own_cap, uint64_t &cap) {
  const CallArgs d = *call;
  if (d.direct) { cap = d.cap < own_cap ? d.cap : own_cap; return d.out; }
  cap = own_cap;
  return own;
}

// Slice i rewound for a new call of `count` start elements (one lane per slice): both buffers empty under fresh tags,
// buffer 0 standing for the slice's share of the start elements (which the first launch makes up, StartSrc), buffer 1
// the first one written, no results yet.
__device__ __forceinline__ void rewind_slice(FrontierCtl *__restrict__ ctl, uint32_t i, uint64_t count) {
  SliceCtl &q = ctl->q[i];
  q.tail[0] = count > i ? (count - i + kSub - 1) / kSub : 0;
  q.tail[1] = 0; q.head[0] = 0; q.head[1] = 0;
  q.tag[0] = next_tag(q.tag[0]); q.tag[1] = next_tag(q.tag[1]);
  q.wsel = 1;
  ctl->res_count[i].v = 0;
}

// A call starts from rewound slices (workgroup 0's first wave, lane = slice); a chain that continues a call only
// takes note of it.  The whole grid clears the per-regex result counts.
__global__ __launch_bounds__(256) void k_frontier_reset(FrontierCtl *__restrict__ ctl, uint64_t count, const CallArgs *__restrict__ call /* pinned host */,
                                                         uint32_t *__restrict__ rcnt, uint32_t k, StartSrc start) {
  const uint32_t fresh = call->fresh;
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const uint32_t i = threadIdx.x;
    const uint32_t max_len = call->max_len, deep_len = call->deep_len;
    if (i == 0) { ctl->fresh = fresh; ctl->deep_len = deep_len; ctl->start = start; }
    if (fresh) {
      rewind_slice(ctl, i, count);
      if (i == 0) { ctl->overflow = 0; ctl->truncated = 0; ctl->max_len = max_len; ctl->left = count; }
    }
  }
  if (!fresh) return;                      // a chain that continues a call
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= k; r += (uint64_t)gridDim.x * blockDim.x) rcnt[r] = 0;      // the frontier kernel counts results per regex
}

// Results leave the device grouped by regex: the frontier kernel counts them per regex where it flushes them; then
// offsets (a scan), scatter, order -- THREE launches behind the frontier's (round 3 had seven: the start elements' own
// launch, scan in two, scatter, two sorts, export; at ~5 us each they were a fifth of a C4 call and over half of a
// call on a real text, where the frontier dies early).
// Exclusive prefix sums of cnt[0..k] in two parts: start[i] = the sum inside i's chunk of 1024 counts, part[chunk] = the
// chunk's total.  The consumers add the chunks before theirs themselves (a hundred values for 100 k regexes, summed
// up in LDS by every workgroup: part_prefix) -- no launch for the scan of the chunk totals, none to add them.
constexpr uint32_t kMaxPartsLds = 2048;      // chunk totals a consumer sums up itself (2 M regexes); beyond: k_res_scan_add
__device__ __forceinline__ uint32_t block_excl_scan_1024(uint32_t v, uint32_t *s_wave /* [16] */, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t wtot = 0;
  const uint32_t ex = wave_excl_scan(v, wtot);          // inside the wave
  if (lane == 0) s_wave[wv] = wtot;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t j = 0; j < 16; j++) {                   // 16 wave totals: every thread adds them up itself
    const uint32_t x = s_wave[j];
    before += j < wv ? x : 0u;
    all += x;
  }
  __syncthreads();
  total = all;
  return before + ex;
}

// Between launches (workgroup 0's first wave, lane = slice): a buffer that has been emptied is rewound under its next
// tag; when that is the buffer the slice was emptying and the written one holds entries, the two swap roles.  Also
// sums up what the host wants to know after a chain.  Behind a chain's LAST launch the same grid starts the grouping:
// every workgroup scans its chunk of the per-regex counts (n != 0).
__global__ __launch_bounds__(kScanChunk) void k_frontier_advance(FrontierCtl *__restrict__ ctl, uint64_t sub_cap, FrontierSummary *__restrict__ sum,
                                                                 const uint32_t *__restrict__ cnt, uint32_t n, uint32_t *__restrict__ start,
                                                                 uint32_t *__restrict__ part, uint32_t *__restrict__ fill, BigGroups *__restrict__ big,
                                                                 uint32_t *__restrict__ zero_next /* the count array the NEXT call counts into, or null */) {
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    SliceCtl &q = ctl->q[threadIdx.x];
    const uint32_t wr = q.wsel, ot = 1u - wr;
    // the launch has worked off (or carried over) everything in the buffer it was not writing
    const unsigned long long tl = q.tail[wr] < sub_cap ? q.tail[wr] : sub_cap;
    const unsigned long long lw = tl > q.head[wr] ? tl - q.head[wr] : 0ull;
    if (q.tail[ot] | q.head[ot]) { q.tail[ot] = 0; q.head[ot] = 0; q.tag[ot] = next_tag(q.tag[ot]); }
    if (lw) q.wsel = ot;
    else if (q.tail[wr] | q.head[wr]) { q.tail[wr] = 0; q.head[wr] = 0; q.tag[wr] = next_tag(q.tag[wr]); }
    const unsigned long long left = wave_sum(lw), results = wave_sum(ctl->res_count[threadIdx.x].v);
    if (threadIdx.x == 0) { ctl->left = left; sum->left = left; sum->results = results; sum->overflow = ctl->overflow; sum->truncated = ctl->truncated; }
  }
  if (!n) return;                                       // uniform over the grid
  __shared__ uint32_t s_wave[16];
  const uint32_t i = blockIdx.x * kScanChunk + threadIdx.x;
  uint32_t total = 0;
  const uint32_t ex = block_excl_scan_1024(i < n ? cnt[i] : 0u, s_wave, total);
  if (i < n) { start[i] = ex; fill[i] = 0; if (zero_next) zero_next[i] = 0; }      // the scatter's cursors start from zero in every grouping
  if (threadIdx.x == 0) part[blockIdx.x] = total;
  if (blockIdx.x == 0 && threadIdx.x == 0) { big->n = 0; big->done = 0; big->total = 0; }
}

// More chunks than a consumer sums up in LDS: their totals are added here, once, and the consumers get part = null.
__global__ __launch_bounds__(kScanChunk) void k_res_scan_add(uint32_t *__restrict__ start, uint32_t n,
                                                             const uint32_t *__restrict__ part) {
  __shared__ unsigned long long s_sum[kScanChunk / 64];
  unsigned long long mine = 0;
  for (uint32_t q = threadIdx.x; q < blockIdx.x; q += kScanChunk) mine += part[q];
  mine = wave_sum(mine);
  if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = mine;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t j = 0; j < kScanChunk / 64; j++) before += (uint32_t)s_sum[j];
  const uint32_t i = blockIdx.x * kScanChunk + threadIdx.x;
  if (i < n) start[i] += before;
}

// s_pre[c] = part[0] + .. + part[c - 1] for c = 0 .. nparts, by a workgroup of 256 threads (ends with a barrier).
// part == null: the offsets are absolute already (k_res_scan_add ran), s_pre is all zeros.
struct PartPrefix {
  uint32_t pre[kMaxPartsLds + 8];
  uint32_t wave[4];
};
__device__ __forceinline__ void part_prefix(const uint32_t *__restrict__ part, uint32_t nparts, PartPrefix &pp) {
  const uint32_t per = (nparts + 256u) / 256u;          // entries per thread, covering 0 .. nparts
  const uint32_t lo = threadIdx.x * per;
  uint32_t mine = 0;
  if (part)
    for (uint32_t q = lo; q < lo + per && q < nparts; q++) mine += part[q];
  uint32_t wtot = 0;
  uint32_t ex = wave_excl_scan(mine, wtot);
  if ((threadIdx.x & 63u) == 0) pp.wave[threadIdx.x >> 6] = wtot;
  __syncthreads();
  for (uint32_t j = 0; j < (threadIdx.x >> 6); j++) ex += pp.wave[j];
  for (uint32_t q = lo; q < lo + per && q <= nparts; q++) {
    pp.pre[q] = ex;
    if (part && q < nparts) ex += part[q];
  }
  __syncthreads();
}
__device__ __forceinline__ uint32_t offset_of(const uint32_t *__restrict__ start, const PartPrefix &pp, uint32_t r) {
  return start[r] + pp.pre[r / kScanChunk];
}

__global__ __launch_bounds__(256) void k_res_scatter(const fmx_result *__restrict__ seg, uint64_t seg_cap,
                                                      const FrontierCtl *__restrict__ ctl,
                                                      const uint32_t *__restrict__ start, const uint32_t *__restrict__ part, uint32_t nparts,
                                                      uint32_t *__restrict__ fill,
                                                      fmx_result *__restrict__ own, uint64_t own_cap, const CallArgs *__restrict__ dst) {
  __shared__ PartPrefix s_pp;
  uint64_t out_cap;
  fmx_result *out = group_out(dst, own, own_cap, out_cap);
  const uint32_t sl = blockIdx.y;
  const uint64_t mine = min((uint64_t)ctl->res_count[sl].v, seg_cap);
  if ((uint64_t)blockIdx.x * blockDim.x >= mine) return;             // uniform over the workgroup: nothing of this slice is ours
  part_prefix(part, nparts, s_pp);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < mine; i += (uint64_t)gridDim.x * blockDim.x) {
    const fmx_result r = seg[(uint64_t)sl * seg_cap + i];
    const uint64_t at = (uint64_t)offset_of(start, s_pp, r.regex) + atomicAdd(&fill[r.regex], 1u);
    if (at < out_cap) out[at] = r;
  }
}

// Orders each regex's group by (len, sp, ep).  The results of a workgroup's 256 regexes are one contiguous stretch of
// `out`; it is read into LDS (it nearly always fits), and EVERY RESULT FINDS ITS OWN PLACE: a thread takes a result,
// counts the results of the same group that sort before it (ties by position) -- independent LDS reads, no chain of
// dependent accesses -- and writes it to that place of `out` (groups of up to 64; C4's 100 k regexes: 11 000 groups of
// 2 .. 23 results, 1.2 ms of single-thread insertion sorts in round 3's kernel).  Larger groups, up to 1024 results, are
// ordered one after the other by a bitonic sort in LDS with all the workgroup's threads; groups beyond that are listed
// for the host.  The workgroup that finishes last reports the call's totals to the host's page-locked GroupTotals;
// with the results delivered in device memory (CallArgs::direct) every workgroup also copies its regexes' counts
// out, and nothing is left for k_res_export to do: it is not launched then.
constexpr uint32_t kRankGroup = 64;
__global__ __launch_bounds__(256) void k_res_sort(fmx_result *__restrict__ own, uint64_t own_cap, const uint32_t *__restrict__ start,
                                                   const uint32_t *__restrict__ part, uint32_t nparts, uint32_t k,
                                                   const uint32_t *__restrict__ rcnt, BigGroups *__restrict__ big,
                                                   const CallArgs *__restrict__ dst, GroupTotals *__restrict__ tot /* pinned host */,
                                                   FrontierCtl *__restrict__ ctl, uint64_t count, StartSrc start_src, uint32_t pre_next) {
  __shared__ fmx_result s_r[kMidGroup];
  __shared__ uint32_t s_last;
  __shared__ PartPrefix s_pp;
  __shared__ uint32_t s_off[257];             // offsets of the workgroup's regexes (and of the one behind them)
  __shared__ uint32_t s_mid[2 * 256], s_nmid;
  if (threadIdx.x == 0) s_nmid = 0;
  part_prefix(part, nparts, s_pp);
  const CallArgs d = *dst;
  uint64_t out_cap;
  fmx_result *out = group_out(dst, own, own_cap, out_cap);
  const uint32_t r0 = blockIdx.x * blockDim.x, r = r0 + threadIdx.x;
  const uint32_t r_end = r0 + blockDim.x < k ? r0 + blockDim.x : k, nr = r_end - r0;
  for (uint32_t t = threadIdx.x; t <= nr; t += blockDim.x) s_off[t] = offset_of(start, s_pp, r0 + t);
  const uint32_t total = offset_of(start, s_pp, k);
  __syncthreads();
  const uint32_t base = s_off[0], span = s_off[nr] - base;      // uniform over the workgroup
  auto less = [](const fmx_result &a, const fmx_result &b) {
    if (a.len != b.len) return a.len < b.len;
    if (a.sp != b.sp) return a.sp < b.sp;
    return a.ep < b.ep;
  };
  // more results than the buffer holds: the call fails with FMX_ERR_OVERFLOW, nothing to order
  if ((uint64_t)base + span <= out_cap) {
    const bool staged = span <= kMidGroup;
    if (staged) {
      for (uint32_t i = threadIdx.x; i < span; i += blockDim.x) s_r[i] = out[base + i];
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < span; i += blockDim.x) {
        const fmx_result x = s_r[i];
        const uint32_t t = x.regex - r0;
        if (t >= nr) continue;                 // (cannot happen: the stretch holds this workgroup's regexes only)
        const uint32_t lo = s_off[t] - base, m = s_off[t + 1] - s_off[t];
        if (m < 2) continue;
        if (m <= kRankGroup) {
          uint32_t rank = 0;
          for (uint32_t j = 0; j < m; j++) {
            const fmx_result y = s_r[lo + j];
            rank += (less(y, x) || (!less(x, y) && lo + j < i)) ? 1u : 0u;
          }
          if (lo + rank != i) out[base + lo + rank] = x;
        } else if (i == lo) {                  // the group's first result lists it (m <= span <= kMidGroup)
          const uint32_t at = atomicAdd(&s_nmid, 1u);
          s_mid[2 * at] = base + lo;
          s_mid[2 * at + 1] = m;
        }
      }
    } else if (r < r_end) {
      // a stretch that does not fit (a group of hundreds of results among the 256): one thread per regex, insertion
      // sort in `out` for the small groups, the others listed
      const uint32_t lo = s_off[threadIdx.x], m = s_off[threadIdx.x + 1] - lo;
      if (m > kMidGroup) {
        const uint32_t at = atomicAdd(&big->n, 1u);
        if (at < kBigMax) { big->ent[2 * at] = lo; big->ent[2 * at + 1] = m; }
      } else if (m > kSmallGroup) {
        const uint32_t at = atomicAdd(&s_nmid, 1u);
        s_mid[2 * at] = lo;
        s_mid[2 * at + 1] = m;
      } else if (m >= 2) {
        fmx_result *g = out + lo;
        for (uint32_t i = 1; i < m; i++) {
          const fmx_result x = g[i];
          uint32_t j = i;
          while (j > 0 && less(x, g[j - 1])) { g[j] = g[j - 1]; j--; }
          g[j] = x;
        }
      }
    }
    __syncthreads();
    const uint32_t nmid = s_nmid;               // the listed groups still lie in `out` as the scatter left them
    for (uint32_t g = 0; g < nmid; g++) {
      const uint32_t lo = s_mid[2 * g], m = s_mid[2 * g + 1];
      uint32_t p2 = 16;
      while (p2 < m) p2 <<= 1;
      for (uint32_t i = threadIdx.x; i < p2; i += blockDim.x) {
        fmx_result x;
        if (i < m) x = out[lo + i];
        else { x.regex = 0; x.len = 0xFFFFFFFFu; x.sp = ~0ull; x.ep = ~0ull; }      // padding sorts last
        s_r[i] = x;
      }
      __syncthreads();
      for (uint32_t size = 2; size <= p2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
          for (uint32_t i = threadIdx.x; i < p2 / 2; i += blockDim.x) {
            const uint32_t a = 2 * i - (i & (stride - 1));          // lower index of the pair
            const uint32_t bidx = a + stride;
            const bool up = (a & size) == 0;
            const fmx_result x = s_r[a], y = s_r[bidx];
            if (less(y, x) == up) { s_r[a] = y; s_r[bidx] = x; }
          }
          __syncthreads();
        }
      for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) out[lo + i] = s_r[i];
      __syncthreads();
    }
  }
  if (d.direct && d.per && r < k) d.per[r] = rcnt[r];
  // No fence here (an agent-scope release writes back the XCD's whole L2: 30 us per launch when every workgroup
  // asks for one).  What the last workgroup reads of the others is big->n, a device atomic whose returned value each
  // of their threads has already used, so it has been performed before that thread reaches the barrier below; the
  // lists and results themselves are read by the host or the next launch, behind the kernel's end.
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = atomicAdd(&big->done, 1u) == gridDim.x - 1u;
    s_last = last ? 1u : 0u;
    if (last) {
      big->total = total;
      tot->n_results = total;
      tot->n_big = atomicAdd(&big->n, 0u);
    }
  }
  if (pre_next) {                          // uniform over the grid
    // The call is over when its last launch left nothing queued: the workgroup that finishes last then leaves the batch
    // READY for a next call with the same limits -- the slices rewound as k_frontier_reset's first wave does it -- so that
    // such a call begins with the frontier launch itself (the host skips the reset launch: CallPlan::pre_now).  Nothing
    // of this grouping reads the slices any more (the scatter is done); a call that is NOT over (left != 0) keeps its
    // state and resets as before.
    __syncthreads();
    if (s_last && threadIdx.x < kSub && ctl->left == 0 && ctl->overflow == 0) {
      const uint32_t i = threadIdx.x;
      rewind_slice(ctl, i, count);
      if (i == 0) { ctl->fresh = 1; ctl->deep_len = d.deep_len; ctl->start = start_src; ctl->truncated = 0; ctl->max_len = d.max_len; ctl->left = count; }
    }
  }
}

// Results delivered to the HOST's page-locked buffers (or, in an A/B run, to device memory without the direct form):
// the ordered results and the per-regex counts are copied there, behind the grouping and before the host's one
// synchronisation.  Not launched when the grouping worked in the caller's device memory itself.
__global__ __launch_bounds__(256) void k_res_export(const fmx_result *__restrict__ res, uint32_t k,
                                                     const uint32_t *__restrict__ rcnt, const BigGroups *__restrict__ big,
                                                     const CallArgs *__restrict__ dst) {
  const CallArgs d = *dst;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  if (d.out && !d.direct) {
    const uint64_t n = big->total < d.cap ? big->total : d.cap;
    // 24-byte results as 16-byte words (both buffers are 16-byte aligned: hipMalloc / page-locked memory), the odd
    // eight bytes at the end on their own
    const uint64_t words = 3 * n;                                   // 8-byte words
    const uint4 *src = reinterpret_cast<const uint4 *>(res);
    uint4 *out = reinterpret_cast<uint4 *>(d.out);
    const bool aligned = (reinterpret_cast<uintptr_t>(d.out) & 15u) == 0;
    if (aligned) {
      for (uint64_t i = tid; i < words / 2; i += nth) out[i] = src[i];
      if ((words & 1u) && tid == 0) reinterpret_cast<uint2 *>(d.out)[words - 1] = reinterpret_cast<const uint2 *>(res)[words - 1];
    } else {
      for (uint64_t i = tid; i < words; i += nth) reinterpret_cast<uint2 *>(d.out)[i] = reinterpret_cast<const uint2 *>(res)[i];
    }
  }
  if (d.per && !d.direct)
    for (uint64_t i = tid; i < k; i += nth) d.per[i] = rcnt[i];
}

// ---- the host's two ways in (fmx_frontier.h).  Launches are chained on the stream without host round trips; a launch
// that finds the queue empty returns at once.
static void launch_pass(const Index *h, const RegexBatch *b, const CallPlan &p, hipStream_t s, int grid, uint32_t j, uint32_t rounds) {
  if (h->layout == kLayoutBytes)
    k_frontier<true, kLayoutBytes><<<grid, kFThreads, 0, s>>>(h->dev, p.kt, b->nfa, b->fq, j, rounds, p.sub_cap, b->d_res_seg, p.seg_cap, b->d_ctl, b->d_rcnt, h->d_counters);
  else if (h->n > (1ull << 32))
    k_frontier<true, kLayoutOneHot><<<grid, kFThreads, 0, s>>>(h->dev, p.kt, b->nfa, b->fq, j, rounds, p.sub_cap, b->d_res_seg, p.seg_cap, b->d_ctl, b->d_rcnt, h->d_counters);
  else
    k_frontier<false, kLayoutOneHot><<<grid, kFThreads, 0, s>>>(h->dev, p.kt, b->nfa, b->fq, j, rounds, p.sub_cap, b->d_res_seg, p.seg_cap, b->d_ctl, b->d_rcnt, h->d_counters);
}

hipError_t enqueue_chain(const Index *h, const RegexBatch *b, const CallPlan &p, const ChainShape &shape, hipStream_t s) {
  const uint32_t n_scan = (uint32_t)b->k + 1, nparts = (n_scan + kScanChunk - 1) / kScanChunk;     // cnt[k] is 0: its offset = the total
  // a call's first chain begins with the reset (CallArgs::fresh; a later chain's only takes note that it continues one)
  if (!(p.pre_now && b->h_args->fresh))
    k_frontier_reset<<<(int)std::min<size_t>((b->k + 256) / 256, 256), 256, 0, s>>>(b->d_ctl, b->n_first, b->h_args, b->d_rcnt, (uint32_t)b->k, p.ss);
  for (uint32_t j = 0; j < shape.launches; j++) {
    launch_pass(h, b, p, s, shape.grid, j, shape.rounds);
    // the summary goes straight to pinned host memory; behind the chain's last launch the same grid scans the result counts
    if (j + 1 < shape.launches) k_frontier_advance<<<1, kScanChunk, 0, s>>>(b->d_ctl, p.sub_cap, b->h_sum, nullptr, 0u, nullptr, nullptr, nullptr, nullptr, nullptr);
    else k_frontier_advance<<<nparts, kScanChunk, 0, s>>>(b->d_ctl, p.sub_cap, b->h_sum, b->d_rcnt, n_scan, b->d_rstart, b->d_rpart, b->d_rfill, b->d_big, p.pre_next ? b->d_rcnt2[b->rc_sel ^ 1u] : nullptr);
  }
  return hipGetLastError();
}

// The results leave the device grouped by regex (count, scan, scatter, order small groups, totals to pinned host
// memory).  These launches are enqueued right behind every chain, before the host knows whether the search is
// over: when it is -- the usual case -- the grouped results are ready at the same synchronisation; when it is
// not, the grouping is simply done again behind the next chain.
hipError_t enqueue_group(const RegexBatch *b, const CallPlan &p, hipStream_t s) {
  const uint32_t n_scan = (uint32_t)b->k + 1, nparts = (n_scan + kScanChunk - 1) / kScanChunk;
  const bool parts_in_lds = nparts <= kMaxPartsLds;      // the consumers of the offsets add the chunk totals up themselves
  const dim3 rg(8, kSub);
  if (!parts_in_lds) k_res_scan_add<<<nparts, kScanChunk, 0, s>>>(b->d_rstart, n_scan, b->d_rpart);
  const uint32_t *part = parts_in_lds ? b->d_rpart : nullptr;
  k_res_scatter<<<rg, 256, 0, s>>>(b->d_res_seg, p.seg_cap, b->d_ctl, b->d_rstart, part, nparts, b->d_rfill, b->d_res, (uint64_t)b->rcap, b->h_args);
  k_res_sort<<<(int)((b->k + 255) / 256), 256, 0, s>>>(b->d_res, (uint64_t)b->rcap, b->d_rstart, part, nparts, (uint32_t)b->k, b->d_rcnt, b->d_big, b->h_args, b->h_tot, b->d_ctl, (uint64_t)b->n_first, p.ss, p.pre_next ? 1u : 0u);
  if (!p.direct) k_res_export<<<256, 256, 0, s>>>(b->d_res, (uint32_t)b->k, b->d_rcnt, b->d_big, b->h_args);
  return hipGetLastError();
}

}  // namespace fmx

using namespace fmx;

extern "C" {
#ifdef FMX_WAVELOG
int fmx_debug_phaselog(void *out, size_t bytes) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phaselog), std::min(bytes, sizeof g_phaselog)) == hipSuccess ? FMX_OK : FMX_ERR_HIP;
}
int fmx_debug_wavetrace(void *out, size_t bytes) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavetrace), std::min(bytes, sizeof g_wavetrace)) == hipSuccess ? FMX_OK : FMX_ERR_HIP;
}
int fmx_debug_wavelog(void *out, size_t bytes, int clear) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavelog), std::min(bytes, sizeof g_wavelog)) != hipSuccess) return FMX_ERR_HIP;
  if (clear) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_wavelog)) != hipSuccess || hipMemset(p, 0, sizeof g_wavelog) != hipSuccess) return FMX_ERR_HIP;
  }
  return FMX_OK;
}
#endif
}  // extern "C"
