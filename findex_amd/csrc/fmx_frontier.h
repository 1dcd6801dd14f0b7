// fmx_frontier.h -- what the regex frontier's device side (fmx_frontier.hip: the kernels and the two functions that
// enqueue them) and its host side (fmx_regex_batch.hip: resident batches and the match call) share.
#pragma once
#include <fmx.h>

#include <memory>
#include <vector>

#include "fmx_device.h"
#include "fmx_host.h"
#include "fmx_nfa.h"

namespace fmx {

#ifndef FMX_FTHREADS
#define FMX_FTHREADS 256
#endif
constexpr int kFThreads = FMX_FTHREADS;      // threads of a frontier workgroup
constexpr int kFWaves = kFThreads / 64;       // waves of a workgroup (they share one mailbox)
#ifndef FMX_FWAVES
#define FMX_FWAVES 4                          // waves per SIMD the frontier kernel is built for (its launch bounds; the full grid's size)
#endif

// The work queue in HBM.  An entry is three 8-byte GRANULES, each written by one aligned agent-scope (write-through)
// store and carrying the tag of its buffer's current generation in its top 16 bits -- the data is its own "ready"
// flag (cdna_hip_programming.md, Guideline 16, form R2), so a wave may take entries that another wave appended
// earlier IN THE SAME LAUNCH: it re-reads a granule until the tag matches.
//   g0 = tag:16 | byte:8 | sp:40        g1 = tag:16 | 0:8 | ep:40        g2 = tag:16 | len:16 | state:32
struct FlowQueue {
  unsigned long long *g0, *g1, *g2;    // kSub slices x 2 buffers x sub_cap entries each
};
// A call's START elements (states = the regexes' firsts, length 0, every row) are not queued: the first launch of a
// call makes them up where it would have read them from slice `s`, position `p` of the queue -- elem[s * cap + p] =
// state | its byte << 40, laid out slice by slice when the batch was made resident (round 3 wrote them to the queue
// in a launch of their own: 12 us of a 0.4 ms call).
struct StartSrc {                     // (kept in FrontierCtl and read there when a wave takes a batch: no registers held over the rounds)
  const unsigned long long *elem;
  unsigned long long cap;             // entries per slice in `elem`
  unsigned long long ep;              // what a start element carries as its interval's end: n, or 0 = the empty k-mer code
};
constexpr uint32_t kMaxLen = 0xFFFFu;
constexpr uint64_t kMaxRows = 1ull << 40;     // sp / ep fields of a granule

// The queue and the result buffer are cut into kSub slices with their own counters, every slice on its own
// 128-byte line: a single tail cannot take the appends of a whole launch (same-address device atomics complete at
// ~100 per microsecond).  A wave appends to slice (wave + number of its earlier appends) % kSub, so slices stay
// balanced even when one wave produces everything.
// Every slice has TWO linear buffers.  Appends go to buffer `wsel`; takers empty the other one first.  Between
// launches (k_frontier_advance) a buffer that has been emptied is rewound -- tail = head = 0, next tag -- and
// becomes the slice's write buffer, so the memory a search needs follows the frontier's width, not its total work.
constexpr uint32_t kSub = 64;
struct alignas(128) SliceCtl {
  unsigned long long tail[2];      // entries appended (agent-scope atomic adds)
  unsigned long long head[2];      // entries taken (atomic add on the buffer that is not written; CAS on the other)
  uint32_t tag[2];                 // generation tag of each buffer: 1..65535, 0 = never written
  uint32_t wsel;                   // the buffer this launch appends to
  uint32_t pad_[21];
};
struct alignas(128) PaddedCount {
  unsigned long long v;
  unsigned long long pad[15];
};
constexpr uint32_t kTagLimit = 60000;          // host-side bound on a buffer's generation tag before everything is zeroed

struct FrontierCtl {     // device-resident counters
  SliceCtl q[kSub];
  PaddedCount res_count[kSub];
  unsigned long long overflow;     // bit 0: queue, bit 1: results, bit 2: an appended entry never became readable
  unsigned long long truncated;    // some element was not expanded because its follows would have len >= max_len
  uint32_t max_len;
  uint32_t deep_len;               // the length past which an interval has narrowed to a row (CallArgs::deep_len; no kernel reads it now)
  uint32_t fresh;                  // this chain of launches begins a call (k_frontier_reset): its first launch makes up the start elements
  unsigned long long left;         // entries queued when the launch began (k_frontier_reset / k_frontier_advance): 0 = nothing to do
  StartSrc start;                  // this call's start elements (k_frontier_reset)
};
struct FrontierSummary { // what the host reads after a chain of launches (k_frontier_advance)
  unsigned long long left;         // entries still queued
  unsigned long long results;
  unsigned long long overflow;
  unsigned long long truncated;
};

// The offsets of the per-regex result groups are a scan of the counts in chunks of kScanChunk (k_frontier_advance)
constexpr uint32_t kScanChunk = 1024;
// result groups the device leaves to the host (k_res_sort)
constexpr uint32_t kSmallGroup = 12;
constexpr uint32_t kBigMax = 16384;
constexpr uint32_t kMidGroup = 1024;   // groups up to this size are ordered by a workgroup in LDS (k_res_sort's second phase)
struct BigGroups {
  uint32_t n;                    // groups of more than kMidGroup results: left to the host
  uint32_t done;                 // workgroups of k_res_sort that have finished (the last one reports the totals)
  uint32_t total;                // results of the call (k_res_export reads it)
  uint32_t pad_;
  uint32_t ent[2 * kBigMax];     // (first result, count) of each such group
};

// What the host needs to fetch the grouped results: how many there are and how many groups were left unsorted
// (written to pinned host memory by k_res_sort's last workgroup).
struct GroupTotals {
  uint32_t n_results;
  uint32_t n_big;
};
// A call's own values.  The struct lives in pinned host memory; the host fills it before it starts the launches and
// the kernels read it there.
struct CallArgs {
  // Where the grouped results go when the caller's buffers are page-locked (fmx_host_alloc) or device memory: the
  // device writes them there itself, behind the grouping and before the host's one synchronisation (null pointers:
  // the host copies after the synchronisation).
  fmx_result *out;
  unsigned long long cap;
  uint32_t *per;
  // what a call's first chain of launches starts from (k_frontier_reset reads it)
  uint32_t max_len;
  uint32_t fresh;        // 1: this chain begins a call (reset the queue, write the start elements); 0: it continues one
  uint32_t direct;       // 1: `out` is device memory (fmx_regex_batch_match_dev): the grouping kernels scatter and order the
                         // results right there, no export copy of them
  uint32_t deep_len;     // FrontierCtl::deep_len of this call
};

// A batch of compiled regexes made resident on one device: concatenated Glushkov tables plus
// the level-0 frontier (root.firsts x (0, 0, n), retree.scala:576).  Reusable across calls.
struct RegexBatch {
  int device = 0;
  size_t k = 0;
  uint64_t index_serial = 0;           // the fmx_index this batch was made for (Index::serial): the tables' state bytes, the
                                       // start elements and the work estimate that ordered them were made for that index
                                       // and its device, so no other handle may match against the batch
  size_t n_first = 0, n_states = 0, n_fol = 0;
  std::vector<uint32_t> start_final;   // DFA engines whose start state is final: result (len 0, 0, n)
  DevMem mem;
  // scratch reused across matches of this batch (one match at a time per batch object)
  std::unique_ptr<DevMem> scratch;
  FlowQueue fq{};
  uint32_t tag_bound = 0;              // upper bound of the buffers' generation tags (fmx_regex_batch.hip, count_tags)
  fmx_result *d_res = nullptr;        // packed results
  fmx_result *d_res_seg = nullptr;    // kSub result slices the levels append to
  FrontierCtl *d_ctl = nullptr;
  uint32_t *d_rcnt = nullptr, *d_rstart = nullptr, *d_rfill = nullptr;   // per-regex result counts / offsets
  // Round 5: a call that ends normally leaves the batch READY for the next one -- k_res_sort's last workgroup rewinds the
  // queue's slices (what k_frontier_reset's first wave did), and the scan of the per-regex counts zeroes the OTHER of two
  // count arrays, which the next call counts into -- so that a call with the same limits starts with the frontier launch
  // (one launch and ~6 us less per call; C4text: a twentieth of the call).  pre_* = what the batch was left ready for.
  uint32_t *d_rcnt2[2] = {nullptr, nullptr};
  uint32_t rc_sel = 0;
  bool pre_ok = false;
  uint32_t pre_max_len = 0, pre_deep = 0;
  size_t pre_count = 0;
  StartSrc pre_ss{nullptr, 0, 0};
  uint32_t *d_rpart = nullptr;         // chunk totals of the offsets' scan
  BigGroups *d_big = nullptr;
  FrontierSummary *h_sum = nullptr;    // pinned: what a chain reports (written by k_frontier_advance)
  CallArgs *h_args = nullptr;          // pinned: the call's own values (set per call)
  GroupTotals *h_tot = nullptr;        // pinned: the grouping's totals, written by k_res_sort's last workgroup
  ~RegexBatch() {
    if (h_tot) (void)hipHostFree(h_tot);
    if (h_sum) (void)hipHostFree(h_sum);
    if (h_args) (void)hipHostFree(h_args);
  }
  uint64_t qcap = 0;
  size_t rcap = 0;
  NfaTables nfa{};
  uint32_t *d_first_state = nullptr;   // root.firsts of every regex, regex by regex
  unsigned long long *d_start_elem = nullptr;   // the frontier kernel's start elements (StartSrc), balanced over the waves, slice by slice
  uint64_t start_cap = 0;              // entries per slice there
  // reference-order mode (ReTree batches only): heap keys, per-regex firsts, the largest fan-out
  uint32_t *d_st_num = nullptr, *d_first_off = nullptr;
  FolRec *d_fol_rec = nullptr, *d_first_rec = nullptr;
  uint32_t max_fanout = 1, max_num = 0;
  bool all_retree = true;
};

// One match call's plan: what the host decides before the first launch and both enqueue functions read.
struct ChainShape {
  int grid;                // workgroups of a frontier launch
  uint32_t launches;       // frontier launches per chain, i.e. per host look at the summary
  uint32_t rounds;         // rounds a wave works at most in one launch
};
struct CallPlan {
  uint32_t max_len;        // fmx_limits.max_steps
  uint64_t sub_cap;        // entries of one buffer of a queue slice
  uint64_t seg_cap;        // results of one result slice
  // Two grids: the full one for a batch's wide phase, and a small one (64 workgroups: lanes for 16384 elements) for a
  // single regex or the thin end of a batch, whose launches cost a fraction of the full grid's when most of them find
  // nothing to do.
  ChainShape full, small;
  KTab kt;                 // the handle's k-mer and row tables as this call's launches see them
  StartSrc ss;
  uint32_t deep_len;
  bool pre_next;           // this call leaves the batch ready for the next one (RegexBatch::pre_ok)
  bool pre_now;            // the LAST call left it ready for exactly this one: no reset launch
  bool direct;             // the grouping works in the caller's device memory (CallArgs::direct)
  bool export_out, export_per;     // the device writes the results / the per-regex counts where the caller wants them
};

// fmx_frontier.hip.  Both only enqueue on `s`; they return hipGetLastError().
// One chain = the reset (not when the batch was left ready for this call) + the shape's launches, each followed by
// k_frontier_advance; behind the chain's last launch that grid also scans the per-regex result counts.
hipError_t enqueue_chain(const Index *h, const RegexBatch *b, const CallPlan &p, const ChainShape &shape, hipStream_t s);
// The grouping of the results by regex behind a chain: scatter, order, and the export unless the grouping worked in
// the caller's device memory.
hipError_t enqueue_group(const RegexBatch *b, const CallPlan &p, hipStream_t s);

}  // namespace fmx
