// fmx_api.cpp -- the C ABI of libfmx.so (include/fmx.h): file loaders, handle lifetime, and the
// host-pointer wrappers around the device entry points.  No compute happens on the host.
#include <fmx.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "fmx_host.h"
#include "fmx_hostpar.h"
#include "fmx_regex.h"

namespace fmx {

static thread_local std::string g_err;

void set_error(const std::string &msg) { g_err = msg; }

int hip_fail(hipError_t e, const char *what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return FMX_ERR_HIP;
}

static std::atomic<int> g_layout_pref{-1};       // fmx_config_set may race with fmx_open* on other threads
int layout_preference() { return g_layout_pref.load(std::memory_order_relaxed); }
static std::atomic<uint64_t> g_serial{0};
static std::atomic<int> g_force_superblocks{0};
static std::atomic<int> g_validate{0};
// fmx_config_set("pipeline", ..): large host batches in page-locked memory cut into chunks over three streams
static std::atomic<int> g_pipeline{0};
bool validate_device_operands() { return g_validate.load(std::memory_order_relaxed) != 0; }
bool force_superblocks() { return g_force_superblocks.load(std::memory_order_relaxed) != 0; }

int arg_fail(const char *msg) {
  g_err = msg;
  return FMX_ERR_ARG;
}

int use_device(const Index *h) {
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  return FMX_OK;
}

int use_device_index(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_err = "no HIP device available (libfmx has no CPU fallback)"; return FMX_ERR_HIP; }
  if (device < 0 || device >= ndev) return arg_fail("device index out of range");
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  return FMX_OK;
}

int no_capture(hipStream_t st, const char *text) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(st, &cs), "hipStreamIsCapturing");
  if (cs != hipStreamCaptureStatusNone) {
    g_err = text;
    return FMX_ERR_HIP;
  }
  return FMX_OK;
}

int not_capturing(hipStream_t st, const char *what) {
  return no_capture(st, (std::string(what) + " allocates and synchronises: not under a stream capture").c_str());
}

int device_room(uint64_t need, const std::string &what, const char *verb) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
  if (need > free_b) {
    g_err = what + " " + verb + " " + std::to_string(need) + " bytes of device memory, " + std::to_string(free_b) + " are free";
    return FMX_ERR_NOMEM;
  }
  return FMX_OK;
}

// What a handle builds at first use (the locate samples, the LCP array, ..) is built here when a call finds none.
int ensure_built(const Index *h, Side &side, int (*prepare)(const Index *, hipStream_t), hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(side.mu);
    if (side.ready) return FMX_OK;
  }
  if (st) return prepare(h, st);
  CtxLease lease(h);
  if (!lease.c) return FMX_ERR_HIP;
  return prepare(h, lease.c->stream);
}

static void free_ctx(CallCtx *c) {
  if (!c) return;
  for (void *b : c->buf) if (b) (void)hipFree(b);
  if (c->pin) (void)hipHostFree(c->pin);
  if (c->ev_a) (void)hipEventDestroy(c->ev_a);
  if (c->ev_b) (void)hipEventDestroy(c->ev_b);
  for (hipEvent_t e : c->chunk_ev) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

CallCtx *ctx_acquire(const Index *h) {
  CallCtx *c = nullptr;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->ctx_pool.empty()) { c = h->ctx_pool.back(); h->ctx_pool.pop_back(); }
  }
  if (!c) c = new (std::nothrow) CallCtx();
  if (!c) { g_err = "out of host memory"; return nullptr; }
  hipError_t e = hipSuccess;
  // non-blocking: no implicit ties to the legacy stream (another host thread may be capturing a graph, or torch may
  // be working on stream 0)
  if (!c->stream) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess && !c->ev_a) e = hipEventCreate(&c->ev_a);
  if (e == hipSuccess && !c->ev_b) e = hipEventCreate(&c->ev_b);
  if (e != hipSuccess) { (void)hip_fail(e, "hipStreamCreate/hipEventCreate"); free_ctx(c); return nullptr; }
  return c;
}

// Contexts holding more than kKeepBytes of scratch, and contexts beyond kKeep idle ones, are released.
void ctx_release(const Index *h, CallCtx *c) {
  constexpr size_t kKeep = 4;
  constexpr size_t kKeepBytes = 2048ull << 20;    // the reference-order match of a 100 k batch holds ~0.5 GiB (element slabs + raw results)
  bool keep = c->total() <= kKeepBytes;
  if (keep) {
    std::lock_guard<std::mutex> lk(h->mu);
    keep = h->ctx_pool.size() < kKeep;
    if (keep) h->ctx_pool.push_back(c);
  }
  if (!keep) free_ctx(c);
}

hipError_t ctx_scratch(CallCtx *c, int i, size_t bytes, void **out) {
  if (bytes < 16) bytes = 16;
  if (c->cap[i] < bytes) {
    if (c->buf[i]) { (void)hipFree(c->buf[i]); c->buf[i] = nullptr; c->cap[i] = 0; }
    const size_t want = bytes + bytes / 4;          // some slack: batches of similar size reuse the buffer
    hipError_t e = hipMalloc(&c->buf[i], want);
    if (e != hipSuccess) return e;
    c->cap[i] = want;
  }
  *out = c->buf[i];
  return hipSuccess;
}

// One host-pointer call: borrows a context from the handle (or makes one), hands out scratch buffers from it,
// runs the enqueue function on its stream between its two events, and returns the context on scope exit.
class Call {
 public:
  explicit Call(const Index *h) : h_(h) {}
  ~Call() { if (c_) ctx_release(h_, c_); }
  int init() {
    if (!c_) c_ = ctx_acquire(h_);
    return c_ ? FMX_OK : FMX_ERR_HIP;
  }
  // next scratch buffer of the call, at least `bytes` long
  hipError_t alloc(void **p, size_t bytes) {
    if (next_ >= CallCtx::kBufs) return hipErrorOutOfMemory;
    return ctx_scratch(c_, next_++, bytes, p);
  }
  // pinned host staging of at least `bytes`
  hipError_t pinned(void **out, size_t bytes) {
    if (c_->pin_cap < bytes) {
      if (c_->pin) { (void)hipHostFree(c_->pin); c_->pin = nullptr; c_->pin_cap = 0; }
      hipError_t e = hipHostMalloc(&c_->pin, bytes, hipHostMallocDefault);
      if (e != hipSuccess) return e;
      c_->pin_cap = bytes;
    }
    *out = c_->pin;
    return hipSuccess;
  }
  hipStream_t stream() const { return c_->stream; }
  hipError_t chunk_events(size_t n, hipEvent_t **out) {      // n events that live with the context
    while (c_->chunk_ev.size() < n) {
      hipEvent_t e = nullptr;
      const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
      if (rc != hipSuccess) return rc;
      c_->chunk_ev.push_back(e);
    }
    *out = c_->chunk_ev.data();
    return hipSuccess;
  }
  hipEvent_t ev_a() const { return c_->ev_a; }
  hipEvent_t ev_b() const { return c_->ev_b; }
  // Runs enqueue(stream, ev_a, ev_b) on the context's stream, waits for it and records the device time between the two
  // events.  events = false: it gets null events and records none; the call counts as a launch, its time is not taken.
  template <class F>
  int timed(F enqueue, bool events = true) {
    int rc = enqueue(c_->stream, events ? c_->ev_a : nullptr, events ? c_->ev_b : nullptr);
    if (rc != FMX_OK) { (void)hipStreamSynchronize(c_->stream); return rc; }
    HIP_TRY(hipStreamSynchronize(c_->stream), "hipStreamSynchronize");
    float ms = 0;
    if (!events || hipEventElapsedTime(&ms, c_->ev_a, c_->ev_b) == hipSuccess) {
      std::lock_guard<std::mutex> lk(h_->mu);
      if (events) h_->last_kernel_ms = ms;
      h_->launches++;
    }
    return FMX_OK;
  }
  // One launch alone between the two events: launch(stream) -> hipError_t
  template <class L>
  int timed_launch(L launch, const char *what) {
    return timed([&](hipStream_t st, hipEvent_t ev_a, hipEvent_t ev_b) {
      HIP_TRY(hipEventRecord(ev_a, st), "hipEventRecord");
      HIP_TRY(launch(st), what);
      HIP_TRY(hipEventRecord(ev_b, st), "hipEventRecord");
      return (int)FMX_OK;
    });
  }

 private:
  const Index *h_;
  CallCtx *c_ = nullptr;
  int next_ = 0;
};

// ---- file formats
static uint64_t rd_u64(const uint8_t *p, bool be) {
  uint64_t v = 0;
  if (be) for (int i = 0; i < 8; i++) v = (v << 8) | p[i];
  else for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}

// BWTLoader, bwtmerger.scala:144-174: int64 size, int64 eof, then `size` bytes; size+16 == file length.
// Checks the header and leaves the file positioned at the payload; the payload is then streamed to the
// device in chunks (stream_file_to_device) -- a 16 GiB .bwt never sits in host memory whole.
static int open_bwt_file(const char *path, bool be, FILE **out, uint64_t &n, uint64_t &eof) {
  FILE *f = std::fopen(path, "rb");
  if (!f) { g_err = std::string("File ") + path + " does not exists"; return FMX_ERR_IO; }
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
  uint8_t hdr[16];
  if (std::fread(hdr, 1, 16, f) != 16) { g_err = std::string("File ") + path + " bad size"; return FMX_ERR_FORMAT; }
  n = rd_u64(hdr, be);
  eof = rd_u64(hdr + 8, be);
  if (fseeko(f, 0, SEEK_END) != 0) { g_err = "seek failed"; return FMX_ERR_IO; }
  const uint64_t flen = (uint64_t)ftello(f);
  if (n + 16 != flen) {
    g_err = std::string("File ") + path + " bad size " + std::to_string(n) + " != " + std::to_string(flen) + " + 16";
    return FMX_ERR_FORMAT;
  }
  if (fseeko(f, 16, SEEK_SET) != 0) { g_err = "seek failed"; return FMX_ERR_IO; }
  *out = guard.release();
  return FMX_OK;
}

// n bytes from the file's current position to device memory through two pinned staging buffers: the read of
// chunk i+1 overlaps the DMA of chunk i.
static int stream_file_to_device(FILE *f, void *dst, uint64_t n, hipStream_t st) {
  constexpr size_t kChunk = 32u << 20;
  struct Pin {
    void *p[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~Pin() {
      for (int i = 0; i < 2; i++) { if (p[i]) (void)hipHostFree(p[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); }
    }
  } pin;
  const size_t chunk = (size_t)std::min<uint64_t>(kChunk, n ? n : 1);
  for (int i = 0; i < 2; i++) {
    HIP_TRY(hipHostMalloc(&pin.p[i], chunk, hipHostMallocDefault), "hipHostMalloc(staging)");
    HIP_TRY(hipEventCreateWithFlags(&pin.ev[i], hipEventDisableTiming), "hipEventCreate");
  }
  bool used[2] = {false, false};
  int slot = 0;
  for (uint64_t o = 0; o < n; o += chunk, slot ^= 1) {
    const size_t len = (size_t)std::min<uint64_t>(chunk, n - o);
    if (used[slot]) HIP_TRY(hipEventSynchronize(pin.ev[slot]), "hipEventSynchronize");     // its last DMA is done
    if (std::fread(pin.p[slot], 1, len, f) != len) { g_err = "short read on the .bwt payload"; return FMX_ERR_IO; }
    HIP_TRY(hipMemcpyAsync(static_cast<uint8_t *>(dst) + o, pin.p[slot], len, hipMemcpyHostToDevice, st), "H2D(bwt)");
    HIP_TRY(hipEventRecord(pin.ev[slot], st), "hipEventRecord");
    used[slot] = true;
  }
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");     // the staging buffers are freed on return
  return FMX_OK;
}

// AUXLoader, bwtmerger.scala:130-142: 256 int64 counts.
static int load_aux(const char *path, bool be, int64_t counts[256]) {
  FILE *f = std::fopen(path, "rb");
  if (!f) { g_err = std::string("File ") + path + " does not exists"; return FMX_ERR_IO; }
  uint8_t buf[2048];
  size_t got = std::fread(buf, 1, sizeof buf, f);
  int extra = std::fgetc(f);
  std::fclose(f);
  if (got != sizeof buf || extra != EOF) { g_err = std::string("File ") + path + " bad aux size"; return FMX_ERR_FORMAT; }
  for (int i = 0; i < 256; i++) counts[i] = (int64_t)rd_u64(buf + 8 * i, be);
  return FMX_OK;
}

Worker *worker_of(const Index *h) {
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->worker) h->worker.reset(new Worker());
  return h->worker.get();
}

// What a handle derives outside the table budget, by its fmx_prepare / fmx_drop_tables flag.  In this order: the extract
// samples take a short cut through locate samples at the same rate, and the line table's build reads the locate samples.
static const struct DerivedFlag {
  unsigned flag;
  int (*check)(const Index *);
  int (*prepare)(const Index *, hipStream_t);
  void (*drop)(Index *);
} kDerived[] = {
    {FMX_PREPARE_LOCATE, locate_check, locate_prepare, [](Index *h) { h->loc.drop(); }},
    {FMX_PREPARE_LCP, lcp_check, lcp_prepare, [](Index *h) { h->lcp.drop(); }},
    {FMX_PREPARE_EXTRACT, extract_check, extract_prepare, [](Index *h) { h->ext.drop(); }},
    {FMX_PREPARE_LINES, lines_check, lines_prepare, [](Index *h) { h->lin.drop(); }},
};
static unsigned derived_flags() {
  unsigned all = 0;
  for (const DerivedFlag &d : kDerived) all |= d.flag;
  return all;
}
static constexpr unsigned kDroppableTables = FMX_PREPARE_KTAB | FMX_PREPARE_JUMP | FMX_PREPARE_FRONTIER;      // those of the budget

// fmx_drop_tables and fmx_close: the budgeted tables (fmx_jump.hip), then the rest by the table above
static int drop_derived(Index *h, unsigned what) {
  const int rc = drop_tables(h, what);
  for (const DerivedFlag &d : kDerived)
    if (what & d.flag) d.drop(h);
  return rc;
}

static void destroy(Index *h) {
  if (!h) return;
  h->worker.reset();                  // finishes what was submitted, joins
  (void)hipSetDevice(h->device);
  (void)drop_derived(h, kDroppableTables | FMX_PREPARE_SELECT | derived_flags());      // (the select directory goes only here)
  if (h->d_bv) (void)hipFree(h->d_bv);
  if (h->d_chk) (void)hipFree(h->d_chk);
  if (h->d_sup) (void)hipFree(h->d_sup);
  if (h->d_bwt) (void)hipFree(h->d_bwt);
  if (h->d_cf) (void)hipFree(h->d_cf);
  if (h->d_slot) (void)hipFree(h->d_slot);
  if (h->d_counters) (void)hipFree(h->d_counters);
  for (CallCtx *c : h->ctx_pool) free_ctx(c);
  delete h;
}

// Common tail of the three open flavours: `src` is host or device memory holding n BWT bytes.
struct BlockSpec {       // fmx_open_block: NaiveBWTSearcher's constructor arguments beside the BWT
  const int64_t *bs;
  int first, skipped;    // BWT bytes at position 0 (-1 when that is the skipped row) and at the skipped row
};

static int open_common(const void *src, bool src_on_device, FILE *src_file, uint64_t n, uint64_t eof,
                       const int64_t *counts, int device, hipStream_t user_stream, fmx_index **out,
                       const BlockSpec *block = nullptr) {
  if (!out) return arg_fail("out is null");
  *out = nullptr;
  if (!src && !src_file && n) return arg_fail("bwt is null");
  if (n < 1 || eof >= n) return arg_fail("need n >= 1 and eof < n");
  if (n >= (1ull << 38)) { g_err = "n >= 2^38 is not supported"; return FMX_ERR_UNSUPPORTED; }
  int rc = use_device_index(device);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  Index *h = new (std::nothrow) Index();
  if (!h) { g_err = "out of host memory"; return FMX_ERR_NOMEM; }
  h->serial = ++g_serial;
  h->policy = default_policy();        // this handle's own copy from here on
  if (block) {
    h->block_mode = true;
    std::memcpy(h->block_bs, block->bs, sizeof h->block_bs);
    h->block_first = block->first;
    h->block_skipped = block->skipped;
  }
  h->device = device;
  h->n = n;
  h->eof = eof;
  h->nblocks = n / kBlockBits + 1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->cu_count = prop.multiProcessorCount;
  StreamGuard own;
  hipStream_t st = user_stream;
  do {
    if (!st) {
      if ((e = hipStreamCreate(&own.s)) != hipSuccess) { rc = hip_fail(e, "hipStreamCreate"); break; }
      st = own.s;
    }
    // device copy of the BWT: zero-padded to whole 128-position blocks, slot eof set to 0 (BWT' has the
    // EOF symbol there; the stored byte is a filler, bwtmerger.scala:799-806)
    const uint64_t padded = (n / kByteBlock + 2) * kByteBlock;
    if ((e = hipMalloc(&h->d_bwt, padded)) != hipSuccess) { rc = hip_fail(e, "hipMalloc(bwt)"); break; }
    if ((e = hipMemsetAsync((uint8_t *)h->d_bwt + n, 0, padded - n, st)) != hipSuccess) { rc = hip_fail(e, "memset"); break; }
    if (src_file) {
      if ((rc = stream_file_to_device(src_file, h->d_bwt, n, st)) != FMX_OK) break;
    } else {
      e = hipMemcpyAsync(h->d_bwt, src, n, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
      if (e != hipSuccess) { rc = hip_fail(e, "copy bwt"); break; }
    }
    if ((e = hipMemsetAsync((uint8_t *)h->d_bwt + eof, 0, 1, st)) != hipSuccess) { rc = hip_fail(e, "memset"); break; }
    const int pref = layout_preference();
    h->layout = pref == (int)kLayoutBytes ? kLayoutBytes : kLayoutOneHot;
    if (n >= kOneHotMaxN) {              // the one-hot block split is exact below 2^37 only
      if (pref == (int)kLayoutOneHot) { g_err = "layout onehot needs n < 2^37"; rc = FMX_ERR_UNSUPPORTED; break; }
      h->layout = kLayoutBytes;
    }
    rc = build_index(h, st, counts);
    if (rc == -1) {                      // one-hot vectors do not fit: fall back unless one-hot was forced
      if (pref == (int)kLayoutOneHot) { rc = FMX_ERR_NOMEM; break; }
      h->layout = kLayoutBytes;
      rc = build_index(h, st, counts);
    }
  } while (0);
  if (rc != FMX_OK) { destroy(h); return rc; }
  *out = reinterpret_cast<fmx_index *>(h);
  return FMX_OK;
}

// Operands in, kernel, results out.  Where the kernel finds its operands and leaves its results depends on how much travels:
//   tiny (the single-query forms a per-call adapter makes: getPrevRange / occ / search): in the page-locked staging buffer
//     itself -- the kernel reads its few operand bytes over the link and writes its results there (the buffer is mapped into
//     the device's address space like every hipHostMalloc allocation).  No copies, and no events around the kernel either
//     (19.7 against 24.4 against 33.1 us per fmx_occ_batch of one query): fmx_stats_t.last_kernel_ms is not updated by such a call;
//   small: all operands packed into the staging buffer travel as ONE copy each way;
//   large: every array is copied between the caller's memory and its own device buffer.
struct HostIn { const void *src; size_t bytes; };
struct HostOut { void *dst; size_t bytes; };      // dst == nullptr: device scratch of that size, nothing comes back
constexpr size_t kSmallCall = 256u << 10;
constexpr size_t kTinyCall = 2048;

template <class Launch>
static int run_io(const Index *h, const HostIn *ins, int nin, const HostOut *outs, int nout, Launch launch) {
  Call call(h);
  int rc = call.init();
  if (rc != FMX_OK) return rc;
  auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  size_t in_total = 0, out_total = 0;
  for (int j = 0; j < nin; j++) in_total += up16(ins[j].bytes);
  for (int j = 0; j < nout; j++) out_total += up16(outs[j].bytes);
  const bool staged = in_total + out_total <= kSmallCall, tiny = in_total + out_total <= kTinyCall;
  const void *din[CallCtx::kBufs] = {nullptr};
  void *dout[CallCtx::kBufs] = {nullptr};
  uint8_t *hin = nullptr, *hout = nullptr;          // staging: the operands, and the results behind them
  void *a = nullptr, *b = nullptr;                  // their device images
  if (staged) {
    void *pin = nullptr;
    HIP_TRY(call.pinned(&pin, kSmallCall), "hipHostMalloc");
    HIP_TRY(call.alloc(&a, kSmallCall), "hipMalloc");
    HIP_TRY(call.alloc(&b, kSmallCall), "hipMalloc");
    hin = static_cast<uint8_t *>(pin);
    hout = hin + in_total;
    uint8_t *ibase = tiny ? hin : static_cast<uint8_t *>(a), *obase = tiny ? hout : static_cast<uint8_t *>(b);
    size_t o = 0;
    for (int j = 0; j < nin; j++) {
      if (ins[j].bytes) std::memcpy(hin + o, ins[j].src, ins[j].bytes);
      din[j] = ibase + o;
      o += up16(ins[j].bytes);
    }
    o = 0;
    for (int j = 0; j < nout; j++) { dout[j] = obase + o; o += up16(outs[j].bytes); }
  } else {
    for (int j = 0; j < nin; j++) { void *p = nullptr; HIP_TRY(call.alloc(&p, ins[j].bytes), "hipMalloc"); din[j] = p; }
    for (int j = 0; j < nout; j++) HIP_TRY(call.alloc(&dout[j], outs[j].bytes), "hipMalloc");
  }
  rc = call.timed([&](hipStream_t st, hipEvent_t ev_a, hipEvent_t ev_b) {
    if (!staged) {
      for (int j = 0; j < nin; j++)
        if (ins[j].bytes) HIP_TRY(hipMemcpyAsync(const_cast<void *>(din[j]), ins[j].src, ins[j].bytes, hipMemcpyHostToDevice, st), "H2D");
    } else if (!tiny && in_total) {
      HIP_TRY(hipMemcpyAsync(a, hin, in_total, hipMemcpyHostToDevice, st), "H2D");
    }
    if (ev_a) HIP_TRY(hipEventRecord(ev_a, st), "hipEventRecord");
    HIP_TRY(launch(st, din, dout), "kernel launch");
    if (ev_b) HIP_TRY(hipEventRecord(ev_b, st), "hipEventRecord");
    if (!staged) {
      for (int j = 0; j < nout; j++)
        if (outs[j].bytes && outs[j].dst) HIP_TRY(hipMemcpyAsync(outs[j].dst, dout[j], outs[j].bytes, hipMemcpyDeviceToHost, st), "D2H");
    } else if (!tiny && out_total) {
      HIP_TRY(hipMemcpyAsync(hout, b, out_total, hipMemcpyDeviceToHost, st), "D2H");
    }
    return (int)FMX_OK;
  }, !tiny);
  if (rc != FMX_OK || !staged) return rc;
  size_t o = 0;
  for (int j = 0; j < nout; j++) {
    if (outs[j].bytes && outs[j].dst) std::memcpy(outs[j].dst, hout + o, outs[j].bytes);
    o += up16(outs[j].bytes);
  }
  return FMX_OK;
}

bool offsets_monotonic(const uint64_t *off, size_t a, size_t b) {
  unsigned bad = 0;
  for (size_t q = a; q < b; q++) bad |= off[q + 1] < off[q];
  return bad == 0;
}

// ---- the host-pointer calls of the metered features (fmx_host.h, HostCall)
int HostCall::upload(const char *pat_what, const void *pat, uint64_t bytes, const char *off_what, const uint64_t *off, size_t k,
                     bool rebase, void **d_pat, uint64_t **d_off) {
  const uint64_t off_bytes = 8 * ((uint64_t)k + 1);
  int rc;
  if ((rc = mem.take(d_pat, bytes, pat_what)) || (rc = mem.take((void **)d_off, off_bytes, off_what))) return rc;
  if (rebase && !k) return FMX_OK;
  std::vector<uint64_t> rebased;                           // only the bytes in use travel
  if (rebase) {
    rebased.resize(k + 1);
    for (size_t q = 0; q <= k; q++) rebased[q] = off[q] - off[0];
    off = rebased.data();
  }
  if (k) HIP_TRY(hipMemcpyAsync(*d_off, off, off_bytes, hipMemcpyHostToDevice, own.s), "H2D(offsets)");
  else HIP_TRY(hipMemsetAsync(*d_off, 0, 8, own.s), "memset");
  if (bytes) HIP_TRY(hipMemcpyAsync(*d_pat, pat, bytes, hipMemcpyHostToDevice, own.s), "H2D(patterns)");
  return sync();
}

int csr_overflow(const char *prefix, uint64_t total, size_t cap) {
  g_err = std::string(prefix) + ": " + std::to_string(total) + " hits, room for " + std::to_string(cap);
  return FMX_ERR_OVERFLOW;
}

}  // namespace fmx

using namespace fmx;

extern "C" {

const char *fmx_last_error(void) { return g_err.c_str(); }
int fmx_abi_version(void) { return FMX_ABI_VERSION; }

int fmx_config_set(const char *key, const char *value) {
  if (!key || !value) return arg_fail("null argument");
  if (std::strcmp(key, "layout") == 0) {
    if (std::strcmp(value, "auto") == 0) g_layout_pref.store(-1);
    else if (std::strcmp(value, "onehot") == 0) g_layout_pref.store((int)kLayoutOneHot);
    else if (std::strcmp(value, "bytes") == 0) g_layout_pref.store((int)kLayoutBytes);
    else return arg_fail("layout must be auto, onehot or bytes");
    return FMX_OK;
  }
  if (std::strcmp(key, "validate") == 0) {
    g_validate.store(std::strcmp(value, "0") != 0);
    return FMX_OK;
  }
  if (std::strcmp(key, "checkpoints") == 0) {
    if (std::strcmp(value, "auto") == 0) g_force_superblocks.store(0);
    else if (std::strcmp(value, "superblock") == 0) g_force_superblocks.store(1);
    else return arg_fail("checkpoints must be auto or superblock");
    return FMX_OK;
  }
  if (std::strcmp(key, "pipeline") == 0) {
    if (std::strcmp(value, "on") == 0) g_pipeline.store(1, std::memory_order_relaxed);
    else if (std::strcmp(value, "off") == 0) g_pipeline.store(0, std::memory_order_relaxed);
    else return arg_fail("pipeline must be on or off");
    return FMX_OK;
  }
  if (std::strcmp(key, "threads") == 0) {
    char *end = nullptr;
    const long v = std::strtol(value, &end, 10);
    if (end == value || *end || v < 0) return arg_fail("threads must be a non-negative integer");
    set_host_threads((unsigned)v);
    return FMX_OK;
  }
  {
    const char *lq_why = nullptr;
    const int lr = lq_config(key, value, &lq_why);
    if (lr == 0) return FMX_OK;
    if (lr == 2) return arg_fail(lq_why);
  }
  // the table policy's keys: the defaults a handle copies when it is opened (fmx_index_config_set: one handle's own)
  const char *why = nullptr;
  const int pr = policy_set(default_policy(), key, value, &why);
  if (pr == 0) return FMX_OK;
  if (pr == 2) return arg_fail(why);
  return arg_fail("unknown configuration key");
}

int fmx_index_config_set(fmx_index *idx, const char *key, const char *value) {
  if (!idx || !key || !value) return arg_fail("null argument");
  const char *why = nullptr;
  const int pr = policy_set(H(idx)->policy, key, value, &why);
  if (pr == 0) return FMX_OK;
  if (pr == 2) return arg_fail(why);
  return arg_fail("not a per-handle key (ktab, jump, jump_pairs, search_lanes, jump_chars, tables_after, table_budget, locate_sample, extract_sample, lines_shift)");
}

int fmx_host_alloc(size_t bytes, void **out) {
  if (!out) return arg_fail("out is null");
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault), "hipHostMalloc");
  return FMX_OK;
}
int fmx_host_free(void *p) {
  if (p) HIP_TRY(hipHostFree(p), "hipHostFree");
  return FMX_OK;
}

int fmx_device_count(int *count) {
  if (!count) return arg_fail("count is null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return FMX_OK;
}

// The X.fm sibling of X.bwt (BWTTempStorage.genFMFilename, bwtmerger.scala:33-36: the extension swapped).  The reference
// cannot open an index without it -- NaiveFMSearcher takes n = fm.size (bwtmerger.scala:339) and FMLoader throws on a bad
// header (:259-262): element size 4, size * 4 + 9 == file length.  This engine derives its rank dictionary from the .bwt
// and never reads the lists, so a MISSING .fm is fine; a .fm that is there is held to the reference's checks, and to
// describing the same n rows as the .bwt -- an index whose files do not belong together fails here as it does there.
static int check_fm_sibling(const char *bwt_path, bool be, uint64_t n) {
  std::string p(bwt_path);
  const size_t slash = p.find_last_of("/\\"), dot = p.find_last_of('.');
  if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) p.erase(dot);
  p += ".fm";
  FILE *f = std::fopen(p.c_str(), "rb");
  if (!f) return FMX_OK;
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
  uint8_t hdr[9];
  if (std::fread(hdr, 1, 9, f) != 9) { g_err = "File " + p + " bad size"; return FMX_ERR_FORMAT; }
  const unsigned el = hdr[0];
  const uint64_t size = rd_u64(hdr + 1, be);
  if (el != 4) { g_err = "File " + p + " bad elSize " + std::to_string(el); return FMX_ERR_FORMAT; }
  if (fseeko(f, 0, SEEK_END) != 0) { g_err = "seek failed"; return FMX_ERR_IO; }
  const uint64_t flen = (uint64_t)ftello(f);
  if (size > (1ull << 40) || size * 4 + 9 != flen) {
    g_err = "File " + p + " bad size " + std::to_string(size) + " + 0x9 != " + std::to_string(flen) + "(filelen)";
    return FMX_ERR_FORMAT;
  }
  if (size != n) {
    g_err = "File " + p + " holds " + std::to_string(size) + " rows, " + bwt_path + " " + std::to_string(n) + ": not one index";
    return FMX_ERR_FORMAT;
  }
  return FMX_OK;
}

int fmx_open(const char *bwt_path, const char *aux_path, int big_endian, int device, fmx_index **out) {
  if (!bwt_path || !aux_path) return arg_fail("path is null");
  uint64_t n = 0, eof = 0;
  int64_t counts[256];
  FILE *f = nullptr;
  int rc = open_bwt_file(bwt_path, big_endian != 0, &f, n, eof);
  if (rc != FMX_OK) return rc;
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
  rc = load_aux(aux_path, big_endian != 0, counts);
  if (rc != FMX_OK) return rc;
  rc = check_fm_sibling(bwt_path, big_endian != 0, n);
  if (rc != FMX_OK) return rc;
  return open_common(nullptr, false, f, n, eof, counts, device, nullptr, out);
}

int fmx_open_mem(const uint8_t *bwt, uint64_t n, uint64_t eof, const int64_t counts[256], int device,
                 fmx_index **out) {
  if (!counts) return arg_fail("counts is null");
  return open_common(bwt, false, nullptr, n, eof, counts, device, nullptr, out);
}

int fmx_open_dev(const void *d_bwt, uint64_t n, uint64_t eof, const int64_t *counts_or_null, int device, void *stream,
                 fmx_index **out) {
  return open_common(d_bwt, true, nullptr, n, eof, counts_or_null, device, (hipStream_t)stream, out);
}

// NaiveBWTSearcher(bwt, bucketStarts, rk0), findex.scala:459-506: the searcher BWTMerger2.calcGaps uses over one
// block's BWT.  The skipped row plays the part of the EOF slot; everything else that differs from NaiveFMSearcher
// is settled when the dictionary is built (build_index, block mode).
int fmx_open_block(const uint8_t *bwt, uint64_t n, const int64_t bucket_starts[256], uint64_t rk0, int device,
                   fmx_index **out) {
  if (!bwt || !bucket_starts) return arg_fail("null argument");
  if (n < 1 || rk0 >= n) return arg_fail("need n >= 1 and rk0 < n");
  for (int c = 0; c < 256; c++)
    if (bucket_starts[c] < 0 || (uint64_t)bucket_starts[c] > n) return arg_fail("bucket start out of range");
  BlockSpec spec{bucket_starts, rk0 == 0 ? -1 : (int)bwt[0], (int)bwt[rk0]};
  return open_common(bwt, false, nullptr, n, rk0, nullptr, device, nullptr, out, &spec);
}

int fmx_prepare(const fmx_index *idx, unsigned what) {
  if (!idx) return arg_fail("null argument");
  if (what & ~(kDroppableTables | FMX_PREPARE_SELECT | FMX_PREPARE_SEARCH | derived_flags())) return arg_fail("unknown fmx_prepare flag");
  const Index *h = H(idx);
  int rc;
  for (const DerivedFlag &d : kDerived)
    if ((what & d.flag) && (rc = d.check(h))) return rc;
  if ((rc = use_device(h))) return rc;
  CtxLease lease(h);
  if (!lease.c) return FMX_ERR_HIP;
  if (what & FMX_PREPARE_KTAB) {
    h->prepared_ktab.store(true, std::memory_order_relaxed);      // (its own flag: the row tables stay under their threshold)
    KTab kt;
    HIP_TRY(ktab_get(h, lease.c->stream, &kt), "k-mer table");
  }
  if (what & FMX_PREPARE_SELECT) HIP_TRY(select_prepare(h, lease.c->stream), "select directory");
  if (what & FMX_PREPARE_JUMP) {
    h->prepared_rows.store(true, std::memory_order_relaxed);      // from now on searches use (and may build) the row tables
    JumpView jt;
    HIP_TRY(jump_get(h, lease.c->stream, &jt), "jump table");
    const unsigned long long *r3 = nullptr;
    HIP_TRY(row3_get(h, lease.c->stream, &r3), "three-step row table");      // beside the jump table, or instead of it
  }
  if (what & FMX_PREPARE_FRONTIER) {
    const unsigned long long *r1 = nullptr;
    HIP_TRY(row1_get(h, lease.c->stream, &r1), "row table");
  }
  for (const DerivedFlag &d : kDerived)
    if ((what & d.flag) && (rc = d.prepare(h, lease.c->stream))) return rc;
  // the literal search kernel this handle's tables select, calibrated here (its residency census: fmx_search.hip) so that no
  // _dev call ever has to read anything back
  if (what & (FMX_PREPARE_KTAB | FMX_PREPARE_JUMP | FMX_PREPARE_SEARCH)) HIP_TRY(search_calibrate(h, lease.c->stream), "search calibration");
  return FMX_OK;
}

int fmx_prepare_ex(fmx_index *idx, unsigned what, uint64_t budget_bytes) {
  if (!idx) return arg_fail("null argument");
  if (budget_bytes) {
    H(idx)->policy.budget_bytes.store(budget_bytes, std::memory_order_relaxed);
    H(idx)->policy.budget_ppb.store(0, std::memory_order_relaxed);
  }
  return fmx_prepare(idx, what);
}

int fmx_drop_tables(fmx_index *idx, unsigned what) {
  if (!idx) return arg_fail("null argument");
  if (!what || (what & ~(kDroppableTables | derived_flags()))) return arg_fail("fmx_drop_tables frees the k-mer table, the row tables, the locate samples, the LCP array, the extract samples and the line table (FMX_PREPARE_KTAB, FMX_PREPARE_JUMP, FMX_PREPARE_FRONTIER, FMX_PREPARE_LOCATE, FMX_PREPARE_LCP, FMX_PREPARE_EXTRACT, FMX_PREPARE_LINES)");
  Index *h = H(idx);
  int rc = use_device(h);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  return drop_derived(h, what);
}

int fmx_close(fmx_index *idx) {
  if (!idx) return FMX_OK;            // closing nothing is not an error (a wrapper whose handle was already taken: hipfm.scala)
  destroy(H(idx));
  return FMX_OK;
}

int fmx_n(const fmx_index *idx, uint64_t *n) {
  if (!idx || !n) return arg_fail("null argument");
  *n = H(idx)->n;
  return FMX_OK;
}
int fmx_eof(const fmx_index *idx, uint64_t *eof) {
  if (!idx || !eof) return arg_fail("null argument");
  *eof = H(idx)->eof;
  return FMX_OK;
}
int fmx_cf(const fmx_index *idx, int c, uint64_t *out) {
  if (!idx || !out) return arg_fail("null argument");
  if (c < 0 || c > 255) return arg_fail("symbol out of range (reference: ArrayIndexOutOfBounds)");
  *out = H(idx)->cf[c];
  return FMX_OK;
}
int fmx_counts(const fmx_index *idx, int64_t out[256]) {
  if (!idx || !out) return arg_fail("null argument");
  std::memcpy(out, H(idx)->counts, sizeof H(idx)->counts);
  return FMX_OK;
}
int fmx_device(const fmx_index *idx, int *device) {
  if (!idx || !device) return arg_fail("null argument");
  *device = H(idx)->device;
  return FMX_OK;
}

// ---------------------------------------------------------------- device-pointer entry points
int fmx_occ_batch_dev(const fmx_index *idx, const void *d_c, const void *d_i, void *d_out, size_t k, void *stream) {
  if (!idx || (k && (!d_c || !d_i || !d_out))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  HIP_TRY(launch_occ(H(idx), d_c, d_i, d_out, k, (hipStream_t)stream), "k_occ");
  return FMX_OK;
}

int fmx_search_batch_ex_dev(const fmx_index *idx, const void *d_pat, const void *d_off, void *d_sp, void *d_ep, size_t k,
                            const fmx_search_opts *opts, void *stream) {
  const uint32_t fixed = opts ? opts->fixed_len : 0u;
  if (!idx || (k && ((!d_off && !fixed) || !d_sp || !d_ep))) return arg_fail("null argument");
  if (k && fixed && !d_pat) return arg_fail("pat is null");
  int rc = use_device(H(idx));
  if (rc) return rc;
  if (k && !fixed && validate_device_operands()) {
    bool ok = true;
    HIP_TRY(check_offsets(H(idx), d_off, k, (hipStream_t)stream, &ok), "k_check_offsets");
    if (!ok) return arg_fail("pattern offsets must be non-decreasing");
  }
  // packed: by the search kernel itself where it finishes every pattern, else in place behind it (d_sp's first k words)
  if (opts && (opts->packed & ~(FMX_SEARCH_PACKED | FMX_SEARCH_MISS_NONE))) return arg_fail("fmx_search_opts.packed: unknown bits");
  HIP_TRY(launch_search(H(idx), d_pat, fixed ? nullptr : d_off, d_sp, d_ep, k, (hipStream_t)stream, fixed,
                        (opts && (opts->packed & FMX_SEARCH_PACKED)) ? (uint64_t)opts->escape_cap : ~0ull,
                        (opts && (opts->packed & FMX_SEARCH_MISS_NONE)) ? kSearchMissNone : 0u), "k_search");
  return FMX_OK;
}

int fmx_search_batch_dev(const fmx_index *idx, const void *d_pat, const void *d_off, void *d_sp, void *d_ep, size_t k,
                         void *stream) {
  return fmx_search_batch_ex_dev(idx, d_pat, d_off, d_sp, d_ep, k, nullptr, stream);
}

size_t fmx_packed_words(size_t k, size_t escape_cap) { return k + 1 + 2 * escape_cap; }

int fmx_pack_intervals_dev(const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, size_t escape_cap, void *d_packed,
                           void *stream) {
  if (!idx || !d_packed || (k && (!d_sp || !d_ep))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  HIP_TRY(launch_pack_intervals(H(idx), d_sp, d_ep, k, escape_cap, d_packed, (hipStream_t)stream), "k_pack_intervals");
  return FMX_OK;
}

int fmx_unpack_intervals_dev(const fmx_index *idx, const void *d_packed, size_t k, size_t escape_cap, void *d_sp, void *d_ep,
                             void *stream) {
  if (!idx || !d_packed || (k && (!d_sp || !d_ep))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  HIP_TRY(launch_unpack_intervals(H(idx), d_packed, k, escape_cap, d_sp, d_ep, (hipStream_t)stream), "k_unpack_intervals");
  return FMX_OK;
}

// Host-side decode of the 8-byte form (format arithmetic on the caller's own result buffer: no search happens here).
int fmx_unpack_intervals(const uint64_t *packed, size_t k, size_t escape_cap, uint64_t *sp, uint64_t *ep) {
  if (!packed || (k && (!sp || !ep))) return arg_fail("null argument");
  for (size_t q = 0; q < k; q++) {
    const uint64_t a = packed[q] & ((1ull << 40) - 1);
    sp[q] = a;
    ep[q] = a + (packed[q] >> 40);
  }
  const uint64_t cnt = packed[k];
  for (uint64_t j = 0; j < cnt && j < escape_cap; j++) {
    const uint64_t q = packed[k + 1 + 2 * j];
    if (q >= k) { g_err = "packed intervals: escape entry names pattern " + std::to_string(q) + " of " + std::to_string(k); return FMX_ERR_FORMAT; }
    ep[q] = packed[k + 2 + 2 * j];
  }
  if (cnt > escape_cap) {
    g_err = std::to_string(cnt) + " intervals of 2^24 - 1 rows or more, the escape list holds " + std::to_string(escape_cap);
    return FMX_ERR_OVERFLOW;
  }
  return FMX_OK;
}

int fmx_prev_range_batch_dev(const fmx_index *idx, const void *d_sp, const void *d_ep, const void *d_c, void *d_sp1,
                             void *d_ep1, size_t k, void *stream) {
  if (!idx || (k && (!d_sp || !d_ep || !d_c || !d_sp1 || !d_ep1))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  HIP_TRY(launch_prev_range(H(idx), d_sp, d_ep, d_c, d_sp1, d_ep1, k, (hipStream_t)stream), "k_prev_range");
  return FMX_OK;
}

int fmx_lf_walk_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, uint32_t len, void *d_out_bytes,
                          void *d_end_rows, void *stream) {
  if (!idx || (k && !d_rows)) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  HIP_TRY(launch_lf_walk(H(idx), d_rows, k, len, d_out_bytes, d_end_rows, (hipStream_t)stream), "k_lf_walk");
  return FMX_OK;
}

// A Psi launch that found the select directory missing on a capturing stream has recorded its own message
// (ensure_select, fmx_select.hip): keep it.
static int select_status(hipError_t e, const char *what) {
  if (e == hipSuccess) return FMX_OK;
  return e == hipErrorStreamCaptureUnsupported ? FMX_ERR_HIP : hip_fail(e, what);
}

int fmx_psi_batch_dev(const fmx_index *idx, const void *d_rows, void *d_out, size_t k, void *stream) {
  if (!idx || (k && (!d_rows || !d_out))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  return select_status(launch_psi(H(idx), d_rows, d_out, k, (hipStream_t)stream), "k_psi");
}

int fmx_next_substr_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, uint32_t len, void *d_out,
                              void *d_out_len, void *stream) {
  if (!idx || (k && (!d_rows || !d_out_len || (len && !d_out)))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  return select_status(launch_next_substr(H(idx), d_rows, k, len, d_out, d_out_len, (hipStream_t)stream), "k_next_substr");
}

// ---------------------------------------------------------------- host-pointer entry points
int fmx_occ_batch(const fmx_index *idx, const uint8_t *c, const int64_t *i, uint64_t *out, size_t k) {
  if (!idx || (k && (!c || !i || !out))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = use_device(h);
  if (rc || !k) return rc;
  const HostIn ins[] = {{c, k}, {i, k * 8}};
  const HostOut outs[] = {{out, k * 8}};
  return run_io(h, ins, 2, outs, 1, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_occ(h, di[0], di[1], dout[0], k, st);
  });
}

// ---- fmx_search_batch_ex: the checks, the batch they describe, and the three ways it travels
constexpr size_t kPipelineMin = 128u << 10;       // patterns: smaller batches go through run_io

struct HostBatch {
  const uint8_t *pat = nullptr;           // the `total` pattern bytes in use (null: none)
  const uint64_t *off = nullptr;          // k + 1 offsets into pat, the first 0 (null: k patterns of fixed_len bytes each)
  std::vector<uint64_t> rebased;          // ... their storage where the caller's do not begin at 0
  uint64_t total = 0, pack_cap = ~0ull;   // pack_cap != ~0: the 8-byte form into sp alone, an escape list of that many entries
  size_t k = 0, out_words = 0;            // k == 0: nothing to search; out_words: u64 words of sp (k, or fmx_packed_words)
  uint32_t fixed_len = 0, flags = 0;      // flags: kSearchMissNone
  uint64_t *sp = nullptr, *ep = nullptr;
  bool packed() const { return pack_cap != ~0ull; }
  hipError_t launch(const Index *h, const void *d_pat, const void *d_off, void *d_sp, void *d_ep, hipStream_t st) const {
    return launch_search(h, d_pat, off ? d_off : nullptr, d_sp, d_ep, k, st, fixed_len, pack_cap, flags);
  }
};

// (i) Whatever refuses a batch before a byte travels, in the order the failures are reported, and the batch as the paths
// below take it (b->k == 0: an empty one, answered here).  The lean forms (round 4): equal-length patterns travel without
// offsets (8 B per pattern less up the link) and the intervals come back in the 8-byte form (8 B per pattern less down):
// 56 -> 40 B per 32-character pattern.
// Offsets must be non-decreasing (a kernel would read a "negative" pattern as 2^64 bytes).  Walking a million of them on
// the host takes 0.37 ms -- a quarter of a large call -- so large batches are checked where it is free: by a kernel on the
// uploaded copy (search_whole_arrays), or chunk by chunk on the host while the uploads run (search_pipelined).
static int search_batch_checks(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, uint64_t *sp, uint64_t *ep, size_t k,
                               const fmx_search_opts *opts, HostBatch *b) {
  if (opts && (opts->packed & ~(FMX_SEARCH_PACKED | FMX_SEARCH_MISS_NONE))) return arg_fail("fmx_search_opts.packed: unknown bits");
  const uint32_t fixed = b->fixed_len = opts ? opts->fixed_len : 0u;
  const bool packed = opts && (opts->packed & FMX_SEARCH_PACKED);
  if (!idx || (k && ((!off && !fixed) || !sp || (!ep && !packed)))) return arg_fail("null argument");
  int rc = use_device(H(idx));
  if (rc) return rc;
  if (!k) { if (packed && sp) sp[0] = 0; return FMX_OK; }
  uint64_t lo = 0;
  b->total = (uint64_t)fixed * k;
  if (!fixed) {
    if ((k < kPipelineMin && !offsets_monotonic(off, 0, k)) || off[k] < off[0]) return arg_fail("pattern offsets must be non-decreasing");
    lo = off[0];
    b->total = off[k] - lo;
    b->off = off;
  }
  if (b->total && !pat) return arg_fail("pat is null");
  if (lo) {                             // offsets are rebased so that only the bytes in use travel
    b->rebased.resize(k + 1);
    for (size_t q = 0; q <= k; q++) b->rebased[q] = off[q] - lo;
    b->off = b->rebased.data();
  }
  b->pat = b->total ? pat + lo : nullptr;
  b->k = k;
  b->flags = (opts && (opts->packed & FMX_SEARCH_MISS_NONE)) ? kSearchMissNone : 0u;
  if (packed) b->pack_cap = opts->escape_cap;
  b->out_words = packed ? fmx_packed_words(k, (size_t)opts->escape_cap) : k;
  b->sp = sp;
  b->ep = ep;
  return FMX_OK;
}

// (iii) Large batches: whole arrays up with one synchronous copy each, one chain of kernels, whole arrays down (1.30 ms for
// 1M x 32 bytes here, from pageable and page-locked memory alike: the copies run at the link's 53 GB/s).  "Asynchronous"
// copies of pageable caller memory are staged piecewise by the runtime and block the calling thread (measured: 8 chunks,
// 0.37 ms each, nothing overlapped).
static int search_whole_arrays(const Index *h, const HostBatch &b, Call &c0, void *d_pat, void *d_off, void *d_sp, void *d_ep) {
  if (b.total) HIP_TRY(hipMemcpy(d_pat, b.pat, (size_t)b.total, hipMemcpyHostToDevice), "H2D(patterns)");
  if (b.off) {
    HIP_TRY(hipMemcpy(d_off, b.off, (b.k + 1) * 8, hipMemcpyHostToDevice), "H2D(offsets)");
    bool ok = true;
    HIP_TRY(check_offsets(h, d_off, b.k, c0.stream(), &ok), "k_check_offsets");
    if (!ok) return arg_fail("pattern offsets must be non-decreasing");
  }
  const int rc = c0.timed_launch([&](hipStream_t st) { return b.launch(h, d_pat, d_off, d_sp, d_ep, st); }, "k_search");
  if (rc != FMX_OK) return rc;
  HIP_TRY(hipMemcpy(b.sp, d_sp, b.out_words * 8, hipMemcpyDeviceToHost), b.packed() ? "D2H(packed)" : "D2H(sp)");
  if (!b.packed()) HIP_TRY(hipMemcpy(b.ep, d_ep, b.k * 8, hipMemcpyDeviceToHost), "D2H(ep)");
  return FMX_OK;
}

// Page-locked at both ends: a partly registered buffer must not take the asynchronous path.
static bool host_pinned(const void *p, size_t bytes) {
  auto pinned1 = [](const void *q) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
  };
  return pinned1(p) && (bytes == 0 || pinned1(static_cast<const uint8_t *>(p) + bytes - 1));
}

// (iv) With fmx_config_set("pipeline", "on") large batches of the default form in page-locked caller memory (fmx_host_alloc,
// or the caller's own hipHostMalloc / registered pages) are pipelined instead: the batch is cut into chunks of patterns,
// chunk j's bytes and offsets go up on one stream, are searched on a second and come back on a third, so the copies of one
// chunk run beside the kernels of another and both directions of the link are busy.  Offsets stay absolute: every chunk is
// copied to its own place of one device image of the batch.  Off by default: on this platform asynchronous copies are
// slower than synchronous ones (one chunk, no overlap at all: 1.67 ms) and the overlap does not reliably win that back --
// 1.08 to 1.7 ms with 4 chunks from box to box.
static int search_pipelined(const Index *h, const HostBatch &b, Call &c0, void *d_pat, void *d_off, void *d_sp, void *d_ep) {
  const size_t k = b.k;
  const uint64_t *offp = b.off, total = b.total;
  uint64_t *sp = b.sp, *ep = b.ep;
  Call c1(h), c2(h);
  int rc;
  if ((rc = c1.init()) != FMX_OK || (rc = c2.init()) != FMX_OK) return rc;
  static const size_t nchunk = [] { const char *e = getenv("FMX_PIPE_CHUNKS"); const int v = e ? atoi(e) : 4; return (size_t)(v < 1 ? 1 : (v > 64 ? 64 : v)); }();
  static const bool trace = getenv("FMX_TRACE") != nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  auto mark = [&](const char *what, size_t j) {
    if (trace) fprintf(stderr, "[fmx] search_batch %s %zu +%.3f ms\n", what, j,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  };
  // Three streams, one per engine: `up` carries the chunks' uploads in order, one event after each; `run` waits for
  // chunk j's event and searches it; `down` waits for that search and sends the chunk's intervals back.  So the link
  // is busy in both directions beside the kernels, and no stream alternates between kernels and copies (every such
  // change of engine inside one stream costs a hand-over of ~0.1 ms: with the copies behind each chunk's kernels on
  // `run`, eight chunks took 2.4 ms where the kernels are 0.23 ms and the copies 0.75 ms).
  hipStream_t up = c1.stream(), run = c0.stream(), down = c2.stream();
  // Whatever ends this call early -- a failed enqueue, a bad offset -- the streams are drained first: copies still in
  // flight read and write the CALLER's buffers, and the device buffers go back to the handle's pool on return.
  struct Drain {
    hipStream_t a, b, c;
    bool armed = true;
    ~Drain() { if (armed) { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(c); } }
  } drain{up, run, down};
  for (size_t j = 0; j <= nchunk; j++)            // the chunks' byte ranges come from these: checked before any copy
    if (offp[k * j / nchunk] > total || (j && offp[k * j / nchunk] < offp[k * (j - 1) / nchunk]))
      return arg_fail("pattern offsets must be non-decreasing");
  hipEvent_t *cev = nullptr, *kev = nullptr;
  HIP_TRY(c0.chunk_events(nchunk, &cev), "hipEventCreate");
  HIP_TRY(c2.chunk_events(nchunk, &kev), "hipEventCreate");
  HIP_TRY(hipEventRecord(c0.ev_a(), run), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(up, c0.ev_a(), 0), "hipStreamWaitEvent");      // the buffers' previous users are done
  for (size_t j = 0; j < nchunk; j++) {
    const size_t a = k * j / nchunk, e = k * (j + 1) / nchunk;
    const uint64_t b0 = offp[a], b1 = offp[e];
    if (b1 > b0)
      HIP_TRY(hipMemcpyAsync((uint8_t *)d_pat + b0, b.pat + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, up), "H2D(patterns)");
    // chunk j needs offsets a .. e: entry e is also the next chunk's first, copied by both (same value)
    HIP_TRY(hipMemcpyAsync((uint64_t *)d_off + a, offp + a, (e - a + 1) * 8, hipMemcpyHostToDevice, up), "H2D(offsets)");
    HIP_TRY(hipEventRecord(cev[j], up), "hipEventRecord");
  }
  mark("uploads enqueued", nchunk);
  for (size_t j = 0; j < nchunk; j++) {
    const size_t a = k * j / nchunk, e = k * (j + 1) / nchunk;
    HIP_TRY(hipStreamWaitEvent(run, cev[j], 0), "hipStreamWaitEvent");
    if (a == e) continue;
    if (!offsets_monotonic(offp, a, e)) return arg_fail("pattern offsets must be non-decreasing");      // while the uploads are under way
    HIP_TRY(launch_search(h, d_pat, (const uint64_t *)d_off + a, (uint64_t *)d_sp + a, (uint64_t *)d_ep + a, e - a, run),
            "k_search");
    HIP_TRY(hipEventRecord(kev[j], run), "hipEventRecord");
    HIP_TRY(hipStreamWaitEvent(down, kev[j], 0), "hipStreamWaitEvent");
    HIP_TRY(hipMemcpyAsync(sp + a, (uint64_t *)d_sp + a, (e - a) * 8, hipMemcpyDeviceToHost, down), "D2H(sp)");
    HIP_TRY(hipMemcpyAsync(ep + a, (uint64_t *)d_ep + a, (e - a) * 8, hipMemcpyDeviceToHost, down), "D2H(ep)");
    mark("chunk enqueued", j);
  }
  HIP_TRY(hipEventRecord(c2.ev_a(), down), "hipEventRecord");
  HIP_TRY(hipStreamWaitEvent(run, c2.ev_a(), 0), "hipStreamWaitEvent");     // `run` ends when the last download has
  HIP_TRY(hipEventRecord(c0.ev_b(), run), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(run), "hipStreamSynchronize");      // `run` waited for every upload and download: all three are idle
  drain.armed = false;
  mark("synchronized", 0);
  float ms = 0;
  if (hipEventElapsedTime(&ms, c0.ev_a(), c0.ev_b()) == hipSuccess) {
    std::lock_guard<std::mutex> lk(h->mu);
    h->last_kernel_ms = ms;            // for a pipelined call: the whole device side, copies included
    h->launches += nchunk;
  }
  return FMX_OK;
}

int fmx_search_batch_ex(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, uint64_t *sp, uint64_t *ep,
                        size_t k, const fmx_search_opts *opts) {
  HostBatch b;
  int rc = search_batch_checks(idx, pat, off, sp, ep, k, opts, &b);
  if (rc != FMX_OK || !b.k) return rc;
  const Index *h = H(idx);
  if (k < kPipelineMin) {               // (ii) small batches: one copy each way
    const HostIn ins[] = {{b.pat, (size_t)b.total}, {b.off, b.off ? (k + 1) * 8 : 0}};
    const HostOut outs[] = {{sp, b.out_words * 8}, {b.packed() ? nullptr : ep, k * 8}};
    return run_io(h, ins, 2, outs, 2, [&](hipStream_t st, const void *const *di, void *const *dout) {
      return b.launch(h, di[0], di[1], dout[0], dout[1], st);
    });
  }
  Call c0(h);
  if ((rc = c0.init()) != FMX_OK) return rc;
  void *d_pat = nullptr, *d_off = nullptr, *d_sp = nullptr, *d_ep = nullptr;
  HIP_TRY(c0.alloc(&d_pat, (size_t)b.total + 16), "hipMalloc");
  HIP_TRY(c0.alloc(&d_off, b.off ? (k + 1) * 8 : 16), "hipMalloc");
  HIP_TRY(c0.alloc(&d_sp, b.out_words * 8), "hipMalloc");
  HIP_TRY(c0.alloc(&d_ep, k * 8), "hipMalloc");
  const bool lean = b.fixed_len || b.packed() || b.flags;
  if (!lean && g_pipeline.load(std::memory_order_relaxed) && host_pinned(sp, k * 8) && host_pinned(ep, k * 8) &&
      host_pinned(b.off, (k + 1) * 8) && (!b.total || host_pinned(b.pat, (size_t)b.total)))
    return search_pipelined(h, b, c0, d_pat, d_off, d_sp, d_ep);
  return search_whole_arrays(h, b, c0, d_pat, d_off, d_sp, d_ep);
}

int fmx_search_batch(const fmx_index *idx, const uint8_t *pat, const uint64_t *off, uint64_t *sp, uint64_t *ep,
                     size_t k) {
  return fmx_search_batch_ex(idx, pat, off, sp, ep, k, nullptr);
}

int fmx_search_batch_multi(fmx_index *const *idxs, size_t n_idx, const uint8_t *pat, const uint64_t *off,
                           uint64_t *sp, uint64_t *ep, size_t k) {
  if (!idxs || !n_idx || (k && (!off || !sp || !ep))) return arg_fail("null argument");
  for (size_t r = 0; r < n_idx; r++) {
    if (!idxs[r]) return arg_fail("null index handle");
    if (H(idxs[r])->n != H(idxs[0])->n || H(idxs[r])->eof != H(idxs[0])->eof) return arg_fail("the handles are not replicas of one index");
  }
  if (!k) return FMX_OK;
  for (size_t q = 0; q < k; q++)
    if (off[q + 1] < off[q]) return arg_fail("pattern offsets must be non-decreasing");
  // contiguous slices balanced by pattern bytes (by count when every pattern is empty)
  std::vector<size_t> cut(n_idx + 1, k);
  cut[0] = 0;
  const uint64_t total = off[k] - off[0];
  for (size_t r = 1; r < n_idx; r++) {
    if (!total) { cut[r] = k * r / n_idx; continue; }
    const uint64_t want = off[0] + total / n_idx * r;
    cut[r] = (size_t)(std::lower_bound(off, off + k + 1, want) - off);
    if (cut[r] < cut[r - 1]) cut[r] = cut[r - 1];
    if (cut[r] > k) cut[r] = k;
  }
  // slice r runs on handle r's own host thread (kept with the handle: a call wakes it, it does not create it)
  std::vector<int> rc(n_idx, FMX_OK);
  std::vector<std::string> msg(n_idx);
  std::vector<Worker *> busy;
  for (size_t r = 0; r < n_idx; r++) {
    const size_t a = cut[r], b = cut[r + 1];
    if (a == b) continue;
    Worker *w = worker_of(H(idxs[r]));
    w->submit([&, r, a, b]() {
      rc[r] = fmx_search_batch(idxs[r], pat, off + a, sp + a, ep + a, b - a);
      if (rc[r] != FMX_OK) msg[r] = fmx_last_error();        // the message is thread-local: carry it over
    });
    busy.push_back(w);
  }
  for (Worker *w : busy) w->wait();
  for (size_t r = 0; r < n_idx; r++)
    if (rc[r] != FMX_OK) { g_err = msg[r]; return rc[r]; }
  return FMX_OK;
}

int fmx_gather(fmx_index *const *idxs, size_t n_idx, const void *const *d_src, const size_t *cnt, size_t elem,
               void *dst) {
  if (!idxs || !n_idx || !d_src || !cnt || !elem || !dst) return arg_fail("null argument");
  std::vector<CallCtx *> ctx(n_idx, nullptr);
  size_t at = 0;
  int rc = FMX_OK;
  for (size_t r = 0; r < n_idx && rc == FMX_OK; r++) {
    if (!idxs[r]) { rc = arg_fail("null index handle"); break; }
    const Index *h = H(idxs[r]);
    if (cnt[r]) {
      if (!d_src[r]) { rc = arg_fail("null slice pointer"); break; }
      if ((rc = use_device(h)) != FMX_OK) break;
      ctx[r] = ctx_acquire(h);
      if (!ctx[r]) { rc = FMX_ERR_HIP; break; }
      const hipError_t e = hipMemcpyAsync(static_cast<uint8_t *>(dst) + at * elem, d_src[r], cnt[r] * elem,
                                          hipMemcpyDeviceToHost, ctx[r]->stream);
      if (e != hipSuccess) rc = hip_fail(e, "D2H(gather)");
    }
    at += cnt[r];
  }
  for (size_t r = 0; r < n_idx; r++) {
    if (!ctx[r]) continue;
    const Index *h = H(idxs[r]);
    (void)hipSetDevice(h->device);
    const hipError_t e = hipStreamSynchronize(ctx[r]->stream);
    if (e != hipSuccess && rc == FMX_OK) rc = hip_fail(e, "hipStreamSynchronize(gather)");
    ctx_release(h, ctx[r]);
  }
  return rc;
}

int fmx_prev_range_batch(const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, const uint8_t *c,
                         uint64_t *sp1, uint64_t *ep1, size_t k) {
  if (!idx || (k && (!sp || !ep || !c || !sp1 || !ep1))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = use_device(h);
  if (rc || !k) return rc;
  for (size_t q = 0; q < k; q++)
    if (sp[q] > ep[q] || ep[q] > h->n) return arg_fail("need sp <= ep <= n");
  const HostIn ins[] = {{sp, k * 8}, {ep, k * 8}, {c, k}};
  const HostOut outs[] = {{sp1, k * 8}, {ep1, k * 8}};
  return run_io(h, ins, 3, outs, 2, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_prev_range(h, di[0], di[1], di[2], dout[0], dout[1], k, st);
  });
}

// getIntervalPrevRange, findex.scala:37-51: one prev_range batch over the class, then the
// reference's filter (occ1 < occ2) and its prepend order (descending c).
int fmx_interval_prev_range(const fmx_index *idx, uint64_t sp, uint64_t ep, int cstart, int cend, uint64_t *out_sp,
                            uint64_t *out_ep, uint8_t *out_c, size_t *n_out) {
  if (!idx || !n_out) return arg_fail("null argument");
  *n_out = 0;
  if (cstart < 0 || cstart > 255 || (cstart <= cend && cend > 255))
    return arg_fail("symbol out of range (reference: ArrayIndexOutOfBounds)");
  if (cend < cstart) return FMX_OK;
  const size_t k = (size_t)(cend - cstart + 1);
  if (!out_sp || !out_ep) return arg_fail("null argument");
  std::vector<uint64_t> vsp(k, sp), vep(k, ep), sp1(k), ep1(k);
  std::vector<uint8_t> vc(k);
  for (size_t j = 0; j < k; j++) vc[j] = (uint8_t)(cstart + (int)j);
  int rc = fmx_prev_range_batch(idx, vsp.data(), vep.data(), vc.data(), sp1.data(), ep1.data(), k);
  if (rc) return rc;
  size_t w = 0;
  for (size_t j = k; j-- > 0;) {
    if (sp1[j] < ep1[j]) {
      out_sp[w] = sp1[j];
      out_ep[w] = ep1[j];
      if (out_c) out_c[w] = vc[j];
      w++;
    }
  }
  *n_out = w;
  return FMX_OK;
}

int fmx_lf_walk_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint32_t len, uint8_t *out_bytes,
                      uint64_t *end_rows) {
  if (!idx || (k && !rows)) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = use_device(h);
  if (rc || !k) return rc;
  for (size_t q = 0; q < k; q++)
    if (rows[q] >= h->n) return arg_fail("row out of range (reference: seek past .bwt / ArrayIndexOutOfBounds)");
  const HostIn ins[] = {{rows, k * 8}};
  const HostOut outs[] = {{out_bytes, out_bytes ? k * (size_t)len : 0}, {end_rows, end_rows ? k * 8 : 0}};
  return run_io(h, ins, 1, outs, 2, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_lf_walk(h, di[0], k, len, out_bytes ? dout[0] : nullptr, end_rows ? dout[1] : nullptr, st);
  });
}

int fmx_prev_substr(const fmx_index *idx, uint64_t sp, uint32_t len, uint8_t *out) {
  if (len && !out) return arg_fail("null argument");
  return fmx_lf_walk_batch(idx, &sp, 1, len, out, nullptr);
}

int fmx_psi_batch(const fmx_index *idx, const uint64_t *rows, uint64_t *out, size_t k) {
  if (!idx || (k && (!rows || !out))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = use_device(h);
  if (rc || !k) return rc;
  for (size_t q = 0; q < k; q++)
    if (rows[q] >= h->n) return arg_fail("row out of range");
  const HostIn ins[] = {{rows, k * 8}};
  const HostOut outs[] = {{out, k * 8}};
  return run_io(h, ins, 1, outs, 1, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_psi(h, di[0], dout[0], k, st);
  });
}

// nextSubstr for k rows in one call: out is k x len bytes (row q's string at q*len, out_len[q] bytes of it used).
int fmx_next_substr_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint32_t len, uint8_t *out,
                          uint32_t *out_len) {
  if (!idx || (k && (!rows || !out_len || (len && !out)))) return arg_fail("null argument");
  const Index *h = H(idx);
  for (size_t q = 0; q < k; q++) {
    out_len[q] = 0;
    if (rows[q] >= h->n) return arg_fail("row out of range");
  }
  int rc = use_device(h);
  if (rc || !k) return rc;
  const HostIn ins[] = {{rows, k * 8}};
  const HostOut outs[] = {{out, k * (size_t)len}, {out_len, k * 4}};
  rc = run_io(h, ins, 1, outs, 2, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_next_substr(h, di[0], k, len, dout[0], dout[1], st);
  });
  if (rc) return rc;
  for (size_t q = 0; q < k; q++)                  // the kernel writes in walk order: ret.reverse, bwtmerger.scala:404
    std::reverse(out + q * (size_t)len, out + q * (size_t)len + out_len[q]);
  return FMX_OK;
}

int fmx_next_substr(const fmx_index *idx, uint64_t sp, uint32_t len, uint8_t *out, uint32_t *out_len) {
  if (!out_len) return arg_fail("null argument");
  return fmx_next_substr_batch(idx, &sp, 1, len, out, out_len);
}

int fmx_extract(const fmx_index *idx, uint64_t row, uint32_t len, int direction, uint8_t *out, uint32_t *out_len) {
  if (!out_len) return arg_fail("null argument");
  if (direction == 0) return arg_fail("direction must be positive (nextSubstr) or negative (prevSubstr)");
  if (direction > 0) return fmx_next_substr(idx, row, len, out, out_len);
  *out_len = 0;
  int rc = fmx_prev_substr(idx, row, len, out);
  if (rc == FMX_OK) *out_len = len;
  return rc;
}

// ---------------------------------------------------------------- .fm writer (FMCreator.create)
// Wire format, bwtmerger.scala:483-485,476-481: byte elSize (=4), int64 big-endian size, then
// `size` big-endian int32 entries.  elSize 8 is `???` in the reference (:465-469), so n must stay
// below 0xffffffff here too.
int fmx_write_fm(const fmx_index *idx, const char *path) {
  if (!idx || !path) return arg_fail("null argument");
  const Index *h = H(idx);
  if (h->n >= 0xffffffffull) { g_err = "the .fm format has no 8-byte entries (bwtmerger.scala:465-469)"; return FMX_ERR_UNSUPPORTED; }
  int rc = use_device(h);
  if (rc) return rc;
  Call call(h);
  if ((rc = call.init()) != FMX_OK) return rc;
  void *dfm = nullptr;
  HIP_TRY(call.alloc(&dfm, h->n * 4), "hipMalloc(fm)");
  rc = call.timed_launch([&](hipStream_t st) { return launch_fm_fill(h, dfm, st); }, "k_fm_fill");
  if (rc) return rc;
  FILE *f = std::fopen(path, "wb");
  if (!f) { g_err = std::string("cannot create ") + path; return FMX_ERR_IO; }
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
  uint8_t hdr[9];
  hdr[0] = 4;
  for (int i = 0; i < 8; i++) hdr[1 + i] = (uint8_t)(h->n >> (56 - 8 * i));
  if (std::fwrite(hdr, 1, 9, f) != 9) { g_err = "short write"; return FMX_ERR_IO; }
  const size_t chunk = 64u << 20;
  std::vector<uint8_t> buf(std::min<uint64_t>(chunk, h->n * 4));
  for (uint64_t o = 0; o < h->n * 4; o += chunk) {
    const size_t len = (size_t)std::min<uint64_t>(chunk, h->n * 4 - o);
    HIP_TRY(hipMemcpy(buf.data(), (const uint8_t *)dfm + o, len, hipMemcpyDeviceToHost), "D2H(fm)");
    if (std::fwrite(buf.data(), 1, len, f) != len) { g_err = "short write"; return FMX_ERR_IO; }
  }
  return FMX_OK;
}

// ---------------------------------------------------------------- locate (fmx_locate.hip; SALoader / SACreator / bwtFm2sa)
int fmx_locate_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint64_t *out_pos) {
  if (!idx || (k && (!rows || !out_pos))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = locate_check(h);
  if (rc) return rc;
  for (size_t q = 0; q < k; q++)
    if (rows[q] >= h->n) return arg_fail("row out of range (reference: SALoader reads past X.sa)");
  if ((rc = use_device(h)) || !k) return rc;
  if ((rc = ensure_built(h, h->loc, locate_prepare, nullptr))) return rc;
  const HostIn ins[] = {{rows, k * 8}};
  const HostOut outs[] = {{out_pos, k * 8}};
  return run_io(h, ins, 1, outs, 1, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_locate(h, di[0], k, dout[0], st);
  });
}

int fmx_locate_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, void *d_out_pos, void *stream) {
  if (!idx || (k && (!d_rows || !d_out_pos))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = locate_check(h);
  if (rc) return rc;
  if ((rc = use_device(h)) || !k) return rc;
  if ((rc = ensure_built(h, h->loc, locate_prepare, (hipStream_t)stream))) return rc;
  HIP_TRY(launch_locate(h, d_rows, k, d_out_pos, (hipStream_t)stream), "k_locate");
  return FMX_OK;
}

int fmx_locate_intervals(const fmx_index *idx, const uint64_t *sp, const uint64_t *ep, size_t k, uint64_t max_per,
                         uint64_t *out_off, uint64_t *out_pos, size_t cap) {
  if (!idx || !out_off || (k && (!sp || !ep)) || (cap && !out_pos)) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = locate_check(h);
  if (rc) return rc;
  const uint64_t lim = max_per ? max_per : ~0ull;
  uint64_t total = 0;
  for (size_t i = 0; i < k; i++) {
    if (sp[i] > h->n || ep[i] > h->n) return arg_fail("interval out of range (sp, ep <= n)");
    out_off[i] = total;
    total += ep[i] > sp[i] ? std::min<uint64_t>(ep[i] - sp[i], lim) : 0;
  }
  out_off[k] = total;
  const uint64_t m = std::min<uint64_t>(total, cap);
  std::vector<uint64_t> rows(m);
  for (size_t i = 0, o = 0; i < k && o < m; i++)
    for (uint64_t t = 0; t < out_off[i + 1] - out_off[i] && o < m; t++) rows[o++] = sp[i] + t;
  if (m && (rc = fmx_locate_batch(idx, rows.data(), m, out_pos))) return rc;
  if (total > cap) {
    g_err = "locate_intervals: " + std::to_string(total) + " positions, room for " + std::to_string(cap);
    return FMX_ERR_OVERFLOW;
  }
  return FMX_OK;
}

int fmx_locate_intervals_dev(const fmx_index *idx, const void *d_sp, const void *d_ep, size_t k, uint64_t max_per,
                             void *d_out_off, void *d_out_pos, size_t cap, void *stream) {
  if (!idx || !d_out_off || (k && (!d_sp || !d_ep)) || (cap && !d_out_pos)) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = locate_check(h);
  if (rc) return rc;
  if ((rc = use_device(h))) return rc;
  if ((rc = ensure_built(h, h->loc, locate_prepare, (hipStream_t)stream))) return rc;
  HIP_TRY(launch_locate_intervals(h, d_sp, d_ep, k, max_per, d_out_off, d_out_pos, cap, (hipStream_t)stream), "k_locate");
  return FMX_OK;
}

int fmx_locate_info(const fmx_index *idx, uint32_t *rate, uint64_t *bytes, double *build_ms) {
  if (!idx) return arg_fail("null argument");
  const Index *h = H(idx);
  std::lock_guard<std::mutex> lk(h->loc.mu);
  if (rate) *rate = h->loc.ready ? h->loc.rate : (uint32_t)h->policy.locate_sample.load(std::memory_order_relaxed);
  if (bytes) *bytes = h->loc.ready ? h->loc.bytes : 0;
  if (build_ms) *build_ms = h->loc.ready ? h->loc.build_ms : 0.0;
  return FMX_OK;
}

// SACreator.create (bwtmerger.scala:542-555): n big-endian int32 values, SA[row] at byte 4 row.
int fmx_write_sa(const fmx_index *idx, const char *path) {
  if (!idx || !path) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = locate_check(h);
  if (rc) return rc;
  if (h->n >= (1ull << 32)) { g_err = "X.sa holds 4-byte entries (SACreator, bwtmerger.scala:548): n must be < 2^32"; return FMX_ERR_UNSUPPORTED; }
  FILE *f = std::fopen(path, "wb");
  if (!f) { g_err = std::string("cannot create ") + path; return FMX_ERR_IO; }
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
  if ((rc = use_device(h)) || (rc = device_room(locate_write_sa_bytes(h), "fmx_write_sa"))) return rc;
  DevMem mem;
  void *d_sa = nullptr;
  HIP_TRY(mem.get(&d_sa, h->n * 4), "hipMalloc(sa)");
  CtxLease lease(h);
  if (!lease.c) return FMX_ERR_HIP;
  if ((rc = locate_write_sa(h, lease.c->stream, (uint32_t *)d_sa))) return rc;
  const size_t chunk = 64u << 20;
  std::vector<uint8_t> buf(std::min<uint64_t>(chunk, h->n * 4));
  for (uint64_t o = 0; o < h->n * 4; o += chunk) {
    const size_t len = (size_t)std::min<uint64_t>(chunk, h->n * 4 - o);
    HIP_TRY(hipMemcpy(buf.data(), (const uint8_t *)d_sa + o, len, hipMemcpyDeviceToHost), "D2H(sa)");
    if (std::fwrite(buf.data(), 1, len, f) != len) { g_err = "short write"; return FMX_ERR_IO; }
  }
  return FMX_OK;
}

// ---------------------------------------------------------------- LCP (fmx_lcp.hip; LCPSuffixWalkingAlgo / LCPLoader / LCPCreator)
static thread_local double g_lcp_phases[3] = {0.0, 0.0, 0.0};

int fmx_lcp_batch(const fmx_index *idx, const uint64_t *rows, size_t k, uint32_t *out) {
  if (!idx || (k && (!rows || !out))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = lcp_check(h);
  if (rc) return rc;
  for (size_t q = 0; q < k; q++)
    if (rows[q] >= h->n) return arg_fail("row out of range (reference: LCPLoader reads past X.lcp)");
  if ((rc = use_device(h)) || !k) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, nullptr))) return rc;
  const HostIn ins[] = {{rows, k * 8}};
  const HostOut outs[] = {{out, k * 4}};
  return run_io(h, ins, 1, outs, 1, [&](hipStream_t st, const void *const *di, void *const *dout) {
    return launch_lcp_gather(h, di[0], k, dout[0], st);
  });
}

int fmx_lcp_batch_dev(const fmx_index *idx, const void *d_rows, size_t k, void *d_out, void *stream) {
  if (!idx || (k && (!d_rows || !d_out))) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = lcp_check(h);
  if (rc) return rc;
  if ((rc = use_device(h)) || !k) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, (hipStream_t)stream))) return rc;
  HIP_TRY(launch_lcp_gather(h, d_rows, k, d_out, (hipStream_t)stream), "k_lcp_rows");
  return FMX_OK;
}

static int lcp_range_args(const fmx_index *idx, uint64_t first, uint64_t count, const void *out) {
  if (!idx || (count && !out)) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = lcp_check(h);
  if (rc) return rc;
  if (first > h->n || count > h->n - first) return arg_fail("range out of the array (first + count <= n)");
  return FMX_OK;
}

int fmx_lcp_range(const fmx_index *idx, uint64_t first, uint64_t count, uint32_t *out) {
  int rc = lcp_range_args(idx, first, count, out);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h)) || !count) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, nullptr))) return rc;
  HIP_TRY(hipMemcpy(out, static_cast<const uint32_t *>(h->lcp.lcp) + first, count * 4, hipMemcpyDeviceToHost), "D2H(lcp)");
  return FMX_OK;
}

int fmx_lcp_range_dev(const fmx_index *idx, uint64_t first, uint64_t count, void *d_out, void *stream) {
  int rc = lcp_range_args(idx, first, count, d_out);
  if (rc) return rc;
  const Index *h = H(idx);
  if ((rc = use_device(h)) || !count) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, (hipStream_t)stream))) return rc;
  HIP_TRY(hipMemcpyAsync(d_out, static_cast<const uint32_t *>(h->lcp.lcp) + first, count * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream),
          "D2D(lcp)");
  return FMX_OK;
}

int fmx_lcp_info(const fmx_index *idx, uint64_t *bytes, double *build_ms, uint32_t *max_lcp, uint64_t *max_row, uint64_t *sum_lcp) {
  if (!idx) return arg_fail("null argument");
  const Index *h = H(idx);
  std::lock_guard<std::mutex> lk(h->lcp.mu);
  if (bytes) *bytes = h->lcp.ready ? h->lcp.bytes : 0;
  if (build_ms) *build_ms = h->lcp.ready ? h->lcp.build_ms : 0.0;
  if (max_lcp) *max_lcp = h->lcp.ready ? h->lcp.max : 0;
  if (max_row) *max_row = h->lcp.ready ? h->lcp.max_row : 0;
  if (sum_lcp) *sum_lcp = h->lcp.ready ? h->lcp.sum : 0;
  return FMX_OK;
}

// LCPCreator.create (bwtmerger.scala:558-652): big-endian int32, LCP[r] at byte 4 r, slots 0 .. n - 2 (the loop never
// writes slot n - 1): 4 (n - 1) bytes.
int fmx_write_lcp(const fmx_index *idx, const char *path) {
  if (!idx || !path) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = lcp_check(h);
  if (rc) return rc;
  if ((rc = use_device(h))) return rc;
  if ((rc = ensure_built(h, h->lcp, lcp_prepare, nullptr))) return rc;
  FILE *f = std::fopen(path, "wb");
  if (!f) { g_err = std::string("cannot create ") + path; return FMX_ERR_IO; }
  std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
  const uint64_t entries = h->n - 1, chunk = 16u << 20;
  std::vector<uint32_t> buf((size_t)std::min<uint64_t>(chunk, entries));
  for (uint64_t o = 0; o < entries; o += chunk) {
    const size_t len = (size_t)std::min<uint64_t>(chunk, entries - o);
    HIP_TRY(hipMemcpy(buf.data(), static_cast<const uint32_t *>(h->lcp.lcp) + o, len * 4, hipMemcpyDeviceToHost), "D2H(lcp)");
    for (size_t i = 0; i < len; i++) buf[i] = __builtin_bswap32(buf[i]);
    if (std::fwrite(buf.data(), 4, len, f) != len) { g_err = "short write"; return FMX_ERR_IO; }
  }
  return FMX_OK;
}

int fmx_lcp_last_phases(double *phi_ms, double *plcp_ms, double *gather_ms) {
  if (phi_ms) *phi_ms = g_lcp_phases[0];
  if (plcp_ms) *plcp_ms = g_lcp_phases[1];
  if (gather_ms) *gather_ms = g_lcp_phases[2];
  return FMX_OK;
}

// ---------------------------------------------------------------- construction from text (fmx_sufsort.hip)
static constexpr uint64_t kMaxTextLen = 0xfffffffeull;       // 2^32 - 2: len + 1 suffixes fit u32

// What is checked before the device is touched; host text (may be null for the _dev form) is scanned for byte 0.
static int text_args(const void *text, uint64_t len, const uint8_t *host_text) {
  if (!text) return arg_fail("text is null");
  if (len == 0) return arg_fail("len must be >= 1");
  if (len > kMaxTextLen) {
    g_err = "text of " + std::to_string(len) + " bytes: construction takes at most 2^32 - 2 bytes (u32 suffix indices)";
    return FMX_ERR_UNSUPPORTED;
  }
  if (host_text && std::memchr(host_text, 0, (size_t)len)) {
    g_err = "the text contains byte 0 (findex's readers escape it; counts[0] must be 0)";
    return FMX_ERR_UNSUPPORTED;
  }
  return FMX_OK;
}

// The host-pointer forms: text to HBM, construction, BWT to `bwt_out` (host) or into a handle (fmx_open_text).
static int text_to_device_bwt(const uint8_t *text, uint64_t len, int device, uint8_t *bwt_out, uint64_t *eof,
                              int64_t counts[256], fmx_index **idx_out) {
  int rc = use_device_index(device);
  if (rc) return rc;
  const uint64_t n = len + 1;
  if ((rc = device_room(sufsort_peak_bytes(len, false) + len + n, "suffix sort of " + std::to_string(len) + " bytes"))) return rc;
  DevMem mem;
  void *d_text = nullptr, *d_bwt = nullptr;
  StreamGuard own;
  HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
  DEV_ALLOC(mem, d_text, len, "text, bwt");
  DEV_ALLOC(mem, d_bwt, n, "text, bwt");
  HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, own.s), "H2D(text)");
  rc = sufsort_bwt(d_text, len, d_bwt, nullptr, eof, counts, own.s, 0);
  if (rc) return rc;
  mem.free_now(d_text);               // before the handle's dictionary is built
  if (bwt_out) {
    HIP_TRY(hipMemcpyAsync(bwt_out, d_bwt, n, hipMemcpyDeviceToHost, own.s), "D2H(bwt)");
    HIP_TRY(hipStreamSynchronize(own.s), "hipStreamSynchronize");
    return FMX_OK;
  }
  return open_common(d_bwt, true, nullptr, n, *eof, counts, device, own.s, idx_out);
}

int fmx_bwt_from_text(const uint8_t *text, uint64_t len, uint8_t *bwt, uint64_t *eof, int64_t counts[256], int device) {
  int rc = text_args(text, len, text);
  if (rc) return rc;
  if (!bwt || !eof || !counts) return arg_fail("null argument");
  return text_to_device_bwt(text, len, device, bwt, eof, counts, nullptr);
}

int fmx_bwt_from_text_dev(const void *d_text, uint64_t len, void *d_bwt, void *d_sa_or_null, uint64_t *eof,
                          int64_t counts[256], int device, void *stream) {
  int rc = text_args(d_text, len, nullptr);
  if (rc) return rc;
  if (!d_bwt || !eof || !counts) return arg_fail("null argument");
  if ((rc = use_device_index(device))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "index construction"))) return rc;
  return sufsort_bwt(d_text, len, d_bwt, d_sa_or_null, eof, counts, st, 0);
}

// The LCP array without a handle: s = reverse(text) + sentinel on the device, then the core (fmx_lcp.hip).
static int lcp_from_device_text(const void *d_text, uint64_t len, const void *d_sa, void *d_lcp, int device, hipStream_t st,
                                uint64_t extra) {
  const uint64_t n = len + 1;
  int rc = device_room(lcp_text_bytes(n) + lcp_core_bytes(n) + extra, "the LCP array of " + std::to_string(len) + " bytes");
  if (rc) return rc;
  DevMem mem;
  uint8_t *s = nullptr;
  DEV_ALLOC(mem, s, lcp_text_bytes(n), "LCP");
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  lcp_reverse_text(static_cast<const uint8_t *>(d_text), len, s, cus, st);
  HIP_TRY(hipGetLastError(), "k_lcp_reverse");
  LcpInfo info;
  rc = lcp_core(s, n, static_cast<const uint32_t *>(d_sa), static_cast<uint32_t *>(d_lcp), cus, st, &info);
  if (rc) return rc;
  for (int i = 0; i < 3; i++) g_lcp_phases[i] = info.phase_ms[i];
  return FMX_OK;
}

int fmx_lcp_from_text_dev(const void *d_text, uint64_t len, const void *d_sa, void *d_lcp, int device, void *stream) {
  if (!d_text || !d_sa || !d_lcp) return arg_fail("null argument");
  int rc = text_args(d_text, len, nullptr);
  if (rc) return rc;
  if ((rc = use_device_index(device))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = not_capturing(st, "index construction"))) return rc;
  return lcp_from_device_text(d_text, len, d_sa, d_lcp, device, st, 0);
}

int fmx_lcp_from_text(const uint8_t *text, uint64_t len, uint32_t *lcp, int device) {
  if (!text || !lcp) return arg_fail("null argument");
  int rc = text_args(text, len, text);
  if (rc) return rc;
  if ((rc = use_device_index(device))) return rc;
  const uint64_t n = len + 1;
  // the sort's temporaries are gone when the LCP's come; text, BWT / LCP (one buffer, 4 n) and the suffix array stay throughout
  const uint64_t need = len + 4 * n + 4 * n + std::max<uint64_t>(sufsort_peak_bytes(len, true), lcp_text_bytes(n) + lcp_core_bytes(n));
  if ((rc = device_room(need, "suffix sort and LCP array of " + std::to_string(len) + " bytes", "need"))) return rc;
  DevMem mem;
  void *d_text = nullptr, *d_sa = nullptr, *d_out = nullptr;
  StreamGuard own;
  HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
  DEV_ALLOC(mem, d_text, len, "text, sa, lcp");
  DEV_ALLOC(mem, d_sa, 4 * n, "text, sa, lcp");
  DEV_ALLOC(mem, d_out, 4 * n, "text, sa, lcp");              // the BWT first (n bytes of it), then the LCP array
  HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, own.s), "H2D(text)");
  uint64_t eof = 0;
  int64_t counts[256];
  if ((rc = sufsort_bwt(d_text, len, d_out, d_sa, &eof, counts, own.s, 0))) return rc;
  if ((rc = lcp_from_device_text(d_text, len, d_sa, d_out, device, own.s, 0))) return rc;
  HIP_TRY(hipMemcpyAsync(lcp, d_out, 4 * n, hipMemcpyDeviceToHost, own.s), "D2H(lcp)");
  HIP_TRY(hipStreamSynchronize(own.s), "hipStreamSynchronize");
  return FMX_OK;
}

int fmx_open_text(const uint8_t *text, uint64_t len, int device, fmx_index **out) {
  if (!out) return arg_fail("out is null");
  *out = nullptr;
  int rc = text_args(text, len, text);
  if (rc) return rc;
  uint64_t eof = 0;
  int64_t counts[256];
  return text_to_device_bwt(text, len, device, nullptr, &eof, counts, out);
}

// BWTLoader / AUXLoader's formats (bwtmerger.scala:130-174): int64 size, int64 eof, the bytes; 256 int64 counts.
int fmx_write_bwt(const char *bwt_path, const char *aux_path, const uint8_t *bwt, uint64_t n, uint64_t eof,
                  const int64_t counts[256], int big_endian) {
  if (!bwt_path || !aux_path || !bwt || !counts) return arg_fail("null argument");
  if (n < 1 || eof >= n) return arg_fail("need n >= 1 and eof < n");
  auto put = [big_endian](uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[big_endian ? i : 7 - i] = (uint8_t)(v >> (56 - 8 * i));
  };
  {
    FILE *f = std::fopen(bwt_path, "wb");
    if (!f) { g_err = std::string("cannot create ") + bwt_path; return FMX_ERR_IO; }
    std::unique_ptr<FILE, int (*)(FILE *)> guard(f, std::fclose);
    uint8_t hdr[16];
    put(hdr, n);
    put(hdr + 8, eof);
    if (std::fwrite(hdr, 1, 16, f) != 16 || std::fwrite(bwt, 1, (size_t)n, f) != n) {
      g_err = std::string("short write on ") + bwt_path;
      return FMX_ERR_IO;
    }
    if (std::fclose(guard.release()) != 0) { g_err = std::string("short write on ") + bwt_path; return FMX_ERR_IO; }
  }
  uint8_t aux[2048];
  for (int c = 0; c < 256; c++) put(aux + 8 * c, (uint64_t)counts[c]);
  FILE *f = std::fopen(aux_path, "wb");
  if (!f) { g_err = std::string("cannot create ") + aux_path; return FMX_ERR_IO; }
  const bool ok = std::fwrite(aux, 1, sizeof aux, f) == sizeof aux;
  if ((std::fclose(f) != 0) || !ok) { g_err = std::string("short write on ") + aux_path; return FMX_ERR_IO; }
  return FMX_OK;
}

// ---------------------------------------------------------------- statistics
int fmx_stats(const fmx_index *idx, fmx_stats_t *out) {
  if (!idx || !out) return arg_fail("null argument");
  const Index *h = H(idx);
  int rc = use_device(h);
  if (rc) return rc;
  unsigned long long cnt[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::memset(out, 0, sizeof *out);
  HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  {   // the counters live in per-workgroup slots (fmx_device.h): sum them
    std::vector<unsigned long long> slots((size_t)kCounterSlots * kCounterStride);
    HIP_TRY(hipMemcpy(slots.data(), h->d_counters, kCounterBytes, hipMemcpyDeviceToHost), "D2H(counters)");
    for (uint32_t sl = 0; sl < kCounterSlots; sl++)
      for (int j = 0; j < 12; j++) cnt[j] += slots[(size_t)sl * kCounterStride + j];
  }
  const TablesSnapshot tab = tables_snapshot(h);      // (before h->mu: each table's own lock, one at a time)
  std::lock_guard<std::mutex> lk(h->mu);
  out->rank_queries = cnt[0];
  out->backward_steps = cnt[1];
  out->launches = h->launches;
  out->last_kernel_ms = h->last_kernel_ms;
  out->index_bytes = h->index_bytes + tab.sel_held + tab.kmer_held + tab.jump_held + tab.row1_held + tab.row3_held;
  out->jump_lookups = cnt[10];
  out->jump_bytes = tab.jump_held;
  out->row_lookups = cnt[11];
  out->row_bytes = tab.row1_held + tab.row3_held;
  out->n_blocks = h->nblocks;
  out->n_symbols = h->nslots;
  out->block_bytes = h->layout == kLayoutBytes ? kByteBlock + 4 : kBlockBytes;
  out->layout = h->layout;
  out->search_requests = cnt[2];
  out->frontier_requests = cnt[3];
  out->frontier_queue_writes = cnt[4];
  out->frontier_results = cnt[5];
  out->frontier_elements = cnt[6];
  out->frontier_queue_reads = cnt[7];
  out->frontier_records = cnt[8];
  out->ktab_lookups = cnt[9];
  out->ktab_k = tab.kmer_k;
  out->search_residency = h->search_residency.load();
  out->jump_chars = tab.jump_jc;      // (0 while there is no J)
  out->build_ms = h->build_ms;
  out->tables_build_ms = h->tables_ms.load(std::memory_order_relaxed);
  out->tables_alloc_ms = (double)h->tables_alloc_us.load(std::memory_order_relaxed) * 1e-3;
  out->peak_table_build_bytes = h->peak_table_build_bytes.load(std::memory_order_relaxed);
  out->patterns_seen = h->patterns_seen.load(std::memory_order_relaxed);
  out->tables_held_bytes = h->tables_held.load(std::memory_order_relaxed);
  out->hbm_free_after_tables = h->hbm_free_after_tables.load(std::memory_order_relaxed);
  {
    const uint32_t ppm = h->policy.budget_ppb.load(std::memory_order_relaxed);
    uint64_t budget = h->policy.budget_bytes.load(std::memory_order_relaxed);
    size_t free_b = 0, total_b = 0;
    if (ppm && hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = (uint64_t)((double)(free_b + out->tables_held_bytes) * ((double)ppm * 1e-9));
    out->table_budget_bytes = budget;
  }
  return FMX_OK;
}

int fmx_last_kernel_ms(const fmx_index *idx, double *ms) {
  if (!idx || !ms) return arg_fail("null argument");
  const Index *h = H(idx);
  std::lock_guard<std::mutex> lk(h->mu);
  *ms = h->last_kernel_ms;
  return FMX_OK;
}

int fmx_stats_reset(fmx_index *idx) {
  if (!idx) return arg_fail("null argument");
  Index *h = H(idx);
  int rc = use_device(h);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  HIP_TRY(hipMemset(h->d_counters, 0, kCounterBytes), "memset(counters)");
  std::lock_guard<std::mutex> lk(h->mu);
  h->launches = 0;
  h->last_kernel_ms = 0;
  return FMX_OK;
}

}  // extern "C"
