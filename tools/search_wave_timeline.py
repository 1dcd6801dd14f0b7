#!/usr/bin/env python3
"""When do the waves of k_search4 begin and end?  Diagnostic build -DFMX_SEARCHLOG (works in the round-3 worktree too,
patched with the same log):
    tools/build_variant.sh slog -DFMX_SEARCHLOG && FMX_LIB=findex_amd/lib/variants/libfmx_slog.so python tools/search_wave_timeline.py c5
Prints the launch's span on the device's 100 MHz clock, when the waves began / entered their batch loop / issued their first
table lookup / drew their first ticket / left the loop / ended (percentiles), how long a batch took, and how many waves were
alive at tenths of the span, and per class of ticket counter (by its number of drawers) what its waves drew from the pool and
when they ended, when the class's pool ran dry (its last draw that gave a batch), how far behind that the launch ends and which
share of the claims was made beside a row-jump lookup.  Last, what-ifs on the logged launch: the partial round to the fastest
waves, and the pool replayed under three claim rules (claim_replay below).  A second argument 4 or 6 reads the log of a build
from before the two marks (four words per wave) or from before the claim's words (six; the default is eight); a third is the
number of full rounds the build draws (2); a fourth the round trip of a draw the replay assumes, in us (2.5)."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
wl = sys.argv[1] if len(sys.argv) > 1 else "c5"
words = int(sys.argv[2]) if len(sys.argv) > 2 else 8
pooled_rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2      # full rounds the build draws with the partial one (fmx_search.hip, kPoolRounds)
round_trip = float(sys.argv[4]) if len(sys.argv) > 4 else 2.5     # us from a draw's issue to its ticket, as the replay assumes it
if os.environ.get("FMX_SEARCHLOG_LOAD"):      # a log kept by an earlier run (FMX_SEARCHLOG_SAVE=file.npy): no device needed
    log = np.load(os.environ["FMX_SEARCHLOG_LOAD"])
    words = log.shape[1]
else:
    import torch
    import bench, findex_amd
    from findex_amd import _lib
    log2n, sigma, k, m, seed = bench.LITERAL[wl]
    n = 1 << log2n
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    bwt, eof = bench.make_bwt(torch, n, sigma, seed, dev); torch.cuda.synchronize()
    hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, None, device=0, stream=stream)
    if hasattr(hip, "prepare"):
        hip.prepare(ktab=True, jump=True)
    del bwt
    pats, off = bench.make_patterns(torch, hip, n, sigma, k, m, seed * 1000, dev, stream)
    sp = torch.empty(k, dtype=torch.int64, device=dev)
    ep = torch.empty(k, dtype=torch.int64, device=dev)
    for _ in range(5):
        hip.search_batch_dev(pats.data_ptr(), off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k, stream)
    torch.cuda.synchronize()
    L = _lib.load()
    L.fmx_debug_searchlog.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    log = np.zeros((1 << 15, words), dtype=np.uint64)
    assert L.fmx_debug_searchlog(log.ctypes.data_as(ctypes.c_void_p), log.nbytes) == 0
    print("device ms of the logged call (all its kernels): %.4f" % hip.last_kernel_ms())
    if os.environ.get("FMX_SEARCHLOG_SAVE"):
        np.save(os.environ["FMX_SEARCHLOG_SAVE"], log)
t3 = log[:, 3] & np.uint64((1 << 48) - 1)
nb = (log[:, 3] >> np.uint64(48)).astype(np.int64)
live = log[:, 0] != 0
live &= log[:, 0] + np.uint64(100000) > log[live, 0].max()      # the log is never cleared: entries of earlier, larger launches (within 1 ms of the newest: this launch)
t0 = log[live, 0].astype(np.int64)
t1 = t0 + (log[live, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)      # (entry 1: the batch loop's begin and the last walk's, both from t0)
tw = t0 + (log[live, 1] >> np.uint64(32)).astype(np.int64)
t2, t3, nb = log[live, 2].astype(np.int64), t3[live].astype(np.int64), nb[live]
T = 0.01      # us per tick
z = t0.min()
span = (t3.max() - z) * T
print("%d waves; span of the launch %.1f us" % (live.sum(), span))
def pct(name, v):
    q = np.percentile(v, [0, 10, 50, 90, 99, 100])
    print("%-34s min %7.1f  p10 %7.1f  p50 %7.1f  p90 %7.1f  p99 %7.1f  max %7.1f us" % ((name,) + tuple(q)))
pct("wave begins at", (t0 - z) * T)
pct("enters its batch loop at", (t1 - z) * T)
if words >= 6:
    look, draw = log[live, 4].astype(np.int64), log[live, 5].astype(np.int64)
    pct("issues its first table lookup at", (look[look != 0] - z) * T)
    if (draw != 0).any():
        pct("draws its first ticket at", (draw[draw != 0] - z) * T)
        pct("first ticket to the wave's end", (t3[draw != 0] - draw[draw != 0]) * T)
        print("first ticket of the launch at %.1f us, median one at %.1f us; the launch ends %.1f us behind the median first ticket"
              % ((draw[draw != 0].min() - z) * T, (np.median(draw[draw != 0]) - z) * T, (t3.max() - np.median(draw[draw != 0])) * T))
pct("begins its last walk at", (tw - z) * T)
pct("last walk takes", (t2 - tw) * T)
pct("has walked at", (t2 - z) * T)
pct("ends at", (t3 - z) * T)
pct("alive for", (t3 - t0) * T)
pct("set-up (tables into LDS)", (t1 - t0) * T)
pct("per batch", (tw - t1) * T / np.maximum(nb, 1))
for b in sorted(set(nb.tolist())):
    sel = nb == b
    print("waves with %d batches: %5d; batch loop ends p50 %6.1f p99 %6.1f, wave ends p50 %6.1f p99 %6.1f max %6.1f us" % (b, sel.sum(), np.percentile((tw[sel] - z) * T, 50), np.percentile((tw[sel] - z) * T, 99), np.percentile((t3[sel] - z) * T, 50), np.percentile((t3[sel] - z) * T, 99), ((t3[sel] - z) * T).max()))
print("batches per wave: min %d max %d" % (nb.min(), nb.max()))
# The pool by class of ticket counter (fmx_pool_deal.h): wave w draws from counter (w / 32) mod min(groups, 64), so the counters
# have unequal numbers of drawers whenever the groups are no multiple of 64; a counter's share of the pool should be in
# proportion.  What its waves drew is measured: their batches beyond the strided rounds.
if words >= 6 and (draw != 0).any():
    wv = np.nonzero(live)[0]
    nw, total = int(wv.max()) + 1, int(nb.sum())
    strided = total // nw - pooled_rounds                    # full rounds every wave takes by stride
    nsh = min((nw + 31) // 32, 64)
    shard = (wv >> 5) % nsh
    drawers = np.bincount(shard, minlength=nsh)
    took = np.bincount(shard, weights=nb - strided, minlength=nsh)
    print("the pool: %d batches behind %d strided rounds, %d counters" % (total - strided * nw, strided, nsh))
    if words >= 8:
        last_ok = log[live, 6].astype(np.int64)                  # the wave's last draw that gave it a batch goes out (0: none did)
        beside = (log[live, 7] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        behind = (log[live, 7] >> np.uint64(32)).astype(np.int64)
    for d in sorted(set(drawers.tolist()), reverse=True):
        cs = drawers == d
        sel = cs[shard]
        print("  counters with %3d drawers: %2d (%5d waves); pool batches per counter %6.1f (a share in proportion: %6.1f), batches per wave %d + %.2f; waves end p50 %6.1f max %6.1f us"
              % (d, cs.sum(), sel.sum(), took[cs].mean(), (total - strided * nw) * d / nw, strided, took[cs].sum() / sel.sum(),
                 np.percentile((t3[sel] - z) * T, 50), ((t3[sel] - z) * T).max()))
        if words >= 8 and (last_ok[sel] != 0).any():
            # a counter's pool is dry when its last ticket below its share has been drawn
            dry = np.array([(last_ok[sel & (shard == c)].max() - z) * T for c in np.nonzero(cs)[0] if (last_ok[sel & (shard == c)] != 0).any()])
            nclaims = int(beside[sel].sum() + behind[sel].sum())
            print("    its pool runs dry at p50 %6.1f max %6.1f us (per counter); the launch ends %5.1f us behind the median; claims beside a lookup %d, behind the loop %d (%s beside)"
                  % (np.percentile(dry, 50), dry.max(), span - np.percentile(dry, 50), int(beside[sel].sum()), int(behind[sel].sum()),
                     "%.1f %%" % (100.0 * beside[sel].sum() / nclaims) if nclaims else "none made in a batch: the draw stands in front of it"))
    if words >= 8 and (last_ok != 0).any():
        nclaims = int(beside.sum() + behind.sum())
        print("  the launch: the last ticket that gave a batch is drawn at %.1f us, %.1f us before the launch ends; claims beside a lookup %d, behind the loop %d%s"
              % ((last_ok.max() - z) * T, span - (last_ok.max() - z) * T, int(beside.sum()), int(behind.sum()),
                 " (%.1f %% beside)" % (100.0 * beside.sum() / nclaims) if nclaims else ""))
for f in range(0, 11):
    at = z + int(f / 10 * (t3.max() - z))
    print("  at %3d %% of the span: %5d waves alive, %5d not begun, %5d ended" % (10 * f, int(((t0 <= at) & (t3 > at)).sum()), int((t0 > at).sum()), int((t3 <= at).sum())))
# by XCD (workgroup id mod 8) and by the order of the waves
wid = np.nonzero(live)[0]
for x in range(8):
    sel = ((wid // 4) % 8) == x
    print("  XCD %d: waves begin p50 %6.1f, end p50 %6.1f max %6.1f us" % (x, np.percentile((t0[sel] - z) * T, 50), np.percentile((t3[sel] - z) * T, 50), ((t3[sel] - z) * T).max()))
# What handing the partial last round to the FAST waves would give: every wave keeps its own pace (us per batch);
# statically the first (batches mod waves) waves take the extra batch, dynamically the ones with the lowest pace do.
pace = (t2 - t1) * T / np.maximum(nb, 1)
base_n = int(nb.min())
n_extra = int((nb > base_n).sum())
start = (t1 - z) * T
static_end = start + nb * pace
fast = np.argsort(pace)[:n_extra]
dyn_n = np.full(nb.shape, base_n)
dyn_n[fast] += 1
dyn_end = start + dyn_n * pace
print("last round to the fastest waves (same paces): static ends p50 %.1f p99 %.1f max %.1f us; by pace p50 %.1f p99 %.1f max %.1f us"
      % (np.percentile(static_end, 50), np.percentile(static_end, 99), static_end.max(),
         np.percentile(dyn_end, 50), np.percentile(dyn_end, 99), dyn_end.max()))
# and with perfect balance (work stealing at batch granularity): total work / waves
print("perfect balance: %.1f us" % (start.mean() + (nb * pace).sum() / nb.size))
# What another claim rule would give: the pool of the logged launch replayed.  Every wave arrives at the pool when it did (its
# first draw), takes the time per drawn batch it took (arrival to the end of its batch loop over its drawn batches; a wave that drew
# none: its time per batch overall) and the time behind its loop it took; every counter hands out the batches it handed out.  A draw
# takes `round_trip`; a counter serves draws in order of issue.  The rules differ in WHEN a wave issues the draw for its next batch:
#   two batches at arrival   at the start of the batch before (the draw in front of one_batch: two claimed within a round trip)
#   one batch and a trip     a round trip before the batch before ends (the draw beside the batch's last lookup)
#   after the batch          when the batch before has ended (the round trip is paid every time)
def claim_replay(rule):
    import heapq
    ends, dry = np.zeros(nb.size), 0.0
    for c in range(nsh):
        ws = np.nonzero(shard == c)[0]
        left = int(took[c])
        heap = [(arr[w], int(w)) for w in ws]
        heapq.heapify(heap)
        free = {int(w): arr[w] for w in ws}
        while heap:
            at, w = heapq.heappop(heap)
            if left == 0:
                ends[w] = max(free[w], at + round_trip) + tail[w]
                continue
            left -= 1
            dry = max(dry, at)
            begin = max(free[w], at + round_trip)
            free[w] = begin + ppace[w]
            heapq.heappush(heap, ({"arrival": begin, "trip": max(begin, free[w] - round_trip), "after": free[w]}[rule], w))
    return ends, dry
if words >= 6 and (draw != 0).any() and (draw != 0).all():
    arr = (draw - z) * T
    npool = nb - strided
    # (a wave's drawn batches begin with the round trip of its first draw, which the replay pays again)
    ppace = np.where(npool > 0, np.maximum((tw - draw) * T - round_trip, 0.0) / np.maximum(npool, 1), (tw - t1) * T / np.maximum(nb, 1))
    tail = (t3 - tw) * T
    print("the pool replayed (same arrivals, same time per drawn batch, a draw's round trip %.1f us); measured: waves end p50 %.1f p99 %.1f max %.1f us"
          % (round_trip, np.percentile((t3 - z) * T, 50), np.percentile((t3 - z) * T, 99), span))
    for rule, name in (("arrival", "two batches at arrival"), ("trip", "one batch and a round trip"), ("after", "after the batch")):
        e, dry = claim_replay(rule)
        print("  %-27s the pool is dry at %5.1f us; waves end p50 %5.1f p99 %5.1f max %5.1f us" % (name + ":", dry, np.percentile(e, 50), np.percentile(e, 99), e.max()))
