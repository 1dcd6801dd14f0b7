#!/usr/bin/env python3
"""N-gram measurements: fmx_ngrams on texts of tools/text_bwt.py at L = 8 and L = 32, min_count 2, the 1000
most frequent by count, a spectrum of 1024 bins -- with positions and without -- beside the route a caller had before the
call existed, measured in the same run on the same handle: hip.lcp() and the full suffix array (X.sa, fmx_write_sa) brought
to the host, 8 n bytes, then the passes in numpy (run boundaries from lcp < L, np.diff, np.maximum.reduceat over SA,
np.bincount, a lexsort by (-count, sp)).  For the call without positions the host route is also timed without the suffix
array (4 n bytes and the closed form for the short rows).  Records, summaries and spectra are asserted equal.

    python tools/ngrams_bench.py [--bits 24,28] [--lengths 8,32] [--out profiles/ngrams_bench.jsonl]

One JSON line per text, length and mode, and one per text for a second length in the same call, appended to --out.  Times are
wall-clock around the calls (ms) unless they are named after a phase (device events)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

TOP, BINS, MIN_COUNT = 1000, 1024, 2
# bytes per row each phase must move ("the passes") when every row is the last row of its run, which is
# nearly so on these texts: the streaming kernels' reads and writes and the scans (a scan reads and writes its array twice: 16)
PHASE_BYTES = {True: {"class": 12 + 16 + 4 + 16, "select": 16 + 4}, False: {"class": 8 + 16 + 12, "select": 16 + 4}}
SORT_BYTES_PER_PASS = 8 + 24               # per selected class: the histogram's read of the key, the scatter's read and write of the pair


def numpy_route(lcp, sa, L):
    """The passes of fmx_ngrams.hip over the downloaded arrays, no stop byte; sa None: no positions -> (records, summary, spectrum)"""
    n = lcp.size
    m = n - 1
    ends = np.flatnonzero(lcp < L)                              # (LCP[n - 1] == 0: the last row ends a run)
    heads = np.concatenate(([0], ends[:-1] + 1))
    size = np.diff(np.concatenate(([0], ends + 1)))
    if sa is not None:
        pmax = np.maximum.reduceat(sa, heads).astype(np.int64)
        win = pmax + L <= m
        sp, cnt, first = heads[win], size[win], (m - L - pmax)[win]
        spectrum = np.bincount(np.where(cnt < BINS, cnt, 0), minlength=BINS).astype(np.uint64)
        distinct, windows, singles = int(cnt.size), int(cnt.sum()), int((cnt == 1).sum())
    else:
        sp, cnt, first = heads, size, None
        spectrum = np.bincount(np.where(cnt < BINS, cnt, 0), minlength=BINS).astype(np.uint64)
        spectrum[1] -= np.uint64(L)
        distinct, windows, singles = int(cnt.size) - L, int(cnt.sum()) - L, int((cnt == 1).sum()) - L
    sel = np.flatnonzero(cnt >= MIN_COUNT)
    order = sel[np.lexsort((sp[sel], -cnt[sel]))][:TOP]
    rec = np.zeros((order.size, 3), dtype=np.uint64)
    rec[:, 0], rec[:, 1] = sp[order], cnt[order]
    rec[:, 2] = first[order] if first is not None else np.uint64(2 ** 64 - 1)
    largest = int(cnt[sel].max()) if sel.size else 1
    big = np.flatnonzero(cnt == largest)
    at = big[0] if sel.size else None                           # (sp ascends with the runs: the first is the smallest)
    summary = dict(records=int(order.size), selected=int(sel.size), distinct=distinct, windows=windows, singletons=singles,
                   largest_count=largest, largest_sp=int(sp[at]) if at is not None else None,
                   largest_pos=int(first[at]) if at is not None and first is not None else None)
    return rec, summary, spectrum


def agree(rec, summary, want_rec, want_s, want_spec):
    assert np.array_equal(rec.view(np.uint64).reshape(-1, 3), want_rec)
    assert np.array_equal(summary["spectrum"], want_spec)
    for f, v in want_s.items():
        assert v is None or summary[f] == v, (f, summary[f], v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="24,28")
    ap.add_argument("--lengths", default="8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngrams_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import make_text
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    lengths = [int(x) for x in a.lengths.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lib = _lib.load()

    def emit(r):
        print(json.dumps(r), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(r) + "\n")

    def sized_call(hip, lv, positions, total):
        """one sized fmx_ngrams call -> wall ms"""
        lv = np.array(lv, dtype=np.uint32)
        opts = _lib.fmx_ngram_opts(_lib.FMX_NGRAMS_BY_COUNT, 0 if positions else _lib.FMX_NGRAMS_NO_POS, MIN_COUNT, TOP, BINS, 0, (0, 0, 0))
        off = np.zeros(lv.size + 1, dtype=np.uint64)
        out = np.zeros((max(total, 1), 3), dtype=np.uint64)
        spec = np.zeros(lv.size * BINS, dtype=np.uint64)
        n_out = ctypes.c_size_t()
        t0 = time.perf_counter()
        _lib.check(lib.fmx_ngrams(hip.handle, lv.ctypes.data, lv.size, ctypes.byref(opts), off.ctypes.data, out.ctypes.data, total,
                                  ctypes.byref(n_out), None, spec.ctypes.data))
        return (time.perf_counter() - t0) * 1e3

    for bits in [int(b) for b in a.bits.split(",")]:
        text = make_text(torch, 1 << bits, 1, dev)
        length = text.numel()
        n = length + 1
        bwt = torch.empty(n, dtype=torch.uint8, device=dev)
        eof, counts = findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), 0, device=0, stream=st)
        del text
        torch.cuda.empty_cache()
        hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, counts)
        hip.prepare(ktab=False, lcp=True)                      # every route starts from a handle that has its LCP array
        t0 = time.perf_counter()
        lcp = hip.lcp()
        lcp_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        with tempfile.TemporaryDirectory() as tmp:
            hip.write_sa(os.path.join(tmp, "x.sa"))
            sa = np.fromfile(os.path.join(tmp, "x.sa"), dtype=">u4").astype(np.uint32)
        sa_ms = (time.perf_counter() - t0) * 1e3
        for L in lengths:
            host = {}
            for positions in (True, False):
                t0 = time.perf_counter()
                host[positions] = numpy_route(lcp, sa if positions else None, L) + ((time.perf_counter() - t0) * 1e3,)
            for positions in (True, False):
                kw = dict(min_count=MIN_COUNT, top=TOP, order="count", spectrum=BINS, positions=positions)
                hip.ngrams(L, **kw)                             # warm-up
                t0 = time.perf_counter()
                rec, summary = hip.ngrams(L, **kw)              # the counting call and the sized call
                api_ms = (time.perf_counter() - t0) * 1e3
                call_ms = sized_call(hip, [L], positions, rec.size)
                invert_ms, class_ms, select_ms, sort_ms = hip.ngrams_last()
                want_rec, want_s, want_spec, passes_ms = host[positions]
                agree(rec, summary, want_rec, want_s, want_spec)
                route_ms = lcp_ms + (sa_ms if positions else 0.0) + passes_ms
                full_ms = lcp_ms + sa_ms + host[True][3]
                pb = PHASE_BYTES[positions]
                passes = (max(1, int(n - 1).bit_length()) + max(1, int(summary["largest_count"] - MIN_COUNT).bit_length()) + 7) // 8
                sort_bytes = SORT_BYTES_PER_PASS * passes * summary["selected"]
                emit({"text_bits": bits, "n": n, "length": L, "positions": positions, "min_count": MIN_COUNT, "top": TOP, "bins": BINS,
                      "invert_ms": round(invert_ms, 3), "class_ms": round(class_ms, 3), "select_ms": round(select_ms, 3),
                      "sort_ms": round(sort_ms, 3), "device_call_ms": round(call_ms, 2), "device_api_ms": round(api_ms, 2),
                      "phase_bytes": {k: v * n for k, v in pb.items()}, "sort_bytes": sort_bytes, "sort_passes": passes,
                      "phase_GBps": {"class": round(pb["class"] * n / max(class_ms, 1e-9) / 1e6, 1),
                                     "select": round(pb["select"] * n / max(select_ms, 1e-9) / 1e6, 1),
                                     "sort": round(sort_bytes / max(sort_ms, 1e-9) / 1e6, 1)},
                      "summary": {k: v for k, v in summary.items() if k != "spectrum"},
                      "host_lcp_download_ms": round(lcp_ms, 1), "host_sa_download_ms": round(sa_ms, 1), "host_passes_ms": round(passes_ms, 1),
                      "host_route_ms": round(full_ms, 1), "host_route_same_inputs_ms": round(route_ms, 1),
                      "host_route_over_device_api": round(full_ms / api_ms, 2),
                      "host_route_same_inputs_over_device_api": round(route_ms / api_ms, 2), "results_equal": True})
        # a further length in the same call: both lengths against the first alone
        for positions in (True, False):
            res = hip.ngrams(lengths, min_count=MIN_COUNT, top=TOP, order="count", spectrum=BINS, positions=positions)
            total = sum(r.size for r, _ in res)
            one = min(sized_call(hip, lengths[:1], positions, res[0][0].size) for _ in range(3))
            both = min(sized_call(hip, lengths, positions, total) for _ in range(3))
            emit({"text_bits": bits, "n": n, "lengths": lengths, "positions": positions, "first_length_call_ms": round(one, 2),
                  "all_lengths_call_ms": round(both, 2), "further_lengths_ms": round(both - one, 2)})
        hip.close()
        del bwt, lcp, sa
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
