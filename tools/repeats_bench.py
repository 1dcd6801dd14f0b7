#!/usr/bin/env python3
"""Repeats measurements: fmx_repeats on texts of tools/text_bwt.py at L = 32 in both modes -- the four
phase times of fmx_repeats_last, the bytes each phase must move and the rate that makes, the summary -- beside the route a
caller had before the call existed, measured in the same run on the same handle: hip.lcp() and the full suffix array (X.sa,
fmx_write_sa) brought to the host, 8 n bytes, then the passes in numpy.  The two results are asserted equal.

    python tools/repeats_bench.py [--bits 24,28] [--min-len 32] [--out profiles/repeats_bench.jsonl]

One JSON line per text and mode, appended to --out.  Times are wall-clock around the calls (ms) unless they are named
after a phase (device events)."""
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

# bytes per row each phase must move ("the passes"): reads and writes of the streaming kernels and the scans (a
# scan reads and writes its array twice: 16).  ROW: a row of no repeated class -- it reads its LCP entries and nothing else in
# the class kernels, and its text byte is not covered; REPEATED: a row of a repeated class whose byte is covered -- SA, the
# class id, the gathered class maximum, the scattered flag byte and the numbering of its range on top.
PHASE_BYTES = {"class": 12 + 16 + 4 + 4 + 1, "cover": 5 + 16 + 8, "compact": 16 + 4}
PHASE_BYTES_REPEATED = {"class": 12 + 16 + 12 + 17 + 1, "cover": 5 + 16 + 8, "compact": 16 + 8}


def numpy_route(lcp, sa, L, later):
    """The passes of fmx_repeats.hip over the downloaded arrays, no stop byte -> (ranges, summary)"""
    n = lcp.size
    m = n - 1
    ge = lcp >= L                                              # rows r and r + 1 are of one class
    rep = ge.copy()
    rep[1:] |= ge[:-1]
    head = np.ones(n, dtype=bool)
    head[1:] = ~ge[:-1]
    rows = np.flatnonzero(rep)
    zero = dict(ranges=0, covered_bytes=0, classes=0, windows=0, largest_class=0, largest_class_pos=0)
    if rows.size == 0:
        return np.zeros((0, 2), dtype=np.uint64), zero
    cid = np.cumsum(head, dtype=np.int64)[rows]
    p = sa[rows].astype(np.int64)
    bounds = np.flatnonzero(np.concatenate(([True], cid[1:] != cid[:-1])))
    size = np.diff(np.concatenate((bounds, [cid.size])))
    cmax = np.maximum.reduceat(p, bounds)
    flagged = p != np.repeat(cmax, size) if later else np.ones(p.size, dtype=bool)
    starts = m - L - p[flagged]
    delta = np.bincount(starts, minlength=m + 1) - np.bincount(starts + L, minlength=m + 1)
    cov = np.cumsum(delta[:m]) > 0
    edge = np.diff(np.concatenate(([0], cov.astype(np.int8), [0])))
    ranges = np.stack([np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)], axis=1).astype(np.uint64)
    largest = int(size.max())
    return ranges, dict(ranges=int(ranges.shape[0]), covered_bytes=int(cov.sum()), classes=int(size.size), windows=int(starts.size),
                        largest_class=largest, largest_class_pos=int((m - L - cmax[size == largest]).min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="24,28")
    ap.add_argument("--min-len", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeats_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import make_text
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    L = a.min_len
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for bits in [int(b) for b in a.bits.split(",")]:
        text = make_text(torch, 1 << bits, 1, dev)
        length = text.numel()
        n = length + 1
        bwt = torch.empty(n, dtype=torch.uint8, device=dev)
        eof, counts = findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), 0, device=0, stream=st)
        del text
        torch.cuda.empty_cache()
        hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, counts)
        hip.prepare(ktab=False, lcp=True)                      # both routes start from a handle that has its LCP array
        lcp_build_ms = hip.lcp_info()[1]
        # the route of a caller without the call: the two arrays over the link, once for both modes
        t0 = time.perf_counter()
        lcp = hip.lcp()
        with tempfile.TemporaryDirectory() as tmp:
            hip.write_sa(os.path.join(tmp, "x.sa"))
            sa = np.fromfile(os.path.join(tmp, "x.sa"), dtype=">u4").astype(np.uint32)
        download_ms = (time.perf_counter() - t0) * 1e3
        lib = _lib.load()
        for later in (False, True):
            hip.repeats(L, keep_first=later)                   # warm-up
            t0 = time.perf_counter()
            ranges, summary = hip.repeats(L, keep_first=later)     # the counting call and the sized call
            api_ms = (time.perf_counter() - t0) * 1e3
            # one sized call alone, and its phases
            lv = np.array([L], dtype=np.uint32)
            opts = _lib.fmx_repeat_opts(1 if later else 0, 0, (0, 0, 0))
            off = np.zeros(2, dtype=np.uint64)
            out = np.zeros((max(ranges.shape[0], 1), 2), dtype=np.uint64)
            n_out = ctypes.c_size_t()
            t0 = time.perf_counter()
            _lib.check(lib.fmx_repeats(hip.handle, lv.ctypes.data, 1, ctypes.byref(opts), off.ctypes.data, out.ctypes.data,
                                       ranges.shape[0], ctypes.byref(n_out), None))
            call_ms = (time.perf_counter() - t0) * 1e3
            invert_ms, class_ms, cover_ms, compact_ms = hip.repeats_last()
            assert np.array_equal(out[:ranges.shape[0]], ranges)
            t0 = time.perf_counter()
            want_r, want_s = numpy_route(lcp, sa, L, later)
            passes_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(ranges, want_r) and summary == want_s, (summary, want_s)
            phases = {"class": class_ms, "cover": cover_ms, "compact": compact_ms}
            r = {"text_bits": bits, "n": n, "min_len": L, "mode": "later" if later else "all", "lcp_build_ms": round(lcp_build_ms, 1),
                 "invert_ms": round(invert_ms, 2), "class_ms": round(class_ms, 3), "cover_ms": round(cover_ms, 3),
                 "compact_ms": round(compact_ms, 3),
                 "passes_over_invert": round((class_ms + cover_ms + compact_ms) / max(invert_ms, 1e-9), 4),
                 "phase_bytes": {k: v * n for k, v in PHASE_BYTES.items()},
                 "phase_bytes_all_rows_repeated": {k: v * n for k, v in PHASE_BYTES_REPEATED.items()},
                 "rows_in_repeated_classes": summary["windows"] + (summary["classes"] if later else 0),
                 "phase_GBps": {k: round(PHASE_BYTES[k] * n / max(phases[k], 1e-9) / 1e6, 1) for k in PHASE_BYTES},
                 "summary": summary, "device_call_ms": round(call_ms, 1), "device_api_ms": round(api_ms, 1),
                 "host_route_ms": round(download_ms + passes_ms, 1), "host_download_ms": round(download_ms, 1),
                 "host_passes_ms": round(passes_ms, 1), "host_route_over_device_api": round((download_ms + passes_ms) / api_ms, 2),
                 "host_route_over_device_call": round((download_ms + passes_ms) / call_ms, 2), "results_equal": True}
            print(json.dumps(r), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")
        hip.close()
        del bwt, lcp, sa
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
