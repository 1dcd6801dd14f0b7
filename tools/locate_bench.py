#!/usr/bin/env python3
"""Locate measurements: build time and bytes of the locate samples, located rows per second for random
rows and for every row of the intervals of searched patterns.

    python tools/locate_bench.py words30|iid32 [--rates 8,32,128] [--out FILE]

words30: 2^30 bytes of the words text of tools/text_bwt.py; iid32: 2^32 - 2 i.i.d. bytes 1..128.  Both indexes are built
by fmx_bwt_from_text_dev.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input", choices=["words30", "iid32"])
    ap.add_argument("--rates", default="8,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    L = _lib.load()
    dev = "cuda"
    t0 = time.time()
    if a.input == "words30":
        from text_bwt import make_text
        length = 1 << 30
        text = make_text(torch, length, 1, dev)
    else:
        length = (1 << 32) - 2
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        text = torch.randint(1, 129, (length,), dtype=torch.uint8, device=dev, generator=g)
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), None, ctypes.byref(eof),
                                       counts.ctypes.data, 0, None))
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    torch.cuda.synchronize()
    res = {"input": a.input, "n": n, "layout": hip.stats()["layout"], "index_s": round(time.time() - t0, 2),
           "rates": {}}
    # patterns: 100 000 substrings of the text (length 6), reversed for the search
    rng = np.random.default_rng(3)
    k = 100_000
    m = 6
    at = torch.from_numpy(rng.integers(0, length - m, k).astype(np.int64)).to(dev)
    pats = text[(at[:, None] + torch.arange(m, device=dev)[None, :])].flip(1).contiguous().reshape(-1)
    del text
    off = torch.arange(0, (k + 1) * m, m, dtype=torch.int64, device=dev)
    sp = torch.empty(k, dtype=torch.int64, device=dev)
    ep = torch.empty(k, dtype=torch.int64, device=dev)
    hip.search_batch_dev(pats.data_ptr(), off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k)
    torch.cuda.synchronize()
    total = int((ep - sp).clamp(min=0).sum().item())
    rows = torch.from_numpy(rng.integers(0, n, 1 << 20, dtype=np.uint64).view(np.int64)).to(dev)
    out = torch.empty(rows.numel(), dtype=torch.int64, device=dev)
    ioff = torch.empty(k + 1, dtype=torch.int64, device=dev)
    ipos = torch.empty(max(total, 1), dtype=torch.int64, device=dev)

    def timed(fn):
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    for s in [int(x) for x in a.rates.split(",")]:
        hip.config_set("locate_sample", s)
        hip.drop_tables(jump=False, frontier=False, locate=True)
        torch.cuda.synchronize()
        t = time.time()
        hip.prepare(ktab=False, locate=True)
        wall = time.time() - t
        rate, nbytes, ms = hip.locate_info()
        hip.locate_dev(rows.data_ptr(), rows.numel(), out.data_ptr())          # warm
        ms_rows = timed(lambda: hip.locate_dev(rows.data_ptr(), rows.numel(), out.data_ptr()))
        ms_iv = timed(lambda: hip.locate_intervals_dev(sp.data_ptr(), ep.data_ptr(), k, ioff.data_ptr(), ipos.data_ptr(), total))
        r = {"build_ms": round(ms, 1), "build_wall_s": round(wall, 3), "bytes": nbytes,
             "random_1M_ms": round(ms_rows, 3), "random_rows_per_s": round(rows.numel() / ms_rows * 1e3),
             "intervals_100k_rows": total, "intervals_ms": round(ms_iv, 3),
             "interval_rows_per_s": round(total / ms_iv * 1e3) if total else 0}
        res["rates"][str(s)] = r
        print(json.dumps({"rate": s, **r}), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    hip.close()


if __name__ == "__main__":
    main()
