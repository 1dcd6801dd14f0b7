#!/usr/bin/env python3
"""Approximate-search measurements: patterns per second, hits, executed backward steps and rank-dictionary
requests of fmx_search_approx_batch_dev, and for e = 0 the ratio to fmx_search_batch_dev on the same handle with every
derived table off.

    python tools/approx_bench.py words30|iid28 [--k 100000] [--reps 5] [--out profiles/approx_bench.jsonl]

words30: 2^30 bytes of the words text of tools/text_bwt.py; iid28: 2^28 i.i.d. bytes over four letters.  Both indexes are
built by fmx_bwt_from_text_dev.  Batches: k patterns of 16 and of 32 bytes taken from the index by LF walks (so each occurs),
0 - 3 of their bytes replaced, at e = 0, 1, 2.  One JSON line per (length, e) is printed and appended to --out.
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

REQUEST_CEILING = 46.5e9        # tools/ubench/mix.hip, distinct rank-line requests per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input", choices=["words30", "iid28"])
    ap.add_argument("--k", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budgets", default="0,1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_bench.jsonl"))
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
        letters = np.arange(97, 123)
    else:
        length = 1 << 28
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        text = torch.randint(97, 101, (length,), dtype=torch.uint8, device=dev, generator=g)
        letters = np.arange(97, 101)
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), None, ctypes.byref(eof),
                                       counts.ctypes.data, 0, None))
    del text
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    hip.config_set("jump", "off")            # rank_only: the exact search this is compared with steps on the dictionary too
    hip.config_set("ktab", "off")
    torch.cuda.synchronize()
    head = {"input": a.input, "n": n, "layout": hip.stats()["layout"], "index_s": round(time.time() - t0, 2), "k": a.k}
    print(json.dumps(head), flush=True)
    rng = np.random.default_rng(5)
    k = a.k
    lines = []
    for m in (16, 32):
        # LF walks emit the pattern's bytes last one first; replace 0 - 3 bytes (pattern j: j % 4 of them)
        walked, _ = hip.lf_walk_batch(rng.integers(0, n, k, dtype=np.uint64), m)
        pats = np.ascontiguousarray(walked[:, ::-1])
        pats[pats == 0] = letters[0]                                      # a walk that passed the EOF row
        order = np.argsort(rng.random((k, m)), axis=1)
        for t in range(3):
            sel = np.nonzero(np.arange(k) % 4 > t)[0]
            pats[sel, order[sel, t]] = rng.choice(letters, sel.size)
        d_pat = torch.from_numpy(pats.reshape(-1)).to(dev)
        d_off = torch.arange(0, (k + 1) * m, m, dtype=torch.int64, device=dev)
        d_sp = torch.empty(k, dtype=torch.int64, device=dev)
        d_ep = torch.empty(k, dtype=torch.int64, device=dev)
        d_out_off = torch.empty(k + 1, dtype=torch.int64, device=dev)
        # the exact search of the same batch: its time and its steps
        hip.search_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(), k)       # warm
        torch.cuda.synchronize()
        hip.stats_reset()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.search_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(), k)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        exact_ms = float(np.median(ts))
        exact_steps = hip.stats()["backward_steps"] // a.reps
        for e in [int(x) for x in a.budgets.split(",")]:
            opts = _lib.fmx_approx_opts(e, 0, 0, 0)
            n_out = ctypes.c_size_t()
            rc = L.fmx_search_approx_batch_dev(hip.handle, d_pat.data_ptr(), d_off.data_ptr(), k, ctypes.byref(opts),
                                               d_out_off.data_ptr(), None, 0, ctypes.byref(n_out), None)      # the counting call
            if rc != 9:
                _lib.check(rc)
            total = int(n_out.value)
            d_out = torch.empty(max(total, 1) * 24, dtype=torch.uint8, device=dev)
            search, sort, wall = [], [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                got = hip.search_approx_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, e, d_out_off.data_ptr(), d_out.data_ptr(), total)
                wall.append((time.perf_counter() - t) * 1e3)
                s_ms, o_ms, steps, reqs = hip.approx_last()
                search.append(s_ms)
                sort.append(o_ms)
                assert got == total
            s_ms, o_ms, w_ms = float(np.median(search)), float(np.median(sort)), float(np.median(wall))
            r = {"input": a.input, "n": n, "k": k, "m": m, "e": e, "hits": total, "search_ms": round(s_ms, 4),
                 "sort_ms": round(o_ms, 4), "call_wall_ms": round(w_ms, 4), "patterns_per_s": round(k / s_ms * 1e3),
                 "steps": steps, "requests": reqs, "requests_per_s": round(reqs / s_ms * 1e3),
                 "request_frac": round(reqs / s_ms * 1e3 / REQUEST_CEILING, 4)}
            if e == 0:
                r["exact_rank_only_ms"] = round(exact_ms, 4)
                r["exact_steps"] = int(exact_steps)
                r["steps_equal_exact"] = bool(steps == exact_steps)
                r["time_ratio_to_exact"] = round(s_ms / exact_ms, 2)
            print(json.dumps(r), flush=True)
            lines.append(r)
            del d_out
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    hip.close()


if __name__ == "__main__":
    main()
