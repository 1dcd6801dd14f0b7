#!/usr/bin/env python3
"""Matching-statistics measurements: executed backward steps, rank-dictionary requests and device time of
fmx_match_stats_batch (the walk kernel) and of fmx_mems_batch's compaction for two 1 MiB queries, beside the device time of
what the library offered before for the same answer: a binary search on the length per query position, each round one
fmx_search_batch_dev call over one pattern per query byte (the caller gathers the patterns; only the search calls' device
time is counted).

    python tools/mstat_bench.py [--log2 28] [--query 1048576] [--max-len 4096] [--reps 3] [--out profiles/mstat_bench.jsonl]

The text is 2^log2 bytes of the words text of tools/text_bwt.py, indexed by fmx_bwt_from_text_dev (the index of
reverse(text), so a query is handed over reversed).  Queries: `like_text`, bytes drawn like the text from another seed
(short walks), and `copy`, a stretch of the text with one substituted byte about every 200 (long walks, uneven per wave).
One JSON line per query is printed and appended to --out.
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

REQUEST_CEILING = 46.5e9        # README: distinct rank-line requests per second of this access pattern
CHUNK_BYTES = 1 << 28           # pattern bytes per search call of the rounds


def rounds_by_search(torch, hip, d_q, limit):
    """len[j] by binary search: lo = a length known to occur, hi = the largest that may; a round searches the suffix of
    length (lo + hi + 1) / 2 of every position that is still open.  -> (len int64 tensor, device ms of the search calls,
    rounds, patterns searched, pattern bytes gathered)."""
    dev = d_q.device
    nb = d_q.numel()
    lo = torch.zeros(nb, dtype=torch.int64, device=dev)
    hi = limit.clone()
    ms, rounds, searched, gathered = 0.0, 0, 0, 0
    while True:
        open_ = torch.nonzero(lo < hi).reshape(-1)
        if open_.numel() == 0:
            break
        rounds += 1
        mid_all = (lo[open_] + hi[open_] + 1) // 2
        csum = torch.cumsum(mid_all, 0)
        a = 0
        while a < open_.numel():
            # as many positions as CHUNK_BYTES pattern bytes hold
            base = int(csum[a - 1]) if a else 0
            b = int(torch.searchsorted(csum, torch.tensor([base + CHUNK_BYTES], device=dev), right=True)[0])
            b = max(b, a + 1)
            pos, mid = open_[a:b], mid_all[a:b]
            k = pos.numel()
            off = torch.zeros(k + 1, dtype=torch.int64, device=dev)
            off[1:] = torch.cumsum(mid, 0)
            total = int(off[-1])
            owner = torch.repeat_interleave(torch.arange(k, device=dev), mid)
            src = pos[owner] - mid[owner] + 1 + (torch.arange(total, device=dev) - off[:-1][owner])
            pat = d_q[src]
            del owner, src
            sp = torch.empty(k, dtype=torch.int64, device=dev)
            ep = torch.empty(k, dtype=torch.int64, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.search_batch_dev(pat.data_ptr(), off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k)
            e1.record()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            found = sp < ep
            lo[pos[found]] = mid[found]
            hi[pos[~found]] = mid[~found] - 1
            searched += k
            gathered += total
            a = b
    return lo, ms, rounds, searched, gathered


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--query", type=int, default=1 << 20)
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mstat_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import make_text
    L = _lib.load()
    dev = "cuda"
    t0 = time.time()
    length = 1 << a.log2
    text = make_text(torch, length, 1, dev)
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), None, ctypes.byref(eof),
                                       counts.ctypes.data, 0, None))
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    torch.cuda.synchronize()
    head = {"text": "words", "n": n, "layout": hip.stats()["layout"], "index_s": round(time.time() - t0, 2),
            "query_bytes": a.query, "max_len": a.max_len}
    print(json.dumps(head), flush=True)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    copy = text[length // 3: length // 3 + a.query].clone()
    where = torch.arange(100, a.query, 200, device=dev) + torch.randint(-60, 61, ((a.query - 100 + 199) // 200,), device=dev, generator=g)
    copy[where] = ((copy[where].to(torch.int64) - 97 + 1 + torch.randint(0, 24, (where.numel(),), device=dev, generator=g)) % 26 + 97).to(torch.uint8)
    queries = {"like_text": make_text(torch, a.query, 77, dev), "copy": copy}
    del text
    hip.prepare(ktab=True, jump=True, search=True)           # the exact search of the rounds with every table it can have
    lines = []
    for name, fwd in queries.items():
        d_q = torch.flip(fwd, dims=[0]).contiguous()         # the index holds reverse(text)
        nb = d_q.numel()
        d_off = torch.tensor([0, nb], dtype=torch.int64, device=dev)
        d_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        d_sp = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_ep = torch.zeros(nb, dtype=torch.int64, device=dev)
        d_out_off = torch.zeros(2, dtype=torch.int64, device=dev)
        walk, enq = [], []
        q_host, off_host = d_q.cpu().numpy(), np.array([0, nb], dtype=np.uint64)
        for _ in range(a.reps + 1):                          # the first run is the warm-up
            hip.match_stats_batch(q_host, off_host, a.max_len, intervals=True)
            w_ms, _, steps, reqs = hip.mstat_last()
            walk.append(w_ms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.match_stats_batch_dev(d_q.data_ptr(), d_off.data_ptr(), 1, nb, d_len.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(),
                                      max_len=a.max_len)
            e1.record()
            torch.cuda.synchronize()
            enq.append(e0.elapsed_time(e1))
        w_ms, enq_ms = float(np.median(walk[1:])), float(np.median(enq[1:]))
        n_out = ctypes.c_size_t()
        opts = _lib.fmx_mstat_opts(a.max_len, 20, (0, 0))
        rc = L.fmx_mems_batch_dev(hip.handle, d_q.data_ptr(), d_off.data_ptr(), 1, nb, ctypes.byref(opts), d_out_off.data_ptr(), None, 0,
                                  ctypes.byref(n_out), None)
        if rc != 9:
            _lib.check(rc)
        _, compact_ms, _, _ = hip.mstat_last()
        limit = torch.clamp(torch.arange(1, nb + 1, dtype=torch.int64, device=dev), max=a.max_len)
        rounds_by_search(torch, hip, d_q[: 1 << 14], limit[: 1 << 14])      # warm-up
        lens, r_ms, rounds, searched, gathered = rounds_by_search(torch, hip, d_q, limit)
        same = bool(torch.equal(lens, d_len.to(torch.int64)))
        ln = d_len.to(torch.int64)
        r = {"query": name, "n": n, "query_bytes": nb, "max_len": a.max_len, "steps": steps, "requests": reqs,
             "walk_ms": round(w_ms, 4), "enqueue_form_ms": round(enq_ms, 4), "positions_per_s": round(nb / w_ms * 1e3),
             "requests_per_s": round(reqs / w_ms * 1e3), "request_frac": round(reqs / w_ms * 1e3 / REQUEST_CEILING, 4),
             "mean_len": round(float(ln.double().mean()), 2), "max_len_seen": int(ln.max()), "mems_min20": int(n_out.value),
             "compact_ms": round(compact_ms, 4), "rounds_ms": round(r_ms, 4), "rounds": rounds, "rounds_patterns": searched,
             "rounds_pattern_bytes": gathered, "rounds_equal": same, "rounds_over_walk": round(r_ms / w_ms, 2)}
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    hip.close()


if __name__ == "__main__":
    main()
