#!/usr/bin/env python3
"""Corpus measurements: the stream build against the suffix sort of the same stream, the position map, and
the document listing split into its phases.

    python tools/corpus_bench.py [--log2 30] [--reps 5] [--out profiles/corpus_bench.jsonl]

Input: 2^log2 bytes of the words text of tools/text_bwt.py, cut into documents of geometric length around 16 KiB, with 1 % of
the bytes replaced by 0, 1 or 255.  Appends one JSON line to --out.  Kernel times per kernel come from a run of this script
under `rocprofv3 --kernel-trace --stats` (profiles/corpus_kernels.txt); the times here are device events around whole calls.
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

HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--doc-mean", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corpus_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import make_text
    L = _lib.load()
    dev = "cuda"
    raw_len = 1 << a.log2
    raw = make_text(torch, raw_len, 1, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    hit = torch.rand(raw_len, generator=g, device=dev) < 0.01
    vals = torch.tensor([0, 1, 255], dtype=torch.uint8, device=dev)[torch.randint(0, 3, (raw_len,), generator=g, device=dev)]
    raw = torch.where(hit, vals, raw)
    del hit, vals
    rng = np.random.default_rng(5)
    lens = rng.geometric(1.0 / a.doc_mean, size=int(raw_len / a.doc_mean * 1.5) + 16)
    ends = np.cumsum(lens).astype(np.uint64)
    ends = ends[ends < raw_len]
    ends = np.concatenate([ends, np.array([raw_len], dtype=np.uint64)])
    n_docs = int(ends.size)
    torch.cuda.synchronize()

    def timed(fn, reps=a.reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    # ---- the stream build (the call: two small allocations, count, scan, a read-back, three allocations, emit)
    built = []

    def build():
        h = ctypes.c_void_p()
        _lib.check(L.fmx_corpus_build_dev(raw.data_ptr(), raw_len, ends.ctypes.data, n_docs, 0, None, ctypes.byref(h)))
        built.append(h)

    build()                                                       # warm: code objects, first allocations
    L.fmx_corpus_free(built.pop())
    walls = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.time()
        build()
        walls.append((time.time() - t) * 1e3)
        if len(built) > 1:
            L.fmx_corpus_free(built.pop(0))
    corpus = findex_amd.Corpus(built[0], [b"%d" % d for d in range(n_docs)])
    _, stream_len, n_esc, held, _, tile = corpus.info()
    build_call_ms = float(np.median(walls))
    model_bytes = 2.0 * raw_len + stream_len + 4.0 * n_esc + 8.0 * n_docs
    res = {"log2": a.log2, "raw_len": raw_len, "n_docs": n_docs, "stream_len": stream_len, "n_esc": n_esc, "tile": tile,
           "corpus_bytes": held, "build_call_ms": round(build_call_ms, 3), "build_model_bytes": model_bytes,
           "build_call_share_of_6.3TBps": round(model_bytes / (build_call_ms * 1e-3) / HBM, 4)}
    del raw

    # ---- the yardstick: the suffix sort of the same stream, same process
    d_stream, _ = corpus.stream_dev()
    n = stream_len + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    torch.cuda.synchronize()
    t = time.time()
    _lib.check(L.fmx_bwt_from_text_dev(d_stream, stream_len, d_bwt.data_ptr(), None, ctypes.byref(eof), counts.ctypes.data, 0, None))
    sort_ms = (time.time() - t) * 1e3
    res["sufsort_call_ms"] = round(sort_ms, 1)
    res["build_over_sort"] = round(build_call_ms / sort_ms, 5)
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt

    # ---- the map: 1 M random stream positions
    k_map = 1 << 20
    pos = torch.from_numpy(rng.integers(0, stream_len, k_map, dtype=np.uint64).view(np.int64)).to(dev)
    o_doc = torch.empty(k_map, dtype=torch.int32, device=dev)
    o_eo = torch.empty(k_map, dtype=torch.int64, device=dev)
    o_ro = torch.empty(k_map, dtype=torch.int64, device=dev)
    corpus.map_dev(pos.data_ptr(), k_map, o_doc.data_ptr(), o_eo.data_ptr(), o_ro.data_ptr())
    ms = timed(lambda: corpus.map_dev(pos.data_ptr(), k_map, o_doc.data_ptr(), o_eo.data_ptr(), o_ro.data_ptr()))
    steps = int(np.ceil(np.log2(n_docs + 1))) + int(np.ceil(np.log2(max(n_esc, 2)))) + 2
    res["map_1M_ms"] = round(ms, 4)
    res["map_positions_per_s"] = round(k_map / ms * 1e3)
    res["map_dependent_requests_model"] = steps

    # ---- the rows of the intervals of 100 k patterns (m = 6) taken from the stream, as tools/locate_bench.py takes them
    k, m = 100_000, 6
    at = torch.from_numpy(rng.integers(0, stream_len - m, k).astype(np.int64)).to(dev)
    hstream = corpus.stream()
    sview = torch.from_numpy(hstream).to(dev)
    pats = sview[(at[:, None] + torch.arange(m, device=dev)[None, :])].flip(1).contiguous().reshape(-1)
    del sview, hstream
    off = torch.arange(0, (k + 1) * m, m, dtype=torch.int64, device=dev)
    sp = torch.empty(k, dtype=torch.int64, device=dev)
    ep = torch.empty(k, dtype=torch.int64, device=dev)
    hip.search_batch_dev(pats.data_ptr(), off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k)
    torch.cuda.synchronize()
    total = int((ep - sp).clamp(min=0).sum().item())
    hip.prepare(ktab=False, locate=True)
    ioff = torch.empty(k + 1, dtype=torch.int64, device=dev)
    ipos = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    i_doc = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    i_eo = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    i_ro = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    hip.locate_intervals_dev(sp.data_ptr(), ep.data_ptr(), k, ioff.data_ptr(), ipos.data_ptr(), total)
    ms_loc = timed(lambda: hip.locate_intervals_dev(sp.data_ptr(), ep.data_ptr(), k, ioff.data_ptr(), ipos.data_ptr(), total))

    def locate_and_map():
        hip.locate_intervals_dev(sp.data_ptr(), ep.data_ptr(), k, ioff.data_ptr(), ipos.data_ptr(), total)
        tp = (stream_len - m) - ipos                              # text offsets: n - 1 - SA - m
        corpus.map_dev(tp.data_ptr(), total, i_doc.data_ptr(), i_eo.data_ptr(), i_ro.data_ptr())

    locate_and_map()
    ms_both = timed(locate_and_map)
    res.update({"interval_rows": total, "locate_intervals_ms": round(ms_loc, 3), "locate_rows_per_s": round(total / ms_loc * 1e3),
                "locate_plus_map_ms": round(ms_both, 3), "locate_plus_map_rows_per_s": round(total / ms_both * 1e3)})

    # ---- the listing, split by the library's own events (its temporaries take ~36 bytes per row: the map's outputs go first)
    del i_doc, i_eo, i_ro, ipos
    torch.cuda.empty_cache()
    cap = total
    l_off = torch.empty(k + 1, dtype=torch.int64, device=dev)
    l_doc = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    l_cnt = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)

    def listing():
        _lib.check(L.fmx_corpus_doc_list_dev(corpus.handle, hip.handle, sp.data_ptr(), ep.data_ptr(), k, m, 0, l_off.data_ptr(),
                                             l_doc.data_ptr(), l_cnt.data_ptr(), cap, None))

    listing()
    phases, walls = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.time()
        listing()
        walls.append((time.time() - t) * 1e3)
        p = [ctypes.c_double() for _ in range(4)]
        L.fmx_corpus_doc_list_phases(*[ctypes.byref(x) for x in p])
        phases.append([x.value for x in p])
    med = np.median(np.array(phases), axis=0)
    res.update({"list_call_ms": round(float(np.median(walls)), 3), "list_pairs": int(l_off[-1].item()),
                "list_locate_ms": round(float(med[0]), 3), "list_map_ms": round(float(med[1]), 3),
                "list_sort_ms": round(float(med[2]), 3), "list_compact_ms": round(float(med[3]), 3)})
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    hip.close()
    corpus.close()


if __name__ == "__main__":
    main()
