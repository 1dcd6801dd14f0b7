#!/usr/bin/env python3
"""Whole-word ranking measurements: HipCorpusSearcher.rank(words=True) -- the context search, the filter
and fmx_corpus_rank_sets -- against rank(words=False), the parent commit's substring call, on the same queries.

    python tools/words_bench.py [--log2 28] [--reps 9] [--batches 1,64,4096] [--out profiles/words_bench.jsonl]

Input and query mix are those of tools/rank_bench.py (§26): 2^log2 bytes of the words text cut into documents of geometric
length around 16 KiB; queries of three words, one common, one mid, one rare; and the worst single query, the two-letter word
that stands in nearly every document.  For every batch size both ways run alternately in this process, all shapes warmed up
first; the times are wall-clock medians of --reps repetitions of the whole call, the searches included on both sides.  Per
line: both calls' times, the rows each located (fmx_corpus_rank_last), fmx_context_last's phases for the words call, and the
filter's rate -- the rows tested per second of its own device time, and the BWT bytes that implies (one byte per row, read
twice: once to count, once to emit).  Appends one JSON line per batch size to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K1, B, TOP = 1.2, 0.75, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--doc-mean", type=int, default=16384)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "words_bench.jsonl"))
    a = ap.parse_args()
    import ctypes
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import WORDS, make_text
    L = _lib.load()
    raw_len = 1 << a.log2
    raw = make_text(torch, raw_len, 1, "cuda")
    rng = np.random.default_rng(5)
    lens = rng.geometric(1.0 / a.doc_mean, size=int(raw_len / a.doc_mean * 1.5) + 16)
    ends = np.cumsum(lens).astype(np.uint64)
    ends = np.concatenate([ends[ends < raw_len], np.array([raw_len], dtype=np.uint64)])
    n_docs = int(ends.size)
    h = ctypes.c_void_p()
    torch.cuda.synchronize()
    _lib.check(L.fmx_corpus_build_dev(raw.data_ptr(), raw_len, ends.ctypes.data, n_docs, 0, None, ctypes.byref(h)))
    del raw
    corpus = findex_amd.Corpus(h, [b"%d" % d for d in range(n_docs)])
    cs = findex_amd.HipCorpusSearcher(corpus)
    corpus.drop_stream()
    torch.cuda.empty_cache()
    cs.searcher.prepare(ktab=True, locate=True)

    words = [w for w in open(WORDS, "rb").read().split() if w.isalpha() and w.islower()]
    sample = [words[i] for i in rng.choice(len(words), min(20000, len(words)), replace=False)]
    _, sp, ep = cs._intervals(sample)
    rows = np.where(ep > sp, ep - sp, 0).astype(np.int64)
    band = lambda lo, hi: [sample[i] for i in np.nonzero((rows >= lo) & (rows <= hi))[0]]
    common, mid, rare = band(4096, 16384), band(512, 2048), band(1, 256)
    two = [w for w in set(words) if len(w) == 2]
    _, sp2, ep2 = cs._intervals(two)
    worst = two[int(np.argmax(ep2.astype(np.int64) - sp2.astype(np.int64)))]
    counts = cs.searcher.counts()
    lefts = sum(1 for c in findex_amd.boundary_class() if c >= 1 and counts[c] > 0)
    base = {"log2": a.log2, "n_docs": n_docs, "stream_len": corpus.stream_len, "top": TOP, "reps": a.reps,
            "left_bytes_that_occur": lefts}

    def measure(queries, label):
        sub = lambda: cs.rank(queries, top=TOP, k1=K1, b=B)
        wrd = lambda: cs.rank(queries, top=TOP, k1=K1, b=B, words=True)
        s_out, w_out = sub(), wrd()                              # warm both ways
        t_sub, t_wrd, p_sub, p_wrd, ctx = [], [], [], [], []
        for _ in range(a.reps):
            for fn, ts in ((sub, t_sub), (wrd, t_wrd)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t) * 1e3)
                if fn is sub:
                    p_sub.append(cs.rank_last())
                else:
                    p_wrd.append(cs.rank_last())
                    ctx.append(cs.searcher.context_last())
        med = lambda xs: float(np.median(xs))
        filter_ms = med([c[2] for c in ctx])
        tested, runs = ctx[-1][3], ctx[-1][4]
        res = dict(base)
        res.update({"what": label, "n_queries": len(queries), "n_terms": int(s_out[3].size),
                    "substring_call_ms": round(med(t_sub), 3), "words_call_ms": round(med(t_wrd), 3),
                    "substring_rows": p_sub[-1]["rows"], "words_rows": p_wrd[-1]["rows"],
                    "substring_results": int(s_out[1].size), "words_results": int(w_out[1].size),
                    "substring_locate_ms": round(med([p["locate_ms"] for p in p_sub]), 3),
                    "words_locate_ms": round(med([p["locate_ms"] for p in p_wrd]), 3),
                    "ctx_search_ms": round(med([c[0] for c in ctx]), 3), "ctx_chain_ms": round(med([c[1] for c in ctx]), 3),
                    "ctx_filter_ms": round(filter_ms, 3), "rows_tested": tested, "runs": runs,
                    "filter_rows_per_s": round(tested / max(filter_ms, 1e-6) * 1e3),
                    "filter_bwt_GBps": round(2.0 * tested / max(filter_ms, 1e-6) / 1e6, 3)})
        res["words_over_substring"] = round(res["words_call_ms"] / max(res["substring_call_ms"], 1e-9), 3)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(res) + "\n")

    for nq in [int(x) for x in a.batches.split(",") if x]:
        pick = lambda pool: pool[int(rng.integers(0, len(pool)))]
        measure([[pick(common), pick(mid), pick(rare)] for _ in range(nq)], "three words: common, mid, rare")
    measure([[worst]], "worst single query: %r, in nearly every document" % worst.decode())
    # the filter alone on the largest interval there is: every row of the index against the boundary class
    # (device form: the runs stay in HBM)
    rec = findex_amd.HipFMSearcher.pack_records(0, 1, 0, cs.searcher.n)
    cls = findex_amd.boundary_class()
    d_rec = torch.from_numpy(rec.view(np.int64)).cuda()
    d_off = torch.zeros(2, dtype=torch.int64, device="cuda")
    total = cs.searcher.context_filter_dev(d_rec.data_ptr(), 0, 1, cls, d_off.data_ptr(), 0, 0)
    d_out = torch.empty(3 * max(total, 1), dtype=torch.int64, device="cuda")
    ms = []
    for _ in range(a.reps + 1):
        cs.searcher.context_filter_dev(d_rec.data_ptr(), 0, 1, cls, d_off.data_ptr(), d_out.data_ptr(), total)
        ms.append(cs.searcher.context_last())
    ms = ms[1:]
    f_ms = float(np.median([m[2] for m in ms]))
    res = dict(base)
    res.update({"what": "the filter alone: one record [0, n), the boundary class", "ctx_filter_ms": round(f_ms, 3),
                "rows_tested": ms[-1][3], "runs": ms[-1][4], "filter_rows_per_s": round(ms[-1][3] / f_ms * 1e3),
                "filter_bwt_GBps": round(2.0 * ms[-1][3] / f_ms / 1e6, 3)})
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    cs.close()


if __name__ == "__main__":
    main()
