#!/usr/bin/env python3
"""Ranked retrieval measurements: fmx_corpus_rank against what a caller did before it existed -- the
document listing per term, every (document, count) pair over PCIe, BM25 in numpy and np.lexsort per query.

    python tools/rank_bench.py [--log2 28] [--reps 9] [--batches 1,64,4096] [--out profiles/rank_bench.jsonl]

Input: 2^log2 bytes of the words text of tools/text_bwt.py, cut into documents of geometric length around 16 KiB, as
tools/corpus_bench.py cuts it.  Queries of three words drawn from the text's own words by their frequency in the text
(rows of the word's interval, counted for a sample of 20 000 words): one common (4096 .. 16384 rows), one mid (512 .. 2048),
one rare (1 .. 256); top = 10.  For every batch size both ways run alternately in this process, all shapes warmed up first;
the outputs are compared before anything is timed (same documents, bit-equal scores); the times are wall-clock medians of
--reps repetitions of the whole call, the search for the terms' intervals included on both sides.  One more line: the worst
single query, one two-letter word that occurs in nearly every document, with the selection's share of the call.  Appends
one JSON line per batch size to --out.  Per-kernel times come from a run of this script under `rocprofv3 --kernel-trace
--stats`, in a run of its own.
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


def yardstick(cs, queries, raw_len, avglen, weights=None):
    """The parent commit's way: list_docs for the batch's terms, then numpy.  -> (off, doc, score, d2h bytes)."""
    terms = [t for q in queries for t in q]
    off, doc, cnt = cs.list_docs(terms)
    d2h = off.nbytes + doc.nbytes + cnt.nbytes
    off = off.astype(np.int64)
    n_docs = raw_len.size
    df = np.diff(off)
    w = np.log(1.0 + ((n_docs - df).astype(np.float64) + 0.5) / (df.astype(np.float64) + 0.5)) if weights is None else weights
    nd_all = K1 * ((1.0 - B) + B * (raw_len.astype(np.float64) / avglen))
    o_off, o_doc, o_score, t = [0], [], [], 0
    for q in queries:
        lists = [(doc[off[t + s]:off[t + s + 1]], cnt[off[t + s]:off[t + s + 1]], w[t + s]) for s in range(len(q))]
        t += len(q)
        docs = np.unique(np.concatenate([d for d, _, _ in lists])) if lists else np.zeros(0, np.uint32)
        score = np.zeros(docs.size, dtype=np.float64)
        for d, c, wt in lists:
            at = np.searchsorted(docs, d)
            tf = c.astype(np.float64)
            score[at] = score[at] + wt * ((tf * (K1 + 1.0)) / (tf + nd_all[d]))
        order = np.lexsort((docs, -score))[:TOP]
        o_doc.append(docs[order])
        o_score.append(score[order])
        o_off.append(o_off[-1] + order.size)
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
    return np.array(o_off, dtype=np.uint64), cat(o_doc, np.uint32), cat(o_score, np.float64), d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--doc-mean", type=int, default=16384)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.jsonl"))
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
    _, doc_raw_len, _ = corpus.tables()
    avglen = float(corpus.stream_len - n_docs - corpus.n_esc) / float(n_docs)

    # the text's own words by frequency: the rows of a sample's intervals
    words = [w for w in open(WORDS, "rb").read().split() if w.isalpha() and w.islower()]
    sample = [words[i] for i in rng.choice(len(words), min(20000, len(words)), replace=False)]
    _, sp, ep = cs._intervals(sample)
    rows = np.where(ep > sp, ep - sp, 0).astype(np.int64)
    band = lambda lo, hi: [sample[i] for i in np.nonzero((rows >= lo) & (rows <= hi))[0]]
    common, mid, rare = band(4096, 16384), band(512, 2048), band(1, 256)
    two = [w for w in set(words) if len(w) == 2]
    _, sp2, ep2 = cs._intervals(two)
    worst = two[int(np.argmax(ep2.astype(np.int64) - sp2.astype(np.int64)))]
    base = {"log2": a.log2, "n_docs": n_docs, "stream_len": corpus.stream_len, "top": TOP, "k1": K1, "b": B, "reps": a.reps,
            "bands": {"common": len(common), "mid": len(mid), "rare": len(rare)}}

    def measure(queries, label):
        new = lambda: cs.rank(queries, top=TOP, k1=K1, b=B)
        old = lambda: yardstick(cs, queries, doc_raw_len, avglen)
        # warm both ways, then compare: the same documents, bit-equal scores (the yardstick scored with the library's weights)
        off, doc, score, df, w = new()
        old()
        y_off, y_doc, y_score, y_d2h = yardstick(cs, queries, doc_raw_len, avglen, weights=w)
        equal = bool(np.array_equal(off, y_off) and np.array_equal(doc, y_doc) and
                     np.array_equal(score.view(np.uint64), y_score.view(np.uint64)))
        w_own = np.log(1.0 + ((n_docs - df.astype(np.int64)).astype(np.float64) + 0.5) / (df.astype(np.float64) + 0.5))
        t_new, t_old, phases = [], [], []
        for _ in range(a.reps):
            for fn, ts in ((new, t_new), (old, t_old)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t) * 1e3)
                if fn is new:
                    phases.append(cs.rank_last())
        med = {k: float(np.median([p[k] for p in phases])) for k in ("locate_ms", "postings_ms", "score_ms", "select_ms")}
        res = dict(base)
        res.update({"what": label, "n_queries": len(queries), "n_terms": int(df.size), "outputs_equal": equal,
                    "weights_bit_equal_to_numpy": bool(np.array_equal(w.view(np.uint64), w_own.view(np.uint64))),
                    "rank_call_ms": round(float(np.median(t_new)), 3), "yardstick_call_ms": round(float(np.median(t_old)), 3),
                    "locate_ms": round(med["locate_ms"], 3), "postings_ms": round(med["postings_ms"], 3),
                    "score_ms": round(med["score_ms"], 3), "select_ms": round(med["select_ms"], 3),
                    "rows": phases[-1]["rows"], "postings": phases[-1]["postings"], "candidates": phases[-1]["candidates"],
                    "rank_d2h_bytes": int(off.nbytes + doc.nbytes + score.nbytes + df.nbytes + w.nbytes), "yardstick_d2h_bytes": int(y_d2h)})
        res["speedup"] = round(res["yardstick_call_ms"] / res["rank_call_ms"], 2)
        res["select_share_of_device_ms"] = round(med["select_ms"] / max(sum(med.values()), 1e-9), 3)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(res) + "\n")

    for nq in [int(x) for x in a.batches.split(",") if x]:
        pick = lambda pool: pool[int(rng.integers(0, len(pool)))]
        measure([[pick(common), pick(mid), pick(rare)] for _ in range(nq)], "three words: common, mid, rare")
    measure([[worst]], "worst single query: %r, in nearly every document" % worst.decode())
    cs.close()


if __name__ == "__main__":
    main()
