#!/usr/bin/env python3
"""Passage measurements: rank_passages -- one term search, the ranking, fmx_corpus_passages -- against what
a caller did before it existed: rank, then locate_docs for every distinct term of the batch (every occurrence in the whole
corpus over PCIe), then numpy restricted to the hit files, sliding the same windows.

    python tools/passages_bench.py [--log2 28] [--reps 9] [--batches 1,64,4096] [--window 160] [--out profiles/passages_bench.jsonl]

Corpus and queries are those of tools/rank_bench.py: 2^log2 bytes of the words text cut into documents of geometric length
around 16 KiB, queries of one common, one mid and one rare word, top = 10; one more line for the worst single query, the
two-letter word that occurs in nearly every document.  The text holds no escaped byte, so the yardstick's stream position of
an occurrence is doc_start + raw offset.  For every batch size both ways run alternately in this process, all shapes warmed
up first; the outputs are compared before anything is timed (records and counts, values bit for bit); the times are wall-clock
medians of --reps repetitions of the whole call with the profiler off.  The ranking alone is timed in the same rotation, so
the reader sees what the passages add to it.  Appends one JSON line per batch size to --out.
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


def best_window(occ, lens, weights, window, sep):
    """One hit in numpy.  occ[s]: the ascending stream positions of slot s' occurrences in the file, lens[s] their length,
    sep the file's separator.  -> (a, mask, value, b, n_occ), or None without occurrences."""
    starts = np.unique(np.concatenate(occ)) if occ else np.zeros(0, np.uint64)
    if starts.size == 0:
        return None
    value = np.zeros(starts.size, dtype=np.float64)
    mask = np.zeros(starts.size, dtype=np.uint64)
    for s, f in enumerate(occ):
        if f.size == 0:
            continue
        x = np.searchsorted(f, starts)
        covered = (x < f.size) & (f[np.minimum(x, f.size - 1)] + np.uint64(lens[s]) <= starts + np.uint64(window))
        value = np.where(covered, value + weights[s], value)          # slot order: one addition per covered slot
        mask |= covered.astype(np.uint64) << np.uint64(s)
    i = int(np.argmax(value))                                          # the first of equal values: the smallest start
    a = int(starts[i])
    return a, int(mask[i]), float(value[i]), min(a + window, sep), int(sum(f.size for f in occ))


def yardstick(cs, queries, window, doc_start, rank_out=None):
    """The parent commit's way.  -> (off, doc, score, records, tf, d2h bytes).  rank_out: a ranking to explain instead of
    ranking here (the comparison uses the new call's own, so that both ways see the same weights)."""
    off, doc, score, df, w = rank_out if rank_out is not None else cs.rank(queries, top=TOP, k1=K1, b=B)
    d2h = off.nbytes + doc.nbytes + score.nbytes + df.nbytes + w.nbytes
    where = {}
    for t in {t for q in queries for t in q}:
        d, raw = cs.locate_docs(t)
        d2h += d.size * (8 + 4 + 8 + 8)                              # the positions, then the map's document, offset and raw offset
        where[t] = (d, doc_start[d] + raw)
    stride = max([len(q) for q in queries] + [0])
    recs = np.zeros(doc.size, dtype=cs.PASSAGE)
    tf = np.zeros((doc.size, stride), dtype=np.uint32)
    at = 0
    for i, q in enumerate(queries):
        for h in range(int(off[i]), int(off[i + 1])):
            d = int(doc[h])
            occ = []
            for t in q:
                dd, f = where[t]
                lo, hi = np.searchsorted(dd, d), np.searchsorted(dd, d, side="right")
                occ.append(f[lo:hi])
            tf[h, :len(q)] = [f.size for f in occ]
            got = best_window(occ, [len(t) for t in q], w[at:at + len(q)], window, int(doc_start[d + 1]) - 1)
            if got is not None:
                a, mask, value, b, n_occ = got
                recs[h] = (a - int(doc_start[d]), mask, value, b - a, n_occ)
        at += len(q)
    return off, doc, score, recs, tf, d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--doc-mean", type=int, default=16384)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--window", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "passages_bench.jsonl"))
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
    if corpus.n_esc:
        raise SystemExit("the yardstick takes a text without escaped bytes")
    doc_start = corpus.tables()[0].astype(np.uint64)

    words = [w for w in open(WORDS, "rb").read().split() if w.isalpha() and w.islower()]
    sample = [words[i] for i in rng.choice(len(words), min(20000, len(words)), replace=False)]
    _, sp, ep = cs._intervals(sample)
    rows = np.where(ep > sp, ep - sp, 0).astype(np.int64)
    band = lambda lo, hi: [sample[i] for i in np.nonzero((rows >= lo) & (rows <= hi))[0]]
    common, mid, rare = band(4096, 16384), band(512, 2048), band(1, 256)
    two = [w for w in set(words) if len(w) == 2]
    _, sp2, ep2 = cs._intervals(two)
    worst = two[int(np.argmax(ep2.astype(np.int64) - sp2.astype(np.int64)))]
    base = {"log2": a.log2, "n_docs": n_docs, "stream_len": corpus.stream_len, "top": TOP, "window": a.window, "reps": a.reps}

    def measure(queries, label):
        new = lambda: cs.rank_passages(queries, top=TOP, window=a.window, k1=K1, b=B)
        old = lambda: yardstick(cs, queries, a.window, doc_start)
        rank = lambda: cs.rank(queries, top=TOP, k1=K1, b=B)
        # warm all three, then compare: the same records and counts, the values bit for bit
        off, doc, score, df, w, psg, tf = new()
        old()
        rank()
        _, _, _, y_psg, y_tf, y_d2h = yardstick(cs, queries, a.window, doc_start, rank_out=(off, doc, score, df, w))
        equal = bool(psg.tobytes() == y_psg.tobytes() and np.array_equal(tf, y_tf))
        t_new, t_old, t_rank, phases = [], [], [], []
        for _ in range(a.reps):
            for fn, ts in ((new, t_new), (old, t_old), (rank, t_rank)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t) * 1e3)
                if fn is new:
                    phases.append(cs.passages_last())
        med = {k: float(np.median([p[k] for p in phases])) for k in ("locate_ms", "filter_ms", "sort_ms", "window_ms")}
        res = dict(base)
        res.update({"what": label, "n_queries": len(queries), "n_hits": int(doc.size), "outputs_equal": equal,
                    "rank_passages_call_ms": round(float(np.median(t_new)), 3), "yardstick_call_ms": round(float(np.median(t_old)), 3),
                    "rank_alone_call_ms": round(float(np.median(t_rank)), 3),
                    "locate_ms": round(med["locate_ms"], 3), "filter_ms": round(med["filter_ms"], 3), "sort_ms": round(med["sort_ms"], 3),
                    "window_ms": round(med["window_ms"], 3), "rows": phases[-1]["rows"], "occurrences": phases[-1]["occurrences"],
                    "max_occurrences_of_a_hit": int(psg["n_occ"].max()) if psg.size else 0,
                    "new_d2h_bytes": int(off.nbytes + doc.nbytes + score.nbytes + df.nbytes + w.nbytes + psg.nbytes + tf.nbytes),
                    "yardstick_d2h_bytes": int(y_d2h)})
        res["ratio_yardstick_over_new"] = round(res["yardstick_call_ms"] / res["rank_passages_call_ms"], 2)
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
