#!/usr/bin/env python3
"""Case-folding measurements: HipCorpusSearcher.rank(ignore_case=True) -- the fold search and
fmx_corpus_rank_sets -- against rank(ignore_case=False), the parent commit's substring call, on the same queries.

    python tools/fold_bench.py [--log2 28] [--reps 9] [--batches 1,64,4096] [--upper 0.15] [--out profiles/fold_bench.jsonl]

Input and query mix are those of tools/rank_bench.py and tools/words_bench.py (§26, §27): 2^log2 bytes of the words text cut
into documents of geometric length around 16 KiB; queries of three words, one common, one mid, one rare; and the worst single
query.  The text holds almost no capitals, so a deterministic share --upper of its letters is upper-cased first (a seeded
device generator): a word of m letters then stands in up to 2^m spellings.  For every batch size both ways run alternately
in this process, all shapes warmed up first; the times are wall-clock medians of --reps repetitions of the whole call, the
searches included on both sides.  Per line: both calls' times, the rows each located (fmx_corpus_rank_last), the variants the
fold search found and fmx_fold_last's figures (search kernel ms, ordering ms, backward steps, requests), and the same batch of
terms through fmx_search_fold_batch_dev and through fmx_search_approx_batch_dev at e = 0, the yardstick for the kernel's
device time.  One relation is checked, not timed: with the identity map the fold search makes exactly the backward steps of
the exact search on the rank dictionary for the batch (counted by the approximate search at e = 0, §15).  Appends one JSON line per batch size to --out.
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

K1, B, TOP = 1.2, 0.75, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--doc-mean", type=int, default=16384)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--upper", type=float, default=0.15, help="share of the letters that is upper-cased")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import WORDS, make_text
    L = _lib.load()
    raw_len = 1 << a.log2
    raw = make_text(torch, raw_len, 1, "cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(28)
    step = 1 << 26
    for lo in range(0, raw_len, step):                           # upper-case a share of the letters, a piece at a time
        piece = raw[lo:lo + step]
        up = (torch.rand(piece.numel(), generator=g, device="cuda") < a.upper) & (piece >= 97) & (piece <= 122)
        piece -= up.to(torch.uint8) * 32
    capitals = int(((raw >= 65) & (raw <= 90)).sum().item())
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
    hip = cs.searcher
    hip.prepare(ktab=True, locate=True)

    words = [w for w in open(WORDS, "rb").read().split() if w.isalpha() and w.islower()]
    sample = [words[i] for i in rng.choice(len(words), min(20000, len(words)), replace=False)]
    # the bands of §26 by the rows of a word in ANY spelling: what the folded query locates
    off = np.zeros(len(sample) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w in sample])
    v_off, hits = hip.search_fold_batch(np.frombuffer(b"".join(w[::-1] for w in sample), dtype=np.uint8), off)
    rows = np.bincount(hits["regex"], weights=(hits["ep"] - hits["sp"]).astype(np.float64), minlength=len(sample)).astype(np.int64)
    band = lambda lo, hi: [sample[i] for i in np.nonzero((rows >= lo) & (rows <= hi))[0]]
    common, mid, rare = band(4096, 16384), band(512, 2048), band(1, 256)
    two = [w for w in set(words) if len(w) == 2]
    worst = two[int(np.argmax([sum(b - s for s, b in hip.search_fold(w[::-1])) for w in two]))]
    base = {"log2": a.log2, "n_docs": n_docs, "stream_len": corpus.stream_len, "top": TOP, "reps": a.reps, "upper": a.upper,
            "capitals": capitals}

    def device_batch(terms):
        esc = [findex_amd.escape(t)[::-1] for t in terms]
        o = np.zeros(len(esc) + 1, dtype=np.uint64)
        o[1:] = np.cumsum([len(e) for e in esc])
        buf = np.frombuffer(b"".join(esc), dtype=np.uint8).copy()
        return buf, o, torch.from_numpy(buf).cuda(), torch.from_numpy(o.view(np.int64)).cuda()

    def kernels_alone(terms):
        """The batch of terms through the fold search (ASCII map, then the identity map) and through the approximate search at
        e = 0, device forms: medians of the kernels' own device times, and the steps."""
        _, _, d_pat, d_off = device_batch(terms)
        k = len(terms)
        d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
        n_out = ctypes.c_size_t()
        L.fmx_search_fold_batch_dev(hip.handle, d_pat.data_ptr(), d_off.data_ptr(), k, None, d_out_off.data_ptr(), None, 0, ctypes.byref(n_out), None)
        total = int(n_out.value)
        d_out = torch.empty(3 * max(total, k, 1), dtype=torch.int64, device="cuda")
        out = {"variants": total}
        for name, fold in (("fold", findex_amd.ASCII_FOLD), ("identity", bytes(range(256)))):
            ms = []
            for _ in range(a.reps + 1):
                hip.search_fold_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), max(total, k, 1), fold=fold)
                ms.append(hip.fold_last())
            ms = ms[1:]
            out.update({name + "_search_ms": round(float(np.median([m[0] for m in ms])), 4),
                        name + "_sort_ms": round(float(np.median([m[1] for m in ms])), 4), name + "_steps": ms[-1][2], name + "_requests": ms[-1][3]})
        ms = []
        for _ in range(a.reps + 1):
            hip.search_approx_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 0, d_out_off.data_ptr(), d_out.data_ptr(), max(total, k, 1))
            ms.append(hip.approx_last())
        ms = ms[1:]
        out.update({"approx_e0_search_ms": round(float(np.median([m[0] for m in ms])), 4),
                    "approx_e0_sort_ms": round(float(np.median([m[1] for m in ms])), 4), "approx_e0_steps": ms[-1][2]})
        # the relation: the identity map makes the exact search's steps.  This handle's exact search is served by its tables, so
        # the count here is the approximate search's at e = 0, which §15 holds to the exact search on the rank dictionary
        # (tests/test_gpu_fold.py holds the fold search to fmx_search_batch itself, tables off)
        out["identity_steps_equal_exact_steps"] = bool(out["identity_steps"] == out["approx_e0_steps"])
        return out

    def measure(queries, label):
        sub = lambda: cs.rank(queries, top=TOP, k1=K1, b=B)
        fld = lambda: cs.rank(queries, top=TOP, k1=K1, b=B, ignore_case=True)
        s_out, f_out = sub(), fld()                              # warm both ways
        t_sub, t_fld, p_sub, p_fld, last = [], [], [], [], []
        for _ in range(a.reps):
            for fn, ts in ((sub, t_sub), (fld, t_fld)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t) * 1e3)
                if fn is sub:
                    p_sub.append(cs.rank_last())
                else:
                    p_fld.append(cs.rank_last())
                    last.append(hip.fold_last())
        med = lambda xs: float(np.median(xs))
        res = dict(base)
        res.update({"what": label, "n_queries": len(queries), "n_terms": int(s_out[3].size),
                    "substring_call_ms": round(med(t_sub), 3), "ignore_case_call_ms": round(med(t_fld), 3),
                    "substring_rows": p_sub[-1]["rows"], "ignore_case_rows": p_fld[-1]["rows"],
                    "substring_results": int(s_out[1].size), "ignore_case_results": int(f_out[1].size),
                    "substring_locate_ms": round(med([p["locate_ms"] for p in p_sub]), 3),
                    "ignore_case_locate_ms": round(med([p["locate_ms"] for p in p_fld]), 3),
                    "in_call_search_ms": round(med([x[0] for x in last]), 4), "in_call_sort_ms": round(med([x[1] for x in last]), 4),
                    "in_call_steps": last[-1][2], "in_call_requests": last[-1][3]})
        res.update(kernels_alone([t for q in queries for t in q]))
        res["ignore_case_over_substring"] = round(res["ignore_case_call_ms"] / max(res["substring_call_ms"], 1e-9), 3)
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
