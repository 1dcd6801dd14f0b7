#!/usr/bin/env python3
"""String-class measurements.  The yardsticks are the parent commit's calls, never the new kernel:

  (a) fmx_search_fold_batch_dev on a batch of ASCII terms under the ASCII fold map, against fmx_search_classes_batch_dev on the
      same terms with the same map written as a class table: the outputs compared byte for byte first, then both kernels'
      device ms, ordering ms, backward steps and requests;
  (b) host enumeration of every spelling of a term through fmx_search_batch (HipFMSearcher.search_batch), for terms whose
      number of spellings stays at most --max-spellings, against one class search of the same terms: the same set of
      non-empty intervals first, then wall-clock times of both;
  (c) HipCorpusSearcher.rank(ignore_case=True) against rank(ignore_case="unicode"), whole calls, the pruning search of the
      members counted inside the second.

    python tools/classes_bench.py [--log2 28] [--reps 9] [--batches 64,4096] [--upper 0.15] [--partners 0.1] [--out profiles/classes_bench.jsonl]

Input and query mix are those of tools/fold_bench.py (§26 words text, §27 three-word queries).  A share --upper of the letters
is upper-cased and a share --partners of the letters s and i is replaced by their two-byte partners (U+017F, U+0131), so that
classes with members of different lengths have all their members in the text.  Every shape is warmed up first, the ways run
alternately in this process, times are medians of --reps.  The one relation that is checked and not timed: an all-literal batch
makes exactly the steps the fold search makes under the identity map (which §28 holds to the exact search).  Appends one JSON
line per measurement to --out.
"""
import argparse
import ctypes
import itertools
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
    ap.add_argument("--batches", default="64,4096")
    ap.add_argument("--upper", type=float, default=0.15)
    ap.add_argument("--partners", type=float, default=0.1)
    ap.add_argument("--max-spellings", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib, unicode_fold
    from text_bwt import WORDS, make_text
    L = _lib.load()
    raw_len = 1 << a.log2
    raw = make_text(torch, raw_len, 1, "cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(30)
    step = 1 << 26
    for lo in range(0, raw_len, step):                           # upper-case a share of the letters, a piece at a time
        piece = raw[lo:lo + step]
        up = (torch.rand(piece.numel(), generator=g, device="cuda") < a.upper) & (piece >= 97) & (piece <= 122)
        piece -= up.to(torch.uint8) * 32
    # a share of s and i becomes the long s and the dotless i: two bytes each, the text grows
    two = (torch.rand(raw_len, generator=g, device="cuda") < a.partners) & ((raw == ord("s")) | (raw == ord("i")))
    second = torch.where(raw == ord("s"), torch.tensor(0xBF, dtype=torch.uint8, device="cuda"), torch.tensor(0xB1, dtype=torch.uint8, device="cuda"))
    first = torch.where(raw == ord("s"), torch.tensor(0xC5, dtype=torch.uint8, device="cuda"), torch.tensor(0xC4, dtype=torch.uint8, device="cuda"))
    counts = two.to(torch.int64) + 1
    start = torch.cumsum(counts, 0) - counts
    text = torch.repeat_interleave(raw, counts)
    at = start[two]
    text[at] = first[two]
    text[at + 1] = second[two]
    n_partners = int(two.sum().item())
    del raw, two, first, second, counts, start, at
    text_len = int(text.numel())
    rng = np.random.default_rng(5)
    lens = rng.geometric(1.0 / a.doc_mean, size=int(text_len / a.doc_mean * 1.5) + 16)
    ends = np.cumsum(lens).astype(np.uint64)
    ends = np.concatenate([ends[ends < text_len], np.array([text_len], dtype=np.uint64)])
    # (a document may end between the two bytes of a partner: a broken character there is a literal to the tokeniser)
    n_docs = int(ends.size)
    h = ctypes.c_void_p()
    torch.cuda.synchronize()
    _lib.check(L.fmx_corpus_build_dev(text.data_ptr(), text_len, ends.ctypes.data, n_docs, 0, None, ctypes.byref(h)))
    del text
    corpus = findex_amd.Corpus(h, [b"%d" % d for d in range(n_docs)])
    cs = findex_amd.HipCorpusSearcher(corpus)
    corpus.drop_stream()
    torch.cuda.empty_cache()
    hip = cs.searcher
    hip.prepare(ktab=True, locate=True)

    words = [w for w in open(WORDS, "rb").read().split() if w.isalpha() and w.islower()]
    sample = [words[i] for i in rng.choice(len(words), min(20000, len(words)), replace=False)]
    off = np.zeros(len(sample) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w in sample])
    _, hits = hip.search_fold_batch(np.frombuffer(b"".join(w[::-1] for w in sample), dtype=np.uint8), off)
    rows = np.bincount(hits["regex"], weights=(hits["ep"] - hits["sp"]).astype(np.float64), minlength=len(sample)).astype(np.int64)
    band = lambda lo, hi: [sample[i] for i in np.nonzero((rows >= lo) & (rows <= hi))[0]]
    common, mid, rare = band(4096, 16384), band(512, 2048), band(1, 256)
    base = {"log2": a.log2, "n_docs": n_docs, "stream_len": corpus.stream_len, "reps": a.reps, "upper": a.upper, "partners": a.partners,
            "two_byte_partners": n_partners}
    med = lambda xs: float(np.median(xs))

    def emit(res):
        res = dict(base, **res)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(res) + "\n")

    def packed(terms):
        esc = [findex_amd.escape(t)[::-1] for t in terms]
        o = np.zeros(len(esc) + 1, dtype=np.uint64)
        o[1:] = np.cumsum([len(e) for e in esc])
        return np.frombuffer(b"".join(esc), dtype=np.uint8).copy(), o

    def yardstick_a(terms):
        """The fold kernel under the ASCII map against the class kernel under the same map as a table, device forms."""
        buf, o = packed(terms)
        k = len(terms)
        cid, cls_off, mem_off, mem_bytes = unicode_fold.fold_map_table(findex_amd.ASCII_FOLD)
        table = (cls_off, mem_off, mem_bytes)
        el = np.array([c if cid[c] < 0 else 256 + cid[c] for c in buf.tolist()], dtype=np.uint16)
        f_off, f_hits = hip.search_fold_batch(buf, o)
        c_off, c_hits = hip.search_classes_batch(el, o, table)
        same = bool(np.array_equal(f_off, c_off) and f_hits.tobytes() == c_hits.tobytes())
        total = max(int(f_hits.size), k, 1)
        d_pat, d_el = torch.from_numpy(buf).cuda(), torch.from_numpy(el.view(np.int16)).cuda()
        d_off = torch.from_numpy(o.view(np.int64)).cuda()
        d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
        d_out = torch.empty(3 * total, dtype=torch.int64, device="cuda")
        fold = lambda m=findex_amd.ASCII_FOLD: (hip.search_fold_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), total, fold=m), hip.fold_last())[1]
        cls = lambda: (hip.search_classes_batch_dev(d_el.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), total, table), hip.classes_last())[1]
        fold(), cls()
        fm, cm = [], []
        for _ in range(a.reps):
            fm.append(fold())
            cm.append(cls())
        # all literals against the identity map: the one relation that is held
        lit = lambda: (hip.search_classes_batch_dev(torch.from_numpy(buf.astype(np.uint16).view(np.int16)).cuda().data_ptr(), d_off.data_ptr(), k,
                                                    d_out_off.data_ptr(), d_out.data_ptr(), total, None), hip.classes_last())[1]
        ident = fold(bytes(range(256)))
        literal = lit()
        spread = lambda xs: round(float(np.max(xs) - np.min(xs)), 4)
        emit({"what": "(a) fold kernel against class kernel, the ASCII map", "n_terms": k, "hits": int(f_hits.size), "same_bytes": same,
              "fold_search_ms": round(med([m[0] for m in fm]), 4), "classes_search_ms": round(med([m[0] for m in cm]), 4),
              "fold_search_ms_spread": spread([m[0] for m in fm]), "classes_search_ms_spread": spread([m[0] for m in cm]),
              "fold_sort_ms": round(med([m[1] for m in fm]), 4), "classes_sort_ms": round(med([m[1] for m in cm]), 4),
              "fold_steps": fm[-1][2], "classes_steps": cm[-1][2], "fold_requests": fm[-1][3], "classes_requests": cm[-1][3],
              "identity_steps": ident[2], "all_literal_steps": literal[2], "all_literal_steps_equal_identity_steps": bool(ident[2] == literal[2])})

    def yardstick_b(terms):
        """Every spelling of every term through the exact search, enumerated on the host, against one class search."""
        classes = unicode_fold.case_classes()
        keep, spell = [], []
        for t in terms:
            parts = [[chr(m).encode("utf-8") for m in classes[c]] if c in classes else [r] for c, r in unicode_fold.tokens(t)]
            n = int(np.prod([len(p) for p in parts]))
            if n <= a.max_spellings:
                keep.append(t)
                spell.append(parts)
        if not keep:
            return

        def enumerate_all():
            every = [b"".join(v)[::-1] for parts in spell for v in itertools.product(*parts)]
            o = np.zeros(len(every) + 1, dtype=np.uint64)
            o[1:] = np.cumsum([len(e) for e in every])
            sp, ep = hip.search_batch(np.frombuffer(b"".join(every), dtype=np.uint8), o)
            return len(every), sp, ep

        def classes_once():
            el, el_off, table = hip.unicode_table(keep)
            return hip.search_classes_batch(el, el_off, table)

        n_spellings, sp, ep = enumerate_all()
        _, hits = classes_once()
        grp = np.repeat(np.arange(len(keep)), [int(np.prod([len(p) for p in parts])) for parts in spell])
        ok = sp < ep
        want = sorted(zip(grp[ok].tolist(), sp[ok].tolist(), ep[ok].tolist()))
        same = want == sorted(zip(hits["regex"].tolist(), hits["sp"].tolist(), hits["ep"].tolist()))
        te, tc = [], []
        for _ in range(a.reps):
            for fn, ts in ((enumerate_all, te), (classes_once, tc)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "(b) host enumeration through fmx_search_batch against one class search", "n_terms": len(keep), "terms_left_out": len(terms) - len(keep),
              "spellings_enumerated": n_spellings, "spellings_that_occur": int(ok.sum()), "same_intervals": bool(same),
              "enumeration_call_ms": round(med(te), 3), "classes_call_ms": round(med(tc), 3),
              "classes_search_ms": round(hip.classes_last()[0], 4), "classes_steps": hip.classes_last()[2]})

    def yardstick_c(queries, label):
        asc = lambda: cs.rank(queries, top=TOP, k1=K1, b=B, ignore_case=True)
        uni = lambda: cs.rank(queries, top=TOP, k1=K1, b=B, ignore_case="unicode")
        a_out, u_out = asc(), uni()
        ta, tu, last = [], [], []
        for _ in range(a.reps):
            for fn, ts in ((asc, ta), (uni, tu)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            last.append(hip.classes_last())
        emit({"what": "(c) rank(ignore_case=True) against rank(ignore_case=\"unicode\"): " + label, "n_queries": len(queries),
              "n_terms": int(a_out[3].size), "ascii_call_ms": round(med(ta), 3), "unicode_call_ms": round(med(tu), 3),
              "unicode_over_ascii": round(med(tu) / max(med(ta), 1e-9), 3), "ascii_df_sum": int(a_out[3].sum()), "unicode_df_sum": int(u_out[3].sum()),
              "in_call_classes_search_ms": round(med([x[0] for x in last]), 4), "in_call_classes_steps": last[-1][2]})

    for nq in [int(x) for x in a.batches.split(",") if x]:
        pick = lambda pool: pool[int(rng.integers(0, len(pool)))]
        queries = [[pick(common), pick(mid), pick(rare)] for _ in range(nq)]
        terms = [t for q in queries for t in q]
        yardstick_a(terms)
        yardstick_b(terms)
        yardstick_c(queries, "three words: common, mid, rare")
    cs.close()


if __name__ == "__main__":
    main()
