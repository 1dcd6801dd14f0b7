#!/usr/bin/env python3
"""Occurrences measurements: fmx_occurrences_dev on the results a regex batch leaves in HBM -- rows located,
occurrences, the four device-event phases and the whole call -- beside the route a caller had before: the results on the
host, fmx_locate_intervals, then numpy (the position arithmetic, lexsort, the run heads) and a Python loop for the greedy
non-overlapping pass.  Both routes' outputs must be equal.

    python tools/occurrences_bench.py [--log2n 28] [--regexes 1000] [--reps 5] [--out profiles/occurrences_bench.jsonl]

The text is the words text of tools/text_bwt.py, the index built by fmx_bwt_from_text_dev.  The regexes are drawn from the
words of the text: a word as it is, with one letter as `.`, with one letter repeated by `+`, with one letter as a class of
five; matched at max_steps 16.  The three modes, with and without max_per; the two routes alternate in one run, after a
warm-up of each.  One JSON line per configuration is printed and appended to --out.
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


def draw_regexes(rng, count):
    from text_bwt import WORDS
    words = [w.decode() for w in open(WORDS, "rb").read().split() if w.isalpha() and w.islower() and len(w) >= 4]
    out = []
    for j in range(count):
        w = words[int(rng.integers(0, len(words)))]
        i = int(rng.integers(1, len(w) - 1))
        c = ord(w[i])
        out.append((w, w[:i] + "." + w[i + 1:], w[:i + 1] + "+" + w[i + 1:],
                    w[:i] + "[%c-%c]" % (max(c - 2, 97), min(c + 2, 122)) + w[i + 1:])[j % 4])
    return out


def host_route(hip, res, k, mode, max_per):
    """(off[k + 1], group, pos, len) of the results `res` by the calls and the numpy a caller had before fmx_occurrences."""
    n = hip.n
    off, sa = hip.locate_intervals(res["sp"], res["ep"], max_per=max_per)
    per = np.diff(off).astype(np.int64)
    g = np.repeat(res["regex"], per).astype(np.int64)
    ln = np.repeat(res["len"], per).astype(np.int64)
    sa = sa.astype(np.int64)
    ok = sa + ln <= n - 1
    g, ln, pos = g[ok], ln[ok], (n - 1 - ln - sa)[ok]
    order = np.lexsort((ln, pos, g))
    g, pos, ln = g[order], pos[order], ln[order]
    if mode == "all":
        keep = np.ones(g.size, dtype=bool)
        keep[1:] = (g[1:] != g[:-1]) | (pos[1:] != pos[:-1]) | (ln[1:] != ln[:-1])
    else:
        keep = np.ones(g.size, dtype=bool)
        keep[:-1] = (g[1:] != g[:-1]) | (pos[1:] != pos[:-1])
    g, pos, ln = g[keep], pos[keep], ln[keep]
    if mode == "disjoint":
        take = np.zeros(g.size, dtype=bool)
        cur, end = -1, 0
        for i, (gi, pi, li) in enumerate(zip(g.tolist(), pos.tolist(), ln.tolist())):
            if gi != cur:
                cur, end = gi, 0
            if pi >= end:
                take[i] = True
                end = pi + li
        g, pos, ln = g[take], pos[take], ln[take]
    out_off = np.searchsorted(g, np.arange(k + 1)).astype(np.uint64)
    return out_off, g, pos, ln


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--regexes", type=int, default=1000)
    ap.add_argument("--max-steps", type=int, default=16)
    ap.add_argument("--max-per", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occurrences_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import make_text
    L = _lib.load()
    dev = "cuda"
    t0 = time.time()
    length = 1 << a.log2n
    text = make_text(torch, length, 1, dev)
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), None, ctypes.byref(eof), counts.ctypes.data, 0, None))
    del text
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    hip.prepare(locate=True, frontier=True)
    torch.cuda.synchronize()
    trees = findex_amd.ReTree.compile_batch(draw_regexes(np.random.default_rng(5), a.regexes))
    trees = trees.select(np.nonzero(trees.ok())[0])
    k = len(trees)
    batch = findex_amd.ReTree.prepare_batch(hip, trees)
    cap = 1 << 22
    d_res = torch.empty(3 * cap, dtype=torch.int64, device=dev)
    n_res = batch.match_dev(d_res.data_ptr(), cap, max_steps=a.max_steps)
    res = d_res[: 3 * n_res].cpu().numpy().view(findex_amd.HipFMSearcher.RESULT)
    d_off = torch.empty(k + 1, dtype=torch.int64, device=dev)
    head = {"input": "words%d" % a.log2n, "n": n, "regexes": k, "max_steps": a.max_steps, "results": int(n_res),
            "truncated": bool(batch.truncated), "locate_rate": hip.locate_info()[0], "setup_s": round(time.time() - t0, 2)}
    print(json.dumps(head), flush=True)
    lines = []
    for max_per in (None, a.max_per):
        for mode in ("all", "longest", "disjoint"):
            total = hip.occurrences_dev(d_res.data_ptr(), n_res, k, d_off.data_ptr(), 0, 0, mode, max_per)       # counts; warms up
            d_out = torch.empty(4 * max(total, 1), dtype=torch.int64, device=dev)
            want = host_route(hip, res, k, mode, max_per)                                                        # warms up
            phases, wall, host_wall = [], [], []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                got = hip.occurrences_dev(d_res.data_ptr(), n_res, k, d_off.data_ptr(), d_out.data_ptr(), total, mode, max_per)
                wall.append((time.perf_counter() - t) * 1e3)                 # (the call ends in a synchronise)
                phases.append(hip.occurrences_last())
                assert got == total
                t = time.perf_counter()
                want = host_route(hip, res, k, mode, max_per)
                host_wall.append((time.perf_counter() - t) * 1e3)
            occ = d_out[: 4 * total].cpu().numpy().view(findex_amd.HipFMSearcher.OCCURRENCE)
            off = d_off.cpu().numpy().view(np.uint64)
            equal = bool(np.array_equal(off, want[0]) and np.array_equal(occ["group"], want[1]) and np.array_equal(occ["pos"], want[2])
                         and np.array_equal(occ["len"], want[3]))
            assert equal, "the two routes' outputs differ"
            ph = np.median(np.array([p[:4] for p in phases]), axis=0)
            r = {"input": head["input"], "n": n, "regexes": k, "max_steps": a.max_steps, "mode": mode, "max_per": max_per or 0,
                 "results": int(n_res), "rows": int(phases[-1][4]), "occurrences": int(total), "locate_ms": round(float(ph[0]), 4),
                 "sort_ms": round(float(ph[1]), 4), "select_ms": round(float(ph[2]), 4), "compact_ms": round(float(ph[3]), 4),
                 "call_wall_ms": round(float(np.median(wall)), 4), "call_wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)],
                 "host_route_wall_ms": round(float(np.median(host_wall)), 3),
                 "host_over_library": round(float(np.median(host_wall) / np.median(wall)), 2), "outputs_equal": equal}
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
