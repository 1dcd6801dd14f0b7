#!/usr/bin/env python3
"""Line-query measurements: fmx_line_query_dev over line-hit lists in HBM, timed with the device events of
fmx_line_query_last, beside the route a user has without it -- download the line hits of the same lists and evaluate in numpy
(np.searchsorted over packed keys, np.setdiff1d against the real lines for -v; the download is part of that route's time).

    python tools/linequery_bench.py [--log2n 28] [--reps 9] [--out profiles/linequery_bench.jsonl]

The text is the words text of tools/text_bwt.py (a newline behind every ~12th word), the index built by
fmx_bwt_from_text_dev.  The hit lists are those of two frequent strings and one rare word; the queries are `A and B`,
`A not B`, `A near/2 B` and `-v A`.  Every call runs over a ring of four distinct copies of the input after a warm-up of each,
with "lq_narrow" on and off alternating in the same run.  Candidates/s and key probes/s are set beside the 46.5 G requests/s
of DESIGN.md §4.  One JSON line per query is printed and appended to --out.  Without a GPU the tool fails.
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

REQUEST_CEILING = 46.5e9
RING = 4


def host_route(torch, d_hits, off, anchor, term, window, negate, n_real):
    """The numpy route: the line hits come down, then the algebra over their line numbers.  -> the kept line numbers."""
    hits = d_hits.cpu().numpy().view(HIT)
    key = hits["line_no"]                                    # (no corpus: the key orders by line_no alone)
    B = key[int(off[term]):int(off[term + 1])]
    if anchor is None:                                       # -v: the real lines less the term's
        return np.setdiff1d(np.arange(1, n_real + 1, dtype=np.uint64), B, assume_unique=True)
    A = key[int(off[anchor]):int(off[anchor + 1])]
    lo = np.where(A > np.uint64(window), A - np.uint64(window), np.uint64(1))
    p = np.searchsorted(B, lo, side="left")
    found = (p < B.size) & (B[np.minimum(p, max(B.size - 1, 0))] <= A + np.uint64(window)) if B.size else np.zeros(A.size, dtype=bool)
    return A[found != negate]


def main():
    global HIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--frequent", default="ing,er", help="two strings that stand on many lines")
    ap.add_argument("--rare", default=None, help="a word that stands on few (default: the middle word of the word list)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linequery_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    import text_bwt
    from text_bwt import make_text
    HIT = findex_amd.HipFMSearcher.LINE_HIT
    L = _lib.load()
    dev = "cuda"
    t0 = time.time()
    length = 1 << a.log2n
    text = make_text(torch, length, 1, dev)
    ends_in_break = int(text[-1].item()) == 10
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), None, ctypes.byref(eof), counts.ctypes.data, 0, None))
    del text
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    hip.prepare(ktab=False, locate=True)
    hip.lines_prepare()
    n_brk = hip.lines_info()[0]
    n_real = n_brk + (0 if ends_in_break else 1)
    words = [w for w in open(text_bwt.WORDS, "rb").read().split() if w.isalpha() and w.islower()]
    rare = a.rare or max(words[len(words) // 2 - 8:len(words) // 2 + 8], key=len).decode()
    regexes = a.frequent.split(",") + [rare]
    off, occ, truncated = hip.finditer(regexes, mode="all", occ_cap=1 << 24)
    loff, hits = hip.occurrence_lines(off, occ)
    del occ
    A, B, R = 0, 1, 2
    sizes = [int(loff[g + 1] - loff[g]) for g in range(3)]
    head = {"input": "words%d" % a.log2n, "n": n, "lines": int(n_real), "lists": dict(zip(a.frequent.split(",") + [rare], sizes)),
            "setup_s": round(time.time() - t0, 2)}
    print(json.dumps(head), flush=True)
    ring = [(torch.from_numpy(loff.view(np.int64).copy()).to(dev), torch.from_numpy(hits.view(np.int64).copy()).to(dev)) for _ in range(RING)]
    d_qoff = torch.empty(2, dtype=torch.int64, device=dev)
    d_out = torch.empty(6 * max(max(sizes), n_real), dtype=torch.int64, device=dev)
    cap = d_out.numel() // 6
    named = [("A and B", A, B, 0, False), ("A not B", A, B, 0, True), ("A near/2 B", A, B, 2, False), ("-v A", None, A, 0, True),
             ("A and rare", A, R, 0, False), ("rare near/2 A", R, A, 2, False)]
    rows = []
    try:
        for name, anchor, term, window, negate in named:
            query = [(anchor, [(term, window, negate)])]

            def call(slot):
                d_off, d_hits = ring[slot]
                return hip.line_query_dev(d_off.data_ptr(), d_hits.data_ptr(), hits.size, 3, query, d_qoff.data_ptr(), d_out.data_ptr(), cap)

            for mode in ("on", "off"):                           # a warm-up of each input, either way
                findex_amd.config_set("lq_narrow", mode)
                for slot in range(RING):
                    kept = call(slot)
            want = host_route(torch, ring[0][1], loff, anchor, term, window, negate, n_real)        # warms up
            got = d_out[: 6 * kept].cpu().numpy().view(HIT)["line_no"]
            equal = bool(np.array_equal(got, want))
            assert equal, "the two routes' outputs differ: " + name
            dev_ms = {"on": [], "off": []}
            probes, wall, host_wall = {}, {"on": [], "off": []}, []
            for r in range(a.reps):
                for mode in (("on", "off"), ("off", "on"))[r % 2]:      # alternating in the same run, either one first in turn
                    findex_amd.config_set("lq_narrow", mode)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    assert call(r % RING) == kept
                    wall[mode].append((time.perf_counter() - t) * 1e3)     # (the call ends in a synchronise)
                    last = hip.line_query_last()
                    dev_ms[mode].append(last[:3])
                    candidates, probes[mode] = last[3], last[4]
                t = time.perf_counter()
                host_route(torch, ring[r % RING][1], loff, anchor, term, window, negate, n_real)
                host_wall.append((time.perf_counter() - t) * 1e3)
            on, offm = np.median(np.array(dev_ms["on"]), axis=0), np.median(np.array(dev_ms["off"]), axis=0)
            r = {"what": "line_query", "input": head["input"], "n": n, "query": name, "hits_uploaded": int(hits.size),
                 "candidates": int(candidates), "kept": int(kept),
                 "keys_ms": round(float(on[0]), 4), "flags_ms_narrow_on": round(float(on[1]), 4), "flags_ms_narrow_off": round(float(offm[1]), 4),
                 "emit_ms": round(float(on[2]), 4), "probes_narrow_on": int(probes["on"]), "probes_narrow_off": int(probes["off"]),
                 "device_ms_narrow_on": round(float(on.sum()), 4), "device_ms_narrow_off": round(float(offm.sum()), 4),
                 "candidates_per_s_flags_on": round(candidates / max(float(on[1]), 1e-6) * 1e3),
                 "candidates_per_s_flags_off": round(candidates / max(float(offm[1]), 1e-6) * 1e3),
                 "probes_per_s_on": round(probes["on"] / max(float(on[1]), 1e-6) * 1e3),
                 "probes_per_s_off": round(probes["off"] / max(float(offm[1]), 1e-6) * 1e3),
                 "probes_off_share_of_request_ceiling": round(probes["off"] / max(float(offm[1]), 1e-6) * 1e3 / REQUEST_CEILING, 4),
                 "call_wall_ms_narrow_on": round(float(np.median(wall["on"])), 4), "call_wall_ms_narrow_off": round(float(np.median(wall["off"])), 4),
                 "host_numpy_wall_ms": round(float(np.median(host_wall)), 3),
                 "host_over_library": round(float(np.median(host_wall) / np.median(wall["off"])), 2), "outputs_equal": equal}
            print(json.dumps(r), flush=True)
            rows.append(r)
    finally:
        findex_amd.config_set("lq_narrow", "off")            # the default
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(head) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")
    hip.close()


if __name__ == "__main__":
    main()
