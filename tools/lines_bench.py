#!/usr/bin/env python3
"""Line-table measurements: the table's build, split as fmx_lines_last gives it, and its lookups per second
for random and for ascending positions at several directory steps 2^S; fmx_occurrence_lines_dev over a list of occurrences in
HBM beside its two host equivalents -- np.searchsorted over the downloaded positions (the download included), and what
findex_amd/grep.py's with_context does per hit (a window of bytes around it, rfind / find for the newlines).

    python tools/lines_bench.py [--log2n 28] [--log2k 24] [--log2occ 22] [--reps 9] [--out profiles/lines_bench.jsonl]

The text is the words text of tools/text_bwt.py (a newline behind every ~12th word), the index built by
fmx_bwt_from_text_dev.  Lookups are timed with device events around one launch, over a ring of four distinct inputs after a
warm-up of each; a lookup is two dependent memory requests at best (the directory pair, then the breaks), so its rate is set
beside the 46.5 G requests/s of DESIGN.md §4.  One JSON line per configuration is printed and appended to --out.
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


def timed(torch, fn, ring, reps):
    """Median, min and max device ms of fn(x) over the ring of inputs, after one warm-up of each."""
    for x in ring:
        fn(x)
    torch.cuda.synchronize()
    ms = []
    for r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(ring[r % len(ring)])
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def host_lines(brk, off, pos):
    """The reduction on the host: line of every position, then per group the distinct lines and their counts."""
    line = np.searchsorted(brk, pos, side="left")
    out_off, lines, counts = [0], [], []
    for g in range(off.size - 1):
        u, c = np.unique(line[int(off[g]):int(off[g + 1])], return_counts=True)
        lines.append(u)
        counts.append(c)
        out_off.append(out_off[-1] + u.size)
    return np.array(out_off, dtype=np.uint64), np.concatenate(lines), np.concatenate(counts)


def window_lines(hip, pos, length, context):
    """What grep.py's with_context does per hit: `context` bytes on either side, cut at the nearest newlines."""
    a = pos - np.minimum(pos, np.uint64(context))
    lead = (pos - a).astype(np.int64)
    n_text = np.uint64(hip.n - 1)
    ln = np.minimum(pos - a + np.uint64(length + context), n_text - a)
    off, data = hip.extract_text_batch(a, ln)
    data = data.tobytes()
    out = []
    for q, ld in enumerate(lead.tolist()):
        buf = data[int(off[q]):int(off[q + 1])]
        lo = buf.rfind(b"\n", 0, ld) + 1
        hi = buf.find(b"\n", ld + length)
        out.append(buf[lo:len(buf) if hi < 0 else hi])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--log2k", type=int, default=24, help="positions per lookup call")
    ap.add_argument("--log2occ", type=int, default=22, help="occurrences of the reduction")
    ap.add_argument("--shifts", default="6,8,10")
    ap.add_argument("--window-hits", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lines_bench.jsonl"))
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
    brk = np.flatnonzero(text.cpu().numpy() == 10).astype(np.int64)      # (the call indexes reverse(text): positions are the text's)
    del text
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    hip.prepare(ktab=False, locate=True, extract=True)
    torch.cuda.synchronize()
    head = {"input": "words%d" % a.log2n, "n": n, "breaks": int(brk.size), "locate_rate": hip.locate_info()[0],
            "setup_s": round(time.time() - t0, 2)}
    print(json.dumps(head), flush=True)
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    k = 1 << a.log2k
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    rnd = [torch.randint(0, length, (k,), generator=g, device=dev, dtype=torch.int64) for _ in range(4)]
    asc = [torch.arange(k, dtype=torch.int64, device=dev) * (length // k) + j for j in range(4)]
    d_line, d_start, d_end = (torch.empty(k, dtype=torch.int64, device=dev) for _ in range(3))
    check = rnd[0][:100000].cpu().numpy()
    default_shift = hip.lines_info()[2]                      # (no table yet: the handle's policy)
    for shift in [int(s) for s in a.shifts.split(",")]:
        hip.config_set("lines_shift", shift)
        builds = []
        for _ in range(3):
            hip.drop_tables(jump=False, frontier=False, lines=True)
            t = time.perf_counter()
            hip.lines_prepare()
            wall = (time.perf_counter() - t) * 1e3
            builds.append(hip.lines_last()[:2] + (wall,))
        n_brk, bset, s, nbytes, _ = hip.lines_info()
        assert n_brk == brk.size and s == shift

        def lookup(x):
            hip.line_of_dev(x.data_ptr(), k, d_line.data_ptr(), d_start.data_ptr(), d_end.data_ptr(), stream=stream)

        r_ms = timed(torch, lookup, rnd, a.reps)
        a_ms = timed(torch, lookup, asc, a.reps)
        lookup(rnd[0])
        torch.cuda.synchronize()
        assert np.array_equal(d_line[:100000].cpu().numpy(), np.searchsorted(brk, check, side="left")), "lookups differ from numpy"
        b = np.median(np.array(builds), axis=0)
        r = {"what": "table", "input": head["input"], "n": n, "shift": shift, "breaks": int(n_brk), "table_bytes": int(nbytes),
             "build_locate_ms": round(float(b[0]), 3), "build_sort_ms": round(float(b[1]), 3), "build_wall_ms": round(float(b[2]), 3),
             "positions": k, "random_ms": round(r_ms[0], 4), "random_ms_min_max": [round(r_ms[1], 4), round(r_ms[2], 4)],
             "random_lookups_per_s": round(k / r_ms[0] * 1e3), "ascending_ms": round(a_ms[0], 4),
             "ascending_ms_min_max": [round(a_ms[1], 4), round(a_ms[2], 4)], "ascending_lookups_per_s": round(k / a_ms[0] * 1e3),
             "random_share_of_request_ceiling_at_2_requests": round(2 * k / r_ms[0] * 1e3 / REQUEST_CEILING, 4)}
        print(json.dumps(r), flush=True)
        rows.append(r)
    del rnd, asc, d_line, d_start, d_end
    # ---- the reduction: four groups of sorted positions, the table at the default shift
    hip.config_set("lines_shift", default_shift)
    hip.drop_tables(jump=False, frontier=False, lines=True)
    hip.lines_prepare()
    n_occ, groups = 1 << a.log2occ, 4
    per = n_occ // groups
    pos = torch.sort(torch.randint(0, length - 8, (groups, per), generator=g, device=dev, dtype=torch.int64), dim=1)[0].reshape(-1)
    rec = torch.zeros((n_occ, 4), dtype=torch.int64, device=dev)
    grp = torch.arange(groups, dtype=torch.int64, device=dev).repeat_interleave(per)
    rec[:, 0] = grp | (4 << 32)
    rec[:, 1] = pos
    rec[:, 2] = 0xFFFFFFFF | (4 << 32)
    rec[:, 3] = pos
    off = np.arange(groups + 1, dtype=np.uint64) * np.uint64(per)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_loff = torch.empty(groups + 1, dtype=torch.int64, device=dev)
    total = hip.occurrence_lines_dev(d_off.data_ptr(), rec.data_ptr(), n_occ, groups, d_loff.data_ptr(), 0, 0)       # counts; warms up
    d_out = torch.empty(6 * max(total, 1), dtype=torch.int64, device=dev)
    want = host_lines(brk, off, rec[:, 1].cpu().numpy())                                                            # warms up
    wall, phases, host_wall = [], [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = hip.occurrence_lines_dev(d_off.data_ptr(), rec.data_ptr(), n_occ, groups, d_loff.data_ptr(), d_out.data_ptr(), total)
        wall.append((time.perf_counter() - t) * 1e3)                 # (the call ends in a synchronise)
        phases.append(hip.lines_last()[2:])
        assert got == total
        t = time.perf_counter()
        want = host_lines(brk, off, rec[:, 1].cpu().numpy())         # the download is part of this route
        host_wall.append((time.perf_counter() - t) * 1e3)
    hits = d_out[: 6 * total].cpu().numpy().view(findex_amd.HipFMSearcher.LINE_HIT)
    equal = bool(np.array_equal(d_loff.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(hits["line_no"] - np.uint64(1), want[1])
                 and np.array_equal(hits["n_hits"], want[2]))
    assert equal, "the two routes' outputs differ"
    ph = np.median(np.array(phases), axis=0)
    r = {"what": "occurrence_lines", "input": head["input"], "n": n, "shift": default_shift, "occurrences": n_occ, "groups": groups,
         "lines": int(total), "lookup_ms": round(float(ph[0]), 4), "compact_ms": round(float(ph[1]), 4),
         "call_wall_ms": round(float(np.median(wall)), 4), "call_wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)],
         "host_searchsorted_wall_ms": round(float(np.median(host_wall)), 3),
         "host_over_library": round(float(np.median(host_wall) / np.median(wall)), 2), "outputs_equal": equal}
    print(json.dumps(r), flush=True)
    rows.append(r)
    # ---- whole lines of 10^4 hits: the table and one extract of exactly the lines, beside the window route of with_context
    w = a.window_hits
    sel = rec[torch.randperm(n_occ, generator=g, device=dev)[:w], 1].cpu().numpy().view(np.uint64)
    window_lines(hip, sel, 4, 256)                                   # warms up

    def table_route():
        _, s, e = hip.line_of(sel)
        o, data = hip.extract_text_batch(s, e - s)
        data = data.tobytes()
        return [data[int(o[q]):int(o[q + 1])] for q in range(w)]

    table_route()
    tw, ww = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        whole = table_route()
        tw.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        cut = window_lines(hip, sel, 4, 256)
        ww.append((time.perf_counter() - t) * 1e3)
    r = {"what": "whole_lines", "input": head["input"], "n": n, "hits": w, "window_context_bytes": 256,
         "table_route_wall_ms": round(float(np.median(tw)), 3), "window_route_wall_ms": round(float(np.median(ww)), 3),
         "lines_the_window_cut": int(sum(1 for x, y in zip(whole, cut) if x != y)),
         "bytes_table_route": int(sum(len(x) for x in whole)), "bytes_window_route_extracted": int(w * (2 * 256 + 4))}
    print(json.dumps(r), flush=True)
    rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    hip.close()


if __name__ == "__main__":
    main()
