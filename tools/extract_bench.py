#!/usr/bin/env python3
"""Extract measurements: build time of the inverse-SA samples both ways, bytes per second of two batch
shapes, and the ratio to fmx_lf_walk_batch_dev making the same number of LF steps from random rows.

    python tools/extract_bench.py [--log2 28] [--rates 8,32,128] [--out profiles/extract_bench.jsonl]

The text is 2^28 bytes of the words text of tools/text_bwt.py, indexed on the device.  Shapes: `short` = 1 M ranges of 64
bytes at random offsets, `long` = one range of 64 MiB.  Times are device events around the enqueue-only form, the median
of --reps runs after a warm-up; steps and requests are fmx_extract_last's of one host-pointer call of the same batch.
One JSON line per rate is appended to --out.
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

REQUESTS_PER_S = 46.5e9         # README.md: what the memory system gives this access pattern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--rates", default="8,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    from text_bwt import make_text
    L = _lib.load()
    dev = "cuda"
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
    rng = np.random.default_rng(5)
    long_bytes = min(64 << 20, length // 2)
    shapes = {
        "short": (rng.integers(0, length - 64, 1 << 20, dtype=np.uint64), np.full(1 << 20, 64, dtype=np.uint64)),
        "long": (np.array([length // 3], dtype=np.uint64), np.array([long_bytes], dtype=np.uint64)),
    }

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def build(s, via_locate):
        hip.config_set("extract_sample", s)
        hip.config_set("locate_sample", s)
        hip.drop_tables(jump=False, frontier=False, locate=True, extract=True)
        if via_locate:
            hip.prepare(ktab=False, locate=True)
        torch.cuda.synchronize()
        t = time.time()
        hip.prepare(ktab=False, extract=True)
        return round(hip.extract_info()[2], 2), round((time.time() - t) * 1e3, 2), hip.extract_info()[1]

    for s in [int(x) for x in a.rates.split(",")]:
        inv_ms, inv_wall, nbytes = build(s, False)
        sc_ms, sc_wall, _ = build(s, True)
        res = {"text": "words", "n": n, "layout": hip.stats()["layout"], "rate": s, "sample_bytes": nbytes,
               "build_inversion_ms": inv_ms, "build_inversion_wall_ms": inv_wall, "build_scatter_ms": sc_ms,
               "build_scatter_wall_ms": sc_wall, "shapes": {}}
        for name, (pos, lens) in shapes.items():
            off = np.zeros(pos.size + 1, dtype=np.uint64)
            off[1:] = np.cumsum(lens)
            nb = int(off[-1])
            _, data = hip.extract_text_batch(pos, lens)
            _, steps, requests = hip.extract_last()
            want = np.concatenate([text[int(p):int(p) + int(l)].cpu().numpy() for p, l in zip(pos[:64].tolist(), lens[:64].tolist())])
            assert np.array_equal(data[:want.size], want), "the extracted bytes are not the text's"
            d_pos = torch.from_numpy(pos.view(np.int64)).to(dev)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_out = torch.empty(nb, dtype=torch.uint8, device=dev)
            ms = timed(lambda: hip.extract_text_batch_dev(d_pos.data_ptr(), d_off.data_ptr(), pos.size, nb, d_out.data_ptr()))
            # the same number of LF steps by the existing walk kernel: walks of 64 steps from random rows
            walks = max(steps // 64, 1)
            rows = torch.from_numpy(rng.integers(0, n, walks, dtype=np.uint64).view(np.int64)).to(dev)
            w_out = torch.empty(walks * 64, dtype=torch.uint8, device=dev)
            w_end = torch.empty(walks, dtype=torch.int64, device=dev)
            ms_walk = timed(lambda: hip.lf_walk_batch_dev(rows.data_ptr(), walks, 64, w_out.data_ptr(), w_end.data_ptr()))
            res["shapes"][name] = {
                "ranges": int(pos.size), "bytes": nb, "steps": steps, "requests": requests, "ms": round(ms, 3),
                "bytes_per_s": round(nb / ms * 1e3), "steps_per_byte": round(steps / nb, 3),
                "requests_per_step": round(requests / steps, 3), "requests_per_s": round(requests / ms * 1e3),
                "share_of_46.5G": round(requests / ms * 1e3 / REQUESTS_PER_S, 3),
                "lf_walk_ms": round(ms_walk, 3), "lf_walk_over_extract": round(ms_walk / ms, 3)}
            del d_out, w_out
        line = json.dumps(res)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    hip.close()


if __name__ == "__main__":
    main()
