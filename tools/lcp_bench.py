#!/usr/bin/env python3
"""LCP measurements: the suffix sort and the LCP core alternated in one process on the same input
(device events around each call, a warm-up call of each first), the core's three phases, the handle's build
(prepare(lcp=True): inversion + core), 1 M random getLCP rows through lcp_dev, max / mean LCP.

    python tools/lcp_bench.py [--inputs text28,text30,iid30] [--reps 2] [--out profiles/lcp_bench.jsonl]

text28 / text30: 2^28 / 2^30 bytes of the words text of tools/text_bwt.py; iid30: 2^30 i.i.d. bytes 1..128.
--core-only skips the handle part (for a kernel trace of the core alone).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_input(torch, name, dev):
    if name.startswith("text"):
        from text_bwt import make_text
        return make_text(torch, 1 << int(name[4:]), 1, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    return torch.randint(1, 129, (1 << int(name[3:]),), dtype=torch.uint8, device=dev, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="text28,text30,iid30")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--core-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd.construct import lcp_last_phases
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    for name in a.inputs.split(","):
        text = make_input(torch, name, dev)
        length = text.numel()
        n = length + 1
        bwt = torch.empty(n, dtype=torch.uint8, device=dev)
        sa = torch.empty(n, dtype=torch.int32, device=dev)
        lcp = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def sort():
            return findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), sa.data_ptr(), device=0, stream=st)

        def core():
            findex_amd.lcp_from_text_dev(text.data_ptr(), length, sa.data_ptr(), lcp.data_ptr(), device=0, stream=st)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), r

        sort()                                                 # warm-up of both
        core()
        sort_ms, core_ms, phases = [], [], []
        for _ in range(a.reps):                                # alternated: the same clocks and the same memory state for both
            ms, (eof, counts) = timed(sort)
            sort_ms.append(ms)
            ms, _ = timed(core)
            core_ms.append(ms)
            phases.append(lcp_last_phases())
        l64 = lcp.to(torch.int64) & 0xFFFFFFFF
        mx, total = int(l64.max().item()), int(l64.sum().item())
        del l64
        best = int(np.argmin(core_ms))
        phi_ms, plcp_ms, gather_ms = phases[best]
        kernels_ms = phi_ms + plcp_ms + gather_ms
        r = {"input": name, "n": n, "sort_ms": [round(x, 2) for x in sort_ms], "core_ms": [round(x, 2) for x in core_ms],
             "k_lcp_phi_ms": round(phi_ms, 2), "k_lcp_plcp_ms": round(plcp_ms, 2), "k_lcp_gather_ms": round(gather_ms, 2),
             "core_kernels_ms": round(kernels_ms, 2), "core_kernels_over_sort": round(kernels_ms / min(sort_ms), 3),
             "core_call_over_sort": round(min(core_ms) / min(sort_ms), 3),
             "max_lcp": mx, "mean_lcp": round(total / n, 3)}
        if not a.core_only:
            del text, sa
            torch.cuda.empty_cache()
            hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, counts)
            builds = []
            for _ in range(a.reps):
                hip.drop_tables(jump=False, frontier=False, lcp=True)
                torch.cuda.synchronize()
                hip.prepare(ktab=False, lcp=True)
                builds.append(hip.lcp_info()[1])
            out = torch.empty(n, dtype=torch.int32, device=dev)
            hip.lcp_range_dev(0, n, out.data_ptr(), stream=st)
            torch.cuda.synchronize()
            r["handle_equals_core"] = bool(torch.equal(out, lcp))
            del out
            rng = np.random.default_rng(3)
            rows = torch.from_numpy(rng.integers(0, n, 1 << 20, dtype=np.uint64).view(np.int64)).to(dev)
            got = torch.empty(rows.numel(), dtype=torch.int32, device=dev)
            hip.lcp_dev(rows.data_ptr(), rows.numel(), got.data_ptr(), stream=st)          # warm
            ts = [timed(lambda: hip.lcp_dev(rows.data_ptr(), rows.numel(), got.data_ptr(), stream=st))[0] for _ in range(5)]
            r["handle_build_ms"] = [round(x, 1) for x in builds]
            r["getLCP_1M_ms"] = round(float(np.median(ts)), 4)
            hip.close()
            del rows, got
        else:
            del text, sa
        del bwt, lcp
        torch.cuda.empty_cache()
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
