#!/usr/bin/env python3
"""Times index construction from text on the device: fmx_bwt_from_text_dev on device-resident text.

    python tools/build_text_bench.py [--sizes 28,30,31,32] [--inputs text,iid] [--torch-sizes 28,30] [--reps 2]

Size 32 stands for 2^32 - 2 bytes, the largest text the construction takes.  Inputs: `text` is
tools/text_bwt.make_text (words of words.txt, natural repeats; pieces of 2^30 bytes with seeds 1, 2, ... one after the
other -- the generator takes fewer than 2^31 bytes at a time), `iid` i.i.d. bytes 1..128.  Per run it prints one JSON
line: the wall time of the call, the allocation time inside it (hipMalloc can wait on a device whose memory was just
released), the rounds of the prefix doubling with the suffixes still active in each, and each round's modelled bytes
over its kernel time as a share of the 6.3 TB/s HBM rate.  At the --torch-sizes it also times the torch prefix-doubling
tool (text_bwt.bwt_of_reversed_text) on the same text, alternating with the new builder in the same process, and checks
that both give the same BWT.  The per-round numbers come from the library's FMX_SUFSORT_LOG file.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BPS = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="28,30,31,32")
    ap.add_argument("--inputs", default="text,iid")
    ap.add_argument("--torch-sizes", default="28,30")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    log_path = tempfile.mktemp(prefix="sufsort_", suffix=".jsonl")
    os.environ["FMX_SUFSORT_LOG"] = log_path
    import torch
    import findex_amd
    import text_bwt
    findex_amd.load()
    dev = torch.device("cuda", 0)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def last_log():
        with open(log_path) as f:
            return json.loads(f.read().strip().split("\n")[-1])

    def build(text, length):
        bwt = torch.empty(length + 1, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eof, _ = findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), 0, device=0)
        wall = time.perf_counter() - t0
        return bwt, eof, wall, last_log()

    def torch_tool(text):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bwt, eof = text_bwt.bwt_of_reversed_text(torch, text)
        torch.cuda.synchronize()
        return bwt, eof, time.perf_counter() - t0

    torch_sizes = {int(x) for x in a.torch_sizes.split(",") if x}
    for lg in (int(x) for x in a.sizes.split(",")):
        length = (1 << 32) - 2 if lg == 32 else 1 << lg
        for kind in a.inputs.split(","):
            if kind == "text":      # in pieces of at most 2^30 bytes: make_text's searchsorted takes < 2^31 positions
                parts, left = [], length
                while left:
                    parts.append(text_bwt.make_text(torch, min(left, 1 << 30), len(parts) + 1, dev))
                    left -= parts[-1].numel()
                text = torch.cat(parts) if len(parts) > 1 else parts[0]
                del parts
            else:
                g = torch.Generator(device=dev)
                g.manual_seed(lg)
                text = torch.randint(1, 129, (length,), generator=g, device=dev, dtype=torch.uint8)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            compare = kind == "text" and lg in torch_sizes
            for rep in range(a.reps):
                bwt, eof, wall, log = build(text, length)
                kern = sum(r["kernel_ms"] for r in log["rounds"])
                rounds = [{"h": r["h"], "active": r["active"], "passes": r["passes"], "kernel_ms": r["kernel_ms"],
                           "hbm_share": round(r["bytes"] / (r["kernel_ms"] * 1e-3) / HBM_BPS, 3) if r["kernel_ms"] else None}
                          for r in log["rounds"]]
                rec = {"what": "fmx_bwt_from_text_dev", "input": kind, "len": length, "rep": rep, "wall_s": round(wall, 4),
                       "alloc_ms": log["alloc_ms"], "rounds_kernel_ms": round(kern, 2), "n_rounds": len(rounds),
                       "peak_bytes": log["peak_bytes"], "bytes_per_text_byte": round(log["peak_bytes"] / length, 2),
                       "modelled_bytes": sum(r["bytes"] for r in log["rounds"]),
                       "hbm_share_overall": round(sum(r["bytes"] for r in log["rounds"]) / (kern * 1e-3) / HBM_BPS, 3),
                       "rounds": rounds}
                emit(rec)
                if compare:
                    del bwt
                    torch.cuda.empty_cache()
                    tb, teof, twall = torch_tool(text)
                    same = None
                    if rep == 0:
                        nb, neof, _, _ = build(text, length)
                        same = bool(neof == teof and torch.equal(nb, tb))
                        del nb
                    del tb
                    torch.cuda.empty_cache()
                    emit({"what": "text_bwt.bwt_of_reversed_text", "input": kind, "len": length, "rep": rep,
                          "wall_s": round(twall, 4), "same_bwt": same})
                else:
                    del bwt
                torch.cuda.empty_cache()
            del text
            torch.cuda.empty_cache()
    os.unlink(log_path)


if __name__ == "__main__":
    main()
