#!/usr/bin/env python3
"""Append measurements on texts of tools/text_bwt.py, one session, three repetitions of every figure.

    python tools/merge_bench.py [--sections append,sweep,slow,beyond] [--a-bits 28] [--out profiles/merge_bench.jsonl]

  append : a = 2^a_bits indexed; b = 2^20, 2^24, 2^26 appended (fmx_append_text_dev, then fmx_open_dev on its output) against
           the construction of A + B from scratch (fmx_bwt_from_text_dev, then fmx_open_dev): wall-clock ms of both routes
           with the handle open, the phases of fmx_merge_last, their ratio.  CONDITION: for b <= a / 16 the append takes less
           time than the rebuild in every repetition (asserted).
  sweep  : b = 2^24 with segment in {64, 256, 1024} x warmup in {16, 32, 64}: walk and fix-up ms, steps, walk steps per second.
  slow   : B = a copy of 2^22 bytes of A inside otherwise new text: the fix-up's time and steps -- the documented slow case.
  beyond : one text of 2^32 + 2^28 bytes through HipFMSearcher.from_text(text, chunk=2^30): seconds per chunk, peak HBM, 10^5
           substrings of the text searched (all must be found), the first and the last MiB extracted and compared.

One JSON line per figure, appended to --out.  Times are wall-clock around the calls (ms) unless they are named after a phase
(device events)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPS = 3


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def make(torch, text_bwt, n, seed, dev):
    """n bytes of text in pieces of at most 2^30 (the generator's searchsorted takes fewer than 2^31 positions)"""
    parts, left = [], n
    while left:
        parts.append(text_bwt.make_text(torch, min(left, 1 << 30), seed, dev))
        left -= parts[-1].numel()
        seed += 1
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def open_index(torch, findex_amd, text):
    """fmx_bwt_from_text_dev + fmx_open_dev -> (handle, ms)"""
    n = text.numel() + 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bwt = torch.empty(n, dtype=torch.uint8, device=text.device)
    eof, counts = findex_amd.bwt_from_text_dev(text.data_ptr(), text.numel(), bwt.data_ptr(), 0, device=0)
    hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, counts)
    torch.cuda.synchronize()
    return hip, (time.perf_counter() - t0) * 1e3, bwt


def append_index(torch, findex_amd, hip, text, **opts):
    """fmx_append_text_dev + fmx_open_dev -> (handle, ms, merge_last, merged bwt)"""
    n_t = hip.n + text.numel()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = torch.empty(n_t, dtype=torch.uint8, device=text.device)
    eof, counts = hip.append_text_dev(text.data_ptr(), text.numel(), out.data_ptr(), **opts)
    new = findex_amd.HipFMSearcher.from_device(out.data_ptr(), n_t, eof, counts)
    torch.cuda.synchronize()
    return new, (time.perf_counter() - t0) * 1e3, hip.merge_last(), out


def section_append(torch, findex_amd, text_bwt, a_bits, out, dev):
    a = 1 << a_bits
    A = make(torch, text_bwt, a, 1, dev)
    base, base_ms, _ = open_index(torch, findex_amd, A)
    emit(out, {"section": "base", "a_bits": a_bits, "build_ms": round(base_ms, 1)})
    for b_bits in (20, 24, 26):
        B = make(torch, text_bwt, 1 << b_bits, 100 + b_bits, dev)
        whole = torch.cat([A, B])
        for rep in range(REPS):
            new, app_ms, st, merged = append_index(torch, findex_amd, base, B)
            new.close()
            ref, reb_ms, rebuilt = open_index(torch, findex_amd, whole)
            ref.close()
            same = bool(torch.equal(merged, rebuilt))
            del merged, rebuilt
            rec = {"section": "append", "a_bits": a_bits, "b_bits": b_bits, "rep": rep, "append_ms": round(app_ms, 1),
                   "rebuild_ms": round(reb_ms, 1), "rebuild_over_append": round(reb_ms / app_ms, 2), "equal": same}
            rec.update({k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()})
            emit(out, rec)
            assert same, "append and rebuild disagree"
            if (1 << b_bits) * 16 <= a:
                assert app_ms < reb_ms, "CONDITION: appending b <= a / 16 must take less time than the rebuild"
        del B, whole
        torch.cuda.empty_cache()
    return base, A


def section_sweep(torch, findex_amd, text_bwt, base, out, dev, request_ceiling):
    B = make(torch, text_bwt, 1 << 24, 124, dev)
    buf = torch.empty(base.n + B.numel(), dtype=torch.uint8, device=dev)
    for S in (64, 256, 1024):
        for W in (16, 32, 64):
            for rep in range(REPS):
                base.append_text_dev(B.data_ptr(), B.numel(), buf.data_ptr(), segment=S, warmup=W)
                st = base.merge_last()
                emit(out, {"section": "sweep", "b_bits": 24, "segment": S, "warmup": W, "rep": rep, "walk_ms": round(st["walk_ms"], 3),
                           "fixup_ms": round(st["fixup_ms"], 3), "walk_steps": st["walk_steps"], "fixup_steps": st["fixup_steps"],
                           "runs": st["runs"], "longest_run": st["longest_run"],
                           "walk_steps_per_s": round(st["walk_steps"] / max(st["walk_ms"], 1e-6) * 1e3),
                           "request_ceiling_per_s": request_ceiling})
    del buf


def section_slow(torch, findex_amd, text_bwt, base, A, out, dev):
    new_text = make(torch, text_bwt, 1 << 23, 200, dev)
    B = torch.cat([new_text[: 1 << 21], A[12345: 12345 + (1 << 22)], new_text[1 << 21:]])
    buf = torch.empty(base.n + B.numel(), dtype=torch.uint8, device=dev)
    for rep in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base.append_text_dev(B.data_ptr(), B.numel(), buf.data_ptr())
        ms = (time.perf_counter() - t0) * 1e3
        st = base.merge_last()
        emit(out, {"section": "slow", "b": B.numel(), "copied": 1 << 22, "rep": rep, "append_ms": round(ms, 1), "walk_ms": round(st["walk_ms"], 3),
                   "fixup_ms": round(st["fixup_ms"], 1), "fixup_steps": st["fixup_steps"], "longest_run": st["longest_run"], "runs": st["runs"],
                   "fixup_steps_per_s": round(st["fixup_steps"] / max(st["fixup_ms"], 1e-6) * 1e3), "context": st["context"], "rounds": st["rounds"]})


def section_beyond(torch, findex_amd, text_bwt, out, dev):
    total, chunk = (1 << 32) + (1 << 28), 1 << 30
    text = make(torch, text_bwt, total, 300, dev).cpu().numpy()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    low, needs = [free0], []
    t0 = time.perf_counter()
    cur = findex_amd.HipFMSearcher.from_text(text[:chunk])
    per_chunk = [round(time.perf_counter() - t0, 2)]
    for lo in range(chunk, total, chunk):
        t1 = time.perf_counter()
        nxt = cur.append_text(text[lo: lo + chunk])
        low.append(torch.cuda.mem_get_info()[0])             # (the old and the new handle both open)
        needs.append(nxt.merge_last()["need_bytes"])
        cur.close()
        cur = nxt
        per_chunk.append(round(time.perf_counter() - t1, 2))
        emit(out, {"section": "beyond-chunk", "rows": cur.n, "seconds": per_chunk[-1], "merge": {k: (round(v, 1) if isinstance(v, float) else v)
                                                                                                 for k, v in cur.merge_last().items()}})
    rng = np.random.default_rng(5)
    starts = rng.integers(0, total - 24, 100000)
    pats = [bytes(text[s: s + 24][::-1]) for s in starts]
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    sp, ep = cur.search_batch(np.frombuffer(b"".join(pats), dtype=np.uint8).copy(), off)
    found = int((sp < ep).sum())
    _, first = cur.extract_text_batch([0], [1 << 20])
    _, last = cur.extract_text_batch([total - (1 << 20)], [1 << 20])
    ok = bool(np.array_equal(first, text[: 1 << 20]) and np.array_equal(last, text[total - (1 << 20):]))
    emit(out, {"section": "beyond", "bytes": total, "chunk": chunk, "seconds_per_chunk": per_chunk, "seconds": round(time.perf_counter() - t0, 1),
               "hbm_free_at_start": free0, "hbm_free_lowest_between_chunks": min(low), "largest_need_bytes": max(needs),
               "searched": len(pats), "found": found, "extract_equal": ok})
    cur.close()
    assert found == len(pats) and ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="append,sweep,slow,beyond")
    ap.add_argument("--a-bits", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.jsonl"))
    ap.add_argument("--request-ceiling", type=float, default=46e9, help="independent 64-byte requests per second (README)")
    a = ap.parse_args()
    import torch
    import findex_amd
    import text_bwt
    dev = torch.device("cuda", 0)
    sections = a.sections.split(",")
    base = A = None
    if any(s in sections for s in ("append", "sweep", "slow")):
        if "append" in sections:
            base, A = section_append(torch, findex_amd, text_bwt, a.a_bits, a.out, dev)
        else:
            A = make(torch, text_bwt, 1 << a.a_bits, 1, dev)
            base, _, _ = open_index(torch, findex_amd, A)
        if "sweep" in sections:
            section_sweep(torch, findex_amd, text_bwt, base, a.out, dev, a.request_ceiling)
        if "slow" in sections:
            section_slow(torch, findex_amd, text_bwt, base, A, a.out, dev)
        base.close()
        del A
        torch.cuda.empty_cache()
    if "beyond" in sections:
        section_beyond(torch, findex_amd, text_bwt, a.out, dev)


if __name__ == "__main__":
    main()
