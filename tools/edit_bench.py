#!/usr/bin/env python3
"""Edit-distance search measurements: patterns per second by the kernel's device time, hits, executed
backward steps and rank-dictionary requests of fmx_search_edit_batch_dev, the time of the ordering step, and the route a
caller had before: every string within e edits of a pattern enumerated on the host and searched with fmx_search_batch.

    python tools/edit_bench.py words28|iid28 [--k 10000] [--reps 5] [--out profiles/edit_bench.jsonl]

words28: 2^28 bytes of the words text of tools/text_bwt.py; iid28: 2^28 i.i.d. bytes over four letters.  Both indexes are
built by fmx_bwt_from_text_dev.  Batches: k patterns of 12 and of 24 bytes taken from the index by LF walks (so each occurs),
then 0 - 2 random edits each (a byte replaced, inserted or deleted; pattern j: j % 3 of them), at e = 0, 1, 2.  The enumerated
route runs at e = 1 on all patterns and at e = 2 on the first --k2 of them; its hits must be the library's.  One JSON line per
(length, e) is printed and appended to --out.
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

REQUEST_CEILING = 46.5e9        # tools/ubench/mix.hip, distinct rank-line requests per second
CHUNK_BYTES = 400 << 20         # strings of the enumerated route searched per call


def edit_patterns(rng, walked, letters):
    """The walked patterns (rows of one length) with j % 3 random edits each -> a list of bytes."""
    out = []
    for j, row in enumerate(walked):
        p = bytearray(row.tobytes())
        for _ in range(j % 3):
            kind, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(p)))
            if kind == 0:
                p[pos] = int(rng.choice(letters))
            elif kind == 1:
                p.insert(pos, int(rng.choice(letters)))
            else:
                del p[pos]
        out.append(bytes(p))
    return out


def pack_patterns(pats):
    off = np.zeros(len(pats) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pats])
    return np.frombuffer(b"".join(pats), dtype=np.uint8).copy(), off


def neighbours(S, owner, letters):
    """Every string one edit from a row of S (r x L), duplicates and the rows themselves included -> [(rows, owner)] by length."""
    r, L = S.shape
    subs, ins = [], []
    for j in range(L + 1):
        for a in letters:
            if j < L:
                T = S.copy()
                T[:, j] = a
                subs.append(T)
            ins.append(np.insert(S, j, a, axis=1))
    out = [(np.concatenate(subs), np.tile(owner, len(subs))), (np.concatenate(ins), np.tile(owner, len(ins)))]
    if L > 1:
        out.append((np.concatenate([np.delete(S, j, axis=1) for j in range(L)]), np.tile(owner, L)))
    return out


def enumerated_route(hip, pats, e, letters):
    """The hits of the patterns within e edits by enumeration: level d holds every string d edits from a pattern (not
    de-duplicated: the searches do not mind), each level is searched with fmx_search_batch, and a non-empty interval is a hit
    with the first level it shows at.  -> rows (pattern, sp, len, ep, d) sorted, the strings searched."""
    found, searched = [], 0

    def search(S, owner, level):
        nonlocal searched
        if S.shape[0] == 0:
            return
        L = S.shape[1]
        sp, ep = hip.search_batch(np.ascontiguousarray(S).reshape(-1), np.arange(S.shape[0] + 1, dtype=np.uint64) * np.uint64(L))
        searched += S.shape[0]
        ok = sp < ep
        found.append(np.stack([owner[ok].astype(np.int64), sp[ok].astype(np.int64), np.full(int(ok.sum()), L, dtype=np.int64),
                               ep[ok].astype(np.int64), np.full(int(ok.sum()), level, dtype=np.int64)], axis=1))

    by_len = {}
    for q, p in enumerate(pats):
        by_len.setdefault(len(p), []).append(q)
    level = [(np.array([np.frombuffer(pats[q], dtype=np.uint8) for q in qs]), np.array(qs)) for _, qs in sorted(by_len.items())]
    for S, owner in level:
        search(S, owner, 0)
    for d in range(1, e + 1):
        nxt = []
        for S, owner in level:
            rows = max(1, CHUNK_BYTES // max(1, (2 * S.shape[1] + 1) * len(letters) * (S.shape[1] + 1)))
            for a in range(0, S.shape[0], rows):
                for T, o in neighbours(S[a:a + rows], owner[a:a + rows], letters):
                    search(T, o, d)
                    if d < e:
                        nxt.append((T, o))
        level = nxt
    rows = np.concatenate(found) if found else np.zeros((0, 5), dtype=np.int64)
    rows = rows[np.lexsort((rows[:, 4], rows[:, 2], rows[:, 1], rows[:, 0]))]
    first = np.ones(rows.shape[0], dtype=bool)
    first[1:] = (rows[1:, :3] != rows[:-1, :3]).any(axis=1)
    return rows[first], searched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input", choices=["words28", "iid28"])
    ap.add_argument("--k", type=int, default=10_000)
    ap.add_argument("--k2", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budgets", default="0,1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import findex_amd
    from findex_amd import _lib
    L = _lib.load()
    dev = "cuda"
    t0 = time.time()
    length = 1 << 28
    if a.input == "words28":
        from text_bwt import make_text
        text = make_text(torch, length, 1, dev)
    else:
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        text = torch.randint(97, 101, (length,), dtype=torch.uint8, device=dev, generator=g)
    letters = torch.unique(text).cpu().numpy().astype(np.uint8)
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), None, ctypes.byref(eof),
                                       counts.ctypes.data, 0, None))
    del text
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    torch.cuda.synchronize()
    head = {"input": a.input, "n": n, "layout": hip.stats()["layout"], "sigma": int(letters.size), "index_s": round(time.time() - t0, 2), "k": a.k}
    print(json.dumps(head), flush=True)
    rng = np.random.default_rng(5)
    k = a.k
    lines = []
    for m in (12, 24):
        walked, _ = hip.lf_walk_batch(rng.integers(0, n, k, dtype=np.uint64), m)
        walked = np.ascontiguousarray(walked[:, ::-1])
        walked[walked == 0] = letters[0]                                  # a walk that passed the EOF row
        pats = edit_patterns(rng, walked, letters)
        buf, off = pack_patterns(pats)
        d_pat = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_sp = torch.empty(k, dtype=torch.int64, device=dev)
        d_ep = torch.empty(k, dtype=torch.int64, device=dev)
        d_out_off = torch.empty(k + 1, dtype=torch.int64, device=dev)
        # the exact search of the same batch on the rank dictionary alone: its steps are those of e = 0
        hip.config_set("jump", "off")
        hip.config_set("ktab", "off")
        hip.stats_reset()
        hip.search_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(), k)
        torch.cuda.synchronize()
        exact_steps = hip.stats()["backward_steps"]
        hip.config_set("jump", "auto")                                    # the enumerated route searches as a caller would
        hip.config_set("ktab", "auto")
        for e in [int(x) for x in a.budgets.split(",")]:
            opts = _lib.fmx_edit_opts(e, 0, 0, 0)
            n_out = ctypes.c_size_t()
            rc = L.fmx_search_edit_batch_dev(hip.handle, d_pat.data_ptr(), d_off.data_ptr(), k, ctypes.byref(opts),
                                             d_out_off.data_ptr(), None, 0, ctypes.byref(n_out), None)      # the counting call
            if rc != 9:
                _lib.check(rc)
            total = int(n_out.value)
            d_out = torch.empty(max(total, 1) * 24, dtype=torch.uint8, device=dev)
            search, sort, wall = [], [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                got = hip.search_edit_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, e, d_out_off.data_ptr(), d_out.data_ptr(), total)
                wall.append((time.perf_counter() - t) * 1e3)
                s_ms, o_ms, steps, reqs = hip.edit_last()
                search.append(s_ms)
                sort.append(o_ms)
                assert got == total
            s_ms, o_ms, w_ms = float(np.median(search)), float(np.median(sort)), float(np.median(wall))
            r = {"input": a.input, "n": n, "k": k, "m": m, "e": e, "hits": total, "search_ms": round(s_ms, 4),
                 "sort_ms": round(o_ms, 4), "call_wall_ms": round(w_ms, 4), "patterns_per_s": round(k / s_ms * 1e3),
                 "steps": steps, "requests": reqs, "requests_per_s": round(reqs / s_ms * 1e3),
                 "request_frac": round(reqs / s_ms * 1e3 / REQUEST_CEILING, 4)}
            if e == 0:
                r["exact_steps"] = int(exact_steps)
                r["steps_equal_exact"] = bool(steps == exact_steps)
                assert steps == exact_steps, (steps, exact_steps)
            else:
                # the route of the parent commit on the first kk patterns, against the host form on the same patterns
                kk = k if e == 1 else min(k, a.k2)
                sub_buf, sub_off = pack_patterns(pats[:kk])
                t = time.perf_counter()
                lib_off, lib_hits = hip.search_edit_batch(sub_buf, sub_off, e)
                lib_wall = time.perf_counter() - t
                t = time.perf_counter()
                rows, searched = enumerated_route(hip, pats[:kk], e, letters)
                enum_wall = time.perf_counter() - t
                mine = np.stack([lib_hits["pattern"].astype(np.int64), lib_hits["sp"].astype(np.int64), lib_hits["len"].astype(np.int64),
                                 lib_hits["ep"].astype(np.int64), lib_hits["edits"].astype(np.int64)], axis=1)
                assert np.array_equal(mine, rows), "the enumerated route's hits differ"
                r.update({"enumerated_patterns": kk, "enumerated_strings": int(searched), "enumerated_hits": int(rows.shape[0]),
                          "enumerated_wall_s": round(enum_wall, 3), "library_wall_s": round(lib_wall, 4),
                          "enumerated_over_library": round(enum_wall / lib_wall, 1)})
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
