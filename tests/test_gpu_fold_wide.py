"""The search under a fold map on an index of more than 2^32 rows (search_forms.WIDE_N = 2^32 + 2^29 + 12345 rows over a..d,
i.i.d.), in both layouts: k_fold<true, kLayoutOneHot> starts only when n > 2^32, and below this size no row field of
k_fold<true, kLayoutBytes> ever held a value of 2^32 or more.  Here rows on both sides of 2^32 pass through all of them: the
{sp, ep, i} entries of a wave's stack, the sort key pattern << 38 | sp, the binary search of the CSR offsets, ix.bwt[sp] and
sp == ix.eof under the one-row rule (the EOF slot lies above 2^32), and the 24-byte records.

The map pairs a with b and c with d, so every position of a pattern branches and a pattern of m bytes has 2^m spellings, all
of which occur while 4^m is well below n; behind depth 16 the nodes hold one row each and the one-row rule thins the tree
again, so a pattern of 24 bytes costs some 300 000 steps and ends with some 300 hits.  Every expectation comes from oracle.SampledFMSearcher: the hits from
fold_ref.dfs_hits, which tries every member at every position and has no one-row shortcut, the step counts from fold_ref.walk,
the patterns themselves from cf / occ (helpers.forward_string).  Nothing of the library produces an expectation; the
conditions the inputs must meet are computed from the expectations alone and asserted before any comparison.  All spellings
of a string share one expectation -- that they do is the definition -- so the references walk each string once.

Seconds on the MI355X: the slowest test is the first, which makes the fixture -- SLOWEST_S, nearly all of it
the fixture; the limit of a test is three times that.
"""
import ctypes
import gc
import time

import numpy as np
import pytest

import approx_ref
import findex_amd
import fold_ref
import search_forms as sf
from findex_amd import _lib
from helpers import ends_at_a_fault, forward_string, pack_patterns

SLOWEST_S = 4
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
SYMS = b"abcd"
PAIRS = fold_ref.make_map([b"ab", b"cd"])
PARTNER = {97: 98, 98: 97, 99: 100, 100: 99}
LAYOUTS = ("onehot", "bytes")
REC = findex_amd.HipFMSearcher.RESULT
OVERFLOW = 9
PREFIX_M = (1, 2, 3, 8, 12)
LONG_M = 24                         # 4^16 = 2^32: some 2^16 spellings are alive at depth 16, and from there on one row each
ROWS_BELOW = (12345, LINE // 3, LINE - 4097)
ROWS_ABOVE = (LINE + 4097, LINE + (1 << 28) + 777, sf.WIDE_N - 2)


def pairings(p):
    """p with its first, a middle and its last byte each as it is or as its partner: all pairings."""
    out = []
    where = sorted({0, len(p) // 2, len(p) - 1})
    for mask in range(1 << len(where)):
        q = bytearray(p)
        for j, pos in enumerate(where):
            if mask >> j & 1:
                q[pos] = PARTNER[q[pos]]
        out.append(bytes(q))
    return out


class Wide:
    pass


def build_expectations(w, orc, eof):
    assert approx_ref.occurring(orc, 1, 255).tolist() == list(SYMS)
    memo = {}                                                # folded string -> (hits, steps)

    def expect(p):
        key = bytes(PAIRS[c] for c in p)
        if key not in memo:
            hits, steps, _ = fold_ref.walk(orc, key, PAIRS)
            assert hits == fold_ref.dfs_hits(orc, key, PAIRS), key
            memo[key] = (hits, steps)
        return memo[key]

    pats = []
    rows = (LINE - 1, LINE, eof) + ROWS_BELOW + ROWS_ABOVE
    for row in rows:
        t = forward_string(orc, row, LONG_M, SYMS)
        for m in PREFIX_M + ((LONG_M,) if row in (LINE - 1, LINE, eof) else ()):
            pats += pairings(t[:m])
    w.stem = forward_string(orc, eof, LONG_M - 1, SYMS)
    pats += [bytes([x]) + w.stem for x in SYMS]              # one byte in front of the EOF row's suffix
    pats += [bytes([a]) for a in SYMS] + [bytes([a, b]) for a in SYMS for b in SYMS]
    w.pats = list(dict.fromkeys(pats))
    w.per = [expect(p)[0] for p in w.pats]
    w.steps = sum(expect(p)[1] for p in w.pats)
    w.short = [j for j, p in enumerate(w.pats) if len(p) <= 12]
    rows = np.array([h for hs in w.per for h in hs], dtype=np.int64).reshape(-1, 2)
    sp, ep = rows[:, 0], rows[:, 1]
    w.fig = {"patterns": len(w.pats), "strings": len(memo), "hits": int(sp.size), "steps": w.steps,
             "sp>=2^32": int((sp >= LINE).sum()), "ep<=2^32": int((ep <= LINE).sum()), "sp<2^32<ep": int(((sp < LINE) & (LINE < ep)).sum()),
             "one_row_above": int(((ep - sp == 1) & (sp >= LINE)).sum()), "most_hits_of_one_pattern": max(len(h) for h in w.per)}


@pytest.fixture(scope="module")
def wide():
    import torch
    import bench
    w = Wide()
    w.torch = torch
    t0 = time.time()
    gc.collect()
    torch.cuda.empty_cache()
    n = sf.WIDE_N
    g = torch.Generator(device="cuda")
    g.manual_seed(4328)
    bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, n, step):
        b = min(n, a + step)
        bwt[a:b] = torch.randint(SYMS[0], SYMS[-1] + 1, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
    eof = n - 4097                                           # above 2^32: sp == ix.eof compares rows that need 33 bits
    torch.cuda.synchronize()
    w.n, w.eof, w.bwt = n, eof, bwt
    w.hip = {}
    try:
        for layout in LAYOUTS:
            findex_amd.set_layout(layout)
            w.hip[layout] = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, None)
    finally:
        findex_amd.set_layout("auto")
    for layout, code in (("onehot", sf.ONEHOT), ("bytes", sf.BYTES)):
        st = w.hip[layout].stats()
        assert st["layout"] == code and w.hip[layout].n == n > LINE and eof > LINE, (layout, st["layout"], w.hip[layout].n)
    t1 = time.time()
    w.cores = bench.effective_cores()
    orc, _ = bench.oracle_index(torch, bwt, eof, w.cores, 0)
    if orc is None or not hasattr(orc, "getPrevRange") or orc.n != n:
        pytest.fail("the host cannot hold the reference of an index of %d rows (about 3 n bytes): no fold search above 2^32 rows ran" % n)
    w.orc = orc
    t2 = time.time()
    build_expectations(w, orc, eof)
    w.fig.update({"seconds_index": round(t1 - t0, 1), "seconds_oracle_index": round(t2 - t1, 1),
                  "seconds_expectations": round(time.time() - t2, 1)})
    print("wide fold inputs:", w.fig)
    yield w
    for h in w.hip.values():
        h.close()
    orc.close()
    del w.bwt, bwt
    gc.collect()
    torch.cuda.empty_cache()


def check_inputs(w):
    fig = w.fig
    assert fig["sp>=2^32"] >= 1000 and fig["ep<=2^32"] >= 1000 and fig["sp<2^32<ep"] >= 10, fig
    assert fig["one_row_above"] >= 100 and fig["most_hits_of_one_pattern"] >= 4096, fig
    # the EOF row's own suffix is found; one byte in front of it the row's BWT' symbol reads 0: no hit on that row
    j = w.pats.index(forward_string(w.orc, w.eof, LONG_M, SYMS))
    assert (w.eof, w.eof + 1) in w.per[j]
    for x in SYMS:
        hits = w.per[w.pats.index(bytes([x]) + w.stem)]
        assert all(sp != w.eof for sp, _ in hits)
    assert [len(w.per[w.pats.index(bytes([a]))]) for a in SYMS] == [2] * 4
    assert [len(w.per[w.pats.index(bytes([a, b]))]) for a in SYMS for b in SYMS] == [4] * 16


def expected_arrays(pats, per):
    off, rows = fold_ref.expected_csr(pats, per)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=REC) if rows else np.zeros(0, dtype=REC)


def opts():
    o = _lib.fmx_fold_opts()
    ctypes.memmove(o.fold, PAIRS, 256)
    return o


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_host_form(wide, layout):
    """Offsets and record bytes exactly, the call's steps those of fold_ref.walk."""
    check_inputs(wide)
    hip = wide.hip[layout]
    buf, off = pack_patterns(wide.pats)
    exp_off, exp = expected_arrays(wide.pats, wide.per)
    t0 = time.time()
    got_off, got = hip.search_fold_batch(buf, off, PAIRS, cap=exp.size)
    _, _, got_steps, requests = hip.fold_last()
    print("%s: %d patterns, %d hits, %d steps (walk: %d), %d requests, %.2f s"
          % (layout, len(wide.pats), got.size, got_steps, wide.steps, requests, time.time() - t0))
    assert np.array_equal(got_off, exp_off)
    assert got.tobytes() == exp.tobytes()
    assert got_steps == wide.steps and 0 < requests <= 4 * got_steps


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_on_a_side_stream(wide, layout):
    """fmx_search_fold_batch_dev on a stream of its own over the patterns of at most 12 bytes, guard bytes behind the output."""
    check_inputs(wide)
    torch = wide.torch
    hip = wide.hip[layout]
    pats = [wide.pats[j] for j in wide.short]
    exp_off, exp = expected_arrays(pats, [wide.per[j] for j in wide.short])
    buf, off = pack_patterns(pats)
    T, k = exp.size, len(pats)
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * REC.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        n = hip.search_fold_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T, fold=PAIRS,
                                      stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * REC.itemsize].tobytes() == exp.tobytes() and (raw[T * REC.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), exp_off)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_capacity_one_short(wide, layout):
    """cap = T - 1: FMX_ERR_OVERFLOW, the exact total, nothing written behind the capacity."""
    check_inputs(wide)
    hip = wide.hip[layout]
    pats = [wide.pats[j] for j in wide.short]
    T = sum(len(wide.per[j]) for j in wide.short)
    buf, off = pack_patterns(pats)
    L = _lib.load()
    o = opts()
    cap, guard = T - 1, 64
    out = np.full((cap + guard) * REC.itemsize, 0xAB, dtype=np.uint8)
    out_off = np.zeros(off.size, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    rc = L.fmx_search_fold_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(o), out_off.ctypes.data,
                                 out.ctypes.data, cap, ctypes.byref(n_out))
    if rc != OVERFLOW:
        _lib.check(rc)                                       # (a HIP error is raised, and ends the module)
    assert rc == OVERFLOW and n_out.value == T, (rc, n_out.value, T)
    assert (out[cap * REC.itemsize:] == 0xAB).all()
    assert str(T).encode() in L.fmx_last_error()
