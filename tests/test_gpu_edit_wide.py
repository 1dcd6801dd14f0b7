"""Edit-distance search on an index of more than 2^32 rows (fmx_search_edit_batch): the index of
tests/test_gpu_approx_wide.py -- 2^32 + 2^29 + 12345 rows over a..d, the EOF row above 2^32 -- in both layouts.

k_edit<true, kLayoutOneHot> runs only when n > 2^32, and what holds a row there needs 33 bits and more: sp and ep in a frame's
csp[] / cep[], sp << 3 in the sort key, ix.bwt[sp] and sp == ix.eof under the one-row rule, the binary search of k_ord_csr_off.
The patterns are prefixes of the suffixes of the rows 2^32 - 1, 2^32 and the EOF row (from cf / occ: helpers.forward_string),
plain and with one byte deleted or inserted; e = 0 .. 2.  The expectation is edit_ref.dfs_hits over oracle.SampledFMSearcher,
the steps are edit_ref.walk's.  The index, both handles and the oracle are made once for the module.

Seconds on the MI355X: the slowest test is the first, which makes the fixture -- SLOWEST_S, nearly all of it
the fixture; the limit of a test is three times that."""
import ctypes
import gc
import time

import numpy as np
import pytest

import approx_ref
import edit_ref
import findex_amd
import search_forms as sf
from findex_amd import _lib
from helpers import ends_at_a_fault, forward_string, pack_patterns

SLOWEST_S = 6
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
SYMS = b"abcd"
LAYOUTS = ("onehot", "bytes")
HIT = findex_amd.HipFMSearcher.EDIT_HIT
OVERFLOW = 9
PREFIX_M = (1, 2, 8, 12, 16, 17, 18, 20, 24)


def budget_of(m):
    """The largest budget a pattern of m bytes is searched with (a few long ones apart): the walk visits every string within
    e edits that occurs, and in this index every string of 16 bytes does."""
    return 2 if m <= 12 else 1


def make_patterns(orc, eof):
    """-> ({pattern: largest budget}, the long patterns that are also searched with e = 2)"""
    pats, long2 = {}, []
    for row in (LINE - 1, LINE, eof):
        t = forward_string(orc, row, max(PREFIX_M) + 1, SYMS)
        for m in PREFIX_M:
            p, mid = t[:m], m // 2
            extra = bytes([SYMS[(SYMS.index(p[mid]) + 1 + m % 3) % 4]])
            for q in (p, p[:mid] + p[mid + 1:], p[:mid] + extra + p[mid:]):
                pats.setdefault(q, budget_of(len(q)))
        long2.append(t[:17])
        if row == LINE:
            long2 += [t[:8] + t[9:18], t[:8] + bytes([SYMS[(SYMS.index(t[8]) + 1) % 4]]) + t[8:17]]
    return pats, list(dict.fromkeys(long2))


class Wide:
    pass


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
    g.manual_seed(4323)
    bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, n, step):
        b = min(n, a + step)
        bwt[a:b] = torch.randint(SYMS[0], SYMS[-1] + 1, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
    eof = n - 4097                                           # above 2^32: sp == ix.eof compares rows that need 33 bits
    torch.cuda.synchronize()
    w.n, w.eof = n, eof
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
        w.hip[layout].config_set("jump", "off")              # the exact search e = 0 is held against is to count every step
        w.hip[layout].config_set("ktab", "off")
    t1 = time.time()
    w.cores = bench.effective_cores()
    orc, _ = bench.oracle_index(torch, bwt, eof, w.cores, 0)
    if orc is None or not hasattr(orc, "prev_range_batch") or orc.n != n:
        pytest.fail("the host cannot hold the reference of an index of %d rows (about 3 n bytes): no edit search above 2^32 rows ran" % n)
    w.orc = orc
    t2 = time.time()
    assert approx_ref.occurring(orc, 1, 255).tolist() == list(SYMS)
    budget, w.long2 = make_patterns(orc, eof)
    w.full = {p: edit_ref.dfs_hits(orc, p, 2 if p in w.long2 else e) for p, e in budget.items()}
    w.batches = {}                                           # e -> (patterns, per-pattern hits, walk steps)
    for e in range(3):
        pats = [p for p, b in budget.items() if b >= e or p in w.long2]
        per = [edit_ref.within(w.full[p], e) for p in pats]
        steps = 0
        for p, want in zip(pats, per):
            hits, s = edit_ref.walk(orc, p, e)
            assert hits == want, (p, e)                      # the restated walk against the walk without shortcuts
            steps += s
        w.batches[e] = (pats, per, steps)
    rows = np.array([h for p in budget for h in w.full[p]], dtype=np.int64).reshape(-1, 4)
    sp, ln, ep, d = rows.T
    w.fig = {"patterns": len(budget), "per_budget": {e: (len(b[0]), sum(len(h) for h in b[1]), b[2]) for e, b in w.batches.items()},
             "sp>=2^32": int((sp >= LINE).sum()), "ep<=2^32": int((ep <= LINE).sum()), "sp<2^32<ep": int(((sp < LINE) & (LINE < ep)).sum()),
             "one_row_from_2^32-1": int(((ep - sp == 1) & (sp >= LINE - 1)).sum()),
             "d=2_above": int(((d == 2) & (sp >= LINE)).sum()), "on_the_eof_row": int((sp == eof).sum()),
             "seconds_index": round(t1 - t0, 1), "seconds_oracle_index": round(t2 - t1, 1), "seconds_expectations": round(time.time() - t2, 1)}
    print("wide edit inputs:", w.fig)
    yield w
    for h in w.hip.values():
        h.close()
    orc.close()
    del bwt
    gc.collect()
    torch.cuda.empty_cache()


def check_inputs(w):
    fig = w.fig
    assert fig["sp>=2^32"] >= 1000 and fig["ep<=2^32"] >= 1000 and fig["sp<2^32<ep"] >= 10, fig
    assert fig["one_row_from_2^32-1"] >= 10 and fig["d=2_above"] >= 100 and fig["on_the_eof_row"] >= 3, fig


def expected_arrays(per_pattern):
    off, rows = edit_ref.expected_csr(per_pattern)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=HIT) if rows else np.zeros(0, dtype=HIT)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_host_form_at_every_budget(wide, layout):
    """Offsets and record bytes exactly, the call's steps those of edit_ref.walk."""
    check_inputs(wide)
    hip = wide.hip[layout]
    for e in range(3):
        pats, per, steps = wide.batches[e]
        buf, off = pack_patterns(pats)
        t0 = time.time()
        got_off, got = hip.search_edit_batch(buf, off, e)
        exp_off, exp = expected_arrays(per)
        _, _, got_steps, requests = hip.edit_last()
        print("%s e = %d: %d patterns, %d hits, %d steps (walk: %d), %d requests, %.2f s"
              % (layout, e, len(pats), got.size, got_steps, steps, requests, time.time() - t0))
        assert np.array_equal(got_off, exp_off), e
        assert got.tobytes() == exp.tobytes(), e
        assert got_steps == steps and 0 < requests <= 4 * steps, (e, got_steps, steps, requests)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_budget_zero_is_the_exact_search(wide, layout):
    """e = 0 against the handle's own search_batch and the oracle's: intervals and steps."""
    check_inputs(wide)
    hip = wide.hip[layout]
    pats, per, steps = wide.batches[0]
    buf, off = pack_patterns(pats)
    hip.stats_reset()
    sp, ep = hip.search_batch(buf, off)
    exact_steps = hip.stats()["backward_steps"]
    osp, oep, osteps = wide.orc.search_batch(buf, off, threads=wide.cores)
    assert exact_steps == int(osteps.sum()) == steps
    found = osp < oep
    assert np.array_equal(sp < ep, found) and 10 < int(found.sum()) < found.size
    got_off, hits = hip.search_edit_batch(buf, off, 0)
    assert np.array_equal(np.diff(got_off.astype(np.int64)), found.astype(np.int64))
    assert np.array_equal(hits["pattern"], np.nonzero(found)[0]) and not hits["edits"].any()
    assert np.array_equal(hits["sp"], osp[found]) and np.array_equal(hits["ep"], oep[found])
    assert np.array_equal(hits["len"], np.diff(off.astype(np.int64))[found])
    _, _, got_steps, requests = hip.edit_last()
    assert got_steps == exact_steps and 0 < requests <= 4 * got_steps
    assert hip.stats()["backward_steps"] == 3 * exact_steps      # the counting call and the call that fetched the hits


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_and_capacity_one_short(wide, layout):
    """fmx_search_edit_batch_dev on a stream of its own, guard bytes behind the output; then cap = T - 1 in the host form."""
    check_inputs(wide)
    torch = wide.torch
    hip = wide.hip[layout]
    pats, per, _ = wide.batches[2]
    exp_off, exp = expected_arrays(per)
    buf, off = pack_patterns(pats)
    T, k = exp.size, len(pats)
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * HIT.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        n = hip.search_edit_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T,
                                      stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * HIT.itemsize].tobytes() == exp.tobytes() and (raw[T * HIT.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), exp_off)
    L = _lib.load()
    opts = _lib.fmx_edit_opts(2, 0, 0, 0)
    cap, guard = T - 1, 64
    out = np.full((cap + guard) * HIT.itemsize, 0xAB, dtype=np.uint8)
    out_off = np.zeros(off.size, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    rc = L.fmx_search_edit_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(opts),
                                 out_off.ctypes.data, out.ctypes.data, cap, ctypes.byref(n_out))
    if rc != OVERFLOW:
        _lib.check(rc)                                       # (a HIP error is raised, and ends the module)
    assert rc == OVERFLOW and n_out.value == T, (rc, n_out.value, T)
    assert (out[cap * HIT.itemsize:] == 0xAB).all()
    assert str(T).encode() in L.fmx_last_error()
