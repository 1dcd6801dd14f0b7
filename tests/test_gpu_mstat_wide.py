"""Matching statistics and MEMs on an index of more than 2^32 rows (search_forms.WIDE_N = 2^32 + 2^29 + 12345 rows over
a..d, i.i.d.), in both layouts.

fmx_match_stats_batch starts k_mstat<true, kLayoutOneHot> only when n > 2^32; k_mstat<true, kLayoutBytes> runs for every
bytes-layout handle, but below this size none of its row fields ever held a value of 2^32 or more.  Here the patterns are
the first bytes of the suffixes of rows on both sides of 2^32 and of the EOF row (which lies above 2^32), each with one
replaced byte in the middle: in front of the replaced byte a walk narrows to the row itself, behind it the walks begin
anew, so row values of 2^32 and more pass through sp, ep and the 32-byte records.

Every expectation is mstat_ref.loop_stats over oracle.SampledFMSearcher (held to the inverted lists by
tests/test_oracle_kat.py), the patterns themselves come from cf / occ (helpers.forward_string); nothing of the library
produces an expectation.  The conditions the inputs must meet are computed from the expectations alone, printed and
asserted before any comparison.  The index, both handles and the oracle are made once for the module.

Seconds on the MI355X: the slowest test is the first, which makes the fixture -- SLOWEST_S, nearly all of it
the fixture; the limit of a test is three times that, the margin tests/test_gpu_search_forms.py takes for the machine's load.
"""
import gc
import time

import numpy as np
import pytest

import findex_amd
import mstat_ref
import search_forms as sf
from helpers import ends_at_a_fault, forward_string, pack_patterns

SLOWEST_S = 4
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
SYMS = b"abcd"
LAYOUTS = ("onehot", "bytes")
HIT = findex_amd.HipFMSearcher.MEM_HIT
M = 40                              # bytes per pattern: a walk is down to one row after about 17 of them
ROWS_BELOW = (12345, LINE // 3, LINE - 4097, LINE - 1)
ROWS_ABOVE = (LINE, LINE + 1, LINE + 4097, LINE + (1 << 28) + 777, sf.WIDE_N - 2)


def replaced(p, pos):
    q = bytearray(p)
    q[pos] = SYMS[0] + (q[pos] - SYMS[0] + 1 + pos % 3) % len(SYMS)
    return bytes(q)


def make_patterns(orc, eof):
    pats = []
    for row in ROWS_BELOW + ROWS_ABOVE + (eof,):
        t = forward_string(orc, row, M, SYMS)
        pats += [replaced(t, M // 2), replaced(t[:M - 7], 9), replaced(t[:31], 25), t]
    return pats


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
    eof = n - 4097                                           # above 2^32
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
    t1 = time.time()
    cores = bench.effective_cores()
    orc, _ = bench.oracle_index(torch, bwt, eof, cores, 0)
    if orc is None or not hasattr(orc, "prev_range_batch") or orc.n != n:
        pytest.fail("the host cannot hold the reference of an index of %d rows (about 3 n bytes): no matching statistics above 2^32 rows ran" % n)
    w.orc = orc
    t2 = time.time()
    w.pats = make_patterns(orc, eof)
    w.buf, w.off = pack_patterns(w.pats)
    w.exp = {cap: mstat_ref.loop_stats(orc, w.buf, w.off, cap) for cap in (4096, 24)}
    ln, sp, ep, steps = w.exp[4096]
    w.fig = {"patterns": len(w.pats), "positions": int(w.buf.size), "steps": int(steps.sum()),
             "sp>=2^32": int(((sp >= LINE) & (ln > 0)).sum()), "ep<=2^32": int(((ep <= LINE) & (ln > 0)).sum()),
             "sp<2^32<ep": int(((sp < LINE) & (LINE < ep) & (ln > 0)).sum()),
             "one_row_above": int(((ep - sp == 1) & (sp >= LINE)).sum()), "on_the_eof_row": int(((sp == eof) & (ep == eof + 1)).sum()),
             "longest": int(ln.max()), "seconds_index": round(t1 - t0, 1), "seconds_oracle_index": round(t2 - t1, 1),
             "seconds_expectations": round(time.time() - t2, 1)}
    print("wide matching statistics inputs:", w.fig)
    yield w
    for h in w.hip.values():
        h.close()
    orc.close()
    del bwt
    gc.collect()
    torch.cuda.empty_cache()


def check_inputs(w):
    fig = w.fig
    assert fig["patterns"] == 40 and fig["longest"] == M, fig
    assert fig["sp>=2^32"] >= 200 and fig["ep<=2^32"] >= 200 and fig["sp<2^32<ep"] >= 20, fig
    assert fig["one_row_above"] >= 100 and fig["on_the_eof_row"] >= 10, fig


def expected_mems(ln, sp, ep, off, min_len):
    out_off, rows = mstat_ref.mems_of(ln, off, min_len)
    hits = np.zeros(len(rows), dtype=HIT)
    for i, (q, l, end) in enumerate(rows):
        j = int(off[q]) + end - 1
        hits[i] = (q, l, end, sp[j], ep[j])
    return np.array(out_off, dtype=np.uint64), hits


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_statistics_above_two_to_the_32(wide, layout):
    """Lengths and intervals exactly, the call's steps the reference's, with and without a cap that binds."""
    check_inputs(wide)
    hip = wide.hip[layout]
    for cap, (ln, sp, ep, steps) in wide.exp.items():
        before = hip.stats()["backward_steps"]
        got_len, got_sp, got_ep = hip.match_stats_batch(wide.buf, wide.off, cap)
        ms, _, got_steps, requests = hip.mstat_last()
        print("%s max_len=%d: %d steps (reference: %d), %d requests, %.3f ms" % (layout, cap, got_steps, int(steps.sum()), requests, ms))
        assert np.array_equal(got_len, ln) and np.array_equal(got_sp, sp) and np.array_equal(got_ep, ep), cap
        assert got_steps == int(steps.sum()) and 0 < requests <= 4 * got_steps
        assert hip.stats()["backward_steps"] - before == got_steps


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_mems_above_two_to_the_32(wide, layout):
    """The CSR and the 32-byte records against mems_of, rows of 2^32 and more in them; the device form's bytes."""
    check_inputs(wide)
    torch = wide.torch
    hip = wide.hip[layout]
    for cap, min_len in ((4096, 1), (4096, 12), (24, 24)):
        ln, sp, ep, _ = wide.exp[cap]
        exp_off, exp = expected_mems(ln, sp, ep, wide.off, min_len)
        got_off, got = hip.mems_batch(wide.buf, wide.off, min_len, cap)
        assert np.array_equal(got_off, exp_off) and got.tobytes() == exp.tobytes(), (cap, min_len)
        assert int((exp["sp"] >= LINE).sum()) >= 10 and int((exp["ep"] <= LINE).sum()) >= 10, (cap, min_len)
    total, k = exp.size, wide.off.size - 1
    d_pat = torch.from_numpy(wide.buf).cuda()
    d_off = torch.from_numpy(wide.off.view(np.int64)).cuda()
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((total * HIT.itemsize + 256,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = hip.mems_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, wide.buf.size, 24, d_out_off.data_ptr(), d_out.data_ptr(), total,
                           max_len=24)
    raw = d_out.cpu().numpy()
    assert n == total and raw[: total * HIT.itemsize].tobytes() == exp.tobytes() and (raw[total * HIT.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), exp_off)
