"""The three features with 32-bit positions -- the LCP array on a handle, fmx_repeats (18) and
fmx_occurrences (20) -- on a text of m = 3 * 2^30 + 4099 bytes, in both layouts.  All three refuse n >= 2^32, so their hard
zone is 2^31 <= n < 2^32: here a third of the rows, of the SA values and of the text positions carry their top bit, and with
them every `row + 1` class id, every `pos << lb` key field (pb = 32) and every u32 sample that locate reads.

The text is tests/planted_text.py's plan written over i.i.d. a..d bytes on the device; every expectation is a closed form of
the plan (held to the from-the-definition references by tests/test_planted_text_cpu.py on the same geometry scaled down).
Nothing of the library produces an expectation: its suffix sort and its search supply inputs only -- the rows and intervals
to ask about -- and their sizes and SA values are asserted against the plan.  The conditions the inputs must meet are
computed from the plan alone, printed and asserted by the fixture before any comparison.  A natural repeat of 64 bytes in the
background (chance below 2^-66) would fail the first LCP test.

The module prints the seconds of the fixture and of every case (DESIGN.md 6 has one run's figures).  Every repeats call
inverts the index once (HipFMSearcher.repeats twice: the counting call and the sized one), every first occurrences call of a
handle builds its locate samples by one more inversion: that is where the seconds of those cases go.
"""
import ctypes
import functools
import gc
import time

import numpy as np
import pytest

import findex_amd
import occ_ref
import planted_text as pt
from findex_amd import _lib
from helpers import ends_at_a_fault
from test_gpu_lcp import _sort_on_device, _verify_on_device
from test_gpu_repeats import raw_call

pytestmark = pytest.mark.gpu

LINE = 1 << 31
LAYOUTS = ("onehot", "bytes")
MODES = ("all", "longest", "disjoint")
OVERFLOW = 9
H = findex_amd.HipFMSearcher
OCC = occ_ref.OCC
M32 = 0xFFFFFFFF


def case(test):
    """ends_at_a_fault, and the case's seconds on stdout."""
    guarded = ends_at_a_fault(test)

    @functools.wraps(test)
    def run(*args, **kw):
        t0 = time.time()
        try:
            return guarded(*args, **kw)
        finally:
            print("top bit: %s(%s) %.1f s" % (test.__name__, ", ".join(str(v) for v in kw.values() if isinstance(v, (str, int))), time.time() - t0))
    return run


class Top:
    pass


def u32(t):
    """An int32 tensor's entries as the unsigned values they hold (int64)."""
    return t.long() & M32


@pytest.fixture(scope="module")
def top():
    import torch
    w = Top()
    w.torch = torch
    t0 = time.time()
    gc.collect()
    torch.cuda.empty_cache()
    plan = w.plan = pt.gpu_plan()
    pt.check_blocks(plan)
    w.fig = pt.check_inputs(plan)
    m = w.m = plan.m
    n = w.n = m + 1
    assert m == (3 << 30) + 4099 and LINE < n < 1 << 32
    free = torch.cuda.mem_get_info()[0]
    if free < 40 * n:
        pytest.fail("%.0f GB of HBM are free, the suffix sort of %d bytes needs about 37 n = %.0f GB beside the text: nothing ran above 2^31 rows"
                    % (free / 1e9, m, 37 * n / 1e9))
    g = torch.Generator(device="cuda")
    g.manual_seed(2031)
    text = torch.empty(m, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, m, step):
        b = min(m, a + step)
        text[a:b] = torch.randint(pt.SYMS[0], pt.SYMS[-1] + 1, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
    for at, data in pt.pieces(plan):
        text[at:at + len(data)] = torch.tensor(list(data), dtype=torch.uint8, device="cuda")
    t1 = time.time()
    bwt, sa, eof, counts = _sort_on_device(torch, text)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    t2 = time.time()
    assert int(counts[pt.STOP]) == 5 and m - 100 < int(counts[pt.SYMS[0]:pt.SYMS[-1] + 1].sum()) < m
    w.hip = {}
    try:
        for layout in LAYOUTS:
            findex_amd.set_layout(layout)
            w.hip[layout] = H.from_device(bwt.data_ptr(), n, eof, counts)
    finally:
        findex_amd.set_layout("auto")
    del bwt
    torch.cuda.empty_cache()
    for layout, code in zip(LAYOUTS, (0, 1)):
        assert w.hip[layout].stats()["layout"] == code and w.hip[layout].n == n
        w.hip[layout].config_set("jump", "off")              # hip.search only supplies intervals here: no table is worth
        w.hip[layout].config_set("ktab", "off")              # its build at this size
    # the inverse of the sort's SA by one scatter, a chunk of rows at a time: row_of[SA[r]] = r
    row_of = torch.empty(n, dtype=torch.int32, device="cuda")
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        r = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        row_of[sa[lo:hi].to(torch.int64) & M32] = torch.where(r >= LINE, r - (1 << 32), r).to(torch.int32)
    del r
    w.text, w.sa, w.row_of = text, sa, row_of
    # what the LCP test asks about, from the plan; the rows from the sort, held to the plan: the suffixes of one class stand
    # in consecutive rows in the order the plan says
    v, nxt, val = pt.lcp_planted(plan)
    w.lcp_val = torch.from_numpy(val.astype(np.int64)).cuda()
    w.lcp_rows = u32(row_of[torch.from_numpy(v.astype(np.int64)).cuda()])
    assert bool(torch.equal(u32(sa[w.lcp_rows + 1]), torch.from_numpy(nxt.astype(np.int64)).cuda()))
    rows = w.lcp_rows.cpu().numpy()
    w.fig.update({"lcp_rows_below": int((rows < LINE).sum()), "lcp_rows_above": int((rows >= LINE).sum()),
                  "rows_above_line": n - LINE, "seconds_text": round(t1 - t0, 1), "seconds_sort": round(t2 - t1, 1),
                  "seconds_handles_and_inverse": round(time.time() - t2, 1)})
    print("top bit inputs:", w.fig)
    assert w.fig["lcp_rows_below"] > 0 and w.fig["lcp_rows_above"] > 0
    w.lcp = {}
    torch.cuda.synchronize()
    print("top bit: fixture %.1f s" % (time.time() - t0))
    yield w
    for h in w.hip.values():
        h.close()
    del w.text, w.sa, w.row_of, w.lcp, text, sa, row_of
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 1. the LCP array of a handle
@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_lcp_on_the_handle_every_row(top, layout):
    torch, plan, n, hip = top.torch, top.plan, top.n, top.hip[layout]
    hip.prepare(ktab=False, lcp=True)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    hip.lcp_range_dev(0, n, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    # every row: a mismatch behind LCP[r] bytes, and the bytes in front of it equal -- all of them where LCP[r] < L0
    mx, total = _verify_on_device(torch, top.text, top.sa, out, cap=plan.L0)
    # the rows of L0 and more are the planted ones, each with the value the plan gives it
    big = torch.cat([lo + torch.nonzero((out[lo:lo + (1 << 30)] >= plan.L0) | (out[lo:lo + (1 << 30)] < 0)).reshape(-1)
                     for lo in range(0, n, 1 << 30)])
    print("top bit: %s LCP: %d rows of %d and more (plan: %d), max %d, mean %.3f" % (layout, big.numel(), plan.L0, top.lcp_rows.numel(), mx, total / n))
    assert big.numel() == top.lcp_rows.numel() == top.fig["lcp_rows"]
    assert bool(torch.equal(big, torch.sort(top.lcp_rows)[0]))
    assert bool(torch.equal(u32(out[top.lcp_rows]), top.lcp_val))
    # lcp_info: the maximum is X whole, at the first of the four rows that hold it
    nbytes, ms, imx, irow, itotal = hip.lcp_info()
    x = len(plan.block["X"])
    first = int(top.lcp_rows[top.lcp_val == x].min().item())
    assert (nbytes, imx, irow) == (4 * n, x, first) and mx == x, (nbytes, imx, irow, first, mx)
    assert itotal == total == int(torch.sum(out, dtype=torch.int64).item())
    # lcp_dev on u64 rows: the range read's values, UINT32_MAX from n on
    planted = top.lcp_rows[[0, top.lcp_rows.numel() // 2, -1]].tolist() + [int(top.lcp_rows.max().item()), first]
    rows = [LINE - 1, LINE, n - 1] + planted + [n, (1 << 32) + 5]
    assert any(r >= LINE for r in planted)
    d_rows = torch.tensor(rows, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
    hip.lcp_dev(d_rows.data_ptr(), len(rows), d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert u32(d_out).tolist() == [int(out[r].item()) & M32 for r in rows[:-2]] + [M32, M32]
    # the two layouts: equal arrays
    top.lcp[layout] = out
    if len(top.lcp) == 2:
        assert bool(torch.equal(top.lcp[LAYOUTS[0]], top.lcp[LAYOUTS[1]]))
        top.lcp.clear()
    del out, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 2. repeats
@pytest.mark.parametrize("stop", (0, pt.STOP))
@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_repeats_against_the_plan(top, layout, stop):
    """Seven thresholds in one call, both modes: every range and every summary field.  Two repeats() calls, four inversions;
    the one-hot handle's first call builds the LCP array as well."""
    plan, hip = top.plan, top.hip[layout]
    if layout == "onehot" and stop == 0:
        hip.drop_tables(jump=False, frontier=False, lcp=True)    # one layout where the call builds the array ...
        assert hip.lcp_info()[0] == 0
    elif layout == "bytes":
        hip.prepare(ktab=False, lcp=True)                         # ... and one with it prepared
        info0 = hip.lcp_info()
    levels = plan.thresholds
    assert levels == [64, 65, 300, 301, 4096, 4099, 4100]
    for later in (False, True):
        got = hip.repeats(levels, keep_first=later, stop=stop)
        assert len(got) == len(levels)
        for L, (ranges, summary) in zip(levels, got):
            want_r, want_s = pt.repeat_ranges(plan, L, later, stop)
            print(layout, "L", L, "later", later, "stop", stop, "got", summary, "want", want_s)
            assert summary == want_s, (L, later, stop)
            assert ranges.dtype == np.uint64 and ranges.shape == want_r.shape and np.array_equal(ranges, want_r), (L, later, stop)
    assert hip.lcp_info()[0] == 4 * top.n and (layout == "onehot" or hip.lcp_info() == info0)
    assert all(x >= 0 for x in hip.repeats_last()) and hip.repeats_last()[0] > 0


FIVE = [301, 64, 4100, 4096, 300]                                 # in no order; 4100 is longer than every block


@case
def test_repeats_five_thresholds_are_five_calls(top):
    """One sized call of five thresholds, five sized calls of one, the counting call, a second run: eight inversions, and one
    case because the calls are compared with each other."""
    plan, hip = top.plan, top.hip["bytes"]
    want = [pt.repeat_ranges(plan, L, True, 0) for L in FIVE]
    want_off = np.cumsum([0] + [r.shape[0] for r, _ in want]).astype(np.uint64)
    total, guard = int(want_off[-1]), 8
    assert total > 20 and want[2][0].shape[0] == 0
    out = np.full((total + guard, 2), 0xABABABABABABABAB, dtype=np.uint64)
    rc, n, off, sums = raw_call(hip, FIVE, True, 0, out, total)
    assert rc == 0 and n == total and np.array_equal(off, want_off) and sums == [s for _, s in want]
    assert np.array_equal(out[:total], np.concatenate([r for r, _ in want])) and (out[total:] == 0xABABABABABABABAB).all()
    first = out[:total].tobytes()
    for j, L in enumerate(FIVE):
        one = np.zeros((max(want[j][0].shape[0], 1), 2), dtype=np.uint64)
        rc, n, off1, sums1 = raw_call(hip, [L], True, 0, one, want[j][0].shape[0])
        assert rc == 0 and n == want[j][0].shape[0] and off1.tolist() == [0, n] and sums1 == [sums[j]], L
        assert one[:n].tobytes() == out[int(off[j]):int(off[j + 1])].tobytes(), L
    rc, n, off, sums = raw_call(hip, FIVE, True, 0, None, 0)      # the counting call
    assert rc == OVERFLOW and n == total and np.array_equal(off, want_off) and sums == [s for _, s in want]
    out[:] = 0
    rc, n, off, sums = raw_call(hip, FIVE, True, 0, out, total)
    assert rc == 0 and out[:total].tobytes() == first and np.array_equal(off, want_off) and sums == [s for _, s in want]


@case
def test_repeats_device_form_one_record_short(top):
    """fmx_repeats_dev with room for all ranges and with cap one short: the exact total, complete offsets and summaries,
    the guard records behind out[cap - 1] untouched.  Two inversions."""
    torch, plan, hip = top.torch, top.plan, top.hip["onehot"]
    want = [pt.repeat_ranges(plan, L, False, pt.STOP) for L in FIVE]
    want_off = np.cumsum([0] + [r.shape[0] for r, _ in want]).astype(np.uint64)
    total = int(want_off[-1])
    rec = np.concatenate([r for r, _ in want])
    lv = np.array(FIVE, dtype=np.uint32)
    opts = _lib.fmx_repeat_opts(0, pt.STOP, (0, 0, 0))
    vp = ctypes.c_void_p
    for cap in (total, total - 1):
        d_off = torch.zeros(len(FIVE) + 1, dtype=torch.int64, device="cuda")
        d_out = torch.full((2 * total + 16,), -1, dtype=torch.int64, device="cuda")
        n_out = ctypes.c_size_t(12345)
        sums = (_lib.fmx_repeat_summary * len(FIVE))()
        torch.cuda.synchronize()
        rc = _lib.load().fmx_repeats_dev(hip.handle, lv.ctypes.data, len(FIVE), ctypes.byref(opts), vp(d_off.data_ptr()),
                                         vp(d_out.data_ptr()), cap, ctypes.byref(n_out), sums, None)
        if rc not in (0, OVERFLOW):
            _lib.check(rc)
        torch.cuda.synchronize()
        assert rc == (0 if cap == total else OVERFLOW) and n_out.value == total, (rc, n_out.value, total)
        assert [{f: int(getattr(x, f)) for f in pt.FIELDS} for x in sums] == [s for _, s in want]
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want_off)
        raw = d_out.cpu().numpy().view(np.uint64)
        assert np.array_equal(raw[:2 * cap].reshape(-1, 2), rec[:cap]) and (raw[2 * cap:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


# ---------------------------------------------------------------- 3. occurrences
def interval(hip, plan, b, lo, hi):
    """(sp, ep) of b.data[lo:hi] from the library's search -- an input: its size must be the plan's copy count."""
    r = hip.search(b.data[lo:hi][::-1])
    assert r is not None and r[1] - r[0] == len(b.copies), (b.name, lo, hi, r)
    return int(r[0]), int(r[1])


def expected_csr(per_group, n_groups, mode):
    """{group: [(pos, len)]} -> (off uint64[n_groups + 1], OCC array) through occ_ref.reduce_pairs, no corpus."""
    off = np.zeros(n_groups + 1, dtype=np.uint64)
    parts = [np.zeros(0, dtype=OCC)]
    for g in sorted(per_group):
        pairs = occ_ref.reduce_pairs(per_group[g], mode)
        part = np.zeros(len(pairs), dtype=OCC)
        part["group"], part["pos"], part["len"] = g, [p for p, _ in pairs], [ln for _, ln in pairs]
        parts.append(part)
        off[g + 1:] += np.uint64(len(pairs))
    occ = np.concatenate(parts)
    occ["doc"], occ["raw_len"], occ["raw_off"] = M32, occ["len"], occ["pos"]
    return off, occ


def same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0][:10], want[0][:10])
    assert got[1].dtype == OCC and got[1].tobytes() == want[1].tobytes(), (got[1][:5], want[1][:5])


def records_of(hip, plan, slices):
    """[(group, block, lo, hi)] -> (the record array, {group: [(pos, len)]}, the rows the intervals hold)"""
    g, ln, sp, ep, per, rows = [], [], [], [], {}, 0
    for grp, b, lo, hi in slices:
        a, e = interval(hip, plan, b, lo, hi)
        g, ln, sp, ep = g + [grp], ln + [hi - lo], sp + [a], ep + [e]
        per.setdefault(grp, []).extend((p, hi - lo) for p in pt.occurrence_pairs(plan, b, lo, hi))
        rows += e - a
    return H.pack_records(g, ln, sp, ep), per, rows


def chain(plan):
    """X[20 j : 20 j + 40], j = 0 .. 200, without the two that hold the stop byte: overlapping occurrences from one end of
    every copy to the other, through the copy that straddles 2^31."""
    x = plan.block["X"]
    out = [(0, x, 20 * j, 20 * j + 40) for j in range(201) if pt.STOP not in x.data[20 * j:20 * j + 40]]
    assert len(out) == 199
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_occurrences_chains_across_the_line(top, layout):
    """(The handle's first occurrences call builds its locate samples: one inversion.)"""
    plan, hip = top.plan, top.hip[layout]
    rec, per, rows = records_of(hip, plan, chain(plan))
    pos = np.array([p for p, _ in per[0]], dtype=np.int64)
    fig = {"below": int((pos + 40 <= LINE).sum()), "above": int((pos >= LINE).sum()), "across": int(((pos < LINE) & (pos + 40 > LINE)).sum())}
    print("top bit: chain positions", fig)
    assert fig["below"] >= 100 and fig["above"] >= 100 and fig["across"] >= 1 and rows == 5 * 199
    for mode in MODES:
        want = expected_csr(per, 1, mode)
        same(hip.occurrences(rec, n_groups=1, mode=mode), want)
        assert hip.occurrences_last()[4] == rows
        same(hip.occurrences(rec[::-1], n_groups=1, mode=mode), want)
    assert expected_csr(per, 1, "disjoint")[1].size < expected_csr(per, 1, "longest")[1].size == rows
    # the text's last 40 bytes and its first 40, a group each
    x = plan.block["X"]
    rec, per, rows = records_of(hip, plan, [(0, x, len(x) - 40, len(x)), (1, x, 0, 40)])
    assert (top.m - 40, 40) in per[0] and (0, 40) in per[1]
    for mode in MODES:
        same(hip.occurrences(rec, n_groups=2, mode=mode), expected_csr(per, 2, mode))
        assert hip.occurrences_last()[4] == rows == 10


def key_width_slices(plan, top_group):
    """Records of at most 63 bytes (6 bits of len) in groups 0, 2^25 and the last one; in the last, two lengths at one
    position and a third slice that overlaps them."""
    x, y, z, zp = (plan.block[k] for k in ("X", "Y", "Z", "Z'"))
    return [(0, x, 100, 163), (0, y, 10, 60), (1 << 25, z, 0, 60), (1 << 25, zp, 2, 50), (1 << 25, y, 200, 263),
            (top_group, x, 4000, 4063), (top_group, x, 4000, 4040), (top_group, x, 4030, 4080), (top_group, x, 4036, 4099)]


@pytest.mark.parametrize("n_groups", ((1 << 26) - 1, 1 << 26), ids=("one_sort_64_bits", "two_sorts"))
@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_occurrences_key_widths(top, layout, n_groups):
    """32 bits of pos, 6 of len and the 26 bits that hold 0 .. 2^26 - 1 groups are a key of exactly 64 bits; with
    n_groups = 2^26 (27 bits) the same records take the form of two sorts.  (Offsets of 2^26 groups: 512 MiB each way.)"""
    plan, hip = top.plan, top.hip[layout]
    rec, per, rows = records_of(hip, plan, key_width_slices(plan, (1 << 26) - 2))
    assert int(rec["len"].max()) == 63 and sorted(per) == [0, 1 << 25, (1 << 26) - 2]
    assert any(p >= LINE for p, _ in per[(1 << 26) - 2]) and any(p < LINE for p, _ in per[(1 << 26) - 2])
    for mode in MODES:
        same(hip.occurrences(rec, n_groups=n_groups, mode=mode), expected_csr(per, n_groups, mode))
        assert hip.occurrences_last()[4] == rows


@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_occurrences_max_per(top, layout):
    """Y whole with max_per 1 and 3: the first rows of its interval, which the plan names -- the copies in the order of the
    byte in front of each."""
    plan, hip = top.plan, top.hip[layout]
    y = plan.block["Y"]
    sp, ep = interval(hip, plan, y, 0, len(y))
    assert ep - sp == 7 and min(y.copies) >= LINE
    order = pt.row_order(plan, y)
    rec = H.pack_records(0, len(y), [sp], [ep])
    for max_per in (1, 3):
        per = {0: [(y.copies[i], len(y)) for i in order[:max_per]]}
        for mode in MODES:
            same(hip.occurrences(rec, n_groups=1, mode=mode, max_per=max_per), expected_csr(per, 1, mode))
            assert hip.occurrences_last()[4] == max_per
    same(hip.occurrences(rec, n_groups=1), expected_csr({0: [(t, len(y)) for t in y.copies]}, 1, "all"))


@case
def test_occurrences_device_form_one_record_short(top):
    torch, plan, hip = top.torch, top.plan, top.hip["bytes"]
    rec, per, rows = records_of(hip, plan, chain(plan))
    want = expected_csr(per, 1, "longest")
    T = want[1].size
    d_rec = torch.from_numpy(rec.view(np.int64)).cuda()
    d_off = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    guard = 256
    d_out = torch.full((T * 32 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    assert hip.occurrences_dev(d_rec.data_ptr(), rec.size, 1, d_off.data_ptr(), 0, 0, mode="longest") == T      # the counting call
    assert hip.occurrences_dev(d_rec.data_ptr(), rec.size, 1, d_off.data_ptr(), d_out.data_ptr(), T, mode="longest") == T
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:T * 32].tobytes() == want[1].tobytes() and (raw[T * 32:] == 0xCD).all()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want[0])
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrences_dev(d_rec.data_ptr(), rec.size, 1, d_off.data_ptr(), d_out.data_ptr(), T - 1, mode="longest")
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy()[(T - 1) * 32:] == 0xCD).all()      # (fmx.h leaves what lies in front of it unspecified)
