"""The features with 32-bit positions -- the LCP array on a handle, fmx_repeats (18), fmx_occurrences (20),
fmx_ngrams (22), the line table and its lookups (23) and fmx_line_query (24) -- on a text of m = 3 * 2^30 + 4099 bytes, in both
layouts.  All of them refuse n >= 2^32, so their hard zone is 2^31 <= n < 2^32: here a third of the rows, of the SA values and
of the text positions carry their top bit, and with them every `row + 1` class id, every `pos << lb` key field (pb = 32) and
every u32 sample that locate reads; with the break set {10, a, b, c} the text has more than 2^31 lines, so line indices, line
numbers and the candidates of an all-lines query carry it too.

The text is tests/planted_text.py's plan written over i.i.d. a..d bytes on the device; every expectation is a closed form of
the plan (held to the from-the-definition references by tests/test_planted_text_cpu.py on the same geometry scaled down) or,
where the background counts -- the lines of a break set, the windows of one to three bytes -- plain torch over the fixture's
text tensor and the inverse of the sort's SA (tests/top_bit_ref.py, held to lines_ref, linequery_ref and ngrams_ref.brute by
tests/test_top_bit_ref_cpu.py).
Nothing of the library produces an expectation: its suffix sort and its search supply inputs only -- the rows and intervals
to ask about -- and their sizes and SA values are asserted against the plan.  The conditions the inputs must meet are
computed from the plan alone, printed and asserted by the fixture before any comparison.  A natural repeat of 64 bytes in the
background (chance below 2^-66) would fail the first LCP test.

The module prints the seconds of the fixture and of every case (DESIGN.md 6 has one run's figures).  Every repeats call
inverts the index once (HipFMSearcher.repeats twice: the counting call and the sized one), every first occurrences call of a
handle builds its locate samples by one more inversion: that is where the seconds of those cases go.  An n-grams call with
positions inverts once as well; the line table of 2.4 * 10^9 breaks is built once, by a fixture of its own that prints its
seconds, and dropped when the module ends.
"""
import ctypes
import functools
import gc
import time

import numpy as np
import pytest

import findex_amd
import linequery_ref
import lines_ref
import ngrams_ref
import occ_ref
import planted_text as pt
import top_bit_ref as tb
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
    w.text, w.sa, w.row_of, w.counts = text, sa, row_of, counts
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
    w.lcp, w.cache = {}, {}
    torch.cuda.synchronize()
    print("top bit: fixture %.1f s" % (time.time() - t0))
    yield w
    for h in w.hip.values():
        h.close()
    w.cache.clear()
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


# ---------------------------------------------------------------- 4. n-grams
LB = _lib.FMX_NGRAMS_LDS_BINS
NO_POS = H.NO_POS


def timed(top, key, make):
    """top.cache[key], made once and its seconds printed: a reference that several cases share."""
    if key not in top.cache:
        t0 = time.time()
        top.cache[key] = make()
        top.torch.cuda.synchronize()
        print("top bit: reference %s %.1f s" % (key, time.time() - t0))
    return top.cache[key]


def lone_window(top, L, stop):
    """(row, first position) of the eligible window of L bytes in the smallest row, from the sort's SA: the window of row r
    begins at t = m - L - SA[r]."""
    t = top.m - L - u32(top.sa[:1 << 20])
    ok = t >= 0
    for p in pt.stop_positions(top.plan, stop):
        ok &= ~((t <= p) & (p < t + L))
    r = int(top.torch.nonzero(ok)[0].item())
    return r, int(t[r].item())


def planted_ngrams(top, L, stop):
    """(classes, summary, sp, lone) of a planted threshold: ngram_classes from the plan, sp from the inverse of the sort's
    SA -- the rows of a class's copies, which must be consecutive."""
    def make():
        torch, plan = top.torch, top.plan
        classes, summary = pt.ngram_classes(plan, L, stop)
        at = pt.ngram_occurrences(plan, classes, L)
        sp = np.zeros(classes.size, dtype=np.int64)
        if classes.size:
            rows = u32(top.row_of[torch.from_numpy(np.concatenate(at)).cuda()]).cpu().numpy()
            lo = 0
            for j, a in enumerate(at):
                r = np.sort(rows[lo:lo + a.size])
                assert np.array_equal(r, r[0] + np.arange(a.size)), (L, stop, j)
                sp[j], lo = r[0], lo + a.size
        lone = None if classes.size or not summary["windows"] else lone_window(top, L, stop)
        return classes, summary, sp, lone
    return timed(top, ("planted n-grams", L, stop), make)


def ngrams_dev_call(w, hip, levels, cap, room, **kw):
    """One fmx_ngrams_dev with `cap`, the buffer `room` records and 8 guard records -> (n or the FmxError, out_off, the first
    min(cap, room) records, summaries); what lies behind out[cap - 1] must be untouched.  (w: the fixture.)"""
    torch = w.torch
    d_off = torch.zeros(len(levels) + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((3 * (room + 8),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        n, sums = hip.ngrams_dev(levels, d_off.data_ptr(), d_out.data_ptr(), cap, **kw)
    except findex_amd.FmxError as e:
        if e.code != OVERFLOW:
            raise
        n, sums = e, None
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy().view(np.uint64)
    assert (raw[3 * cap:] == np.uint64(M32 << 32 | M32)).all()
    return n, d_off.cpu().numpy().view(np.uint64), raw[:3 * cap].copy().view(H.NGRAM), sums


def same_summary(got, want, what, positions=True):
    assert list(ngrams_ref.FIELDS) == list(pt.NGRAM_FIELDS)
    for f in ngrams_ref.FIELDS:
        assert got[f] == (NO_POS if f == "largest_pos" and not positions else want[f]), (what, f, got, want)


@pytest.mark.parametrize("stop", (0, pt.STOP))
@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_ngrams_planted_thresholds(top, layout, stop):
    """Every threshold in one call per order, min_count 2, with positions: records byte for byte, every summary field and a
    spectrum of 6 bins (Y's seven copies are its overflow) against ngram_classes.  One inversion per call."""
    plan, hip = top.plan, top.hip[layout]
    levels = plan.thresholds
    want = [planted_ngrams(top, L, stop) for L in levels]
    sp = np.concatenate([w[2] for w in want])
    pos = np.concatenate([w[0]["first_pos"] for w in want])
    fig = {"classes": int(sp.size), "sp_below": int((sp < LINE).sum()), "sp_above": int((sp >= LINE).sum()),
           "first_pos_below": int((pos < LINE).sum()), "first_pos_above": int((pos >= LINE).sum()),
           "lengths_without_a_class": sum(1 for w in want if not w[0].size)}
    print("top bit: planted n-grams, stop %d:" % stop, fig)
    assert min(fig.values()) > 0
    for order in ("row", "count"):
        exp = [pt.ngram_result(c, s, r, order, 0, lone) for c, s, r, lone in want]
        total = sum(r.size for r, _ in exp)
        n, off, rec, sums = ngrams_dev_call(top, hip, levels, total, total, min_count=2, order=order, stop=stop, spectrum=6)
        assert n == total and np.array_equal(off, np.cumsum([0] + [r.size for r, _ in exp]).astype(np.uint64)), (order, n, total)
        assert rec.tobytes() == np.concatenate([r for r, _ in exp]).tobytes(), order
        for L, (c, s, _, _), (_, ws), g in zip(levels, want, exp, sums):
            same_summary(g, ws, (L, order, stop))
            assert np.array_equal(g["spectrum"], pt.ngram_spectrum(c, s, 6)), (L, order, stop)
    assert all(x >= 0 for x in hip.ngrams_last()) and hip.ngrams_last()[0] > 0


def gram_tables(top):
    """tb.gram_table of 1, 2 and 3 bytes over the fixture's text with the inverse of the sort's SA, as numpy (sp, count, first)
    triples by L; what every small-L case must reach is asserted here."""
    def make():
        out = {}
        for L in (1, 2, 3):
            g = tb.gram_table(top.text, L, top.row_of)
            out[L] = tuple(g[k].cpu().numpy() for k in ("sp", "count", "first"))
            sp, cnt, first = out[L]
            assert int(cnt.sum()) == top.m - L + 1
            big = cnt >= 2
            fig = {"distinct": int(cnt.size), "largest_count": int(cnt.max()), "sp_below": int((sp[big] < LINE).sum()),
                   "sp_above": int((sp[big] >= LINE).sum()), "first_pos_above": int((first >= LINE).sum()),
                   "counts_from_%d_on" % LB: int((cnt >= LB).sum()), "singletons": int((cnt == 1).sum())}
            print("top bit: windows of %d bytes:" % L, fig)
            assert fig["largest_count"] > 1 << 29 if L == 1 else fig["largest_count"] > 1 << 25
            assert fig["sp_below"] > 0 and fig["sp_above"] > 0 and fig["counts_from_%d_on" % LB] >= 4 ** L
        return out
    return timed(top, "gram tables", make)


def small_expected(top, L, min_count, order, k, bins):
    """(records, summary with the spectrum) from the gram table: the selection by ngrams_ref.result, the bins a
    torch.bincount of the counts with those at or above the bound in bin 0."""
    torch = top.torch
    sp, cnt, first = gram_tables(top)[L]
    rec, s = ngrams_ref.result((sp, cnt, first), min_count, order, k, 0)
    c = torch.from_numpy(cnt).cuda()
    s["spectrum"] = torch.bincount(torch.where(c < bins, c, torch.zeros_like(c)), minlength=bins).cpu().numpy().astype(np.uint64)
    return rec, s


SMALL = [(1, "count", 10, LB - 24), (1, "count", 0, 5000), (2, "count", 10, 5000), (2, "count", 0, LB - 24), (1, "row", 0, LB - 24),
         (2, "row", 0, 5000)]


@pytest.mark.parametrize("min_count,order,k,bins", SMALL)
@case
def test_ngrams_windows_of_one_two_and_three_bytes(top, min_count, order, k, bins):
    """L = 1, 2, 3 in one call: counts near 2^30 (the largest class covers more than 2^29 rows, and the count-ordered key
    (largest - count) << 32 | sp uses all 32 position bits), a spectrum bound below and above the LDS histogram."""
    hip = top.hip["bytes"]
    exp = [small_expected(top, L, min_count, order, k, bins) for L in (1, 2, 3)]
    total = sum(r.size for r, _ in exp)
    assert bins != LB and all(s["largest_count"] >= bins for _, s in exp)
    assert any((r["sp"] >= LINE).any() and (r["sp"] < LINE).any() for r, _ in exp)
    n, off, rec, sums = ngrams_dev_call(top, hip, [1, 2, 3], total, total, min_count=min_count, order=order, top=k, spectrum=bins)
    assert n == total and np.array_equal(off, np.cumsum([0] + [r.size for r, _ in exp]).astype(np.uint64)), (n, total)
    for L, (wr, ws), g, a, e in zip((1, 2, 3), exp, sums, off, off[1:]):
        assert rec[int(a):int(e)].tobytes() == wr.tobytes(), (L, rec[int(a):int(e)][:5], wr[:5])
        same_summary(g, ws, L)
        assert g["spectrum"].dtype == np.uint64 and np.array_equal(g["spectrum"], ws["spectrum"]), (L, np.nonzero(g["spectrum"] != ws["spectrum"]))
        assert int(ws["spectrum"][0]) >= 4 ** L and int(ws["spectrum"].sum()) == ws["distinct"]


@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_ngrams_without_positions(top, layout):
    """One planted length and L = 2 without positions: every field of the call with positions but first_pos and largest_pos
    -- the text's last min(L, n) rows, which are no windows, taken off by the closed form -- and no inversion."""
    plan, hip = top.plan, top.hip[layout]
    c, s, sp, lone = planted_ngrams(top, plan.L0, 0)
    want = [pt.ngram_result(c, s, sp, "count", 0, lone), small_expected(top, 2, 2, "count", 0, 7)]
    spectra = [pt.ngram_spectrum(c, s, 7), want[1][1]["spectrum"]]
    assert (want[1][0]["count"] > 1 << 25).any() and int(want[0][0]["count"].max()) == 7
    got = hip.ngrams([plan.L0, 2], min_count=2, order="count", spectrum=7, positions=False)
    assert hip.ngrams_last()[0] == 0
    for (rec, summary), (wrec, ws), spec in zip(got, want, spectra):
        assert rec.dtype == ngrams_ref.RECORD and rec.shape == wrec.shape
        assert np.array_equal(rec["sp"], wrec["sp"]) and np.array_equal(rec["count"], wrec["count"])
        assert (rec["first_pos"] == np.uint64(NO_POS)).all()
        same_summary(summary, ws, layout, positions=False)
        assert np.array_equal(summary["spectrum"], spec)


@case
def test_ngrams_device_form_one_record_short(top):
    """fmx_ngrams_dev with room for all records, twice, and with cap one short: equal bytes, the exact total, complete offsets,
    the guard records behind out[cap - 1] untouched.  Three inversions."""
    hip = top.hip["onehot"]
    exp = [pt.ngram_result(*planted_ngrams(top, L, pt.STOP)[:3], "count", 0, planted_ngrams(top, L, pt.STOP)[3]) for L in FIVE]
    total = sum(r.size for r, _ in exp)
    want_off = np.cumsum([0] + [r.size for r, _ in exp]).astype(np.uint64)
    want = np.concatenate([r for r, _ in exp])
    kw = dict(min_count=2, order="count", stop=pt.STOP)
    assert total > 4000 and exp[2][0].size == 0
    runs = [ngrams_dev_call(top, hip, FIVE, total, total, **kw) for _ in range(2)]
    for n, off, rec, sums in runs:
        assert n == total and np.array_equal(off, want_off) and rec.tobytes() == want.tobytes()
        for L, g, (_, ws) in zip(FIVE, sums, exp):
            same_summary(g, ws, L)
    assert runs[0][2].tobytes() == runs[1][2].tobytes()
    err, off, rec, _ = ngrams_dev_call(top, hip, FIVE, total - 1, total, **kw)
    assert isinstance(err, findex_amd.FmxError) and err.code == OVERFLOW and str(total) in str(err)
    assert np.array_equal(off, want_off) and rec.tobytes() == want[:total - 1].tobytes()


# ---------------------------------------------------------------- 5. lines
BIG = bytes([10, 97, 98, 99])
NO_LINE = H.NO_LINE


def same_u64(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.uint64 and np.array_equal(g, w), (g[:8], w[:8])


@pytest.mark.parametrize("layout", LAYOUTS)
@case
def test_lines_six_lines_of_a_gigabyte(top, layout):
    """The break set {10}: five breaks, X's stop byte in each of its five copies."""
    plan, hip, m = top.plan, top.hip[layout], top.m
    ref = timed(top, "lines {10}", lambda: tb.Lines(top.text, b"\n"))
    brk = ref.brk.tolist()
    assert brk == pt.stop_positions(plan, pt.STOP) and len(brk) == 5 and brk[1] < LINE - 2 and brk[2] > LINE + 2 and brk[0] > 1
    assert max(b - a for a, b in zip([0] + brk, brk + [m])) > 1 << 30
    hip.lines_prepare(b"\n")
    info = hip.lines_info()
    assert info[0] == 5 and info[1] == b"\n"
    pos = [0, m - 1] + [b + d for b in brk for d in (-1, 0, 1)] + [LINE - 1, LINE, m, 1 << 63]
    pos = np.array(pos, dtype=np.uint64)
    want = ref.lookup(pos)
    assert want[0][:-2].tolist() == [0, 5] + [k + d for k in range(5) for d in (0, 0, 1)] + [2, 2] and (want[0][-2:] == np.uint64(NO_LINE)).all()
    assert (want[1][:-2] >= np.uint64(LINE)).any() and (want[2][:-2] >= np.uint64(LINE)).any() and (want[2] < np.uint64(LINE)).any()
    same_u64(hip.line_of(pos), want)
    lines = np.arange(8, dtype=np.uint64)
    spans = ref.spans(lines)
    assert spans[0][:6].tolist() == [0] + [b + 1 for b in brk] and spans[1][:6].tolist() == brk + [m] and (spans[0][6:] == np.uint64(NO_LINE)).all()
    same_u64(hip.line_spans(lines), spans)


def sort_space_bytes(m):
    """fmx_order_math.h: two key and two value buffers, a histogram of 256 digits per tile of 4096 keys, and the block totals
    (one u32 per 2048 elements, level by level, and one) of the longer of the scans over the histograms and over m elements."""
    hist = 256 * ((m + 4095) // 4096)
    length, partials = max(m, hist), 0
    while length > 1:
        length = (length + 2047) // 2048
        partials += length
    return 2 * 8 * m + 2 * 4 * m + 4 * hist + 4 * (partials + 1)


class Big:
    pass


@pytest.fixture(scope="module")
def big(top):
    """The line table of the break set {10, a, b, c} on the one-hot handle -- three bytes of four are breaks, more than 2^31 of
    them -- and the stand-in over the same set; the build's seconds are printed on their own.  Afterwards the table is
    dropped."""
    torch, hip, m = top.torch, top.hip["onehot"], top.m
    w = Big()
    w.hip = hip
    w.n_brk = sum(int(top.counts[c]) for c in BIG)
    if w.n_brk <= LINE:
        pytest.fail("the break bytes 10, a, b, c occur %d times, not more than 2^31: no line index would carry its top bit" % w.n_brk)
    shift = hip.lines_info()[2]
    keep = 4 * w.n_brk + 4 * ((m >> shift) + 2)
    need = keep + 8 * w.n_brk + sort_space_bytes(w.n_brk) + 8192
    gc.collect()
    torch.cuda.empty_cache()
    t0 = time.time()
    w.ref = tb.Lines(top.text, BIG)
    torch.cuda.synchronize()
    t1 = time.time()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.fail("%.0f GB of HBM are free, the line table of %d breaks needs %.0f GB while it is built: no line ran above 2^31"
                    % (free / 1e9, w.n_brk, need / 1e9))
    ends_at_a_fault(hip.lines_prepare)(BIG)
    t2 = time.time()
    info = hip.lines_info()
    w.shift = info[2]
    print("top bit: the line table of %d breaks: reference %.1f s, build %.1f s (locate %.0f ms, sort and directory %.0f ms), %d bytes, shift %d"
          % (w.n_brk, t1 - t0, t2 - t1, hip.lines_last()[0], hip.lines_last()[1], info[3], info[2]))
    assert info[0] == w.n_brk == w.ref.n_brk and info[1] == BIG and info[3] == keep and w.shift == shift
    yield w
    hip.drop_tables(jump=False, frontier=False, lines=True)
    assert hip.lines_info()[0] == 0 and hip.lines_info()[3] == 0
    del w.ref
    gc.collect()
    torch.cuda.empty_cache()


@case
def test_lines_lookups_above_2_31_breaks(top, big):
    """fmx_lines_batch_dev and fmx_line_spans_dev on device arrays, all outputs against the stand-in on the device."""
    torch, hip, ref, m = top.torch, big.hip, big.ref, top.m
    g = torch.Generator(device="cuda")
    g.manual_seed(2032)
    at = [int(ref.brk[j].item()) for j in (LINE - 1, LINE)]
    special = [0, m - 1, LINE - 2, LINE - 1, LINE, LINE + 1, LINE + 2] + [b + d for b in at for d in (-1, 0, 1)]
    special += ref.directory_crossings(big.shift) + [m, m + 1]
    pos = torch.cat([torch.randint(0, m, (1 << 20,), generator=g, device="cuda"), torch.tensor(special, dtype=torch.int64, device="cuda")])
    want = ref.lookup(pos)
    fig = {"lines_below": int(((want[0] >= 0) & (want[0] < LINE)).sum()), "lines_above": int((want[0] >= LINE).sum()),
           "starts_above": int((want[1] >= LINE).sum()), "no_line": int((want[0] < 0).sum())}
    print("top bit: line lookups", fig)
    assert fig["lines_below"] > 1000 and fig["lines_above"] > 1000 and fig["starts_above"] > 1000 and fig["no_line"] == 2
    k = LINE - 1                                                  # brk[2^31 - 1] and brk[2^31], each - 1, 0, + 1: lines 2^31 - 1 .. 2^31 + 1
    assert want[0][-12:-6].tolist()[1:3] == [k, k + 1] and want[0][-12:-6].tolist()[4:] == [k + 1, k + 2]
    cross = want[0][-6:-2].tolist()
    assert cross[0] < LINE <= cross[3] and cross[1] <= cross[2]
    out = [torch.full((pos.numel(),), 7, dtype=torch.int64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    hip.line_of_dev(pos.data_ptr(), pos.numel(), *[o.data_ptr() for o in out], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name, o, wv in zip(("line", "start", "end"), out, want):
        bad = torch.nonzero(o != wv).reshape(-1)
        assert bad.numel() == 0, (name, bad.numel(), pos[bad[:4]].tolist(), o[bad[:4]].tolist(), wv[bad[:4]].tolist())
    # spans
    nb = big.n_brk
    lines = torch.cat([torch.randint(0, nb + 1, (1 << 20,), generator=g, device="cuda"),
                       torch.tensor([0, 1, LINE - 1, LINE, nb - 1, nb, nb + 1], dtype=torch.int64, device="cuda")])
    want = ref.spans(lines)
    assert int((lines >= LINE).sum()) > 1000 and int((lines < LINE).sum()) > 1000 and want[0][-1].item() == -1 and want[1][-2].item() == m
    out = [torch.full((lines.numel(),), 7, dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    hip.line_spans_dev(lines.data_ptr(), lines.numel(), *[o.data_ptr() for o in out], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name, o, wv in zip(("start", "end"), out, want):
        bad = torch.nonzero(o != wv).reshape(-1)
        assert bad.numel() == 0, (name, bad.numel(), lines[bad[:4]].tolist(), o[bad[:4]].tolist(), wv[bad[:4]].tolist())


def planted_hits(top, big):
    """(off, occ) of three groups from the plan -- the chain of 199 slices of X, Y whole, none -- and their line hits by
    lines_ref.occurrence_lines over the stand-in."""
    def make():
        plan = top.plan
        y = plan.block["Y"]
        per = {0: [(p, hi - lo) for _, b, lo, hi in chain(plan) for p in pt.occurrence_pairs(plan, b, lo, hi)],
               1: [(p, len(y)) for p in pt.occurrence_pairs(plan, y, 0, len(y))]}
        off, occ = expected_csr(per, 3, "all")
        assert off.tolist() == [0, 995, 1002, 1002] and all((np.diff(occ["pos"][int(a):int(b)].astype(np.int64)) >= 0).all() for a, b in zip(off, off[1:]))
        hoff, hits = lines_ref.occurrence_lines(big.ref, off, occ)
        fig = {"lines": int(hits.size), "line_no_below": int((hits["line_no"] < LINE).sum()), "line_no_above": int((hits["line_no"] > LINE).sum()),
               "of_them_Y": int((hits["line_no"][int(hoff[1]):] > LINE).sum())}
        print("top bit: occurrence lines", fig)
        assert fig["line_no_below"] > 100 and fig["line_no_above"] > 100 and fig["of_them_Y"] >= 2 and hoff[2] == hoff[3]
        return off, occ, hoff, hits
    return timed(top, "occurrence lines", make)


@case
def test_occurrence_lines_above_2_31_lines(top, big):
    torch, hip = top.torch, big.hip
    off, occ, hoff, hits = planted_hits(top, big)
    got = hip.occurrence_lines(off, occ)
    assert np.array_equal(got[0], hoff) and got[1].dtype == lines_ref.LINE_HIT and got[1].tobytes() == hits.tobytes(), (got[1][:3], hits[:3])
    T = hits.size
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_occ = torch.from_numpy(occ.view(np.int64)).cuda()
    d_loff = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * 48 + 256,), 0xCD, dtype=torch.uint8, device="cuda")
    args = (d_off.data_ptr(), d_occ.data_ptr(), occ.size, 3, d_loff.data_ptr())
    assert hip.occurrence_lines_dev(*args, d_out.data_ptr(), T) == T
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:T * 48].tobytes() == hits.tobytes() and (raw[T * 48:] == 0xCD).all() and np.array_equal(d_loff.cpu().numpy().view(np.uint64), hoff)
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrence_lines_dev(*args, d_out.data_ptr(), T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:(T - 1) * 48].tobytes() == hits[:T - 1].tobytes() and (raw[(T - 1) * 48:] == 0xCD).all()


# ---------------------------------------------------------------- 6. line queries
def same_hits(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert got[1].dtype == lines_ref.LINE_HIT and got[1].tobytes() == want[1].tobytes(), (got[1][:3], want[1][:3])


def bridge(hoff, hits):
    """The smallest window with which a line of X above 2^31 sees a line of Y above 2^31: the least distance of two such lines."""
    x = hits["line_no"][:int(hoff[1])].astype(np.int64)
    y = hits["line_no"][int(hoff[1]):int(hoff[2])].astype(np.int64)
    x, y = x[x > LINE], y[y > LINE]
    assert x.size and y.size
    return int(np.abs(x[:, None] - y[None, :]).min())


@case
def test_line_queries_anchor_and_terms_above_2_31(top, big):
    hip = big.hip
    _, _, hoff, hits = planted_hits(top, big)
    W = bridge(hoff, hits)
    assert 2 < W < M32
    queries = [(0, [(1, 0, False)]), (0, [(1, 1, False)]), (0, [(1, W, False)]), (0, [(1, W - 1, False)]), (0, [(1, W, True)]),
               (0, [(1, M32, False)]), (0, [(1, M32, True)]), (1, [(0, W, False)]), (1, [(0, M32, True), (1, 0, False)])]
    want = linequery_ref.line_query(hoff, hits, queries)
    size = np.diff(want[0].astype(np.int64)).tolist()
    above = [int((want[1]["line_no"][int(a):int(b)] > LINE).sum()) for a, b in zip(want[0], want[0][1:])]
    print("top bit: line queries: window %d, records %s, of them above 2^31 %s" % (W, size, above))
    assert size[0] == size[1] == 0 and size[2] > size[3] and above[2] > above[3] == 0 and size[2] + size[4] == int(hoff[1])
    assert size[5] == int(hoff[1]) and size[6] == 0 and above[5] > 100 and size[7] >= 1 and above[7] >= 1 and size[8] == 0
    same_hits(hip.line_query(hoff, hits, queries), want)
    assert hip.line_query_last()[3] == 7 * int(hoff[1]) + 2 * int(hoff[2] - hoff[1])


@case
def test_line_queries_all_lines_above_2_31_candidates(top, big):
    """An ALL_LINES anchor has n_brk + 1 candidates, more than 2^31; the query behind it in the same call begins at a candidate
    offset above 2^31.  Two of Y's seven copies lie above line 2^31 (three bytes of four are breaks, so line 2^31 begins near
    position 2^31 * 4 / 3), five below: the lines around them stand on both sides."""
    torch, hip = top.torch, big.hip
    _, _, hoff, hits = planted_hits(top, big)
    W = bridge(hoff, hits)
    queries = [(None, [(1, 2, False)]), (0, [(1, W, False)])]
    want = tb.line_query(hoff, hits, queries, big.ref)
    first = want[1][:int(want[0][1])]
    fig = {"records": int(first.size), "line_no_above": int((first["line_no"] > LINE + 1).sum()), "line_no_below": int((first["line_no"] < LINE).sum()),
           "second_query": int(want[0][2] - want[0][1])}
    print("top bit: all-lines query", fig)
    assert 7 <= fig["records"] <= 35 and fig["line_no_above"] >= 2 and fig["second_query"] >= 1 and big.n_brk + 1 > LINE
    T = want[1].size
    d_off = torch.from_numpy(hoff.view(np.int64)).cuda()
    d_hits = torch.from_numpy(hits.view(np.int64)).cuda()
    d_qoff = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * 48 + 48,), 0xCD, dtype=torch.uint8, device="cuda")
    args = (d_off.data_ptr(), d_hits.data_ptr(), hits.size, 3, queries, d_qoff.data_ptr())
    assert hip.line_query_dev(*args, 0, 0) == T                 # the counting call
    assert hip.line_query_last()[3] == big.n_brk + 1 + int(hoff[1])
    assert (d_out.cpu().numpy() == 0xCD).all() and np.array_equal(d_qoff.cpu().numpy().view(np.uint64), want[0])
    assert hip.line_query_dev(*args, d_out.data_ptr(), T) == T
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:T * 48].tobytes() == want[1].tobytes() and (raw[T * 48:] == 0xCD).all(), (raw[:T * 48].view(lines_ref.LINE_HIT)[:3], want[1][:3])
    assert np.array_equal(d_qoff.cpu().numpy().view(np.uint64), want[0]) and hip.line_query_last()[3] == big.n_brk + 1 + int(hoff[1])
    same_hits(hip.line_query(hoff, hits, queries), want)


@case
def test_line_queries_too_many_candidates(top, big):
    """Two ALL_LINES queries are more than 2^32 candidates: refused with FMX_ERR_OVERFLOW before anything is allocated."""
    torch, hip = top.torch, big.hip
    _, _, hoff, hits = planted_hits(top, big)
    assert 2 * (big.n_brk + 1) >= 1 << 32
    d_off = torch.from_numpy(hoff.view(np.int64)).cuda()
    d_hits = torch.from_numpy(hits.view(np.int64)).cuda()
    d_qoff = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((480,), 0xCD, dtype=torch.uint8, device="cuda")
    queries = [(None, [(1, 2, False)]), (None, [(0, 0, True)])]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for cap in (1, 10):
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.line_query_dev(d_off.data_ptr(), d_hits.data_ptr(), hits.size, 3, queries, d_qoff.data_ptr(), d_out.data_ptr(), cap)
        assert ei.value.code == OVERFLOW and "the candidates of all queries together must be below 2^32" in str(ei.value)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert d_qoff.cpu().tolist() == [7] * 3 and (d_out.cpu().numpy() == 0xCD).all()
