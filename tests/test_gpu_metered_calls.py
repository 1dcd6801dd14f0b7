"""What the four metered host forms share -- fmx_search_approx_batch, fmx_match_stats_batch, fmx_mems_batch and
fmx_extract_text_batch each run with counters of their own, fold them into the handle's and report them through a
thread-local *_last record -- in both layouts: the growth of the handle's launches and counters per call, the empty batch,
the record of a second thread, the capacity contract of the two CSR forms, and the device forms that do not meter.

The index is from_text of 3000 bytes of abcd; it holds REV = reverse(text), so patterns are cut from REV and ranges from the
text.  Every answer is held to a reference that uses nothing of the library: approx_ref.window_hits and .walk,
mstat_ref.loop_stats and .mems_of over the oracle, slices of the text.  The expectations are made once and shared by the
layouts.
"""
import ctypes
import threading

import numpy as np
import pytest

import approx_ref
import findex_amd
import mstat_ref
from findex_amd import _lib
from helpers import ends_at_a_fault, pack_patterns

pytestmark = pytest.mark.gpu

LAYOUTS = ["onehot", "bytes"]
OVERFLOW = 9
AP_WAVES = 4                                                 # fmx_approx.hip, kApWaves: patterns per workgroup of k_approx
MS_TILE = _lib.FMX_MSTAT_TILE                                # fmx_mstat.hip, kMsTile: positions per workgroup of k_mstat
EX_TILE = _lib.FMX_EXTRACT_TILE                              # fmx_extract.hip, kExTile: output bytes per workgroup of k_extract
MAXLEN = _lib.FMX_MSTAT_MAX_LEN
AP_HIT = findex_amd.HipFMSearcher.APPROX_HIT
MEM_HIT = findex_amd.HipFMSearcher.MEM_HIT
E, MIN_LEN = 1, 3                                            # the approximate budget and the MEMs' min_len of every call here

# What a call adds to the handle's counters, per step and per request its *_last reports: (rank_queries, backward_steps) per
# step, search_requests per request.  From the code, not from a run: k_approx and k_mstat end with counters_add(2 * steps,
# steps, requests) and their fold reports counter [1] as the steps; k_extract ends with counters_add(steps, 0, requests) and
# its fold reports counter [0].
PER_STEP = {"approx": (2, 1), "mstat": (2, 1), "mems": (2, 1), "extract": (1, 0)}
PER_REQUEST = 1
# ... and to its launches: one per call that has work (approx: a pattern; the others: a byte), however many kernels it runs.
LAUNCHES = 1


class World:
    pass


def open_text(text, layout):
    findex_amd.set_layout(layout)
    try:
        hip = findex_amd.HipFMSearcher.from_text(text)
    finally:
        findex_amd.set_layout("auto")
    hip.prepare(ktab=False, extract=True)                    # the samples: not built inside a call that is being counted
    return hip


def cut(rng, rev, k, m_lo, m_hi):
    """k patterns of m_lo .. m_hi bytes from rev; two in three get one byte replaced, by a letter or by z (absent)."""
    pats = []
    for j in range(k):
        m = int(rng.integers(m_lo, m_hi + 1))
        at = int(rng.integers(0, len(rev) - m + 1))
        p = bytearray(rev[at:at + m])
        if j % 3:
            p[int(rng.integers(0, m))] = int(rng.choice([97, 98, 99, 100, 122]))
        pats.append(bytes(p))
    return pats


@pytest.fixture(scope="module")
def world():
    w = World()
    rng = np.random.default_rng(1617)
    w.text = bytes(rng.integers(97, 101, 3000, dtype=np.uint8))
    w.rev = w.text[::-1]
    w.orc = approx_ref.index_of(w.rev)[0]
    big = cut(rng, w.rev, 48, 50, 50)
    w.pats = {"k0": [], "k1": cut(rng, w.rev, 1, 7, 7), "k65": cut(rng, w.rev, 65, 5, 9), "big": big}
    assert len(big) > 2 * AP_WAVES and sum(map(len, big)) > 2 * max(MS_TILE, EX_TILE)      # two workgroups and more
    w.exp = {}
    for name, pats in w.pats.items():
        x = World()
        x.buf, x.off = pack_patterns(pats)
        x.k, x.nb = len(pats), int(x.off[-1])
        # approximate search: the sliding window's hits, the steps of the walk restated over the oracle
        per = [approx_ref.window_hits(w.rev, p, E) for p in pats]
        x.ap_steps = 0
        for p, want in zip(pats, per):
            hits, steps = approx_ref.walk(w.orc, p, E)
            assert hits == want
            x.ap_steps += steps
        off, rows = approx_ref.expected_csr(per)
        x.ap_off, x.ap = np.array(off, dtype=np.uint64), np.array(rows, dtype=AP_HIT) if rows else np.zeros(0, dtype=AP_HIT)
        # matching statistics and their MEMs
        x.ln, x.sp, x.ep, steps = mstat_ref.loop_stats(w.orc, x.buf, x.off, MAXLEN)
        x.ms_steps = int(steps.sum())
        off, rows = mstat_ref.mems_of(x.ln, x.off, MIN_LEN)
        x.mem_off, x.mem = np.array(off, dtype=np.uint64), np.zeros(len(rows), dtype=MEM_HIT)
        for i, (q, l, end) in enumerate(rows):
            j = int(x.off[q]) + end - 1
            x.mem[i] = (q, l, end, x.sp[j], x.ep[j])
        # extraction: as many ranges, of the patterns' lengths
        x.lens = np.diff(x.off.astype(np.int64)).astype(np.uint64)
        x.pos = np.array([int(rng.integers(0, len(w.text) - int(l) + 1)) for l in x.lens], dtype=np.uint64)
        x.data = b"".join(w.text[int(a):int(a) + int(l)] for a, l in zip(x.pos, x.lens))
        w.exp[name] = x
    assert w.exp["k65"].ap.size >= 65 and w.exp["k65"].mem.size >= 65 and w.exp["big"].mem.size >= 48
    w.hip = {layout: open_text(w.text, layout) for layout in LAYOUTS}
    for hip in w.hip.values():
        assert hip.n == w.orc.n == 3001
    yield w
    for hip in w.hip.values():
        hip.close()


def run_form(hip, form, x):
    """One host call of `form` on the batch x, its answer held to the reference.  -> (steps, requests) of *_last, the steps
    the reference makes (None: it states none), whether the call had work."""
    if form == "approx":
        got_off, got = hip.search_approx_batch(x.buf, x.off, E)
        assert np.array_equal(got_off, x.ap_off) and got.tobytes() == x.ap.tobytes()
        return hip.approx_last()[2:], x.ap_steps, x.k > 0
    if form == "mstat":
        ln, sp, ep = hip.match_stats_batch(x.buf, x.off)
        assert np.array_equal(ln, x.ln) and np.array_equal(sp, x.sp) and np.array_equal(ep, x.ep)
        return hip.mstat_last()[2:], x.ms_steps, x.nb > 0
    if form == "mems":
        got_off, got = hip.mems_batch(x.buf, x.off, MIN_LEN)
        assert np.array_equal(got_off, x.mem_off) and got.tobytes() == x.mem.tobytes()
        return hip.mstat_last()[2:], x.ms_steps, x.nb > 0
    off, data = hip.extract_text_batch(x.pos, x.lens)
    assert np.array_equal(off, x.off) and data.tobytes() == x.data
    return hip.extract_last()[1:], None, x.nb > 0


@pytest.mark.parametrize("form", ["approx", "mstat", "mems", "extract"])
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_counters_and_launches(world, layout, form):
    """Per call: launches grows by LAUNCHES when the call has work and by nothing otherwise, the handle's rank_queries,
    backward_steps and search_requests by PER_STEP and PER_REQUEST times what *_last reports, and by nothing else."""
    hip = world.hip[layout]
    for name in ("k0", "k1", "k65", "big"):
        x = world.exp[name]
        before = hip.stats()
        last = hip.extract_last()
        # mems_batch and search_approx_batch count, then fetch: two library calls, the second one's record stands
        calls = 2 if form in ("approx", "mems") and (x.ap.size if form == "approx" else x.mem.size) else 1
        (steps, requests), ref_steps, work = run_form(hip, form, x)
        after = hip.stats()
        grown = {f: after[f] - before[f] for f in ("launches", "rank_queries", "backward_steps", "search_requests")}
        print("%s %s %s: %d steps, %d requests, %r" % (layout, form, name, steps, requests, grown))
        if form == "extract" and not work:                   # an extract call without a byte returns before it meters:
            assert hip.extract_last() == last                # this thread's record stands, nothing grows
            assert not any(grown.values()), (name, grown)
            continue
        assert grown["launches"] == (LAUNCHES * calls if work else 0), (name, grown)
        assert grown["rank_queries"] == PER_STEP[form][0] * steps * calls, (name, grown, steps)
        assert grown["backward_steps"] == PER_STEP[form][1] * steps * calls, (name, grown, steps)
        assert grown["search_requests"] == PER_REQUEST * requests * calls, (name, grown, requests)
        if ref_steps is not None:
            assert steps == ref_steps, (name, steps, ref_steps)
        else:
            assert steps >= x.nb                             # a step per byte, and the skipped ones
        assert (steps == 0 and requests == 0) or 0 < requests <= 4 * steps
        assert work or steps == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_the_empty_batch(world, layout):
    """k == 0 through the C entry points: FMX_OK from all four host forms, out_off == [0] and n_out == 0 from the CSR ones."""
    hip = world.hip[layout]
    L = _lib.load()
    off = np.zeros(1, dtype=np.uint64)
    n_out = ctypes.c_size_t(77)
    out_off = np.full(1, 77, dtype=np.uint64)
    assert L.fmx_search_approx_batch(hip.handle, None, off.ctypes.data, 0, None, out_off.ctypes.data, None, 0, ctypes.byref(n_out)) == 0
    assert out_off.tolist() == [0] and n_out.value == 0
    n_out.value, out_off[0] = 77, 77
    assert L.fmx_mems_batch(hip.handle, None, off.ctypes.data, 0, None, out_off.ctypes.data, None, 0, ctypes.byref(n_out)) == 0
    assert out_off.tolist() == [0] and n_out.value == 0
    assert L.fmx_match_stats_batch(hip.handle, None, off.ctypes.data, 0, None, None, None, None) == 0
    assert L.fmx_extract_text_batch(hip.handle, None, off.ctypes.data, 0, None) == 0
    assert L.fmx_extract_text_batch(hip.handle, None, None, 0, None) == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_a_second_thread_reads_zeros(world, layout):
    """The *_last records are per thread: a thread that has made no call reads zeros while this thread's values stand."""
    hip = world.hip[layout]
    x = world.exp["k65"]
    for form in ("approx", "mems", "extract"):
        run_form(hip, form, x)
    mine = (hip.approx_last(), hip.mstat_last(), hip.extract_last())
    assert mine[0][2] == x.ap_steps and mine[1][2] == x.ms_steps and mine[2][1] >= x.nb
    seen = []
    t = threading.Thread(target=lambda: seen.append((hip.approx_last(), hip.mstat_last(), hip.extract_last())))
    t.start()
    t.join()
    assert seen == [((0.0, 0.0, 0, 0), (0.0, 0.0, 0, 0), (0.0, 0, 0))]
    assert (hip.approx_last(), hip.mstat_last(), hip.extract_last()) == mine


@pytest.mark.parametrize("form", ["approx", "mems"])
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_capacity_of_the_csr_forms(world, layout, form):
    """cap = total - 1: FMX_ERR_OVERFLOW, n_out the exact total, the total in the message; cap = total: the reference's hits,
    which are also what the counting path (cap=None) returns."""
    hip = world.hip[layout]
    L = _lib.load()
    x = world.exp["k65"]
    exp_off, exp = (x.ap_off, x.ap) if form == "approx" else (x.mem_off, x.mem)
    total = exp.size
    n_out = ctypes.c_size_t()
    out_off = np.zeros(x.k + 1, dtype=np.uint64)
    out = np.zeros(total, dtype=exp.dtype)
    if form == "approx":
        opts = _lib.fmx_approx_opts(E, 1, 255, 0)
        entry = L.fmx_search_approx_batch
    else:
        opts = _lib.fmx_mstat_opts(0, MIN_LEN, (0, 0))
        entry = L.fmx_mems_batch
    rc = entry(hip.handle, x.buf.ctypes.data, x.off.ctypes.data, x.k, ctypes.byref(opts), out_off.ctypes.data, out.ctypes.data,
               total - 1, ctypes.byref(n_out))
    msg = L.fmx_last_error()
    assert rc == OVERFLOW and n_out.value == total and str(total).encode() in msg and str(total - 1).encode() in msg, (rc, msg)
    n_out.value = 0
    rc = entry(hip.handle, x.buf.ctypes.data, x.off.ctypes.data, x.k, ctypes.byref(opts), out_off.ctypes.data, out.ctypes.data,
               total, ctypes.byref(n_out))
    assert rc == 0 and n_out.value == total
    assert np.array_equal(out_off, exp_off) and out.tobytes() == exp.tobytes()
    if form == "approx":
        fit, counted = hip.search_approx_batch(x.buf, x.off, E, cap=total), hip.search_approx_batch(x.buf, x.off, E)
    else:
        fit, counted = hip.mems_batch(x.buf, x.off, MIN_LEN, cap=total), hip.mems_batch(x.buf, x.off, MIN_LEN)
    for got_off, got in (fit, counted):
        assert got_off.dtype == np.uint64 and got.dtype == exp.dtype
        assert np.array_equal(got_off, exp_off) and got.tobytes() == exp.tobytes()
    with pytest.raises(findex_amd.FmxError) as err:
        if form == "approx":
            hip.search_approx_batch(x.buf, x.off, E, cap=total - 1)
        else:
            hip.mems_batch(x.buf, x.off, MIN_LEN, cap=total - 1)
    assert err.value.code == OVERFLOW and str(total) in str(err.value)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_forms_leave_the_records_alone(world, layout):
    """fmx_extract_text_batch_dev and fmx_match_stats_batch_dev add to the handle's counters directly: right bytes, the
    handle's counters grown, launches and this thread's *_last records as they were."""
    import torch
    hip = world.hip[layout]
    x = world.exp["big"]
    run_form(hip, "extract", x)
    run_form(hip, "mstat", x)
    last = (hip.extract_last(), hip.mstat_last())
    d_pos = torch.from_numpy(x.pos.view(np.int64)).cuda()
    d_off = torch.from_numpy(x.off.view(np.int64)).cuda()
    d_pat = torch.from_numpy(x.buf).cuda()
    d_out = torch.zeros(x.nb, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(x.nb, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = hip.stats()
    hip.extract_text_batch_dev(d_pos.data_ptr(), d_off.data_ptr(), x.k, x.nb, d_out.data_ptr())
    torch.cuda.synchronize()
    mid = hip.stats()
    hip.match_stats_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), x.k, x.nb, d_len.data_ptr())
    torch.cuda.synchronize()
    after = hip.stats()
    assert d_out.cpu().numpy().tobytes() == x.data
    assert np.array_equal(d_len.cpu().numpy().view(np.uint32), x.ln)
    assert mid["rank_queries"] - before["rank_queries"] == last[0][1] and mid["backward_steps"] == before["backward_steps"]
    assert after["backward_steps"] - mid["backward_steps"] == x.ms_steps
    assert after["launches"] == before["launches"]
    assert (hip.extract_last(), hip.mstat_last()) == last
