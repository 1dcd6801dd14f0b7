"""Approximate search on an index of more than 2^32 rows (search_forms.WIDE_N = 2^32 + 2^29 + 12345 rows over a..d, i.i.d.),
in both layouts.

fmx_search_approx_batch starts k_approx<true, kLayoutOneHot> only when n > 2^32; k_approx<true, kLayoutBytes> runs for every
bytes-layout handle, but below this size none of its row fields ever held a value of 2^32 or more.  Here rows on both sides
of 2^32 pass through all of them: the sort key pattern << 38 | sp and the radix sort over 38 + ceil(log2 k) bits, the binary
search of k_ord_csr_off, the csp[] / cep[] slots of a frame in LDS, ix.bwt[sp] and sp == ix.eof under the one-row rule (the
EOF slot lies above 2^32), and the 24-byte records.

Every expectation comes from oracle.SampledFMSearcher (held to the inverted lists by tests/test_oracle_kat.py): the hits from
approx_ref.dfs_hits, which tries every symbol at every position and has no one-row shortcut, the step counts from
approx_ref.walk, and the patterns themselves from cf / occ (helpers.forward_string).  Nothing of the library produces an
expectation.  The conditions the inputs must meet are computed from the expectations alone, printed and asserted before any
comparison.  The index, both handles and the oracle are made once for the module.

Seconds on the MI355X: the slowest test is the first, which makes the fixture -- SLOWEST_S, nearly all of it
the fixture; every case after it runs in hundredths of a second.  The limit of a test is three times that, the margin
tests/test_gpu_search_forms.py takes for the machine's load.
"""
import ctypes
import gc
import time

import numpy as np
import pytest

import approx_ref
import findex_amd
import search_forms as sf
from findex_amd import _lib
from helpers import ends_at_a_fault, forward_string, pack_patterns

SLOWEST_S = 6
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
SYMS = b"abcd"
LO, HI = SYMS[0], SYMS[-1]          # the index holds no other symbol: dfs_hits over this range is the default range's
LAYOUTS = ("onehot", "bytes")
HIT = findex_amd.HipFMSearcher.APPROX_HIT
OVERFLOW = 9
PREFIX_M = (1, 2, 3, 8, 12, 14, 16, 17, 18, 20, 24)
ROWS_BELOW = (12345, LINE // 3, LINE - 4097)
ROWS_ABOVE = (LINE + 4097, LINE + (1 << 28) + 777, sf.WIDE_N - 2)
NARROW = (98, 99)


def budget_of(m):
    """The largest budget a pattern of m bytes is searched with (one batch of long ones apart)."""
    return 3 if m <= 3 else 2 if m <= 14 else 1


def replaced(p, pos):
    q = bytearray(p)
    q[pos] = LO + (q[pos] - LO + 1 + pos % 3) % len(SYMS)
    return bytes(q)


def make_patterns(orc, eof):
    """-> ({pattern: largest budget}, the long patterns that are also searched with e = 2, t_eof[:20], the four x + t_eof[:20],
    the four x + t[:20] of the row eof - 2^32)"""
    pats, long2 = {}, []
    rows = (LINE - 1, LINE, eof) + ROWS_BELOW + ROWS_ABOVE
    t_of = {row: forward_string(orc, row, max(PREFIX_M), SYMS) for row in rows}
    for row in rows:
        t = t_of[row]
        for m in PREFIX_M:
            p = t[:m]
            for q in [p] + [replaced(p, pos) for pos in sorted({0, m // 2, m - 1})]:     # P[0], a middle byte, P[m - 1]
                pats.setdefault(q, budget_of(m))
        if row in (LINE - 1, LINE, eof, ROWS_ABOVE[0]):
            long2 += [t[:16], t[:17], t[:24]] + [replaced(t[:20], pos) for pos in (0, 10, 19)]
    stem = t_of[eof][:20]
    extended = [bytes([x]) + stem for x in SYMS]
    # the row whose low 32 bits are the EOF row's, extended likewise: an ordinary row of one symbol, whose string is found
    alias = [bytes([x]) + forward_string(orc, eof - LINE, 20, SYMS) for x in SYMS]
    for q in extended + alias + [alias[0][1:]]:
        pats.setdefault(q, 1)
    long2 += extended + alias
    for a in SYMS:
        pats.setdefault(bytes([a]), 3)
        for b in SYMS:
            pats.setdefault(bytes([a, b]), 3)
    long2 = list(dict.fromkeys(long2))
    assert len(long2) <= 32 and all(len(q) >= 16 for q in long2)
    return pats, long2, stem, extended, alias


def build_expectations(w, orc, eof):
    """Patterns, hits, steps and the inputs' figures, from the oracle alone."""
    assert approx_ref.occurring(orc, 1, 255).tolist() == list(SYMS)
    budget, w.long2, w.stem, w.extended, w.alias = make_patterns(orc, eof)
    w.full = {}                                              # pattern -> its hits at the largest budget it is searched with
    for p, e in budget.items():
        w.full[p] = approx_ref.dfs_hits(orc, p, 2 if p in w.long2 else e, LO, HI)
    w.batches = {}                                           # e -> (patterns, per-pattern hits, walk steps)
    for e in range(4):
        pats = [p for p, b in budget.items() if b >= e or (e == 2 and p in w.long2)]
        per = [approx_ref.within(w.full[p], e) for p in pats]
        steps = 0
        for p, want in zip(pats, per):
            hits, s = approx_ref.walk(orc, p, e)
            assert hits == want, (p, e)                      # the restated walk against the walk without shortcuts
            steps += s
        w.batches[e] = (pats, per, steps)
    pats = w.batches[2][0]
    per = [approx_ref.dfs_hits(orc, p, 2, *NARROW) for p in pats]
    w.narrow = (pats, per, sum(approx_ref.walk(orc, p, 2, *NARROW)[1] for p in pats))
    w.fig = input_figures(w, budget)


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
        bwt[a:b] = torch.randint(LO, HI + 1, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
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
        # the one-hot handle is the n > 2^32 one: FMX_LAYOUT_DISPATCH takes k_approx<true, kLayoutOneHot> for it
        assert st["layout"] == code and w.hip[layout].n == n > LINE and eof > LINE, (layout, st["layout"], w.hip[layout].n)
        w.hip[layout].config_set("jump", "off")              # the approximate search uses the rank dictionary only, and the
        w.hip[layout].config_set("ktab", "off")              # exact search it is held against is to count every step
    t1 = time.time()
    w.cores = bench.effective_cores()
    orc, _ = bench.oracle_index(torch, bwt, eof, w.cores, 0)
    if orc is None or not hasattr(orc, "prev_range_batch") or orc.n != n:
        pytest.fail("the host cannot hold the reference of an index of %d rows (about 3 n bytes): no approximate search above 2^32 rows ran" % n)
    w.orc = orc
    t2 = time.time()
    build_expectations(w, orc, eof)
    w.fig.update({"seconds_index": round(t1 - t0, 1), "seconds_oracle_index": round(t2 - t1, 1),
                  "seconds_expectations": round(time.time() - t2, 1)})
    print("wide approximate inputs:", w.fig)
    yield w
    for h in w.hip.values():
        h.close()
    orc.close()
    del w.bwt, bwt
    gc.collect()
    torch.cuda.empty_cache()


def input_figures(w, budget):
    """What the inputs must hold, from the expectations alone: every (pattern, hit) once, at the pattern's largest budget."""
    rows = np.array([h for p in budget for h in w.full[p]], dtype=np.int64).reshape(-1, 3)
    sp, ep, d = rows[:, 0], rows[:, 1], rows[:, 2]
    return {"patterns": len(budget), "per_budget": {e: (len(b[0]), sum(len(h) for h in b[1]), b[2]) for e, b in w.batches.items()},
            "hits": int(sp.size), "sp>=2^32": int((sp >= LINE).sum()), "ep<=2^32": int((ep <= LINE).sum()),
            "sp<2^32<ep": int(((sp < LINE) & (LINE < ep)).sum()),
            "one_row_from_2^32-1": int(((ep - sp == 1) & (sp >= LINE - 1)).sum()),
            "d=1_above": int(((d == 1) & (sp >= LINE)).sum()), "d=2_above": int(((d == 2) & (sp >= LINE)).sum()),
            "most_hits_of_one_pattern": max(len(h) for h in w.full.values()),
            "narrow_hits": sum(len(h) for h in w.narrow[1]),
            "extended_hits": {p.decode(): w.full[p] for p in w.extended}}


def check_inputs(w):
    fig = w.fig
    assert fig["sp>=2^32"] >= 1000 and fig["ep<=2^32"] >= 1000 and fig["sp<2^32<ep"] >= 10, fig
    assert fig["one_row_from_2^32-1"] >= 10 and fig["d=1_above"] >= 100 and fig["d=2_above"] >= 100, fig
    assert fig["most_hits_of_one_pattern"] >= 256, fig
    assert (w.eof, w.eof + 1, 0) in w.full[w.stem], w.full[w.stem]
    # one byte in front of the EOF row's suffix: the row's BWT' symbol reads 0 and nothing extends it -- what dfs_hits says
    # is no exact hit and no hit on that row; a substituted tail may find the string elsewhere
    for p in w.extended:
        assert all(d >= 1 and sp != w.eof for sp, ep, d in w.full[p]), (p, w.full[p])
        assert not approx_ref.within(w.full[p], 0)
    # ... and one byte in front of the suffix of row eof - 2^32, one row as well: the row's own symbol is found exactly, the
    # three others behind one substitution
    row = w.eof - LINE
    assert approx_ref.within(w.full[w.alias[0][1:]], 0) == [(row, row + 1, 0)]
    assert sorted(min([d for _, _, d in w.full[p]], default=9) for p in w.alias) == [0, 1, 1, 1], [w.full[p] for p in w.alias]
    assert 0 < fig["narrow_hits"] < sum(len(h) for h in w.batches[2][1])


def expected_arrays(per_pattern):
    off, rows = approx_ref.expected_csr(per_pattern)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=HIT) if rows else np.zeros(0, dtype=HIT)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_host_form_at_every_budget(wide, layout):
    """Offsets and record bytes exactly, the call's steps those of approx_ref.walk."""
    check_inputs(wide)
    hip = wide.hip[layout]
    for e in range(4):
        pats, per, steps = wide.batches[e]
        buf, off = pack_patterns(pats)
        t0 = time.time()
        got_off, got = hip.search_approx_batch(buf, off, e)
        exp_off, exp = expected_arrays(per)
        _, _, got_steps, requests = hip.approx_last()
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
    st = hip.stats()
    exact_steps = st["backward_steps"]
    assert st["ktab_lookups"] == 0 and st["jump_lookups"] == 0 and st["row_lookups"] == 0 and st["tables_held_bytes"] == 0
    osp, oep, osteps = wide.orc.search_batch(buf, off, threads=wide.cores)
    assert exact_steps == int(osteps.sum()) == steps
    found = osp < oep
    assert np.array_equal(sp < ep, found) and 100 < int(found.sum()) < found.size
    assert np.array_equal(sp[found], osp[found]) and np.array_equal(ep[found], oep[found])
    got_off, hits = hip.search_approx_batch(buf, off, 0)
    assert np.array_equal(np.diff(got_off.astype(np.int64)), found.astype(np.int64))
    assert np.array_equal(hits["pattern"], np.nonzero(found)[0]) and not hits["mismatches"].any()
    assert np.array_equal(hits["sp"], osp[found]) and np.array_equal(hits["ep"], oep[found])
    assert int((hits["sp"] >= LINE).sum()) >= 30 and int((hits["ep"] <= LINE).sum()) >= 30
    _, _, got_steps, requests = hip.approx_last()
    assert got_steps == exact_steps and 0 < requests <= 4 * got_steps
    assert hip.stats()["backward_steps"] == 3 * exact_steps      # the counting call and the call that fetched the hits


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_an_explicit_range(wide, layout):
    """Substitutions from b..c alone, against dfs_hits over that range."""
    check_inputs(wide)
    hip = wide.hip[layout]
    pats, per, steps = wide.narrow
    buf, off = pack_patterns(pats)
    got_off, got = hip.search_approx_batch(buf, off, 2, sub=NARROW)
    exp_off, exp = expected_arrays(per)
    assert np.array_equal(got_off, exp_off) and got.tobytes() == exp.tobytes()
    _, _, got_steps, requests = hip.approx_last()
    print("%s range %s: %d hits, %d steps (walk: %d)" % (layout, NARROW, got.size, got_steps, steps))
    assert got_steps == steps and 0 < requests <= 4 * steps, (got_steps, steps, requests)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_on_a_side_stream(wide, layout):
    """fmx_search_approx_batch_dev on a stream of its own, guard bytes behind the output: the host form's bytes."""
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
        n = hip.search_approx_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T,
                                        stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * HIT.itemsize].tobytes() == exp.tobytes() and (raw[T * HIT.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), exp_off)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_capacity_one_short(wide, layout):
    """cap = T - 1: FMX_ERR_OVERFLOW, the exact total, nothing written behind the capacity."""
    check_inputs(wide)
    hip = wide.hip[layout]
    pats, per, _ = wide.batches[2]
    T = sum(len(h) for h in per)
    buf, off = pack_patterns(pats)
    L = _lib.load()
    opts = _lib.fmx_approx_opts(2, 0, 0, 0)
    cap, guard = T - 1, 64
    out = np.full((cap + guard) * HIT.itemsize, 0xAB, dtype=np.uint8)
    out_off = np.zeros(off.size, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    rc = L.fmx_search_approx_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(opts),
                                   out_off.ctypes.data, out.ctypes.data, cap, ctypes.byref(n_out))
    if rc != OVERFLOW:
        _lib.check(rc)                                       # (a HIP error is raised, and ends the module)
    assert rc == OVERFLOW and n_out.value == T, (rc, n_out.value, T)
    assert (out[cap * HIT.itemsize:] == 0xAB).all()
    assert str(T).encode() in L.fmx_last_error()
