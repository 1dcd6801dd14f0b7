"""The search under string classes on an index of more than 2^32 rows (search_forms.WIDE_N = 2^32 + 2^29 + 12345 rows over
a..d, i.i.d.), in both layouts: k_classes<true, kLayoutOneHot> starts only when n > 2^32, and below this size no row field of
k_classes<true, kLayoutBytes> ever held a value of 2^32 or more.  The classes over a..d hold members of one and of two bytes,
so that here rows on both sides of 2^32 pass through an intermediate step of a member, the {sp, ep, elements | bytes} entries
of a wave's stack, the sort key pattern << 38 | sp, the CSR offsets, ix.bwt[sp] and sp == ix.eof under the one-row rule (the
EOF slot lies above 2^32), and the 24-byte records.

Every expectation comes from oracle.SampledFMSearcher: the hits from classes_ref.dfs_hits, which tries every member at every
element and has no one-row shortcut, the step counts from classes_ref.walk, the patterns themselves from cf / occ
(helpers.forward_string).  Nothing of the library produces an expectation; the conditions the inputs must meet are computed
from the expectations alone and asserted before any comparison.

Seconds on the MI355X: the slowest test is the first, which makes the fixture -- SLOWEST_S, nearly all of it
the fixture; the limit of a test is three times that.
"""
import ctypes
import gc
import time

import numpy as np
import pytest

import approx_ref
import classes_ref as C
import findex_amd
import search_forms as sf
from findex_amd import _lib
from helpers import ends_at_a_fault, forward_string

SLOWEST_S = 5
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LINE = 1 << 32
SYMS = b"abcd"
TABLE = [[b"a", b"b", b"cd"], [b"c", b"d", b"ab"]]          # a and b stand for class 0, c and d for class 1
LAYOUTS = ("onehot", "bytes")
REC = findex_amd.HipFMSearcher.RESULT
OVERFLOW = 9
PREFIX_M = (1, 2, 3, 8)             # 3^8 = 6561 spellings of at most 16 bytes, and 4^16 = 2^32: nearly all of them occur
TAIL = 18                           # literal bytes that leave one row (4^18 = 2^36 > n) in front of which classes stand
HEAD = 10                           # ... each a branching node of one row; about a ninth of them lie above 2^32
ROWS_BELOW = (12345, LINE // 3, LINE - 4097)
ROWS_ABOVE = tuple(LINE + 4097 + j * ((1 << 21) + 31) for j in range(200)) + (sf.WIDE_N - 2,)


def as_classes(t):
    return [256 if c in b"ab" else 257 for c in t]


class Wide:
    pass


def build_expectations(w, orc, eof):
    assert approx_ref.occurring(orc, 1, 255).tolist() == list(SYMS)
    pats = []
    for row in (LINE - 1, LINE, eof) + ROWS_BELOW + ROWS_ABOVE[:3]:
        t = forward_string(orc, row, 16, SYMS)
        pats += [as_classes(t[:m]) for m in PREFIX_M]
    for row in (LINE - 1, LINE) + ROWS_BELOW + ROWS_ABOVE:   # classes in front of a string that has one row
        t = forward_string(orc, row, HEAD + TAIL, SYMS)
        pats.append(as_classes(t[:HEAD]) + list(t[HEAD:]))
    w.stem = forward_string(orc, eof, TAIL, SYMS)            # a class in front of the EOF row's suffix: its BWT' symbol reads 0
    pats += [[256] + list(w.stem), [257] + list(w.stem), list(w.stem)]
    pats += [[256], [257], [256, 257], [97, 257, 98], []]
    seen, w.pats = set(), []
    for p in pats:
        if tuple(p) not in seen:
            seen.add(tuple(p))
            w.pats.append(p)
    w.per, w.steps, one_rows = [], 0, []
    for p in w.pats:
        hits, steps, _ = C.walk(orc, p, TABLE, one_rows=one_rows)
        assert hits == C.dfs_hits(orc, p, TABLE), p
        w.per.append(hits)
        w.steps += steps
    w.short = [j for j, p in enumerate(w.pats) if len(p) <= 3]
    rows = np.array([h[1:] for hs in w.per for h in hs], dtype=np.int64).reshape(-1, 2)
    sp, ep = rows[:, 0], rows[:, 1]
    w.fig = {"patterns": len(w.pats), "hits": int(sp.size), "steps": w.steps,
             "sp>=2^32": int((sp >= LINE).sum()), "ep<=2^32": int((ep <= LINE).sum()), "sp<2^32<ep": int(((sp < LINE) & (LINE < ep)).sum()),
             "one_row_nodes_above": int(sum(1 for r in one_rows if r >= LINE)), "one_row_nodes_below": int(sum(1 for r in one_rows if r < LINE)),
             "most_hits_of_one_pattern": max(len(h) for h in w.per),
             "lengths_of_one_pattern": max(len({h[0] for h in hs}) for hs in w.per)}


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
    g.manual_seed(4330)
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
        pytest.fail("the host cannot hold the reference of an index of %d rows (about 3 n bytes): no class search above 2^32 rows ran" % n)
    w.orc = orc
    t2 = time.time()
    build_expectations(w, orc, eof)
    w.fig.update({"seconds_index": round(t1 - t0, 1), "seconds_oracle_index": round(t2 - t1, 1),
                  "seconds_expectations": round(time.time() - t2, 1)})
    print("wide classes inputs:", w.fig)
    yield w
    for h in w.hip.values():
        h.close()
    orc.close()
    del w.bwt, bwt
    gc.collect()
    torch.cuda.empty_cache()


def check_inputs(w):
    fig = w.fig
    assert fig["sp>=2^32"] >= 1000 and fig["ep<=2^32"] >= 1000, fig
    assert fig["one_row_nodes_above"] >= 100 and fig["most_hits_of_one_pattern"] >= 4096 and fig["lengths_of_one_pattern"] >= 2, fig
    # the EOF row's own suffix is found; a class in front of it reads the row's BWT' symbol 0: no hit
    assert w.per[w.pats.index(list(w.stem))] == [(TAIL, w.eof, w.eof + 1)]
    assert not w.per[w.pats.index([256] + list(w.stem))] and not w.per[w.pats.index([257] + list(w.stem))]
    assert [len(w.per[w.pats.index(p)]) for p in ([256], [257], [256, 257])] == [3, 3, 9]


def expected_arrays(per):
    off, rows = C.expected_csr(per)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=REC) if rows else np.zeros(0, dtype=REC)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_host_form(wide, layout):
    """Offsets and record bytes exactly, the call's steps those of classes_ref.walk."""
    check_inputs(wide)
    hip = wide.hip[layout]
    el, off = C.pack(wide.pats)
    exp_off, exp = expected_arrays(wide.per)
    t0 = time.time()
    got_off, got = hip.search_classes_batch(el, off, C.abi(TABLE), cap=exp.size)
    _, _, got_steps, requests = hip.classes_last()
    print("%s: %d patterns, %d hits, %d steps (walk: %d), %d requests, %.2f s"
          % (layout, len(wide.pats), got.size, got_steps, wide.steps, requests, time.time() - t0))
    assert np.array_equal(got_off, exp_off)
    assert got.tobytes() == exp.tobytes()
    assert got_steps == wide.steps and 0 < requests <= 4 * got_steps


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_on_a_side_stream(wide, layout):
    """fmx_search_classes_batch_dev on a stream of its own over the patterns of 8 elements and fewer, guard bytes behind the output."""
    check_inputs(wide)
    torch = wide.torch
    hip = wide.hip[layout]
    sel = [j for j, p in enumerate(wide.pats) if len(p) <= 8]
    pats = [wide.pats[j] for j in sel]
    exp_off, exp = expected_arrays([wide.per[j] for j in sel])
    el, off = C.pack(pats)
    T, k = exp.size, len(pats)
    d_el = torch.from_numpy(el.view(np.int16)).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * REC.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        n = hip.search_classes_batch_dev(d_el.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T, C.abi(TABLE),
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
    el, off = C.pack(pats)
    L = _lib.load()
    arrays = C.abi(TABLE)
    tab = _lib.fmx_class_table()
    tab.cls_off, tab.mem_off, tab.mem_bytes = (a.ctypes.data for a in arrays)
    tab.n_classes = len(TABLE)
    cap, guard = T - 1, 64
    out = np.full((cap + guard) * REC.itemsize, 0xAB, dtype=np.uint8)
    out_off = np.zeros(off.size, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    rc = L.fmx_search_classes_batch(hip.handle, el.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(tab), out_off.ctypes.data,
                                    out.ctypes.data, cap, ctypes.byref(n_out))
    if rc != OVERFLOW:
        _lib.check(rc)                                       # (a HIP error is raised, and ends the module)
    assert rc == OVERFLOW and n_out.value == T, (rc, n_out.value, T)
    assert (out[cap * REC.itemsize:] == 0xAB).all()
    assert str(T).encode() in L.fmx_last_error()
