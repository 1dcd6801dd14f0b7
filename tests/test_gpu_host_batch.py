"""The host-pointer batch calls (findex_amd/csrc/fmx_api.cpp) on both sides of every size at which they change path.

run_io moves a call's operands and results one of three ways -- tiny (the kernel reads and writes the page-locked staging
buffer), small (one staged copy each way), large (one copy per array) -- by the bytes the call moves, every array rounded up
to 16; fmx_search_batch_ex leaves run_io for whole arrays at kPipelineMin patterns.  The sizes below are derived from those
constants (read from the source) and from the arrays each entry point moves, so the test follows the thresholds.

Searches: every form of fmx_search_batch_ex at every such k, offsets from 0 and from 5, pageable buffers: the default form
against the oracle, the other forms against the default form's result.  Bad offsets are refused in every regime and the
handle works afterwards.  The other users of run_io are checked on a fixture index at their own tiny / small / large k
against the references the parity tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

import findex_amd
import oracle
from findex_amd import _lib
from helpers import synth_bwt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT_LEN = 12
ESC = 64                    # escape list of the packed form (as tests/search_forms.py, _lean_forms)


def _constants():
    with open(os.path.join(ROOT, "findex_amd", "csrc", "fmx_api.cpp")) as f:
        src = f.read()
    out = {}
    for name in ("kTinyCall", "kSmallCall", "kPipelineMin"):
        expr = re.search(r"constexpr\s+size_t\s+%s\s*=\s*([0-9u<\s]+);" % name, src).group(1)
        out[name] = int(eval(expr.replace("u", "")))
    return out


C = _constants()


def moved(arrays):
    """Bytes run_io counts for a call that moves arrays of these sizes."""
    return sum((b + 15) & ~15 for b in arrays)


def last_inside(limit, arrays_of):
    """The largest k whose call moves at most `limit` bytes."""
    assert moved(arrays_of(1)) <= limit
    lo, hi = 1, 2
    while moved(arrays_of(hi)) <= limit:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if moved(arrays_of(mid)) <= limit else (lo, mid)
    return lo


def boundary_ks(arrays_of):
    """(tiny pair, small pair): the last k inside and the first outside each of run_io's two thresholds."""
    t, s = last_inside(C["kTinyCall"], arrays_of), last_inside(C["kSmallCall"], arrays_of)
    return (t, t + 1), (s, s + 1)


# ---------------------------------------------------------------- fmx_search_batch_ex
FORMS = {                   # name -> search_batch_ex keywords
    "default": {},
    "fixed": {"fixed_len": PAT_LEN},
    "packed": {"packed": True, "escape_cap": ESC},
    "fixed+packed": {"fixed_len": PAT_LEN, "packed": True, "escape_cap": ESC},
    "miss_none": {"miss_none": True},
    "miss_none+packed": {"miss_none": True, "packed": True, "escape_cap": ESC},
}
WITH_OFFSETS = [name for name, kw in FORMS.items() if "fixed_len" not in kw]


def search_arrays(form):
    kw = FORMS[form]

    def arrays_of(k):
        words = k + 1 + 2 * ESC if kw.get("packed") else k
        return [PAT_LEN * k, 0 if "fixed_len" in kw else 8 * (k + 1), 8 * words, 8 * k]
    return arrays_of


def search_ks():
    """name of the boundary -> the ks on both sides of it, for every form's own sizes."""
    tiny, small = set(), set()
    for form in FORMS:
        t, s = boundary_ks(search_arrays(form))
        tiny.update(t)
        small.update(s)
    return {"one": [1], "tiny": sorted(tiny), "small": sorted(small), "whole": [C["kPipelineMin"] - 1, C["kPipelineMin"]]}


SEARCH_KS = search_ks()


@pytest.fixture(scope="module")
def world():
    """The index, the oracle beside it, kPipelineMin patterns of PAT_LEN bytes (every fifth an LF-walk hit) behind 5 bytes
    that belong to no pattern, and the oracle's intervals for them."""
    bwt, eof, counts = synth_bwt(200_000, 1, 6, 31)
    hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
    orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
    rng = np.random.default_rng(32)
    k = C["kPipelineMin"]
    pats = rng.integers(1, 7, (k, PAT_LEN)).astype(np.uint8)
    walk, _ = hip.lf_walk_batch(rng.integers(0, hip.n, (k + 4) // 5).astype(np.uint64), PAT_LEN)
    pats[::5] = walk[:, ::-1]
    buf = np.concatenate([np.full(5, 9, dtype=np.uint8), pats.reshape(-1)])
    off = np.arange(k + 1, dtype=np.uint64) * PAT_LEN
    wsp, wep, _ = orc.search_batch(buf[5:], off)
    hits = int((wsp < wep).sum())
    assert k // 5 <= hits < k // 2
    yield {"hip": hip, "orc": orc, "buf": buf, "wsp": wsp, "wep": wep}
    hip.close()


def batch(w, k, start):
    """(pattern buffer, offsets) of the first k patterns, the offsets beginning at `start` (0 or 5)."""
    off = np.arange(k + 1, dtype=np.uint64) * PAT_LEN + np.uint64(start)
    return (w["buf"] if start else w["buf"][5:])[: start + PAT_LEN * k], off


def run_form(hip, form, buf, off, k):
    kw = FORMS[form]
    if "fixed_len" in kw:
        lo = int(off[0])
        out = hip.search_batch_ex(np.ascontiguousarray(buf[lo:lo + PAT_LEN * k]), **kw)
    else:
        out = hip.search_batch_ex(buf, off, **kw)
    return hip.unpack_intervals(out, k, ESC) if kw.get("packed") else out


def check_form(form, got, dsp, dep):
    gsp, gep = got
    if FORMS[form].get("miss_none"):        # as tests/search_forms.py, _lean_forms: hits equal, misses sp >= ep
        hit = dsp < dep
        assert np.array_equal(gsp[hit], dsp[hit]) and np.array_equal(gep[hit], dep[hit]), form
        assert bool((gsp[~hit] >= gep[~hit]).all()), form
    else:
        assert np.array_equal(gsp, dsp) and np.array_equal(gep, dep), form


@pytest.mark.parametrize("boundary", list(SEARCH_KS))
def test_search_forms_on_both_sides_of(world, boundary):
    hip = world["hip"]
    for k in SEARCH_KS[boundary]:
        for start in (0, 5):
            buf, off = batch(world, k, start)
            dsp, dep = hip.search_batch(buf, off)
            assert np.array_equal(dsp, world["wsp"][:k]) and np.array_equal(dep, world["wep"][:k]), (k, start)
            for form in FORMS:
                if start and form not in WITH_OFFSETS:
                    continue                # no offsets travel: nothing to start at 5
                check_form(form, run_form(hip, form, buf, off, k), dsp, dep)


def regime_ks(form):
    """One k in each of the three regimes of a search with offsets: run_io small, run_io large, whole arrays."""
    _, (s_in, s_out) = boundary_ks(search_arrays(form))
    assert s_out < C["kPipelineMin"]
    return {"small": s_in, "large": s_out, "whole": C["kPipelineMin"]}


@pytest.mark.parametrize("regime", ["small", "large", "whole"])
@pytest.mark.parametrize("form", WITH_OFFSETS)
def test_bad_offsets_are_refused(world, form, regime):
    hip = world["hip"]
    k = regime_ks(form)[regime]
    buf, off = batch(world, k, 5)
    dsp, dep = world["wsp"][:k], world["wep"][:k]
    middle, last = off.copy(), off.copy()
    middle[k // 2] = middle[k // 2 + 1] + np.uint64(1)      # one decreasing offset in the middle
    last[k] = off[0] - np.uint64(1)                         # off[k] < off[0]
    for bad in (middle, last):
        with pytest.raises(findex_amd.FmxError) as e:
            run_form(hip, form, buf, bad, k)
        assert e.value.code == 3 and "non-decreasing" in str(e.value), (form, regime)
        check_form(form, run_form(hip, form, buf, off, k), dsp, dep)        # the handle stays usable


def test_empty_batch(world):
    hip, L = world["hip"], _lib.load()
    pat = np.zeros(16, dtype=np.uint8)
    off = np.zeros(1, dtype=np.uint64)
    for form, kw in FORMS.items():
        opts = _lib.fmx_search_opts(int(kw.get("fixed_len", 0)), (1 if kw.get("packed") else 0) | (2 if kw.get("miss_none") else 0),
                                    int(kw.get("escape_cap", 0)))
        sp = np.full(1 + 2 * ESC, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        ep = np.zeros(1, dtype=np.uint64)
        vp = ctypes.c_void_p
        rc = L.fmx_search_batch_ex(hip.handle, pat.ctypes.data_as(vp), None if "fixed_len" in kw else off.ctypes.data_as(vp),
                                   sp.ctypes.data_as(vp), None if kw.get("packed") else ep.ctypes.data_as(vp), 0, ctypes.byref(opts))
        assert rc == 0, form
        if kw.get("packed"):
            assert int(sp[0]) == 0, form
    assert hip.search_batch(pat[:0], off)[0].size == 0


# ---------------------------------------------------------------- the other users of run_io
@pytest.fixture(scope="module")
def fixture_pair(testdata):
    from test_gpu_lcp import golden_truth
    base = os.path.join(testdata, "test.cmp.bwt")
    hip = findex_amd.HipFMSearcher(base, bigEndian=False)
    orc = oracle.NaiveFMSearcher(base, bigEndian=False)
    sa, lcp = golden_truth("test.cmp", False)
    yield {"hip": hip, "orc": orc, "sa": sa, "lcp": lcp, "fm": orc.fm()}
    hip.close()


WALK = 3                    # bytes per row of the LF walks and the nextSubstr calls
ENTRY_ARRAYS = {            # entry point -> the sizes of the arrays a call of k moves
    "occ_batch": lambda k: [k, 8 * k, 8 * k],
    "prev_range_batch": lambda k: [8 * k, 8 * k, k, 8 * k, 8 * k],
    "lf_walk_batch": lambda k: [8 * k, WALK * k, 8 * k],
    "psi_batch": lambda k: [8 * k, 8 * k],
    "next_substr_batch": lambda k: [8 * k, WALK * k, 4 * k],
    "locate_batch": lambda k: [8 * k, 8 * k],
    "lcp_batch": lambda k: [8 * k, 4 * k],
}


def call_entry(p, entry, k, rng):
    """One call of `entry` for k rows of the fixture index, checked against its reference."""
    hip, orc = p["hip"], p["orc"]
    rows = rng.integers(0, hip.n, k).astype(np.uint64)
    rows[:3] = [0, orc.eof, hip.n - 1][:min(k, 3)]
    idx = rows.astype(np.int64)
    if entry == "occ_batch":
        c = rng.integers(0, 256, k).astype(np.uint8)
        i = rng.integers(-1, hip.n + 2, k, dtype=np.int64)
        assert np.array_equal(hip.occ_batch(c, i).astype(np.int64), orc.occ_batch(c, i))
    elif entry == "prev_range_batch":
        a, b = rng.integers(0, hip.n + 1, k).astype(np.uint64), rng.integers(0, hip.n + 1, k).astype(np.uint64)
        sp, ep = np.minimum(a, b), np.maximum(a, b)
        c = rng.integers(0, 256, k).astype(np.uint8)
        w1, w2 = orc.prev_range_batch(sp, ep, c)
        g1, g2 = hip.prev_range_batch(sp, ep, c)
        assert np.array_equal(g1, w1) and np.array_equal(g2, w2)
    elif entry == "lf_walk_batch":
        b, end = hip.lf_walk_batch(rows, WALK)
        assert [bytes(x) for x in b] == [orc.prevSubstr(int(r), WALK) for r in rows]
        assert end.tolist() == [orc.lf_chain(int(r), WALK) for r in rows]
    elif entry == "psi_batch":
        assert np.array_equal(hip.psi_batch(rows), p["fm"][idx].astype(np.uint64))
    elif entry == "next_substr_batch":
        assert hip.nextSubstr_batch(rows, WALK) == [orc.nextSubstr(int(r), WALK) for r in rows]
    elif entry == "locate_batch":
        assert np.array_equal(hip.locate(rows).astype(np.int64), p["sa"][idx])
    else:
        assert entry == "lcp_batch"
        assert np.array_equal(hip.lcp(rows), p["lcp"][idx])


@pytest.mark.parametrize("entry", list(ENTRY_ARRAYS))
def test_other_entry_points_tiny_small_large(fixture_pair, entry):
    hip = fixture_pair["hip"]
    rng = np.random.default_rng(len(entry))
    call_entry(fixture_pair, entry, 2, rng)             # whatever the entry point builds at first use is built
    before = hip.stats()["launches"]
    call_entry(fixture_pair, entry, 1, rng)
    assert hip.stats()["launches"] == before + 1
    (t_in, t_out), (s_in, s_out) = boundary_ks(ENTRY_ARRAYS[entry])
    for k in (t_in, t_out, s_in, s_out):
        call_entry(fixture_pair, entry, k, rng)
