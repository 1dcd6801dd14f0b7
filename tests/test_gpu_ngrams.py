"""fmx_ngrams on the device against tests/ngrams_ref.py, the count written from the definition: fixture
indexes in both layouts, small and adversarial texts, the edges of the scan's tile and of the LDS histogram, the index's own
answers, the call without positions, several lengths per call, the capacity rules, the device form, the refusals, one text
of 2^20 bytes and a corpus.  Every comparison is on the records, every summary field and the spectrum."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import findex_amd
import ngrams_ref
from corpus_ref import RefCorpus
from findex_amd import _lib
from helpers import ends_at_a_fault, synth_bwt
from test_gpu_build_text import _fib
from test_gpu_lcp import golden_indexes
from test_gpu_repeats import corpus_documents, golden_text, open_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")
T = _lib.FMX_REPEATS_TILE
LB = _lib.FMX_NGRAMS_LDS_BINS
NO_POS = findex_amd.HipFMSearcher.NO_POS
OVERFLOW, HIP_ERR, NOMEM = 9, 5, 4
LAYOUTS = ["onehot", "bytes"]
BIG = 10 ** 9

_classes = {}


def classes(text, L, stop=0):
    """every eligible class of a length as (sp, count, first_pos) arrays: brute for the small texts, hashed for the others
    (tests/test_ngrams_cpu.py holds the two to each other), computed once per text, length and stop byte"""
    key = (len(text), hash(text), L, stop)
    if key not in _classes:
        if len(_classes) > 400:
            _classes.clear()
        rec, _ = (ngrams_ref.brute if len(text) <= 600 else ngrams_ref.hashed)(text, L, min_count=1, order="row", top=0, stop=stop)
        _classes[key] = tuple(rec[f].astype(np.int64) for f in ("sp", "count", "first_pos"))
    return _classes[key]


def reference(text, L, min_count=2, order="count", top=0, stop=0, bins=0):
    return ngrams_ref.result(classes(text, L, stop), min_count, order, top, bins)


def same(got, want, what, positions=True):
    (rec, s), (wrec, ws) = got, want
    assert rec.dtype == ngrams_ref.RECORD and rec.shape == wrec.shape, (what, rec.shape, wrec.shape)
    assert np.array_equal(rec["sp"], wrec["sp"]) and np.array_equal(rec["count"], wrec["count"]), what
    if positions:
        assert np.array_equal(rec["first_pos"], wrec["first_pos"]), what
    else:
        assert (rec["first_pos"] == np.uint64(NO_POS)).all() and s["largest_pos"] == NO_POS, what
    for f in ngrams_ref.FIELDS:
        assert s[f] == ws[f] or (f == "largest_pos" and not positions), (what, f, s, ws)
    assert ("spectrum" in s) == ("spectrum" in ws)
    if "spectrum" in s:
        assert s["spectrum"].dtype == np.uint64 and np.array_equal(s["spectrum"], ws["spectrum"]), (what, s["spectrum"], ws["spectrum"])


def invariants(text, L, stop, s, bins, what):
    m = len(text)
    a = np.frombuffer(text, dtype=np.uint8)
    eligible = 0
    if L <= m:
        hits = np.concatenate(([0], np.cumsum(a == stop))) if stop else np.zeros(m + 1, dtype=np.int64)
        eligible = int((hits[L:] == hits[:m - L + 1]).sum())
    assert s["windows"] == eligible, what                      # m - L + 1 less the windows that hold the stop byte
    assert s["records"] <= s["selected"] <= s["distinct"] <= s["windows"] and s["singletons"] <= s["distinct"], what
    if bins:
        spec = s["spectrum"].astype(np.int64)
        cnt = classes(text, L, stop)[1]
        assert int(spec.sum()) == s["distinct"], what
        assert int((np.arange(bins) * spec).sum()) + int(cnt[cnt >= bins].sum()) == s["windows"], what
        assert bins < 2 or int(spec[1]) == s["singletons"], what


def check(hip, text, levels, variants, stops=(0,), bins=0, what=""):
    """one call per (stop byte, variant) with all the lengths; without a stop byte and with min_count >= 2 the call without
    positions too"""
    levels = list(levels)
    for stop in stops:
        ref_stop = stop if stop in text else 0                  # a byte that does not occur stops nothing
        for min_count, order, top in variants:
            tag = (what, "stop", stop, "min_count", min_count, order, "top", top)
            got = hip.ngrams(levels, min_count=min_count, top=top, order=order, stop=stop, spectrum=bins)
            assert len(got) == len(levels)
            for L, g in zip(levels, got):
                same(g, reference(text, L, min_count, order, top, ref_stop, bins), tag + (L,))
                invariants(text, L, ref_stop, g[1], bins, tag + (L,))
            if stop == 0 and min_count >= 2:
                lean = hip.ngrams(levels, min_count=min_count, top=top, order=order, spectrum=bins, positions=False)
                assert hip.ngrams_last()[0] == 0
                for L, g in zip(levels, lean):
                    same(g, reference(text, L, min_count, order, top, 0, bins), tag + (L, "no positions"), positions=False)


def tie_top(text, L):
    """a `top` that cuts between two classes of one count (by count), or 2"""
    cnt = np.sort(classes(text, L)[1])[::-1]
    ties = np.nonzero((cnt[1:] == cnt[:-1]) & (cnt[1:] >= 2))[0]
    return int(ties[0]) + 1 if ties.size else 2


def above(text):
    return int(classes(text, 1)[1].max()) + 1


# ---------------------------------------------------------------- 1. the fixture indexes
@pytest.mark.parametrize("name,be", golden_indexes())
@ends_at_a_fault
def test_goldens(name, be):
    text, max_lcp = golden_text(name, be)
    levels = [1, 2, 3, 8, max_lcp, max_lcp + 1]
    values, counts = np.unique(np.frombuffer(text, dtype=np.uint8), return_counts=True)
    stop = int(values[np.argsort(counts)[len(counts) // 2]])              # a byte that occurs, neither the rarest nor the commonest
    absent = next(c for c in range(2, 256) if c not in text)
    big = len(text) > 100000
    variants = [(1, "row", 0), (2, "count", tie_top(text, 2)), (above(text), "count", 0)]
    if not big:
        variants += [(1, "count", 1), (2, "row", BIG), (2, "count", 0), (2, "row", 1)]
    rng = np.random.default_rng(5)
    pats = np.frombuffer(b"".join(text[i:i + 3][::-1] for i in rng.integers(0, len(text) - 3, 200).tolist()), dtype=np.uint8)
    off = np.arange(0, 601, 3, dtype=np.uint64)
    for lay in LAYOUTS:
        findex_amd.set_layout(lay)
        try:
            hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, name + ".bwt"), bigEndian=be)
        finally:
            findex_amd.set_layout("auto")
        assert hip.n == len(text) + 1
        sp0, ep0 = hip.search_batch(pats, off)
        if lay == "bytes":
            hip.prepare(ktab=False, lcp=True)                   # one layout with the array there, one where the call builds it
            info0 = hip.lcp_info()
        else:
            assert hip.lcp_info()[0] == 0
        seen0, launches0 = hip.stats()["patterns_seen"], hip.stats()["launches"]
        check(hip, text, levels, variants, stops=(0, stop) if big else (0, stop, absent), bins=0 if big else 16, what="%s/%s" % (name, lay))
        info1 = hip.lcp_info()
        assert info1[0] == 4 * hip.n and info1[2] == max_lcp
        if lay == "bytes":
            assert info1 == info0
        assert hip.stats()["patterns_seen"] == seen0 and hip.stats()["launches"] > launches0
        sp1, ep1 = hip.search_batch(pats, off)
        assert np.array_equal(sp0, sp1) and np.array_equal(ep0, ep1)
        hip.close()


# ---------------------------------------------------------------- 2. small and adversarial texts
def small_texts():
    rng = np.random.default_rng(61)
    return {"one": b"a", "two": b"ab", "two_same": b"aa", "three": b"aba", "ab_repeated": b"ab" * 300, "fibonacci": _fib(3000),
            "sigma2": bytes(rng.integers(1, 3, 3000, dtype=np.uint8) + 96)}


@pytest.mark.parametrize("name", list(small_texts()))
@ends_at_a_fault
def test_small_texts(name):
    text = small_texts()[name]
    m = len(text)
    hip = open_text(text)
    variants = [(1, "row", 0), (1, "count", 0), (2, "count", 0), (2, "row", 1), (2, "count", tie_top(text, 1)), (above(text), "row", 0)]
    check(hip, text, sorted({1, 2, 3, 7, min(64, m), m, m + 1}), variants, stops=(0, text[0]), bins=5, what=name)
    hip.close()


# ---------------------------------------------------------------- 3. the tile's edges
@pytest.mark.parametrize("m", [T - 1, T, T + 1, 3 * T + 5])
@ends_at_a_fault
def test_one_letter_is_one_class_of_every_row(m):
    text = b"a" * m
    hip = open_text(text)
    check(hip, text, [1, 2, 64, m], [(1, "row", 0), (2, "count", 0)], bins=m + 2, what="a x %d" % m)
    rec, summary = hip.ngrams(2)
    assert rec.tolist() == [(2, m - 1, 0)] and summary["distinct"] == 1 and summary["largest_count"] == m - 1
    hip.close()


@pytest.mark.parametrize("sigma", [2, 4])
@ends_at_a_fault
def test_random_texts_put_class_edges_on_every_boundary(sigma):
    m = 3 * T + 5
    rng = np.random.default_rng(70 + sigma)
    text = bytearray((rng.integers(0, sigma, m, dtype=np.uint8) + 97).tobytes())
    stops = (0,)
    if sigma == 4:                                              # stop bytes on a tile's last and first byte, and at both ends
        for t in (T - 1, T, 2 * T - 1, 2 * T, 0, m - 1):
            text[t] = ord("z")
        stops = (0, ord("z"))
    text = bytes(text)
    hip = open_text(text)
    check(hip, text, range(1, 13), [(1, "row", 0), (2, "count", 0), (2, "count", tie_top(text, 6))], stops=stops, bins=64, what="sigma %d" % sigma)
    hip.close()


# ---------------------------------------------------------------- 4. the spectrum's paths
@ends_at_a_fault
def test_spectrum_on_both_sides_of_the_lds_histogram():
    rng = np.random.default_rng(72)
    letters = b"a" * (LB - 1) + b"b" * LB + b"c" * (LB + 1) + b"d" + b"ee"
    text = bytes(rng.permutation(np.frombuffer(letters, dtype=np.uint8)))
    hip = open_text(text)
    for bins in (LB, LB + 1, LB + 2, LB - 1, 1, 2, 3, 65536):
        check(hip, text, [1, 2], [(1, "row", 0), (2, "count", 0)], bins=bins, what="bins %d" % bins)
    _, s = hip.ngrams(1, min_count=1, spectrum=LB)              # counts B - 1, B and B + 1: the last two are the overflow
    assert s["spectrum"][0] == 2 and s["spectrum"][LB - 1] == 1 and s["spectrum"][1] == 1 and s["spectrum"][2] == 1
    hip.close()


# ---------------------------------------------------------------- 5. against the index itself
@ends_at_a_fault
def test_records_are_the_index_own_answers():
    rng = np.random.default_rng(73)
    text = bytes(rng.integers(0, 4, 5000, dtype=np.uint8) + 97)
    hip = open_text(text)
    for L, top in ((3, 0), (6, 150)):
        rec, _ = hip.ngrams(L, min_count=1, top=top)
        windows = hip.ngram_texts(rec, L)
        assert len(windows) == rec.size > 60
        pats = np.frombuffer(b"".join(w[::-1] for w in windows), dtype=np.uint8)
        sp, ep = hip.search_batch(pats, np.arange(rec.size + 1, dtype=np.uint64) * L)
        assert np.array_equal(sp, rec["sp"]) and np.array_equal(ep, rec["sp"] + rec["count"])
        for r, w in zip(rec, windows):
            t = int(r["first_pos"])
            assert w == text[t:t + L]
            pos = hip.locate_text(w)
            assert len(pos) == int(r["count"]) and int(pos[0]) == t
    hip.close()


# ---------------------------------------------------------------- 6. without positions
@ends_at_a_fault
def test_without_positions_no_inversion_is_run():
    rng = np.random.default_rng(74)
    unique = bytes(rng.integers(1, 256, 5000, dtype=np.uint8))               # hardly a window of 3 bytes occurs twice
    planted = bytearray(unique)
    planted[4000:4100] = planted[100:200]
    for text in (unique, bytes(planted)):
        hip = open_text(text)
        m = len(text)
        levels = [1, 2, 3, 4, 5, 50, 100, 101, 1000, m - 1, m, m + 1]
        for order, top in (("count", 0), ("row", 3)):
            full = hip.ngrams(levels, order=order, top=top, spectrum=8)
            assert hip.ngrams_last()[0] > 0
            lean = hip.ngrams(levels, order=order, top=top, spectrum=8, positions=False)
            assert hip.ngrams_last()[0] == 0 and all(x >= 0 for x in hip.ngrams_last())
            for L, (r, s), (r2, s2) in zip(levels, full, lean):
                same((r, s), reference(text, L, 2, order, top, 0, 8), (L, order))
                same((r2, s2), (r, s), (L, order, "no positions"), positions=False)
                if L <= m:
                    assert s2["largest_sp"] == s["largest_sp"] and s2["largest_count"] == s["largest_count"] >= 1
        hip.close()
    # the flag's conditions, from the library
    hip = open_text(b"abcabc")
    for kw in (dict(stop=98), dict(min_count=1)):
        with pytest.raises(findex_amd.FmxError) as err:
            hip.ngrams(2, positions=False, **kw)
        assert err.value.code == 3
    hip.close()


# ---------------------------------------------------------------- 7. lengths, capacity, determinism
@pytest.fixture(scope="module")
def planted():
    """a sigma-4 text of 40000 bytes with copies of 30 to 900 bytes, and its handle"""
    rng = np.random.default_rng(31)
    t = bytearray((rng.integers(0, 4, 40000, dtype=np.uint8) + 97).tobytes())
    for src, dst, ln in ((100, 9000, 30), (500, 12000, 900), (2000, 20000, 64), (2000, 30000, 64), (5000, 5300, 290)):
        t[dst:dst + ln] = t[src:src + ln]
    text = bytes(t)
    hip = findex_amd.HipFMSearcher.from_text(text)
    yield text, hip
    hip.close()


def raw_call(hip, levels, opts, out, cap, bins=0):
    """fmx_ngrams itself -> (status, n_out, out_off, summaries, spectrum)"""
    L = _lib.load()
    lv = np.array(levels, dtype=np.uint32)
    n_out = ctypes.c_size_t(12345)
    off = np.full(len(levels) + 1, 77, dtype=np.uint64)
    sums = (_lib.fmx_ngram_summary * len(levels))()
    spec = np.full(max(len(levels) * bins, 1), 99, dtype=np.uint64)
    rc = L.fmx_ngrams(hip.handle, lv.ctypes.data, len(levels), ctypes.byref(opts), off.ctypes.data,
                      out.ctypes.data if out is not None else None, cap, ctypes.byref(n_out), sums, spec.ctypes.data)
    return rc, int(n_out.value), off, [{f: int(getattr(x, f)) for f in ngrams_ref.FIELDS} for x in sums], spec


@pytest.mark.parametrize("order", ["row", "count"])
@ends_at_a_fault
def test_lengths_capacity_and_determinism(planted, order):
    text, hip = planted
    levels = [8, 3, 64, 50000, 29]                             # in no order, one of them longer than the text
    top = 700
    many = hip.ngrams(levels, order=order, top=top, spectrum=6)
    singles = [hip.ngrams(L, order=order, top=top, spectrum=6) for L in levels]
    for L, g, g1 in zip(levels, many, singles):
        want = reference(text, L, 2, order, top, 0, 6)
        same(g, want, L)
        same(g1, want, (L, "alone"))
    total = sum(r.size for r, _ in many)
    assert many[3][0].size == 0 and many[0][0].size == top and total > top + 10
    want_off = np.cumsum([0] + [r.size for r, _ in many]).astype(np.uint64)
    want_sums = [{f: s[f] for f in ngrams_ref.FIELDS} for _, s in many]
    want_spec = np.concatenate([s["spectrum"] for _, s in many])
    opts = _lib.fmx_ngram_opts(1 if order == "count" else 0, 0, 2, top, 6, 0, (0, 0, 0))
    # the counting call: the exact total, the offsets complete, the summaries and the spectrum valid
    rc, n, off, sums, spec = raw_call(hip, levels, opts, None, 0, 6)
    assert rc == OVERFLOW and n == total and np.array_equal(off, want_off) and sums == want_sums and np.array_equal(spec, want_spec)
    assert str(total).encode() in _lib.load().fmx_last_error()
    guard, fill = 8, 0xABABABABABABABAB
    out = np.full((total + guard, 3), fill, dtype=np.uint64)
    rc, n, off, sums, spec = raw_call(hip, levels, opts, out, total, 6)
    assert rc == 0 and n == total and np.array_equal(off, want_off) and (out[total:] == fill).all()
    assert out[:total].tobytes() == np.concatenate([r for r, _ in many]).tobytes()
    first = out[:total].tobytes()
    # one record short: the exact total again, nothing at or behind out[cap]
    out[:] = fill
    rc, n, off, sums, spec = raw_call(hip, levels, opts, out, total - 1, 6)
    assert rc == OVERFLOW and n == total and np.array_equal(off, want_off) and sums == want_sums and np.array_equal(spec, want_spec)
    assert (out[total - 1:] == fill).all()
    # the same bytes on a second run
    out[:] = 0
    rc, n, off2, sums2, spec2 = raw_call(hip, levels, opts, out, total, 6)
    assert rc == 0 and out[:total].tobytes() == first and np.array_equal(off2, want_off) and sums2 == sums and np.array_equal(spec2, spec)
    assert all(x >= 0 for x in hip.ngrams_last()) and hip.ngrams_last()[0] > 0


# ---------------------------------------------------------------- 8. the device form
@ends_at_a_fault
def test_device_form_and_a_capture(planted):
    import torch
    text, hip = planted
    levels = [12, 5, 300, 8]
    kw = dict(min_count=2, top=500, order="count", stop=ord("d"), spectrum=4)
    host = hip.ngrams(levels, **kw)
    for L, g in zip(levels, host):
        same(g, reference(text, L, 2, "count", 500, ord("d"), 4), L)
    total = sum(r.size for r, _ in host)
    assert total > 100 and host[0][0].size > 0
    records = np.concatenate([r for r, _ in host]).view(np.uint64)
    d_off = torch.zeros(len(levels) + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((3 * total + 24,), -1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        n, sums = hip.ngrams_dev(levels, d_off.data_ptr(), d_out.data_ptr(), total, stream=st.cuda_stream, **kw)
    st.synchronize()
    assert n == total
    for s, (_, ws) in zip(sums, host):
        assert {f: s[f] for f in ngrams_ref.FIELDS} == {f: ws[f] for f in ngrams_ref.FIELDS} and np.array_equal(s["spectrum"], ws["spectrum"])
    raw = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(raw[:3 * total], records) and (raw[3 * total:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), np.cumsum([0] + [r.size for r, _ in host]).astype(np.uint64))
    # one record short
    d_out.fill_(-1)
    torch.cuda.synchronize()
    with pytest.raises(findex_amd.FmxError) as err:
        hip.ngrams_dev(levels, d_off.data_ptr(), d_out.data_ptr(), total - 1, **kw)
    assert err.value.code == OVERFLOW
    raw = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(raw[:3 * (total - 1)], records[:-3]) and (raw[3 * (total - 1):] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    # under a capture: refused before anything is allocated, the capture goes on and ends validly
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):                        # (what a first capture and a first replay themselves take is taken here)
        d_off.zero_()
    g.replay()
    del g
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        with pytest.raises(findex_amd.FmxError) as err:
            hip.ngrams_dev(levels, d_off.data_ptr(), d_out.data_ptr(), total, stream=st.cuda_stream, **kw)
        d_off.zero_()
    assert err.value.code == HIP_ERR and "capture" in str(err.value)
    d_off.fill_(5)
    g.replay()
    torch.cuda.synchronize()
    left = d_off.cpu().numpy()
    del g
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0               # (no tensor was made on the device in between)
    assert not left.any()


# ---------------------------------------------------------------- 9. refusals
@ends_at_a_fault
def test_refusals_leave_the_memory_as_it_was():
    import torch
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    block = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    n = 1 << 22
    sbwt, eof, counts = synth_bwt(n, 1, 4, seed=21)
    synth = findex_amd.HipFMSearcher.from_mem(sbwt, eof, counts)
    d_off = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(96, dtype=torch.int64, device="cuda")

    def refused(hip, code, needle):
        for dev in (False, True):
            for positions in (True, False):
                with pytest.raises(findex_amd.FmxError) as err:
                    if dev:
                        hip.ngrams_dev(4, d_off.data_ptr(), d_out.data_ptr(), 32, positions=positions)
                    else:
                        hip.ngrams(4, positions=positions)
                assert err.value.code == code and needle in str(err.value), str(err.value)

    for hip, code, needle in ((block, 6, "fmx_open_block"), (synth, 2, "not the BWT of one text")):
        refused(hip, code, needle)                              # (the handle's stream and the runtime's first-use memory)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        refused(hip, code, needle)
        torch.cuda.synchronize()
        # Every temporary of the call on the big handle is 4 n bytes or more, so one that stayed would show as at least that;
        # the runtime's own memory for a stream's queue comes in 2 MiB pieces.
        assert abs(torch.cuda.mem_get_info()[0] - free0) < 4 * n
        assert hip.lcp_info()[0] == 0
    block.close()
    synth.close()


@ends_at_a_fault
def test_refused_when_free_memory_is_below_the_need():
    """Free HBM held below the smaller of the two needs (8 bytes per row without positions, some 17 with them): both calls
    are refused with the need in the message, nothing stays allocated, the handle is still good.  What this process' tensor
    cache holds from earlier cases is given back first, and the free memory is looked at again after the hold: the cache
    gives blocks back when a large request does not fit at once."""
    import torch
    rng = np.random.default_rng(75)
    text = bytes(rng.integers(0, 4, 1 << 24, dtype=np.uint8) + 97)
    hip = findex_amd.HipFMSearcher.from_text(text)
    hip.prepare(ktab=False, lcp=True)
    _, s0 = hip.ngrams(16, top=10)
    least = 8 * hip.n                                           # A and S alone: what the call without positions allocates first
    hogs = []
    for _ in range(3):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info()[0]
        if free < least // 2:
            break
        hogs.append(torch.empty(free - least // 4, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("free before the calls: %d MiB, the smaller need: %d MiB" % (free1 >> 20, least >> 20))
    assert free1 < least
    for positions in (True, False):
        with pytest.raises(findex_amd.FmxError) as e:
            hip.ngrams(16, top=10, positions=positions)
        assert e.value.code == NOMEM and "needs" in str(e.value) and "are free" in str(e.value)
        assert abs(torch.cuda.mem_get_info()[0] - free1) < 4 * hip.n      # (every temporary of the call is 4 n bytes or more)
    del hogs
    torch.cuda.empty_cache()
    assert hip.ngrams(16, top=10)[1] == s0                      # what fits still runs
    hip.close()


# ---------------------------------------------------------------- 10. one text of 2^20 bytes
@ends_at_a_fault
def test_a_megabyte():
    rng = np.random.default_rng(47)
    m = 1 << 20
    t = bytearray((rng.integers(0, 4, m, dtype=np.uint8) + 97).tobytes())
    for i, (src, ln) in enumerate([(1000, 40), (20000, 41), (50000, 100), (90000, 777), (200000, 5000), (300000, 2048)]):
        dst = 600000 + 40000 * i + 7 * i
        t[dst:dst + ln] = t[src:src + ln]
    t[1040000:1040777] = t[90000:90777]                         # one of them a third time
    text = bytes(t)
    hip = findex_amd.HipFMSearcher.from_text(text)
    got = hip.ngrams([12, 24], top=1000, order="count", spectrum=1024)
    lean = hip.ngrams([12, 24], top=1000, order="count", spectrum=1024, positions=False)
    for L, g, g2 in zip((12, 24), got, lean):
        want = reference(text, L, 2, "count", 1000, 0, 1024)
        print("2^20 L", L, {f: g[1][f] for f in ngrams_ref.FIELDS})
        same(g, want, L)
        same(g2, want, (L, "no positions"), positions=False)
        invariants(text, L, 0, g[1], 1024, L)
    assert got[1][1]["largest_count"] == 3 and got[0][0].size == 1000
    hip.close()
    _classes.clear()


# ---------------------------------------------------------------- 11. a corpus
def expected_phrases(ref, docs, L, min_count, top):
    """brute over the stream with the separator as the stop byte; text, documents and first occurrence by the per-position table"""
    rec, _ = ngrams_ref.brute(ref.stream, L, min_count=min_count, order="count", top=top, stop=1)
    rows = []
    for r in rec:
        t, count = int(r["first_pos"]), int(r["count"])
        w = ref.stream[t:t + L]
        starts = [i for i in range(len(ref.stream) - L + 1) if ref.stream[i:i + L] == w]
        assert len(starts) == count and starts[0] == t
        d, _, lo = ref.map(t)
        d2, _, hi = ref.map(t + L - 1)
        assert d == d2
        rows.append((docs[d][lo:hi + 1], count, len({ref.map(i)[0] for i in starts}), d, lo))
    return rows


@ends_at_a_fault
def test_corpus_frequent_phrases(tmp_path):
    docs = corpus_documents()
    ref = RefCorpus(docs)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    for L, min_count, top in ((12, 2, 100), (5, 3, 40), (30, 2, 1000)):
        rows = cs.frequent_phrases(L, min_count=min_count, top=top)
        want = expected_phrases(ref, docs, L, min_count, top)
        print("corpus L", L, len(rows), rows[:3])
        assert rows == want and len(rows) > 5
    rows = cs.frequent_phrases(12)
    assert any(b"\x00" in r[0] or b"\x01" in r[0] or b"\xff" in r[0] for r in rows)      # the stretch with the raw 0, 1 and 255
    assert any(r[2] >= 2 for r in rows)
    cs.close()
    # the documents without special bytes: the number of files of every phrase by an `in` test over the raw files
    plain = [d for d in docs if not any(c in d for c in (0, 1, 255))]
    assert len(plain) == 6
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(plain))
    rows = cs.frequent_phrases(12, top=300)
    assert len(rows) > 50
    for text, count, n_docs, doc, raw_off in rows:
        assert n_docs == sum(1 for d in plain if text in d) and plain[doc][raw_off:raw_off + 12] == text
        assert count == sum(sum(1 for i in range(len(d) - 11) if d[i:i + 12] == text) for d in plain)
    cs.close()
    # the command line, the directory form
    src = tmp_path / "docs"
    src.mkdir()
    for d, raw in enumerate(docs):
        (src / ("d%d" % d)).write_bytes(raw)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", "--dir", str(src), "--out", str(tmp_path / "x"), "--no-filter-binary",
                        "--ngrams", "12,5", "--min-count", "3", "--top", "20"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    from findex_amd.index import printable
    want = []
    for L in (12, 5):
        want += [b"%d\t%d\t%d\td%d\t%d\t" % (L, c, nd, d, lo) + printable(w) for w, c, nd, d, lo in expected_phrases(ref, docs, L, 3, 20)]
    lines = (tmp_path / "x.ngrams").read_bytes().split(b"\n")
    assert lines[-1] == b"" and lines[:-1] == want and len(want) > 20
    # and the single-file form: the strings of the file, no stop byte
    one = tmp_path / "one.txt"
    one.write_bytes(docs[0] + docs[3])
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", str(one), "--ngrams", "9", "--top", "0"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    text = docs[0] + docs[3]
    rec, _ = ngrams_ref.brute(text, 9, min_count=2, order="count")
    want = [b"9\t%d\t%d\t" % (int(x["count"]), int(x["first_pos"])) + printable(text[int(x["first_pos"]):int(x["first_pos"]) + 9]) for x in rec]
    lines = (tmp_path / "one.ngrams").read_bytes().split(b"\n")
    assert lines[-1] == b"" and lines[:-1] == want and want
