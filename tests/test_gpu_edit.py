"""Edit-distance search on the device (fmx_search_edit_batch) against tests/edit_ref.py, in both layouts.  Every
expectation is edit_ref.dfs_hits -- all 256 symbols and the full row at every node, no one-row rule -- and every step count
edit_ref.walk, the walk of DESIGN.md 19 restated over the oracle, whose hits are held to dfs_hits' on the way; the corpus
case is held to edit_ref.brute_hits over the stream.  Nothing of the library produces an expectation."""
import ctypes
import os

import numpy as np
import pytest

import approx_ref
import corpus_ref
import edit_ref
import findex_amd
import oracle
from conftest import TESTDATA
from findex_amd import _lib
from helpers import lf_walk_patterns, pack_patterns, synth_bwt
from test_gpu_approx import open_index, open_text, waves_max

pytestmark = pytest.mark.gpu

LAYOUTS = ["onehot", "bytes"]
HIT = findex_amd.HipFMSearcher.EDIT_HIT
ARG, HIP, UNSUPPORTED, OVERFLOW = 3, 5, 6, 9


def expected_arrays(per_pattern):
    off, rows = edit_ref.expected_csr(per_pattern)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=HIT) if rows else np.zeros(0, dtype=HIT)


def reference(orc, pats, sub=(1, 255), budgets=(0, 1, 2)):
    """-> ({e: per-pattern hits}, {e: steps of the batch}): dfs_hits at the largest budget, the smaller budgets its hits
    with d <= e, and walk at every budget, whose hits must be those."""
    top = max(budgets)
    full = [edit_ref.dfs_hits(orc, p, top, *sub) for p in pats]
    per, steps = {}, {}
    for e in budgets:
        per[e] = [edit_ref.within(h, e) for h in full]
        steps[e] = 0
        for p, want in zip(pats, per[e]):
            hits, st = edit_ref.walk(orc, p, e, *sub)
            assert hits == want, (p, e, sub)
            steps[e] += st
    return per, steps


def check(hip, pats, e, per_pattern, sub=(1, 255), what=None, steps=None):
    """One batch against its expectation; with `steps`, also what fmx_edit_last reports of the call."""
    buf, off = pack_patterns(pats)
    got_off, got = hip.search_edit_batch(buf, off, e, sub=sub)
    exp_off, exp = expected_arrays(per_pattern)
    assert np.array_equal(got_off, exp_off), (what, e)
    assert got.tobytes() == exp.tobytes(), (what, e)
    if steps is not None:
        _, _, got_steps, requests = hip.edit_last()
        print("%s e=%d: %d hits, %d steps (walk: %d), %d requests" % (what, e, got.size, got_steps, steps, requests))
        assert got_steps == steps, (what, e, got_steps, steps)
        assert steps == 0 or 0 < requests <= 4 * steps, (what, e, requests, steps)


def edited(rng, s, m, alphabet):
    """Patterns from the text s: a stretch of m bytes as it is, and with one byte deleted, inserted, replaced, at the first, a
    middle and the last position, and two of these combined -- among them two deletions and two insertions: the text's own
    stretch is then a hit of len m' + 2 and of len m' - 2, the two ends of the band."""
    at = int(rng.integers(1, len(s) - m - 1))
    base = s[at:at + m]
    pats = [base]

    def other(c):
        return int(rng.choice([x for x in alphabet if x != c]))

    def dele(p, pos):
        return p[:pos] + p[pos + 1:]

    def ins(p, pos):
        return p[:pos] + bytes([int(rng.choice(alphabet))]) + p[pos:]

    def rep(p, pos):
        return p[:pos] + bytes([other(p[pos])]) + p[pos + 1:]

    where = sorted({0, m // 2, m - 1})
    for pos in where:
        pats += [dele(base, pos), ins(base, pos), rep(base, pos)]
    pats.append(ins(base, m))                                # behind the last byte
    if m >= 3:
        first, mid, last = 0, m // 2, m - 1
        pats += [dele(dele(base, last), first), ins(ins(base, m), 0), rep(rep(base, last), first),
                 dele(rep(base, last), first), ins(dele(base, mid), 0), rep(ins(base, mid), 0), dele(dele(base, mid), mid)]
    return pats


@pytest.fixture(scope="module")
def abcd_text():
    rng = np.random.default_rng(33)
    return bytes(rng.integers(97, 101, 3000, dtype=np.uint8))


# ---------------------------------------------------------------- fixture texts
@pytest.fixture(scope="module")
def texts(abcd_text):
    """text name -> (text, patterns, {e: hits}, {e: steps})"""
    rng = np.random.default_rng(40)
    with open(os.path.join(TESTDATA, "test1024.txt"), "rb") as f:
        t1024 = f.read()
    out = {}
    for name, s in (("test1024", t1024), ("abcd", abcd_text)):
        alphabet = sorted(set(s))
        pats = [p for m in (1, 2, 6, 12, 24) for p in edited(rng, s, m, alphabet)]
        per, steps = reference(approx_ref.index_of(s)[0], pats)
        out[name] = (s, pats, per, steps)
    return out


def test_text_expectations_are_the_ones_the_kernel_needs(texts):
    for name, (s, pats, per, steps) in texts.items():
        rel = [ln - len(p) for p, hs in zip(pats, per[2]) for _, ln, _, d in hs if d == 2]
        print("%s: %d patterns, hits %s, steps %s" % (name, len(pats), {e: sum(map(len, per[e])) for e in per}, steps))
        assert {-2, -1, 0, 1, 2} <= set(rel), name           # the whole band: hits of len m - 2 and of len m + 2
        assert sum(1 for hs in per[0] if hs) >= 6 and sum(1 for hs in per[0] if not hs) >= 20
        assert sum(1 for a, b in zip(per[1], per[2]) if len(a) < len(b)) >= 20
    # two hits of one pattern that share sp: a string and the same string with a byte more in front of it
    assert any(a[0] == b[0] for hs in texts["abcd"][2][2] for a, b in zip(hs, hs[1:]))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["test1024", "abcd"])
def test_fixture_texts(texts, name, layout):
    s, pats, per, steps = texts[name]
    hip = open_text(s, layout)
    for e in (0, 1, 2):
        check(hip, pats, e, per[e], what=name, steps=steps[e])
    hip.close()


# ---------------------------------------------------------------- synthetic BWTs around the block edges
def synth_shapes():
    """sp and ep in one block, in two, at a block's edge, in each layout (448 positions per one-hot block, 128 per bytes
    block); the EOF slot first, in the middle and last."""
    for lo, hi, sizes in ((97, 100, (447, 448, 449)), (1, 200, (127, 128, 129))):
        for n in sizes:
            for eof in (0, n // 2, n - 1):
                yield lo, hi, n, eof


@pytest.fixture(scope="module")
def synth():
    out = []
    for lo, hi, n, eof in synth_shapes():
        index = synth_bwt(n, lo, hi, seed=n + lo, eof=eof)
        orc = oracle.NaiveFMSearcher.from_mem(*index)
        rng = np.random.default_rng(n + eof)
        alphabet = list(range(lo, hi + 1))
        pats = []
        for p in lf_walk_patterns(orc, rng, 4, 8, 0.3, alphabet=alphabet):
            pos = int(rng.integers(0, len(p)))
            pats += [p, p[:pos] + p[pos + 1:], p[:pos] + bytes([int(rng.choice(alphabet))]) + p[pos:]]
        per, steps = reference(orc, pats)
        out.append((index, (lo, hi, n, eof), pats, per, steps))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_synthetic_bwts(synth, layout):
    found = 0
    for index, shape, pats, per, steps in synth:
        hip = open_index(index, layout)
        for e in (0, 1, 2):
            check(hip, pats, e, per[e], what=shape, steps=steps[e])
        found += sum(map(len, per[2]))
        hip.close()
    assert found > 1500


# ---------------------------------------------------------------- m = 0, 1, 2, 255; 256 refused
@pytest.fixture(scope="module")
def lengths(abcd_text):
    s = abcd_text
    p255 = s[700:955]
    pats = [b"", b"a", b"z", b"ab", b"zz", p255, p255[:100] + p255[101:] + b"a", p255[:254] + b"z", s[:255], s[-255:]]
    per, steps = reference(approx_ref.index_of(s)[0], pats)
    return pats, per, steps


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pattern_lengths_and_the_refusal_of_256(lengths, abcd_text, layout):
    import torch
    s = abcd_text
    pats, per, steps = lengths
    n = len(s) + 1
    assert per[2][0][0] == (0, 0, n, 0) and len(per[2][0]) == 1 + 4 + 16          # the empty pattern: every string of 1 .. 2 bytes
    assert (0, 0, n, 1) in per[1][1] and (0, 0, n, 2) in per[2][3]               # m <= e: the empty string
    assert any(ln == 257 for _, ln, _, _ in per[2][5]) and any(ln == 253 for _, ln, _, _ in per[2][5])
    assert [h[3] for h in per[2][6] if h[1] >= 254] and per[1][7]
    hip = open_text(s, layout)
    for e in (0, 1, 2):
        check(hip, pats, e, per[e], what="lengths", steps=steps[e])
    assert hip.search_edit(b"", 0) == [(0, n, 0, 0)]
    off, hits = hip.search_edit_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 2)       # k = 0
    assert off.tolist() == [0] and hits.size == 0
    # 256 bytes: the host form refuses on the host, the device form after its launch, which skips the pattern
    long = [s[10:20], s[100:356], s[30:40]]
    buf, poff = pack_patterns(long)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_edit_batch(buf, poff, 1)
    assert ei.value.code == ARG and "255 bytes" in str(ei.value)
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(poff.view(np.int64)).cuda()
    d_out_off = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((64 * HIT.itemsize,), 0xCD, dtype=torch.uint8, device="cuda")
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_edit_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), 3, 1, d_out_off.data_ptr(), d_out.data_ptr(), 64)
    assert ei.value.code == ARG and "255 bytes" in str(ei.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xCD).all()               # no hits written
    check(hip, [long[0], long[2]], 1, [edit_ref.dfs_hits(approx_ref.index_of(s)[0], p, 1) for p in (long[0], long[2])], what="after")
    hip.close()


# ---------------------------------------------------------------- the beginning of the text, byte 0, ranges
@pytest.fixture(scope="module")
def prefix_case():
    """Patterns at the beginning of the text: when s[0:m] has been matched the interval is the one row of the whole text,
    the EOF row, whose BWT' symbol is 0 -- nothing extends it but a pattern that holds byte 0 there."""
    with open(os.path.join(TESTDATA, "test1024.txt"), "rb") as f:
        s = f.read()
    pats = []
    for m in (8, 24):
        base = s[:m]
        pats += [base, base[1:], b"z" + base, base[:1] + b"z" + base[1:], bytes([s[m]]) + base, b"zz" + base, base[2:],
                 b"\0" + base[:3], b"z\0" + base[:3], b"\0z" + base[:3], b"\0" + base[1:4]]
    pats += [s[-4:] + b"\0", s[-4:] + b"z\0", s[-3:] + b"\0" + s[:3], s[-3:] + b"\0z" + s[:3], b"\0", b"\0\0"]
    per, steps = reference(approx_ref.index_of(s)[0], pats)
    return s, pats, per, steps


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_beginning_of_the_text_and_byte_zero(prefix_case, layout):
    s, pats, per, steps = prefix_case
    orc = approx_ref.index_of(s)[0]
    eof = orc.eof
    assert per[0][0] == [(eof, 8, eof + 1, 0)]               # the row of the whole text
    assert not per[0][2] and (eof, 8, eof + 1, 1) in per[1][2] and (eof, 8, eof + 1, 2) in per[2][5]      # z in front: deleted
    assert per[0][7] == [(0, 4, 1, 0)] and (0, 4, 1, 1) in per[1][8]                                    # behind the sentinel
    assert per[0][-4] and per[0][-3] == [] and per[1][-3]
    hip = open_text(s, layout)
    for e in (0, 1, 2):
        check(hip, pats, e, per[e], what="prefix", steps=steps[e])
    hip.close()


@pytest.fixture(scope="module")
def ranges(abcd_text):
    rng = np.random.default_rng(41)
    s = abcd_text
    pats = [p for m in (3, 6, 12) for p in edited(rng, s, m, [97, 98, 99, 100])][::2] + [b"", b"a"]
    orc = approx_ref.index_of(s)[0]
    return pats, {sub: reference(orc, pats, sub, (1, 2)) for sub in ((98, 99), (2, 254), (100, 255), (1, 96), (97, 97))}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ranges_that_leave_letters_out(ranges, abcd_text, layout):
    pats, by_sub = ranges
    count = {sub: sum(map(len, by_sub[sub][0][2])) for sub in by_sub}
    print("hits at e = 2 per range:", count)
    assert 0 < count[(1, 96)] < count[(97, 97)] < count[(98, 99)] < count[(2, 254)] and count[(100, 255)] < count[(98, 99)]
    hip = open_text(abcd_text, layout)
    for sub, (per, steps) in by_sub.items():
        for e in (1, 2):
            check(hip, pats, e, per[e], sub=sub, what=sub, steps=steps[e])
    hip.close()


# ---------------------------------------------------------------- e = 0 is the exact search
@pytest.mark.parametrize("layout", LAYOUTS)
def test_budget_zero_is_the_exact_search(layout):
    index = synth_bwt(4500, 97, 100, seed=31)
    orc = oracle.NaiveFMSearcher.from_mem(*index)
    rng = np.random.default_rng(32)
    pats = lf_walk_patterns(orc, rng, 3000, 16, 0.5, alphabet=[97, 98, 99, 100]) + [b"", b"a", b"\0", b"a\0"]
    buf, off = pack_patterns(pats)
    hip = open_index(index, layout)
    hip.config_set("jump", "off")
    hip.config_set("ktab", "off")
    hip.stats_reset()
    sp, ep = hip.search_batch(buf, off)
    st = hip.stats()
    exact_steps = st["backward_steps"]
    osp, oep, osteps = orc.search_batch(buf, off)
    assert exact_steps == int(osteps.sum()) and np.array_equal(sp, osp) and np.array_equal(ep, oep)
    seen, launches = st["patterns_seen"], st["launches"]
    got_off, hits = hip.search_edit_batch(buf, off, 0)
    found = sp < ep
    assert 500 < int(found.sum()) < 2700
    assert np.array_equal(np.diff(got_off.astype(np.int64)), found.astype(np.int64))
    assert np.array_equal(hits["pattern"], np.nonzero(found)[0]) and not hits["edits"].any()
    assert np.array_equal(hits["len"], np.diff(off.astype(np.int64))[found])
    assert np.array_equal(hits["sp"], sp[found]) and np.array_equal(hits["ep"], ep[found])
    _, _, steps, requests = hip.edit_last()
    assert steps == exact_steps and 0 < requests <= 4 * steps
    st = hip.stats()
    # the counting call and the call that fetched the hits: their steps are on the handle's counters, and nothing else moved
    assert st["backward_steps"] == 3 * exact_steps and st["launches"] == launches + 2
    assert st["patterns_seen"] == seen and st["tables_held_bytes"] == 0
    # opts == NULL is e = 0 with the default range
    L = _lib.load()
    n_out = ctypes.c_size_t()
    o2 = np.zeros(off.size, dtype=np.uint64)
    h2 = np.zeros(hits.size, dtype=HIT)
    assert L.fmx_search_edit_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, None, o2.ctypes.data,
                                   h2.ctypes.data, h2.size, ctypes.byref(n_out)) == 0
    assert n_out.value == hits.size and np.array_equal(o2, got_off) and h2.tobytes() == hits.tobytes()
    hip.close()


def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_edit(b"abr", 1)
    assert ei.value.code == UNSUPPORTED
    out_off = np.zeros(2, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    opts = _lib.fmx_edit_opts(1, 0, 0, 0)
    assert _lib.load().fmx_search_edit_batch_dev(hip.handle, None, out_off.ctypes.data, 1, ctypes.byref(opts), out_off.ctypes.data,
                                                 None, 0, ctypes.byref(n_out), None) == UNSUPPORTED
    hip.close()


# ---------------------------------------------------------------- capacity, order, determinism, the counters
@pytest.fixture(scope="module")
def batch(abcd_text):
    rng = np.random.default_rng(35)
    s = abcd_text
    pats = [p for _ in range(6) for p in edited(rng, s, 6, [97, 98, 99, 100])]
    per, steps = reference(approx_ref.index_of(s)[0], pats)
    return pats, per, steps


@pytest.mark.parametrize("layout", LAYOUTS)
def test_capacity_order_and_determinism(batch, abcd_text, layout):
    pats, per, _ = batch
    exp_off, exp = expected_arrays(per[2])
    T = exp.size
    assert T > 10_000
    hip = open_text(abcd_text, layout)
    buf, off = pack_patterns(pats)
    L = _lib.load()
    opts = _lib.fmx_edit_opts(2, 0, 0, 0)
    guard = 64

    def call(cap):
        out = np.full((cap + guard) * HIT.itemsize, 0xAB, dtype=np.uint8)
        out_off = np.zeros(off.size, dtype=np.uint64)
        n_out = ctypes.c_size_t()
        rc = L.fmx_search_edit_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(opts),
                                     out_off.ctypes.data, out.ctypes.data if cap else None, cap, ctypes.byref(n_out))
        assert (out[cap * HIT.itemsize:] == 0xAB).all()      # nothing behind out[cap - 1]
        return rc, int(n_out.value), out_off, out[: cap * HIT.itemsize].view(HIT)

    rc, n, o, h = call(T)
    assert rc == 0 and n == T and np.array_equal(o, exp_off) and h.tobytes() == exp.tobytes()
    for cap in (T - 1, 1, 0):                                # one short, and the counting call: the exact total
        rc, n, _, _ = call(cap)
        assert rc == OVERFLOW and n == T, cap
        assert str(T).encode() in L.fmx_last_error()
    rc, n2, o2, h2 = call(n)                                 # the retry at n_out
    assert rc == 0 and n2 == T and h2.tobytes() == h.tobytes() and np.array_equal(o2, o)   # two calls, identical bytes
    # order: (sp, len) ascends strictly inside every pattern, sp alone does not; `pattern` is the CSR segment
    seg = np.repeat(np.arange(len(pats)), np.diff(o.astype(np.int64)))
    assert np.array_equal(h["pattern"], seg)
    same = seg[1:] == seg[:-1]
    key = (h["sp"].astype(np.int64) << 16) | h["len"].astype(np.int64)
    assert (key[1:][same] > key[:-1][same]).all() and (h["sp"] < h["ep"]).all()
    shared = same & (h["sp"][1:] == h["sp"][:-1])
    assert shared.sum() > 100 and (h["len"][1:][shared] > h["len"][:-1][shared]).all()
    assert int(o[-1]) == T
    hip.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_step_count_relation(batch, abcd_text, layout):
    """fmx_edit_last's steps are the walk's, the handle's backward_steps grow by them once per launch (the counting call and
    the sized call), and the requests lie in (0, 4 steps]."""
    pats, per, steps = batch
    hip = open_text(abcd_text, layout)
    buf, off = pack_patterns(pats)
    assert steps[0] < steps[1] < steps[2]
    for e in (0, 1, 2):
        st0 = hip.stats()
        got_off, got = hip.search_edit_batch(buf, off, e)
        st1 = hip.stats()
        assert got.size == sum(map(len, per[e])) > 0
        _, _, got_steps, requests = hip.edit_last()
        print("%s e = %d: %d hits, %d steps (walk: %d), %d requests" % (layout, e, got.size, got_steps, steps[e], requests))
        assert got_steps == steps[e] and 0 < requests <= 4 * steps[e]
        assert st1["launches"] == st0["launches"] + 2
        assert st1["backward_steps"] - st0["backward_steps"] == 2 * steps[e]
        assert st1["patterns_seen"] == st0["patterns_seen"] and st1["tables_held_bytes"] == 0
    hip.close()


# ---------------------------------------------------------------- the device form
@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_form_and_stream_capture(batch, abcd_text, layout):
    import torch
    pats, per, _ = batch
    hip = open_text(abcd_text, layout)
    buf, off = pack_patterns(pats)
    h_off, h_hits = expected_arrays(per[2])
    T, k = h_hits.size, len(pats)
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * HIT.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        n = hip.search_edit_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T,
                                      stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * HIT.itemsize].tobytes() == h_hits.tobytes() and (raw[T * HIT.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), h_off)
    # too small: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_edit_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy()[(T - 1) * HIT.itemsize:] == 0xCD).all()
    # under a stream capture the call is refused before it allocates or launches, and the capture goes on
    launches = hip.stats()["launches"]
    torch.cuda.empty_cache()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g.capture_begin()
        try:
            hip.search_edit_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T,
                                      stream=st.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        d_out_off.zero_()
        g.capture_end()
    assert err is not None and err.code == HIP and "stream capture" in str(err)
    d_out_off.fill_(7)
    g.replay()                                               # the capture is valid: its one node runs
    torch.cuda.synchronize()
    assert not d_out_off.cpu().numpy().any()
    del g
    assert hip.stats()["launches"] == launches
    hip.close()


# ---------------------------------------------------------------- several patterns per wave
class Pool:
    """Distinct patterns with their hits (flat, each pattern's by (sp, len)) and their walk steps at budget `top`: a batch is
    an array of pool indices, and its expectation is expanded from the pool's with numpy."""

    def __init__(self, s, pats, top):
        orc = approx_ref.index_of(s)[0]
        self.pats = pats
        self.len = np.array([len(p) for p in pats])
        full = [edit_ref.dfs_hits(orc, p, top) for p in pats]
        self.hits = np.array([h for hs in full for h in hs], dtype=np.int64).reshape(-1, 4)      # (sp, len, ep, d)
        self.owner = np.repeat(np.arange(len(pats)), [len(hs) for hs in full])
        walks = [edit_ref.walk(orc, p, top) for p in pats]
        assert [w[0] for w in walks] == full
        self.steps = {top: np.array([w[1] for w in walks], dtype=np.int64)}

    def expected(self, idx, e):
        """-> (off, records, steps) of the batch [pats[j] for j in idx] at budget e."""
        keep = self.hits[:, 3] <= e
        hits, owner = self.hits[keep], self.owner[keep]
        cnt = np.bincount(owner, minlength=len(self.pats))
        first = np.cumsum(cnt) - cnt
        per = cnt[idx]
        off = np.concatenate([[0], np.cumsum(per)])
        src = np.repeat(first[idx] - off[:-1], per) + np.arange(int(off[-1]))
        rows = np.zeros(int(off[-1]), dtype=HIT)
        rows["pattern"] = np.repeat(np.arange(idx.size), per)
        rows["sp"], rows["len"], rows["ep"], rows["edits"] = hits[src, 0], hits[src, 1], hits[src, 2], hits[src, 3]
        return off.astype(np.uint64), rows, int(self.steps[e][idx].sum())


@pytest.fixture(scope="module")
def many(abcd_text):
    """k = 3 * waves_max() + 5 patterns drawn with repetition from a pool of about 250 patterns of 0 .. 12 bytes over the abcd
    text; a second draw from the pool's patterns of at most 6 bytes for e = 2."""
    s = abcd_text
    rng = np.random.default_rng(38)
    pats = {b"", b"z" * 4, b"z" * 8, b"z" * 12, s[5:9] + b"zzzz" + s[13:17]}
    while sum(1 for p in pats if len(p) <= 12) < 250:
        m = int(rng.integers(0, 13))
        pats.update(edited(rng, s, m, [97, 98, 99, 100])[: 1 + int(rng.integers(0, 20))] if m else [b""])
    pats = sorted(p for p in pats if len(p) <= 12)
    short = [p for p in pats if len(p) <= 6]
    W = waves_max()
    k = 3 * W + 5
    return Pool(s, pats, 1), rng.integers(0, len(pats), k), Pool(s, short, 2), rng.integers(0, len(short), k), W


def test_many_expectations_are_the_ones_the_kernel_needs(many):
    pool, idx, pool2, idx2, W = many
    k = idx.size
    print("several patterns per wave: k = %d, waves_max = %d, pool of %d (%d of at most 6 bytes)" % (k, W, len(pool.pats), len(pool2.pats)))
    assert k >= 3 * W and k % 4 != 0 and 240 <= len(pool.pats) <= 290 and len(pool2.pats) >= 60
    assert set(pool.len.tolist()) == set(range(13))
    for p, ix in ((pool, idx), (pool2, idx2)):
        assert (ix[:-W] != ix[W:]).mean() > 0.95 and (p.len[ix[:-W]] != p.len[ix[W:]]).mean() > 0.4
    _, rows, steps = pool.expected(idx, 1)
    print("e = 1: %d hits, %d steps" % (rows.size, steps))
    assert 100_000 < rows.size < 5_000_000
    _, rows, steps = pool2.expected(idx2, 2)
    print("e = 2: %d hits, %d steps" % (rows.size, steps))
    assert 1_000_000 < rows.size < 8_000_000 and (rows["edits"] == 2).sum() > 500_000


@pytest.mark.parametrize("layout", LAYOUTS)
def test_several_patterns_per_wave(many, abcd_text, layout):
    """Every wave's loop over the batch goes round three times and more: the wave starts each pattern from the root with an
    empty stack, whatever the one before left in its frames."""
    pool, idx, pool2, idx2, W = many
    hip = open_text(abcd_text, layout)
    for p, ix, e in ((pool, idx, 1), (pool2, idx2, 2)):
        buf, off = pack_patterns([p.pats[j] for j in ix.tolist()])
        exp_off, exp, steps = p.expected(ix, e)
        st0 = hip.stats()
        got_off, got = hip.search_edit_batch(buf, off, e)
        st1 = hip.stats()
        assert np.array_equal(got_off, exp_off), e
        assert got.tobytes() == exp.tobytes(), e
        _, _, got_steps, requests = hip.edit_last()
        print("%s e = %d: k = %d, %d hits, %d steps (walk: %d), %d requests" % (layout, e, ix.size, got.size, got_steps, steps, requests))
        assert got_steps == steps and 0 < requests <= 4 * steps, (e, got_steps, steps, requests)
        assert st1["launches"] == st0["launches"] + 2
        assert st1["backward_steps"] - st0["backward_steps"] == 2 * steps, e
    hip.close()


# ---------------------------------------------------------------- a repetitive text: deep stacks over wide intervals
@pytest.fixture(scope="module")
def fibonacci():
    a, b = b"a", b"ab"
    while len(b) < 3000:
        a, b = b, b + a
    s = b[:3000]
    rng = np.random.default_rng(42)
    pats = []
    for m in (200, 233, 254, 255):
        at = int(rng.integers(100, 2500))
        base = s[at:at + m]
        flip = bytes([195 - base[m // 2]])
        pats += [base, base[:m // 2] + flip + base[m // 2 + 1:], base[:40] + base[41:160] + flip + base[160:]]
    per, steps = reference(approx_ref.index_of(s)[0], pats, budgets=(2,))
    return s, pats, per, steps


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_repetitive_text_with_long_patterns(fibonacci, layout):
    s, pats, per, steps = fibonacci
    assert set(s) == {97, 98} and all(200 <= len(p) <= 255 for p in pats) and max(map(len, pats)) == 255
    wide = max(ep - sp for hs in per[2] for sp, _, ep, _ in hs)
    print("fibonacci: %d patterns, %d hits, widest interval %d, %d steps" % (len(pats), sum(map(len, per[2])), wide, steps[2]))
    assert all(per[2]) and wide >= 5 and steps[2] > 5 * sum(map(len, pats))
    hip = open_text(s, layout)
    check(hip, pats, 2, per[2], what="fibonacci", steps=steps[2])
    hip.close()


# ---------------------------------------------------------------- text offsets
@pytest.mark.parametrize("layout", LAYOUTS)
def test_locate_text_edits(abcd_text, layout):
    """(text offset, len, edits) of every place a string within e edits of q stands at, against a scan of the text for every
    string of edit_ref.brute_strings; each hit is located with its own length."""
    text = abcd_text[:600]
    hip = open_text(text[::-1], layout)                      # the index holds reverse(text) + sentinel
    for q, e in ((text[100:108], 1), (text[200:204] + text[205:210], 2), (text[:6], 1), (text[-6:], 2), (b"ab", 2), (b"zz", 1)):
        strings = edit_ref.brute_strings(text, q, e)
        exp = []
        for Q, d in strings.items():
            at = text.find(Q)
            while at >= 0:
                exp.append((at, len(Q), d))
                at = text.find(Q, at + 1)
        got = hip.locate_text_edits(q, e)
        assert got.dtype == np.uint64 and [tuple(r) for r in got.tolist()] == sorted(exp), (q, e)
        assert hip.locate_text_edits(q, e, max_hits=1).shape == (len(strings), 3)
    assert (0, 6, 0) in [tuple(r) for r in hip.locate_text_edits(text[:6], 1).tolist()]
    hip.close()


# ---------------------------------------------------------------- the corpus
def test_corpus_locate_docs_edits(tmp_path):
    rng = np.random.default_rng(37)
    q = b"needlework"
    letters = np.frombuffer(b"abcfghijmpqstuvxy", dtype=np.uint8)          # none of the query's: what is found was planted
    names = ["a.txt", "b.txt", "c.txt", "d.txt", "e.txt", "f.txt", "g.txt", "h.txt"]
    docs = {nm: bytearray(rng.choice(letters, 120 + 17 * j).tobytes()) for j, nm in enumerate(names)}
    for nm in names:
        (tmp_path / nm).write_bytes(bytes(docs[nm]))
    order = [os.fsdecode(x) for x in findex_amd.list_files(str(tmp_path))]
    assert sorted(order) == names

    def plant(nm, at, text):
        docs[nm][at:at + len(text)] = text

    plant(order[0], 0, q)                                    # exact, at the beginning of the first file
    plant(order[0], 60, b"needlwork")                        # a letter dropped
    plant(order[1], 50, b"needdlework")                      # a letter doubled
    plant(order[2], 40, b"neidlewok")                        # replaced and dropped: two edits
    plant(order[3], 30, b"needle\x01work")                   # a raw byte 1 inside: it is escaped in the stream, never inserted
    plant(order[4], 20, b"\x01needlework\x01")               # ... and next to a hit
    plant(order[7], len(docs[order[7]]) - 9, b"eedlework")   # at the end of the last file, the first letter dropped
    docs[order[5]][-5:] = b"needl"                           # one that straddles two files
    docs[order[6]][:4] = b"work"
    for nm in names:
        (tmp_path / nm).write_bytes(bytes(docs[nm]))
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_dir(str(tmp_path)))
    assert [os.fsdecode(x) for x in cs.corpus.names] == order
    ref = corpus_ref.RefCorpus([bytes(docs[nm]) for nm in order])
    stream = ref.stream
    assert stream.count(b"\\1") == 3 and stream.count(b"\x01") == len(order)
    for e in (0, 1, 2):
        # every distinct string of the stream within e edits (bytes 2 .. 254 inserted or substituted), at each of its places:
        # the library searches the reversed query in the index of the reversed stream, the same strings read backwards
        exp = []                                             # (two strings may begin inside one escape pair: equal rows)
        for Q, d in edit_ref.brute_strings(stream, q, e, 2, 254).items():
            at = stream.find(Q)
            while at >= 0:
                exp.append((ref.table[at][0], ref.table[at][2], len(Q), d))
                at = stream.find(Q, at + 1)
        doc, raw, ln, edits = cs.locate_docs_edits(q, e)
        got = list(zip(doc.tolist(), raw.tolist(), ln.tolist(), edits.tolist()))
        assert got == sorted(exp), e
        at = cs.corpus.to_stream(doc, raw).astype(np.int64)
        assert all(b"\x01" not in stream[a:a + l_] for a, l_ in zip(at.tolist(), ln.tolist()))        # nothing spans two files
        if e == 0:
            assert got == [(0, 0, 10, 0), (4, 21, 10, 0)]
        if e >= 1:
            assert (0, 60, 9, 1) in got and (1, 50, 11, 1) in got and (7, len(docs[order[7]]) - 9, 9, 1) in got
            assert not any(d_ == 5 and r_ >= len(docs[order[5]]) - 5 for d_, r_, _, _ in got)          # the straddling one
            # the raw byte 1 inside a word is two stream bytes, both of the range: two insertions, the escape-pair limit
            assert [x for x in got if x[0] == 3] == ([(3, 30, 12, 2)] if e == 2 else [])
        if e == 2:
            assert (2, 40, 9, 2) in got
    cs.close()
