"""Matching statistics and maximal exact matches on the device (fmx_match_stats_batch, fmx_mems_batch) against
tests/mstat_ref.py, in both layouts: the edges of the walk kernel's tiles and of its halo, every max_len path, the refill
of lane groups inside a wave, many patterns per tile, the pattern edge, special bytes and rows, the counters, the device and
captured forms, the MEM compaction with its capacity contract, and the text and corpus layers.

Every expectation is mstat_ref.loop_stats over the oracle (held to the substring test by tests/test_mstat_cpu.py), computed
once per case and shared by the two layouts; where a case passes steps, fmx_mstat_last and the handle's backward_steps are
held to the reference's step sum exactly.  T is the tile of the walk kernel and GROUPS the lane groups of a wave, both as
findex_amd._lib states them (the tile is held to the header by tests/test_mstat_cpu.py).

Seconds on the MI355X: SLOWEST_S is the measured slowest test; the limit of a test is three times that, the
margin tests/test_gpu_search_forms.py takes for the machine's load.
"""
import ctypes

import numpy as np
import pytest

import findex_amd
import mstat_ref
import oracle
from findex_amd import _lib
from helpers import bwt_of_text, ends_at_a_fault, lf_walk_patterns, pack_patterns, synth_bwt

SLOWEST_S = 2
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(3 * SLOWEST_S)]

LAYOUTS = ["onehot", "bytes"]
T = _lib.FMX_MSTAT_TILE
GROUPS = _lib.MSTAT_GROUPS
MAXLEN = _lib.FMX_MSTAT_MAX_LEN
HIT = findex_amd.HipFMSearcher.MEM_HIT
HIP_ERR, OVERFLOW = 5, 9
TEXT_LEN = 6000


class World:
    pass


def open_index(index, layout):
    findex_amd.set_layout(layout)
    try:
        return findex_amd.HipFMSearcher.from_mem(*index)
    finally:
        findex_amd.set_layout("auto")


@pytest.fixture(scope="module")
def world():
    """The text (abcd, with planted repeats), a synthetic BWT that is no text's, their oracles and a handle of each per
    layout; the expectations of the cases, made at first use."""
    w = World()
    rng = np.random.default_rng(16)
    s = bytearray(rng.integers(97, 101, TEXT_LEN, dtype=np.uint8).tobytes())
    s[3000:3300] = s[500:800]                                # a 300-byte repeat
    s[5200:5260] = s[100:160]
    w.s = bytes(s)
    w.index = bwt_of_text(w.s)
    w.orc = oracle.NaiveFMSearcher.from_mem(*w.index)
    w.synth = synth_bwt(5000, 97, 100, seed=11, eof=4999)
    w.synth_orc = oracle.NaiveFMSearcher.from_mem(*w.synth)
    w.small = w.s[:700]
    w.small_index = bwt_of_text(w.small)
    w.small_orc = oracle.NaiveFMSearcher.from_mem(*w.small_index)
    w.small_orc.eof = int(w.small_index[1])
    w.small_hip = {layout: open_index(w.small_index, layout) for layout in LAYOUTS}
    w.hip = {layout: open_index(w.index, layout) for layout in LAYOUTS}
    w.synth_hip = {layout: open_index(w.synth, layout) for layout in LAYOUTS}
    w.expect = {}
    yield w
    for h in list(w.hip.values()) + list(w.synth_hip.values()) + list(w.small_hip.values()):
        h.close()
    w.orc.close()
    w.small_orc.close()
    w.synth_orc.close()


def expectation(w, name, pats, max_len, orc=None, by_text=False):
    """(buf, off, len, sp, ep, steps) of a case, from the oracle, once.  by_text: mstat_ref.text_stats instead of loop_stats
    (walks of thousands of steps from thousands of positions: one exact search per position on all cores)."""
    key = (name, max_len)
    if key not in w.expect:
        buf, off = pack_patterns(pats)
        if by_text:
            import bench
            w.expect[key] = (buf, off) + mstat_ref.text_stats(w.orc, w.s, buf, off, max_len or MAXLEN, threads=bench.effective_cores())
        else:
            w.expect[key] = (buf, off) + mstat_ref.loop_stats(orc or w.orc, buf, off, max_len or MAXLEN)
    return w.expect[key]


def check(w, hip, name, pats, max_len=None, orc=None, by_text=False):
    """One batch against its expectation: lengths and intervals exactly, the call's steps and the handle's counter the
    reference's step sum.  -> the expectation."""
    exp = expectation(w, name, pats, max_len, orc, by_text)
    buf, off, ln, sp, ep, steps = exp
    before = hip.stats()["backward_steps"]
    got_len, got_sp, got_ep = hip.match_stats_batch(buf, off, max_len)
    walk_ms, _, got_steps, requests = hip.mstat_last()
    print("%s max_len=%s: %d positions, %d steps (reference: %d), %d requests, %.3f ms"
          % (name, max_len, buf.size, got_steps, int(steps.sum()), requests, walk_ms))
    bad = np.nonzero(got_len != ln)[0]
    assert bad.size == 0, (name, max_len, bad[:8].tolist(), got_len[bad[:8]].tolist(), ln[bad[:8]].tolist())
    assert np.array_equal(got_sp, sp) and np.array_equal(got_ep, ep), (name, max_len)
    assert got_steps == int(steps.sum()), (name, got_steps, int(steps.sum()))
    assert hip.stats()["backward_steps"] - before == got_steps
    assert (got_steps == 0 and requests == 0) or 0 < requests <= 4 * got_steps
    only_len, none_sp, none_ep = hip.match_stats_batch(buf, off, max_len, intervals=False)
    assert none_sp is None and none_ep is None and np.array_equal(only_len, ln)
    return exp


def broken_copy(w, at, m, every, shift=0):
    """m bytes of the text from `at`, every `every`-th byte replaced by z (which the text does not hold)."""
    p = bytearray(w.s[at:at + m])
    for j in range(shift, m, every):
        p[j] = 122
    return bytes(p)


# ---------------------------------------------------------------- the walk kernel's shapes
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_tile_edges_and_the_halo(world, layout):
    """Patterns of T - 1, T, T + 1 and 2 T + 3 bytes back to back: matches that cross a tile edge, one match longer than a
    tile (its walks read the halo alone), pattern edges on both sides of a tile edge."""
    w = world
    pats = [broken_copy(w, 40, T - 1, 90), broken_copy(w, 700, T, 90, 45), broken_copy(w, 1300, T + 1, 60, 7),
            w.s[2000:2000 + T + 200] + b"z" + w.s[2100:2100 + T + 2 - 200], w.s[10:10 + T]]
    assert [len(p) for p in pats[:4]] == [T - 1, T, T + 1, 2 * T + 3]
    buf, off, ln, _, _, _ = check(w, w.hip[layout], "tiles", pats)
    assert ln.max() >= T + 200                               # longer than a tile
    edges = np.arange(T, buf.size, T)
    assert (ln[edges] > 1).sum() >= 4                        # matches that run across tile edges
    for cap in (T - 1, T, T + 1):
        check(w, w.hip[layout], "tiles", pats, cap)


@pytest.mark.parametrize("max_len", [1, 7, T, MAXLEN])
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_max_len_with_matches_of_one_less_exactly_and_one_more(world, layout, max_len):
    """z + a copy of max_len - 1, max_len and max_len + 1 bytes of the text each: the first stays below the cap, the
    second reaches it at its last byte, the third is saturated at its last two."""
    w = world
    starts = (150, 900, 1400)
    pats = [b"z".join([b"cc"] + [w.s[a:a + max_len + d] for a, d in zip(starts, (-1, 0, 1))] + [b"ab"])]
    buf, off, ln, _, _, _ = check(w, w.hip[layout], "cap", pats, max_len, by_text=max_len > T)
    ends = np.cumsum([3 + max_len - 1, 1 + max_len, 1 + max_len + 1]) - 1
    assert ln[ends].tolist() == [max_len - 1, max_len, max_len] and ln[ends[2] - 1] == max_len
    if max_len > 1:
        assert ln[ends[1] - 1] == max_len - 1 and ln.max() == max_len


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_refill_with_walks_of_uneven_length(world, layout):
    """One pattern in which 200-byte copies of the text alternate with random bytes, more than 8 * GROUPS * 4 positions: the
    groups of a wave finish at different rounds and draw new positions many times over."""
    w = world
    rng = np.random.default_rng(5)
    parts = []
    for j in range(14):
        parts += [w.s[300 * j + 17:300 * j + 217], bytes(rng.integers(97, 102, 37 + j, dtype=np.uint8))]
    pats = [b"".join(parts)]
    assert len(pats[0]) >= 8 * GROUPS[layout] * 4
    buf, off, ln, _, _, steps = check(w, w.hip[layout], "refill", pats)
    assert (ln >= 200).sum() >= 14 and (ln <= 8).sum() >= 300 and int(steps.max()) >= 200


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_many_patterns_per_tile(world, layout):
    """300 patterns of 0 to 5 bytes with empty ones between (and at both ends): the owner search."""
    w = world
    rng = np.random.default_rng(6)
    pats = [b"", b""]
    for j in range(300):
        m = int(rng.integers(0, 6))
        at = int(rng.integers(0, TEXT_LEN - 8))
        pats.append(w.s[at:at + m] if j % 4 else bytes(rng.integers(97, 101, m, dtype=np.uint8)))
    pats += [b"", w.s[7:12], b"", b""]
    buf, off, ln, _, _, _ = check(w, w.hip[layout], "many", pats)
    _, e, _ = mstat_ref.limits(off, buf.size, MAXLEN)
    assert (ln <= e).all() and (np.diff(off.astype(np.int64)) == 0).sum() >= 40
    check(w, w.hip[layout], "many", pats, 2)
    # no pattern at all, and only empty ones
    for none in ([], [b"", b""]):
        b0, o0 = pack_patterns(none)
        l0, s0, e0 = w.hip[layout].match_stats_batch(b0, o0)
        assert l0.size == s0.size == e0.size == 0 and w.hip[layout].mstat_last()[2] == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_a_walk_stops_at_its_patterns_first_byte(world, layout):
    """A, B with tail(A) + head(B) in the text: the first positions of B do not see A."""
    w = world
    pats = [w.s[100:140], w.s[140:180], w.s[180:181], w.s[181:200]]
    buf, off, ln, _, _, _ = check(w, w.hip[layout], "edge", pats)
    assert w.s[130:150] in w.s and ln[40:80].tolist() == list(range(1, 41)) and ln[80] == 1
    _, e, _ = mstat_ref.limits(off, buf.size, MAXLEN)
    assert (ln <= e).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_special_bytes_and_rows(world, layout):
    """An absent byte, byte 0 in a pattern, the whole text with one byte in front, and a walk through the EOF row with
    one-row intervals throughout (the text's first bytes, byte 0 in front of them, the text's last bytes in front of that)."""
    w = world
    pats = [b"zzz", b"az" + w.s[5:9], b"\0", w.s[-3:] + b"\0", b"a\0b", w.s[-6:] + b"\0" + w.s[:30]]
    buf, off, ln, sp, ep, _ = check(w, w.hip[layout], "special", pats)
    assert ln[:3].tolist() == [0, 0, 0] and (sp[:3] == 0).all() and (ep[:3] == w.orc.n).all()
    assert ln[-1] == 37 and ep[-1] - sp[-1] == 1             # the last byte of the EOF walk: all 37 bytes matched
    check(w, w.hip[layout], "special", pats, 7)
    # the whole of a small text, with one byte in front, with one behind, and as it is
    pats = [b"b" + w.small, w.small + b"b", w.small]
    buf, off, ln, sp, ep, _ = check(w, w.small_hip[layout], "whole", pats, orc=w.small_orc)
    m = len(w.small)
    assert ln[m] == m and ln[-1] == m and ln[int(off[2]) - 1] <= 20 and sp[-1] == w.small_orc.eof == w.small_hip[layout].eof


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_a_bwt_that_is_no_texts(world, layout):
    """helpers.synth_bwt, the EOF slot last: the definition rests on cf / occ alone."""
    w = world
    rng = np.random.default_rng(8)
    pats = lf_walk_patterns(w.synth_orc, rng, 60, 23, 0.5, alphabet=[97, 98, 99, 100, 122])
    pats = [b"".join(pats[:30])] + pats[30:]
    for cap in (None, 5):
        buf, off, ln, _, _, _ = check(w, w.synth_hip[layout], "synth", pats, cap, orc=w.synth_orc)
    assert ln.max() == 5 and check(w, w.synth_hip[layout], "synth", pats, None, orc=w.synth_orc)[2].max() >= 12


# ---------------------------------------------------------------- device and captured forms
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_and_its_capture(world, layout):
    """fmx_match_stats_batch_dev equals the host form; captured in a one-kernel graph on one stream and replayed twice it
    gives the same bytes, with no allocation in between."""
    import torch
    w = world
    hip = w.hip[layout]
    pats = [broken_copy(w, 40, T + 77, 90), w.s[3000:3300], b"", broken_copy(w, 1000, 2 * T, 33)]
    buf, off, ln, sp, ep, steps = expectation(w, "dev", pats, 64)
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    nb, k = buf.size, off.size - 1
    d_len = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_sp = torch.zeros(nb, dtype=torch.int64, device="cuda")
    d_ep = torch.zeros(nb, dtype=torch.int64, device="cuda")

    def same():
        return (np.array_equal(d_len.cpu().numpy().view(np.uint32), ln) and np.array_equal(d_sp.cpu().numpy().view(np.uint64), sp)
                and np.array_equal(d_ep.cpu().numpy().view(np.uint64), ep))

    st = torch.cuda.Stream()
    before = hip.stats()["backward_steps"]
    last = hip.mstat_last()
    with torch.cuda.stream(st):
        hip.match_stats_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, nb, d_len.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(),
                                  max_len=64, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert same()
    assert hip.stats()["backward_steps"] - before == int(steps.sum()) and hip.mstat_last() == last
    # lengths alone
    d_len.zero_()
    with torch.cuda.stream(st):
        hip.match_stats_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, nb, d_len.data_ptr(), max_len=64, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_len.cpu().numpy().view(np.uint32), ln)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        hip.match_stats_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, nb, d_len.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(),
                                  max_len=64, stream=st.cuda_stream)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        d_len.zero_(); d_sp.zero_(); d_ep.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same()
    assert torch.cuda.mem_get_info()[0] == free0
    del g


# ---------------------------------------------------------------- MEMs
def expected_mems(ln, sp, ep, off, min_len):
    out_off, rows = mstat_ref.mems_of(ln, off, min_len)
    hits = np.zeros(len(rows), dtype=HIT)
    for i, (q, l, end) in enumerate(rows):
        j = int(off[q]) + end - 1
        hits[i] = (q, l, end, sp[j], ep[j])
    return np.array(out_off, dtype=np.uint64), hits


def mem_patterns(w):
    return [broken_copy(w, 40, T + 77, 90), w.s[3000:3300], b"", w.s[100:140], w.s[140:180], b"zz", broken_copy(w, 1000, 2 * T, 33),
            w.s[5190:5270]]


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_mems_against_the_rule(world, layout):
    """The CSR equals mems_of for min_len 1, 12 and max_len; two runs give equal bytes."""
    w = world
    hip = w.hip[layout]
    pats = mem_patterns(w)
    for max_len in (64, None):
        buf, off, ln, sp, ep, steps = expectation(w, "mems", pats, max_len)
        for min_len in (1, 12, max_len or MAXLEN):
            exp_off, exp = expected_mems(ln, sp, ep, off, min_len)
            got_off, got = hip.mems_batch(buf, off, min_len, max_len)
            assert np.array_equal(got_off, exp_off), (max_len, min_len)
            assert got.tobytes() == exp.tobytes(), (max_len, min_len)
            assert hip.mstat_last()[2] == int(steps.sum())
            again_off, again = hip.mems_batch(buf, off, min_len, max_len)
            assert again_off.tobytes() == got_off.tobytes() and again.tobytes() == got.tobytes()
            print("%s max_len=%s min_len=%d: %d hits" % (layout, max_len, min_len, exp.size))
        if max_len == 64:
            assert (exp["len"] == 64).all() and exp.size >= 200      # saturated runs, position by position
    exp_off, exp = expected_mems(ln, sp, ep, off, 12)
    assert 10 <= exp.size <= 100 and exp["len"].max() == 300


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_mem_capacity_and_the_device_form(world, layout):
    """The counting call, cap == total, total - 1 and 0: the exact total on overflow, nothing behind the capacity; the
    device form's bytes; under a capture the MEM form is refused and the capture stays valid."""
    import torch
    w = world
    hip = w.hip[layout]
    L = _lib.load()
    buf, off, ln, sp, ep, _ = expectation(w, "mems", mem_patterns(w), None)
    exp_off, exp = expected_mems(ln, sp, ep, off, 3)
    total, k = exp.size, off.size - 1
    opts = _lib.fmx_mstat_opts(0, 3, (0, 0))
    n_out = ctypes.c_size_t()
    out_off = np.zeros(k + 1, dtype=np.uint64)

    def call(out, cap):
        rc = L.fmx_mems_batch(hip.handle, buf.ctypes.data, off.ctypes.data, k, ctypes.byref(opts), out_off.ctypes.data,
                              out.ctypes.data if out is not None else None, cap, ctypes.byref(n_out))
        if rc not in (0, OVERFLOW):
            _lib.check(rc)
        return rc

    assert call(None, 0) == OVERFLOW and n_out.value == total and str(total).encode() in L.fmx_last_error()
    guard = 64
    for cap in (total, total - 1, 0):
        out = np.full((max(cap, 1) + guard) * HIT.itemsize, 0xAB, dtype=np.uint8)
        rc = call(out, cap)
        assert n_out.value == total and rc == (0 if cap == total else OVERFLOW), (cap, rc, n_out.value)
        assert (out[cap * HIT.itemsize:] == 0xAB).all() if cap else True
        if cap == total:
            assert out[: total * HIT.itemsize].tobytes() == exp.tobytes() and np.array_equal(out_off, exp_off)
    # the device form on a side stream, guard bytes behind the output
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((total * HIT.itemsize + 256,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        n = hip.mems_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, buf.size, 3, d_out_off.data_ptr(), d_out.data_ptr(), total,
                               stream=st.cuda_stream)
    st.synchronize()
    raw = d_out.cpu().numpy()
    assert n == total and raw[: total * HIT.itemsize].tobytes() == exp.tobytes() and (raw[total * HIT.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), exp_off)
    # one record short: the first total - 1 records, nothing behind them
    d_out.fill_(0xCD)
    torch.cuda.synchronize()
    with pytest.raises(findex_amd.FmxError) as err:
        hip.mems_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, buf.size, 3, d_out_off.data_ptr(), d_out.data_ptr(), total - 1)
    assert err.value.code == OVERFLOW
    raw = d_out.cpu().numpy()
    assert raw[: (total - 1) * HIT.itemsize].tobytes() == exp[:-1].tobytes() and (raw[(total - 1) * HIT.itemsize:] == 0xCD).all()
    # under a capture: refused before anything is allocated, and the capture goes on
    d_len = torch.zeros(buf.size, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        with pytest.raises(findex_amd.FmxError) as err:
            hip.mems_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, buf.size, 3, d_out_off.data_ptr(), d_out.data_ptr(), total,
                               stream=st.cuda_stream)
        hip.match_stats_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, buf.size, d_len.data_ptr(), stream=st.cuda_stream)
    assert err.value.code == HIP_ERR and "capture" in str(err.value)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_len.cpu().numpy().view(np.uint32), ln)
    del g


@ends_at_a_fault
def test_block_handles_are_refused():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    pat, off = np.frombuffer(b"ab", dtype=np.uint8), np.array([0, 2], dtype=np.uint64)
    with pytest.raises(findex_amd.FmxError) as err:
        hip.match_stats_batch(pat, off)
    assert err.value.code == 6
    with pytest.raises(findex_amd.FmxError) as err:
        hip.mems_batch(pat, off, 1)
    assert err.value.code == 6
    hip.close()


# ---------------------------------------------------------------- text and corpus layers
def open_text(text, layout):
    findex_amd.set_layout(layout)
    try:
        return findex_amd.HipFMSearcher.from_text(text)
    finally:
        findex_amd.set_layout("auto")


def text_mems(text, q, ms, min_len):
    """Rows (q_off, len, text_off) from the statistics ms of q and str.find: position i begins a maximal match of ms[i]
    bytes unless the match of position i - 1 covers it."""
    rows = []
    for i in range(len(q)):
        l = int(ms[i])
        if l < min_len or (i and ms[i - 1] == l + 1):
            continue
        at = text.find(q[i:i + l])
        while at >= 0:
            rows.append((i, l, at))
            at = text.find(q[i:i + l], at + 1)
    return sorted(rows)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_text_terms(world, layout):
    """from_text + match_stats_text against `q[i:i + l] in text`, mems_text against a str.find enumeration."""
    w = world
    text = w.s[:2500] + w.s[500:800] + w.s[2500:3000]
    hip = open_text(text, layout)
    q = bytearray(text[400:900] + w.s[4000:4100] + text[2450:2600] + b"z" + text[550:700] + b"z")      # the last piece stands twice
    q[250] = 122
    q = bytes(q)
    for cap in (None, 40):
        ms = hip.match_stats_text(q, cap)
        for i in range(len(q)):
            l = int(ms[i])
            assert q[i:i + l] in text and l <= (cap or MAXLEN)
            assert l == (cap or MAXLEN) or i + l == len(q) or q[i:i + l + 1] not in text, (i, l)
    ms = hip.match_stats_text(q)
    assert ms.max() >= 249 and ms[250] == 0
    for min_len in (1, 20):
        got = hip.mems_text(q, min_len)
        want = text_mems(text, q, ms, min_len)
        assert [tuple(int(x) for x in r) for r in got] == want, min_len
    assert len(want) >= 4 and any(sum(1 for r in want if r[0] == i) >= 2 for i, _, _ in want)      # a match at two text offsets
    capped = hip.mems_text(q, 20, max_per=1)
    assert 0 < capped.shape[0] < len(want) and {tuple(int(x) for x in r) for r in capped} <= set(want)
    hip.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_shared_passages_of_a_corpus(world, layout):
    """Five small documents, one of which holds bytes 0, 1 and 255, and a query spliced from two of them: every reported
    (doc, raw_off, len) reads the query's bytes in the document, and the two spliced passages are there."""
    w = world
    rng = np.random.default_rng(9)
    docs = [bytes(rng.integers(65, 91, 400 + 30 * j, dtype=np.uint8)) for j in range(5)]
    d3 = bytearray(docs[3])
    d3[100], d3[120], d3[121], d3[200] = 0, 1, 255, 0
    docs[3] = bytes(d3)
    q = b"qq" + docs[1][50:130] + b"##" + docs[3][90:210] + b"q"
    findex_amd.set_layout(layout)
    try:
        cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    finally:
        findex_amd.set_layout("auto")
    rows = cs.shared_passages(q, 10)
    got = [tuple(int(x) for x in r) for r in rows]
    assert got == sorted(got, key=lambda r: (r[0], r[2], r[3])) and len(got) >= 2
    esc = findex_amd.escape
    for q_off, ln, doc, raw_off in got:
        assert ln >= 10 and doc < 5
        assert esc(docs[doc][raw_off:])[:ln] == esc(q[q_off:])[:ln] and len(esc(q[q_off:])) >= ln, (q_off, ln, doc, raw_off)
    assert (2, 80, 1, 50) in got and (84, 124, 3, 90) in got      # 120 raw bytes, four of them escaped
    assert cs.shared_passages(q, 200).shape == (0, 4)
    cs.close()
