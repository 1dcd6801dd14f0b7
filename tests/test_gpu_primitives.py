"""The primitive kernels -- k_occ, k_prev_range, k_lf_walk (fmx_kernels.hip), k_psi, k_next_substr, k_sel_build
(fmx_select.hip) -- against the plain reference of tests/primitives_ref.py (pinned on the CPU by
tests/test_primitives_ref_cpu.py), at the shapes the rest of the suite does not reach:
  (a) batches of one, one less, exactly and more than a grid trip, and partial last trips;
  (b) indexes designed against the select directory (clusters, density 1, every sampling rate, single occurrences at
      block edges, absent symbols between present ones, superblock checkpoints);
  (c) the five device-pointer entry points: equal to the host forms, clamped operands, a captured graph;
  (d) the select directory is not built under a stream capture.
Every comparison is exact equality over the whole batch, in both layouts."""
import ctypes
import functools

import numpy as np
import pytest

import findex_amd
from findex_amd import _lib
from helpers import (ONEHOT_BLOCK, clustered_bwt, geometric_bwt, one_symbol_bwt, sparse_alphabet_bwt, synth_bwt)
from primitives_ref import PlainIndex

pytestmark = pytest.mark.gpu

# the launch geometry of the primitive kernels (grid_for / sel_grid): workgroups of 256 threads, at most 8 per CU, a
# lane group of 4 (one-hot) or 8 (bytes) lanes per query; k_occ and k_prev_range give a group 4 queries per trip
THREADS = 256
GROUP = {"onehot": 4, "bytes": 8}
BLOCKS_PER_CU = 8
QUERIES_PER_GROUP = 4
LAYOUT_ID = {"onehot": 0, "bytes": 1}


@pytest.fixture(params=["onehot", "bytes"])
def layout(request):
    findex_amd.set_layout(request.param)
    try:
        yield request.param
    finally:
        findex_amd.set_layout("auto")
        findex_amd.set_checkpoints("auto")


def trips(layout):
    """(T_occ, T_row): the queries one grid trip of k_occ / k_prev_range covers, and the rows one trip of k_psi /
    k_next_substr covers (k_lf_walk: two trips of T_row are stepped together)."""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    groups = cu * BLOCKS_PER_CU * THREADS // GROUP[layout]
    return QUERIES_PER_GROUP * groups, groups


def open_index(index, layout):
    hip = findex_amd.HipFMSearcher.from_mem(*index)
    assert hip.stats()["layout"] == LAYOUT_ID[layout]
    return hip


def counted(hip):
    st = hip.stats()
    return st["rank_queries"], st["backward_steps"]


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def next_substr_walk_order(hip, rows, length):
    """fmx_next_substr_batch as arrays, turned back into walk order: (bytes [k, length] with 0 behind each walk's
    length, lengths).  The host form reverses each walk, so this is its output reversed again."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    out = np.zeros((rows.size, max(length, 1)), dtype=np.uint8)
    w = np.zeros(rows.size, dtype=np.uint32)
    _lib.check(_lib.load().fmx_next_substr_batch(hip.handle, _vp(rows), rows.size, length, _vp(out), _vp(w)))
    out = out.reshape(-1)[: rows.size * length].reshape(rows.size, length)
    j = w[:, None].astype(np.int64) - 1 - np.arange(length, dtype=np.int64)[None, :]
    return np.where(j >= 0, np.take_along_axis(out, np.maximum(j, 0), axis=1), 0).astype(np.uint8), w


def masked(out, ln):
    return np.where(np.arange(out.shape[1])[None, :] < ln[:, None].astype(np.int64), out, 0).astype(np.uint8)


# ---------------------------------------------------------------- (a) batch shapes
SMALL = synth_bwt(5003, 1, 6, seed=77)          # symbols 1 .. 6: 7 .. 255 are absent


@functools.lru_cache(maxsize=None)
def small_ref():
    return PlainIndex(SMALL[0], SMALL[1])


def rows_with_edges(rng, ref, k):
    """k rows drawn from the whole index; row 0, the EOF row and row n - 1 are among them (as many as k allows), and the
    batch ends on row n - 1 so that a last trip of one row holds an edge too."""
    rows = rng.integers(0, ref.n, size=k).astype(np.uint64)
    edge = np.array([0, ref.eof, ref.n - 1], dtype=np.uint64)[:k]
    free = k - 1 if k > 3 else k
    rows[rng.permutation(free)[: edge.size]] = edge
    if k > 3:
        rows[k - 1] = ref.n - 1
    return rows


def test_occ_batch_shapes(layout):
    ref = small_ref()
    n = ref.n
    hip = open_index(SMALL, layout)
    t_occ, _ = trips(layout)
    rng = np.random.default_rng(1)
    syms = np.array([0, 1, 2, 3, 4, 5, 6, 7, 200, 255], dtype=np.uint8)
    for k in (1, 2, 3, 5, 7, t_occ - 1, t_occ, t_occ + 1, 2 * t_occ + 3):
        c = rng.choice(syms, size=k)
        i = rng.integers(-1, n + 3, size=k, dtype=np.int64)
        edge = np.array([-1, 0, ref.eof, n - 1, n, n + 2], dtype=np.int64)[:k]
        i[k - edge.size:] = edge                            # the last trip holds the edges
        hip.stats_reset()
        got = hip.occ_batch(c, i)
        assert np.array_equal(got.astype(np.int64), ref.occ(c, i)), (layout, k)
        assert counted(hip) == (k, 0), (layout, k)
    hip.close()


def test_prev_range_batch_shapes(layout):
    ref = small_ref()
    n = ref.n
    hip = open_index(SMALL, layout)
    t_occ, _ = trips(layout)
    rng = np.random.default_rng(2)
    syms = np.array([0, 1, 2, 3, 4, 5, 6, 7, 200, 255], dtype=np.uint8)
    for k in (1, 2, 3, 5, 7, t_occ - 1, t_occ, t_occ + 1, 2 * t_occ + 3):
        a = rng.integers(0, n + 1, size=k)
        b = rng.integers(0, n + 1, size=k)
        sp, ep = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
        same = rng.random(k) < 0.1
        ep[same] = sp[same]                                 # sp == ep
        full = rng.random(k) < 0.1
        ep[full] = n                                        # ep == n
        esp = np.array([0, ref.eof, n - 1, n, 0], dtype=np.uint64)[:k]
        eep = np.array([0, ref.eof + 1, n, n, n], dtype=np.uint64)[:k]
        sp[k - esp.size:], ep[k - esp.size:] = esp, eep
        c = rng.choice(syms, size=k)
        hip.stats_reset()
        g1, g2 = hip.prev_range_batch(sp, ep, c)
        w1, w2 = ref.prev_range(sp, ep, c)
        assert np.array_equal(g1.astype(np.int64), w1) and np.array_equal(g2.astype(np.int64), w2), (layout, k)
        assert counted(hip) == (2 * k, k), (layout, k)
    hip.close()


def test_psi_and_next_substr_batch_shapes(layout):
    ref = small_ref()
    hip = open_index(SMALL, layout)
    _, t_row = trips(layout)
    rng = np.random.default_rng(3)
    for k in (1, 3, t_row - 1, t_row, t_row + 1, 2 * t_row + 3):
        rows = rows_with_edges(rng, ref, k)
        assert np.array_equal(hip.psi_batch(rows).astype(np.int64), ref.psi[rows.astype(np.int64)]), (layout, k)
        assert hip.nextSubstr_batch(rows, 5) == ref.next_substr_host(rows, 5), (layout, k)
    hip.close()


def test_lf_walk_batch_shapes(layout):
    ref = small_ref()
    hip = open_index(SMALL, layout)
    _, t_row = trips(layout)
    rng = np.random.default_rng(4)
    # a group steps walks q and q + T_row together: two walks, one walk, and two in one round then one in the next
    for k in (1, 2, t_row, t_row + 1, 2 * t_row - 1, 2 * t_row, 2 * t_row + 1, 3 * t_row + 5):
        rows = rows_with_edges(rng, ref, k)
        for length in (0, 1, 6):
            wb, we = ref.prev_substr(rows, length)
            for want_bytes in (True, False):
                hip.stats_reset()
                gb, ge = hip.lf_walk_batch(rows, length, want_bytes=want_bytes)
                assert np.array_equal(ge.astype(np.int64), we), (layout, k, length, want_bytes)
                assert gb is None if not want_bytes else np.array_equal(gb, wb), (layout, k, length)
                assert counted(hip) == (k * length, 0), (layout, k, length)
    # bytes only: end_rows == NULL
    k = 2 * t_row + 1
    rows = rows_with_edges(rng, ref, k)
    out = np.zeros((k, 6), dtype=np.uint8)
    _lib.check(_lib.load().fmx_lf_walk_batch(hip.handle, _vp(rows), k, 6, _vp(out), None))
    assert np.array_equal(out, ref.prev_substr(rows, 6)[0])
    hip.close()


# ---------------------------------------------------------------- (b) designed indexes
CLASSES = ((0, 255), (97, 122), (255, 255), (5, 4))


def absent_class(absent):
    """The first run of absent symbols as a class (c0, c1): every step of it is empty."""
    a0 = a1 = int(absent[0])
    while a1 + 1 in absent:
        a1 += 1
    return a0, a1


def check_every_row(hip, ref, tag, seed=0):
    """Psi, nextSubstr, LF and occ for every row of the index, class steps and extract at the edges."""
    n = ref.n
    rows = np.arange(n, dtype=np.uint64)
    assert np.array_equal(hip.psi_batch(rows).astype(np.int64), ref.psi), tag
    gb, ge = hip.lf_walk_batch(rows, 1)
    assert np.array_equal(gb[:, 0], ref.B) and np.array_equal(ge.astype(np.int64), ref.lf), tag
    got, gl = next_substr_walk_order(hip, rows, 5)
    want, wl = ref.next_substr(rows, 5)
    assert np.array_equal(gl, wl) and np.array_equal(got, want), tag
    # occ at every row: of the row's own symbol (the rank LF takes) and of a symbol drawn from the whole alphabet
    rng = np.random.default_rng(seed)
    present = np.nonzero(np.bincount(ref.B, minlength=256))[0]
    absent = np.setdiff1d(np.arange(256), present)
    pool = np.concatenate([present, present, [0, 255], absent[:2], absent[-2:]]).astype(np.uint8)
    keys = np.arange(-1, n + 1, dtype=np.int64)
    for c in (ref.B[np.clip(keys, 0, n - 1)], rng.choice(pool, size=keys.size)):
        assert np.array_equal(hip.occ_batch(c, keys).astype(np.int64), ref.occ(c, keys)), tag
    for sp, ep in ((0, n), (n // 4, 3 * n // 4), (ref.eof, min(ref.eof + 1, n)), (n - 1, n), (n // 2, n // 2)):
        for c0, c1 in CLASSES + (absent_class(absent),):
            assert hip.getIntervalPrevRange(sp, ep, c0, c1) == ref.interval_prev_range(sp, ep, c0, c1), (tag, sp, ep, c0, c1)
    for r in (0, ref.eof, n - 1):
        for length in (1, 9):
            assert hip.extract(r, length, 1) == ref.next_substr_host([r], length)[0], (tag, r, length)
            assert hip.extract(r, length, -1) == bytes(ref.prev_substr([r], length)[0][0]), (tag, r, length)


@pytest.mark.parametrize("eof", [0, 200_000 // 3, 199_999])
def test_clustered(eof, layout):
    index = clustered_bwt(eof)
    ref = PlainIndex(index[0], index[1])
    # the case is hard by construction: even at the largest sampling rate (S = 256) and the largest block, some sample
    # of symbol 1 spans more than 16 blocks, so the narrowing loop runs several rounds
    p = ref.positions(1)
    S = 256
    assert int((p[S - 1:] - p[: p.size - (S - 1)]).max()) > 16 * ONEHOT_BLOCK
    hip = open_index(index, layout)
    check_every_row(hip, ref, ("clustered", eof, layout))
    hip.close()


def test_one_symbol(layout):
    for n in ((447, 448, 449, 896, 897, 40_000) if layout == "onehot" else (127, 128, 129, 40_000)):
        for eof in sorted({0, n // 3, n - 1}):
            index = one_symbol_bwt(n, eof)
            hip = open_index(index, layout)
            check_every_row(hip, PlainIndex(index[0], index[1]), ("one_symbol", n, eof, layout))
            hip.close()


def test_geometric(layout):
    index = geometric_bwt()
    hip = open_index(index, layout)
    check_every_row(hip, PlainIndex(index[0], index[1]), ("geometric", layout))
    hip.close()


def test_sparse_alphabet(layout):
    index = sparse_alphabet_bwt()
    hip = open_index(index, layout)
    check_every_row(hip, PlainIndex(index[0], index[1]), ("sparse_alphabet", layout))
    hip.close()


SUPER_N = 2 * (1 << 22) + 77                    # two whole superblocks of the bytes layout and a bit


@functools.lru_cache(maxsize=None)
def super_index():
    index = synth_bwt(SUPER_N, 1, 128, seed=99)
    return index, PlainIndex(index[0], index[1])


@pytest.mark.parametrize("lay,checkpoints", [("onehot", "auto"), ("bytes", "auto"), ("bytes", "superblock")])
def test_superblocks(lay, checkpoints):
    index, ref = super_index()
    n = ref.n
    findex_amd.set_layout(lay)
    findex_amd.set_checkpoints(checkpoints)
    try:
        hip = open_index(index, lay)
        rows = np.arange(n, dtype=np.uint64)
        assert np.array_equal(hip.psi_batch(rows).astype(np.int64), ref.psi)
        _, ge = hip.lf_walk_batch(rows, 1, want_bytes=False)
        assert np.array_equal(ge.astype(np.int64), ref.lf)
        rng = np.random.default_rng(8)
        edge = np.array([-1, 0, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, n - 1, n], dtype=np.int64)
        keys = np.concatenate([rng.integers(-1, n + 1, size=100_000, dtype=np.int64), np.repeat(edge, 8)])
        c = rng.integers(0, 130, size=keys.size).astype(np.uint8)
        assert np.array_equal(hip.occ_batch(c, keys).astype(np.int64), ref.occ(c, keys))
        srows = rng.integers(0, n, size=10_000).astype(np.uint64)
        srows[:3] = [0, ref.eof, n - 1]
        got, gl = next_substr_walk_order(hip, srows, 9)
        want, wl = ref.next_substr(srows, 9)
        assert np.array_equal(gl, wl) and np.array_equal(got, want)
        hip.close()
    finally:
        findex_amd.set_layout("auto")
        findex_amd.set_checkpoints("auto")


# ---------------------------------------------------------------- (c) device forms
U64 = (1 << 64) - 1


def dev(torch, a):
    """A host array on the device (torch has no uint64: the bits travel as int64)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class DeviceCalls:
    """The five device-pointer calls over one set of operands, outputs in torch tensors."""

    def __init__(self, torch, hip, c, i, sp, ep, rows, length):
        self.hip, self.k, self.length = hip, rows.size, length
        k = rows.size
        self.c, self.i, self.sp, self.ep, self.rows = dev(torch, c), dev(torch, i), dev(torch, sp), dev(torch, ep), dev(torch, rows)
        z64 = lambda: torch.zeros(k, dtype=torch.int64, device="cuda")
        self.occ, self.sp1, self.ep1, self.end, self.psi = z64(), z64(), z64(), z64(), z64()
        self.lf_bytes = torch.zeros(k * length, dtype=torch.uint8, device="cuda")
        self.ns_bytes = torch.zeros(k * length, dtype=torch.uint8, device="cuda")
        self.ns_len = torch.zeros(k, dtype=torch.int32, device="cuda")

    def outputs(self):
        return (self.occ, self.sp1, self.ep1, self.end, self.psi, self.lf_bytes, self.ns_bytes, self.ns_len)

    def enqueue(self, stream):
        p = lambda t: t.data_ptr()
        hip, k = self.hip, self.k
        hip.occ_batch_dev(p(self.c), p(self.i), p(self.occ), k, stream=stream)
        hip.prev_range_batch_dev(p(self.sp), p(self.ep), p(self.c), p(self.sp1), p(self.ep1), k, stream=stream)
        hip.lf_walk_batch_dev(p(self.rows), k, self.length, p(self.lf_bytes), p(self.end), stream=stream)
        hip.psi_batch_dev(p(self.rows), p(self.psi), k, stream=stream)
        hip.next_substr_batch_dev(p(self.rows), k, self.length, p(self.ns_bytes), p(self.ns_len), stream=stream)

    def results(self):
        ln = host(self.ns_len, np.uint32)
        return {"occ": host(self.occ, np.uint64), "sp1": host(self.sp1, np.uint64), "ep1": host(self.ep1, np.uint64),
                "lf_bytes": host(self.lf_bytes, np.uint8).reshape(self.k, self.length), "end": host(self.end, np.uint64),
                "psi": host(self.psi, np.uint64), "ns_len": ln,
                "ns_bytes": masked(host(self.ns_bytes, np.uint8).reshape(self.k, self.length), ln)}


def same_results(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a)


def test_device_forms(layout):
    import torch
    index = clustered_bwt(200_000 // 3)
    ref = PlainIndex(index[0], index[1])
    n = ref.n
    hip = open_index(index, layout)
    hip.prepare(ktab=False, select=True)
    rng = np.random.default_rng(12)
    k, length = 70_001, 6
    syms = np.array([0, 1, 2, 7, 200, 3, 255], dtype=np.uint8)
    c = rng.choice(syms, size=k)
    i = rng.integers(-1, n, size=k, dtype=np.int64)
    a, b = rng.integers(0, n + 1, size=k), rng.integers(0, n + 1, size=k)
    sp, ep = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
    rows = rows_with_edges(rng, ref, k)
    s = torch.cuda.Stream()
    calls = DeviceCalls(torch, hip, c, i, sp, ep, rows, length)
    torch.cuda.synchronize()
    calls.enqueue(s.cuda_stream)
    s.synchronize()
    eager = calls.results()
    # each device call against its host form ...
    h1, h2 = hip.prev_range_batch(sp, ep, c)
    hb, he = hip.lf_walk_batch(rows, length)
    hw, hl = next_substr_walk_order(hip, rows, length)          # (the host form is the reverse of the device form)
    host_forms = {"occ": hip.occ_batch(c, i), "sp1": h1, "ep1": h2, "lf_bytes": hb, "end": he, "psi": hip.psi_batch(rows),
                  "ns_len": hl, "ns_bytes": hw}
    for key in eager:
        assert np.array_equal(eager[key], host_forms[key]), (layout, key)
    # ... and the device nextSubstr against the reference's walk-order bytes and lengths
    wb, wl = ref.next_substr(rows, length)
    assert np.array_equal(eager["ns_len"], wl) and np.array_equal(eager["ns_bytes"], wb)
    assert hip.nextSubstr_batch(rows[:2000], length) == [bytes(wb[q, :wl[q]][::-1]) for q in range(2000)]
    assert np.array_equal(eager["psi"].astype(np.int64), ref.psi[rows.astype(np.int64)])
    assert np.array_equal(eager["end"].astype(np.int64), ref.prev_substr(rows, length)[1])

    # operands no host form accepts: the kernels clamp them before they form an address
    big = np.array([n, n + 1, 1 << 63, U64, n - 1, 0, n + 1, U64], dtype=np.uint64)
    ci = np.array([n, n + 9, 1 << 62, n - 1, -1, -(1 << 62), 1 << 62, n + 9], dtype=np.int64)
    cc = np.array([1, 2, 200, 7, 1, 2, 0, 255], dtype=np.uint8)
    csp = np.array([n, n + 1, 1 << 63, U64, 0, 5, n + 1, U64], dtype=np.uint64)
    cep = np.array([n + 1, U64, 1 << 63, U64, n + 1, 1 << 63, n, n + 1], dtype=np.uint64)
    clamp = DeviceCalls(torch, hip, cc, ci, csp, cep, big, length)
    torch.cuda.synchronize()
    clamp.enqueue(s.cuda_stream)
    s.synchronize()
    got = clamp.results()
    crow = np.minimum(big, np.uint64(n - 1)).astype(np.int64)
    assert np.array_equal(got["occ"].astype(np.int64), ref.occ(cc, np.minimum(ci, n - 1)))
    w1, w2 = ref.prev_range(np.minimum(csp, np.uint64(n)), np.minimum(cep, np.uint64(n)), cc)
    assert np.array_equal(got["sp1"].astype(np.int64), w1) and np.array_equal(got["ep1"].astype(np.int64), w2)
    wb, we = ref.prev_substr(crow, length)
    assert np.array_equal(got["lf_bytes"], wb) and np.array_equal(got["end"].astype(np.int64), we)
    assert np.array_equal(got["psi"].astype(np.int64), ref.psi[crow])
    wb, wl = ref.next_substr(crow, length)
    assert np.array_equal(got["ns_len"], wl) and np.array_equal(got["ns_bytes"], wb)

    # the five calls as one linear chain in a captured graph: nothing is built, allocated or copied
    held0 = hip.stats()["tables_held_bytes"]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()        # torch.cuda.graph empties torch's cache itself: what earlier tests left there is not this capture's
    free0 = torch.cuda.mem_get_info(0)[0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        calls.enqueue(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.stats()["tables_held_bytes"] == held0
    assert abs(torch.cuda.mem_get_info(0)[0] - free0) <= 64 << 20
    for _ in range(3):
        for t in calls.outputs():
            t.zero_()
        torch.cuda.synchronize()
        assert not same_results(calls.results(), eager)
        g.replay()
        torch.cuda.synchronize()
        assert same_results(calls.results(), eager), layout
    del g
    hip.close()


# ---------------------------------------------------------------- (d) the select directory and a stream capture
def test_select_directory_is_not_built_under_capture(layout):
    import torch
    index = clustered_bwt(200_000 // 3)
    ref = PlainIndex(index[0], index[1])
    hip = open_index(index, layout)                     # no prepare(select=True): the directory does not exist
    k = 4096
    rng = np.random.default_rng(13)
    hrows = rows_with_edges(rng, ref, k)
    rows = dev(torch, hrows)
    out = torch.zeros(k, dtype=torch.int64, device="cuda")
    obytes = torch.zeros(k * 4, dtype=torch.uint8, device="cuda")
    olen = torch.zeros(k, dtype=torch.int32, device="cuda")
    held0 = hip.stats()["tables_held_bytes"]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    errs = []
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        for call in (lambda: hip.psi_batch_dev(rows.data_ptr(), out.data_ptr(), k, stream=s.cuda_stream),
                     lambda: hip.next_substr_batch_dev(rows.data_ptr(), k, 4, obytes.data_ptr(), olen.data_ptr(), stream=s.cuda_stream)):
            try:
                call()
                errs.append(None)
            except findex_amd.FmxError as e:
                errs.append(e)
        out.zero_()                                     # (the graph is not empty; it is never replayed)
        g.capture_end()
    for e in errs:
        assert e is not None and e.code == 5 and "stream capture" in str(e)
    del g
    torch.cuda.synchronize()
    assert hip.stats()["tables_held_bytes"] == held0
    # outside a capture the first call builds the directory and answers
    assert np.array_equal(hip.psi_batch(hrows).astype(np.int64), ref.psi[hrows.astype(np.int64)])
    assert hip.stats()["tables_held_bytes"] > held0
    with torch.cuda.stream(s):
        hip.psi_batch_dev(rows.data_ptr(), out.data_ptr(), k, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(host(out, np.uint64).astype(np.int64), ref.psi[hrows.astype(np.int64)])
    hip.close()
