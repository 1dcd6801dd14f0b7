"""Locate on the device: the sampled suffix array against Util.bwtFm2sa (util.scala:213-224) over the oracle's inverted list,
fmx_write_sa against SACreator's file layout, text offsets against a naive scan, the inversion against the suffix sort's own
SA across 2^31 rows and on 2^32 + 4100 rows, the refusal of a BWT with several LF cycles, and the prepare contract."""
import ctypes
import glob
import os
import time

import numpy as np
import pytest

import findex_amd
import oracle
from findex_amd import _lib
from helpers import synth_bwt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")


def golden_indexes():
    out = [(os.path.basename(p)[:-4], False) for p in sorted(glob.glob(os.path.join(TESTDATA, "*.cmp.bwt")))]
    return out + [("words", True)]


def bwt_fm2sa(fm, eof):
    """Util.bwtFm2sa: sa(i) = j along i = fm(i) from the eof row."""
    n = fm.size
    sa = np.zeros(n, dtype=np.int64)
    fml = fm.astype(np.int64).tolist()
    i = eof
    out = [0] * n
    for j in range(n):
        out[i] = j
        i = fml[i]
    sa[:] = out
    return sa


@pytest.fixture
def layout():
    yield findex_amd.set_layout
    findex_amd.set_layout("auto")


@pytest.mark.parametrize("name,be", golden_indexes())
def test_goldens_against_bwtfm2sa(name, be, layout, tmp_path):
    base = os.path.join(TESTDATA, name + ".bwt")
    orc = oracle.NaiveFMSearcher(base, bigEndian=be)
    sa = bwt_fm2sa(orc.fm(), orc.eof)
    assert sa[orc.eof] == 0 and sa[0] == orc.n - 1
    for lay in ("onehot", "bytes"):
        layout(lay)
        hip = findex_amd.HipFMSearcher(base, bigEndian=be)
        assert hip.stats()["layout"] == (0 if lay == "onehot" else 1)
        rows = np.arange(hip.n, dtype=np.uint64)
        for s in (1, 3, 32):
            hip.config_set("locate_sample", s)
            hip.drop_tables(jump=False, frontier=False, locate=True)
            hip.prepare(ktab=False, locate=True)
            rate, nbytes, _ = hip.locate_info()
            assert rate == s and nbytes > 0
            got = hip.locate(rows)
            assert np.array_equal(got.astype(np.int64), sa), (name, lay, s)
        path = tmp_path / (name + "." + lay + ".sa")
        hip.write_sa(path)
        assert path.read_bytes() == sa.astype(">u4").tobytes(), (name, lay)
        hip.close()


def _occurrences(text, q):
    out, i = [], text.find(q)
    while i >= 0:
        out.append(i)
        i = text.find(q, i + 1)
    return out


@pytest.fixture(scope="module")
def words():
    txt = open(os.path.join(TESTDATA, "words.txt"), "rb").read()
    hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
    assert hip.n == len(txt) + 1
    yield txt, hip
    hip.close()


def test_text_offsets_against_a_scan(words):
    txt, hip = words
    rng = np.random.default_rng(11)
    pats = []
    for _ in range(2000):
        m = int(rng.integers(2, 12))
        i = int(rng.integers(0, len(txt) - m))
        pats.append(txt[i:i + m])
    pats += [b"aardvark", b"zzzzq", b"qqqqqqqq", b"\x01\x02", b"the"]
    for q in pats:
        got = hip.locate_text(q)
        assert got.tolist() == _occurrences(txt, q), q
    got = hip.locate_text(b"the", max_hits=5)
    assert got.size == 5 and set(got.tolist()) <= set(_occurrences(txt, b"the"))


def test_locate_intervals_and_overflow(words):
    txt, hip = words
    rng = np.random.default_rng(12)
    pats = [txt[i:i + 3] for i in rng.integers(0, len(txt) - 3, 300).tolist()] + [b"zzzzq"]
    rev = [p[::-1] for p in pats]
    off = np.zeros(len(rev) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in rev])
    sp, ep = hip.search_batch(np.frombuffer(b"".join(rev), dtype=np.uint8).copy(), off)
    for max_per in (None, 1, 3):
        o, pos = hip.locate_intervals(sp, ep, max_per=max_per)
        for i in range(len(pats)):
            c = int(ep[i] - sp[i]) if ep[i] > sp[i] else 0
            if max_per is not None:
                c = min(c, max_per)
            assert int(o[i + 1] - o[i]) == c
            want = hip.locate(np.arange(int(sp[i]), int(sp[i]) + c, dtype=np.uint64))
            assert np.array_equal(pos[int(o[i]):int(o[i + 1])], want)
        if max_per is None:
            full = pos
            for i in range(len(pats)):
                q = pats[i]
                got = sorted(hip.text_offsets(pos[int(o[i]):int(o[i + 1])], hip.n, len(q)).tolist())
                assert got == _occurrences(txt, q)
    # cap overflow: FMX_ERR_OVERFLOW, every offset written, the first cap positions written and nothing past them
    L = _lib.load()
    total = int(full.size)
    cap = total - 5
    o2 = np.zeros(sp.size + 1, dtype=np.uint64)
    p2 = np.full(total, 7, dtype=np.uint64)
    rc = L.fmx_locate_intervals(hip.handle, sp.ctypes.data, ep.ctypes.data, sp.size, 0, o2.ctypes.data, p2.ctypes.data, cap)
    assert rc == 9 and b"room" in L.fmx_last_error()
    assert int(o2[-1]) == total and np.array_equal(p2[:cap], full[:cap]) and np.all(p2[cap:] == 7)
    # the device form, with the same cap
    import torch
    dsp, dep = torch.from_numpy(sp.view(np.int64)).cuda(), torch.from_numpy(ep.view(np.int64)).cuda()
    doff = torch.zeros(sp.size + 1, dtype=torch.int64, device="cuda")
    dpos = torch.full((total,), 7, dtype=torch.int64, device="cuda")
    hip.locate_intervals_dev(dsp.data_ptr(), dep.data_ptr(), sp.size, doff.data_ptr(), dpos.data_ptr(), cap)
    torch.cuda.synchronize()
    assert int(doff[-1].item()) == total
    assert np.array_equal(doff.cpu().numpy().view(np.uint64)[:-1], o2[:-1])
    p3 = dpos.cpu().numpy().view(np.uint64)
    assert np.array_equal(p3[:cap], full[:cap]) and np.all(p3[cap:] == 7)


def test_across_2_31_rows_against_the_suffix_sort():
    import torch
    length = (1 << 31) + 4099
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    text = torch.randint(97, 101, (length,), dtype=torch.uint8, device="cuda", generator=g)
    blk = text[1000:1000 + (1 << 22)].clone()                     # long repeats
    for at in (1 << 24, 1 << 28, (1 << 30) + 17, (1 << 31) - (1 << 22)):
        text[at:at + blk.numel()] = blk
    n = length + 1
    d_bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda")
    eof, counts = ctypes.c_uint64(), np.zeros(256, dtype=np.int64)
    L = _lib.load()
    _lib.check(L.fmx_bwt_from_text_dev(text.data_ptr(), length, d_bwt.data_ptr(), d_sa.data_ptr(), ctypes.byref(eof),
                                       counts.ctypes.data, 0, None))
    del text
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, eof.value, counts)
    del d_bwt
    hip.config_set("locate_sample", 32)
    hip.prepare(ktab=False, locate=True)
    chunk = 1 << 27
    out = torch.empty(chunk, dtype=torch.int64, device="cuda")
    for lo in range(0, n, chunk):
        k = min(chunk, n - lo)
        rows = torch.arange(lo, lo + k, dtype=torch.int64, device="cuda")
        hip.locate_dev(rows.data_ptr(), k, out.data_ptr())
        want = d_sa[lo:lo + k].to(torch.int64) & 0xFFFFFFFF
        assert torch.equal(out[:k], want), lo
    hip.close()


def test_above_2_32_rows():
    """text = 'a' x (2^32 + 4099): SA[r] = n - 1 - r.  The BWT is written directly: 'a' x n, eof = n - 1."""
    import torch
    n = (1 << 32) + 4100
    d_bwt = torch.full((n,), 97, dtype=torch.uint8, device="cuda")
    counts = np.zeros(256, dtype=np.int64)
    counts[97] = n - 1
    hip = findex_amd.HipFMSearcher.from_device(d_bwt.data_ptr(), n, n - 1, counts)
    del d_bwt
    hip.config_set("locate_sample", 32)
    hip.prepare(ktab=False, locate=True)
    rate, nbytes, _ = hip.locate_info()
    m = (n - 1) // 32 + 1
    assert rate == 32 and nbytes == (n // 448 + 1) * 64 + m * 8          # u64 samples above 2^32 rows
    rng = np.random.default_rng(13)
    rows = np.concatenate([rng.integers(0, n, 1 << 20, dtype=np.uint64),
                           np.array([0, 1, 2, n - 3, n - 2, n - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1], dtype=np.uint64)])
    got = hip.locate(rows)
    assert np.array_equal(got, np.uint64(n - 1) - rows)
    hip.close()


def _lf_cycles(bwt, eof, counts):
    n = bwt.size
    c = np.array(bwt, dtype=np.int64)
    c[eof] = 0
    order = np.argsort(c, kind="stable")                 # LF is the stable sort of the rows by their BWT byte
    lf = np.empty(n, dtype=np.int64)
    lf[order] = np.arange(n)
    assert lf[eof] == 0
    seen = np.zeros(n, dtype=bool)
    cycles = 0
    for r in range(n):
        if seen[r]:
            continue
        cycles += 1
        while not seen[r]:
            seen[r] = True
            r = lf[r]
    return cycles


def test_bwt_of_several_cycles_is_refused():
    bwt, eof, counts = synth_bwt(20000, 1, 4, seed=21)
    assert _lf_cycles(bwt, eof, counts) > 1
    hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
    orc = oracle.NaiveFMSearcher(_mem=(bwt, bwt.size, eof, counts))
    rng = np.random.default_rng(1)
    pats = rng.integers(1, 5, 4000, dtype=np.uint8)
    off = np.arange(0, 4001, 4, dtype=np.uint64)
    t0 = time.time()
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.prepare(ktab=False, locate=True)
    assert ei.value.code == 2 and "not the BWT of one text" in str(ei.value)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.locate(np.array([0, 1], dtype=np.uint64))
    assert ei.value.code == 2
    assert time.time() - t0 < 60
    assert hip.locate_info()[1] == 0
    sp, ep = hip.search_batch(pats, off)
    wsp, wep, _ = orc.search_batch(pats, off)
    hit = wsp < wep
    assert hit.sum() > 900
    assert np.array_equal(sp[hit], wsp[hit]) and np.array_equal(ep[hit], wep[hit]) and np.all(sp[~hit] >= ep[~hit])
    hip.close()


def test_contract(words, tmp_path):
    import torch
    txt, _ = words
    L = _lib.load()
    hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
    rng = np.random.default_rng(14)
    pats = [txt[i:i + 4][::-1] for i in rng.integers(0, len(txt) - 4, 2000).tolist()]
    pbuf = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    off = np.arange(0, 4 * len(pats) + 1, 4, dtype=np.uint64)
    hip.prepare(ktab=True, jump=True)
    sp0, ep0 = hip.search_batch(pbuf, off)
    held0 = hip.stats()["tables_held_bytes"]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                 # (free HBM below is the driver's: no blocks left in torch's cache)
    free0 = torch.cuda.mem_get_info()[0]
    hip.prepare(ktab=False, locate=True)
    assert hip.stats()["tables_held_bytes"] == held0
    sp1, ep1 = hip.search_batch(pbuf, off)
    assert np.array_equal(sp0, sp1) and np.array_equal(ep0, ep1)
    _, nbytes, ms = hip.locate_info()
    assert nbytes > 0 and ms > 0
    # graph capture of the device form on one stream
    k = 1 << 16
    rows = torch.from_numpy(rng.integers(0, hip.n, k, dtype=np.uint64).view(np.int64)).cuda()
    rows[5] = hip.n + 3                                              # out of range: UINT64_MAX
    out = torch.zeros(k, dtype=torch.int64, device="cuda")
    want = hip.locate(np.delete(rows.cpu().numpy().view(np.uint64), 5))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hip.locate_dev(rows.data_ptr(), k, out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        hip.locate_dev(rows.data_ptr(), k, out.data_ptr(), stream=s.cuda_stream)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        assert got[5] == np.uint64(0xFFFFFFFFFFFFFFFF)
        assert np.array_equal(np.delete(got, 5), want)
    del g
    # free HBM does not move across locate calls
    hrows = rows.cpu().numpy().view(np.uint64).copy()
    hrows[5] = 0
    hip.locate(hrows)
    torch.cuda.synchronize()
    f1 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        hip.locate(hrows)
        hip.locate_dev(rows.data_ptr(), k, out.data_ptr())
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == f1
    # drop and write_sa give their memory back
    hip.drop_tables(jump=False, frontier=False, locate=True)
    assert hip.locate_info()[1] == 0
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    f2 = torch.cuda.mem_get_info()[0]
    assert abs(f2 - free0) <= 64 << 20
    hip.write_sa(tmp_path / "w.sa")
    assert (tmp_path / "w.sa").stat().st_size == 4 * hip.n
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert abs(torch.cuda.mem_get_info()[0] - f2) <= 64 << 20
    # argument errors
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.locate(np.array([hip.n], dtype=np.uint64))
    assert ei.value.code == 3
    assert L.fmx_write_sa(hip.handle, b"/nonexistent/dir/x.sa") == 1
    assert L.fmx_index_config_set(hip.handle, b"locate_sample", b"0") == 3
    hip.close()


def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    L = _lib.load()
    out = (ctypes.c_uint64 * 1)()
    rows = (ctypes.c_uint64 * 1)(0)
    assert L.fmx_locate_batch(hip.handle, rows, 1, out) == 6
    assert L.fmx_prepare(hip.handle, 32) == 6
    assert L.fmx_write_sa(hip.handle, b"/tmp/never.sa") == 6
    hip.close()
