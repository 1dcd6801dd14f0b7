"""The LCP array on the device (fmx_lcp_*) against a linear Kasai over (s, SA) written from the definition
(tests/lcp_checker.py): every row of every input.  SA comes from the oracle's inverted list (Util.bwtFm2sa) for the
fixture indexes and from an independent numpy suffix sort for the adversarial texts; at sizes Python cannot walk, every
row is verified on the device itself (the two suffixes agree on LCP bytes and differ at the next)."""
import ctypes
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import findex_amd
import oracle
from findex_amd import _lib
from helpers import synth_bwt
import lcp_checker
from test_gpu_build_text import _adversarial, np_suffix_array

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")


def golden_indexes():
    out = [(os.path.basename(p)[:-4], False) for p in sorted(glob.glob(os.path.join(TESTDATA, "*.cmp.bwt")))]
    return out + [("words", True)]


def bwt_fm2sa(fm, eof):
    """Util.bwtFm2sa: sa(i) = j along i = fm(i) from the eof row."""
    fml = fm.astype(np.int64).tolist()
    out = [0] * len(fml)
    i = eof
    for j in range(len(fml)):
        out[i] = j
        i = fml[i]
    return np.array(out, dtype=np.int64)


_golden_cache = {}


def golden_truth(name, be):
    """(sa, lcp) of a fixture index: SA from the oracle's fm() walk, s from the BWT (bwt[r] = s[SA[r] - 1]), Kasai."""
    if name not in _golden_cache:
        base = os.path.join(TESTDATA, name + ".bwt")
        orc = oracle.NaiveFMSearcher(base, bigEndian=be)
        sa = bwt_fm2sa(orc.fm(), orc.eof)
        bwt, size, eof = oracle.load_bwt_file(base, bigEndian=be)
        assert size == sa.size and eof == orc.eof and sa[eof] == 0 and sa[0] == size - 1
        s = np.zeros(size, dtype=np.uint8)
        keep = np.arange(size) != eof
        s[sa[keep] - 1] = np.asarray(bwt)[keep]
        assert s[size - 1] == 0 and np.count_nonzero(s) == size - 1
        _golden_cache[name] = (sa, lcp_checker.kasai(s.tobytes(), sa))
    return _golden_cache[name]


@pytest.fixture
def layout():
    yield findex_amd.set_layout
    findex_amd.set_layout("auto")


@pytest.mark.parametrize("name,be", golden_indexes())
def test_goldens_against_kasai(name, be, layout, tmp_path):
    sa, want = golden_truth(name, be)
    n = sa.size
    base = os.path.join(TESTDATA, name + ".bwt")
    rng = np.random.default_rng(41)
    for lay in ("onehot", "bytes"):
        layout(lay)
        hip = findex_amd.HipFMSearcher(base, bigEndian=be)
        assert hip.n == n and hip.stats()["layout"] == (0 if lay == "onehot" else 1)
        assert hip.lcp_info()[0] == 0
        got = hip.lcp()
        assert got.dtype == np.uint32 and np.array_equal(got, want), (name, lay)
        rows = rng.permutation(n).astype(np.uint64)
        assert np.array_equal(hip.lcp(rows), want[rows.astype(np.int64)]), (name, lay)
        for i in rows[:16].tolist() + [0, n - 1]:
            assert hip.getLCP(i) == int(want[i])
        path = tmp_path / (name + "." + lay + ".lcp")
        hip.write_lcp(path)
        data = path.read_bytes()
        assert len(data) == 4 * (n - 1) and data == want[:n - 1].astype(">u4").tobytes(), (name, lay)
        nbytes, ms, mx, row, total = hip.lcp_info()
        assert nbytes == 4 * n and ms > 0
        assert mx == int(want.max()) and row == int(np.argmax(want)) and total == int(want.astype(np.uint64).sum()), (name, lay)
        sa_path = tmp_path / (name + "." + lay + ".sa")
        hip.write_sa(sa_path)                                  # the changed inversion still writes SACreator's file
        assert sa_path.read_bytes() == sa.astype(">u4").tobytes(), (name, lay)
        hip.close()


@pytest.mark.parametrize("name,text", list(_adversarial().items()))
def test_adversarial_against_kasai_over_the_numpy_sort(name, text):
    s = lcp_checker.s_of_text(text)
    sa = np_suffix_array(np.frombuffer(s, dtype=np.uint8))
    want = lcp_checker.kasai(s, sa)
    got = findex_amd.lcp_from_text(text)
    assert got.dtype == np.uint32 and got.size == len(text) + 1
    assert np.array_equal(got, want), name
    assert got[0] == 0 and got[-1] == 0


def _sort_on_device(torch, text):
    """(bwt, sa, eof, counts) of a device text through fmx_bwt_from_text_dev."""
    length = text.numel()
    bwt = torch.empty(length + 1, dtype=torch.uint8, device=text.device)
    sa = torch.empty(length + 1, dtype=torch.int32, device=text.device)
    torch.cuda.synchronize()
    eof, counts = findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), sa.data_ptr(), device=0,
                                               stream=torch.cuda.current_stream().cuda_stream)
    return bwt, sa, eof, counts


def _core_on_device(torch, text, sa):
    length = text.numel()
    lcp = torch.empty(length + 1, dtype=torch.int32, device=text.device)
    torch.cuda.synchronize()
    findex_amd.lcp_from_text_dev(text.data_ptr(), length, sa.data_ptr(), lcp.data_ptr(), device=0,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return lcp


def _verify_on_device(torch, text, sa32, lcp32, chunk=1 << 26, cap=None):
    """Every row r < n - 1, with a = SA[r], b = SA[r + 1], L = LCP[r]: a + L <= n - 1, b + L <= n - 1, s[a + L] != s[b + L]
    and s[a + t] == s[b + t] for all t < L; LCP[n - 1] == 0.  Returns (max, sum) of the array by torch.  With a cap the
    bytes are compared for t < min(L, cap) only: a row with L <= cap is checked whole, and what a longer entry should be
    is the caller's to know."""
    dev = text.device
    n = text.numel() + 1
    s = torch.cat([torch.flip(text, dims=[0]), torch.zeros(1, dtype=torch.uint8, device=dev)])
    assert int(lcp32[n - 1].item()) == 0
    mx, total = 0, 0
    for lo in range(0, n - 1, chunk):
        hi = min(n - 1, lo + chunk)
        a = sa32[lo:hi].to(torch.int64) & 0xFFFFFFFF
        b = sa32[lo + 1:hi + 1].to(torch.int64) & 0xFFFFFFFF
        L = lcp32[lo:hi].to(torch.int64) & 0xFFFFFFFF
        assert bool(((a + L <= n - 1) & (b + L <= n - 1)).all().item()), "an LCP runs past the sentinel in [%d, %d)" % (lo, hi)
        assert bool((s[a + L] != s[b + L]).all().item()), "an LCP is too short in [%d, %d)" % (lo, hi)
        mx = max(mx, int(L.max().item()))
        total += int(L.sum().item())
        t = 0
        while cap is None or t < cap:
            live = L > t
            if not bool(live.any().item()):
                break
            a, b, L = a[live], b[live], L[live]
            assert bool((s[a + t] == s[b + t]).all().item()), "an LCP is too long in [%d, %d) at byte %d" % (lo, hi, t)
            t += 1
        del a, b, L
    return mx, total


def test_core_and_handle_agree_at_size():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import text_bwt
    dev = torch.device("cuda", 0)
    length = (1 << 30) - 1
    n = length + 1
    text = text_bwt.make_text(torch, length, 11, dev)
    bwt, sa, eof, counts = _sort_on_device(torch, text)
    core = _core_on_device(torch, text, sa)
    del text, sa
    torch.cuda.empty_cache()
    hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, counts)
    del bwt
    hip.prepare(ktab=False, lcp=True)
    nbytes, ms, mx, row, total = hip.lcp_info()
    assert nbytes == 4 * n
    out = torch.empty(n, dtype=torch.int32, device=dev)
    hip.lcp_range_dev(0, n, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.equal(out, core))                       # two routes to SA -- the suffix sort and the inversion -- one answer
    c64 = core.to(torch.int64) & 0xFFFFFFFF
    assert mx == int(c64.max().item()) and total == int(c64.sum().item())
    assert row == int(torch.nonzero(c64 == mx)[0].item())
    print("2^30 text: max LCP %d, mean %.3f, handle build %.1f ms" % (mx, total / n, ms))
    hip.close()


def test_across_2_31_every_row_on_the_device():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import text_bwt
    dev = torch.device("cuda", 0)
    length = (1 << 31) + 4099
    parts, left, seed = [], length, 5                        # as test_at_size_across_2_31 builds it
    while left:
        parts.append(text_bwt.make_text(torch, min(left, 1 << 30), seed, dev))
        left -= parts[-1].numel()
        seed += 1
    text = torch.cat(parts)
    del parts
    torch.cuda.empty_cache()
    bwt, sa, eof, counts = _sort_on_device(torch, text)
    del bwt
    torch.cuda.empty_cache()
    lcp = _core_on_device(torch, text, sa)
    mx, total = _verify_on_device(torch, text, sa, lcp)
    l64 = lcp.to(torch.int64) & 0xFFFFFFFF
    assert mx == int(torch.max(l64).item()) and total == int(torch.sum(l64).item())
    print("2^31 + 4099 text: max LCP %d, mean %.3f" % (mx, total / (length + 1)))


def test_long_repeats_core_and_handle():
    import torch
    dev = torch.device("cuda", 0)
    length = 1 << 26
    n = length + 1
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    text = torch.randint(97, 101, (length,), dtype=torch.uint8, device=dev, generator=g)
    blk = text[1000:1000 + (1 << 14)].clone()                # one block at three more places: LCPs of 2^14 and more
    for at in (1 << 20, (1 << 24) + 17, (1 << 26) - (1 << 15)):
        text[at:at + blk.numel()] = blk
    bwt, sa, eof, counts = _sort_on_device(torch, text)
    core = _core_on_device(torch, text, sa)
    mx, total = _verify_on_device(torch, text, sa, core)
    assert mx >= 1 << 14
    hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, counts)
    hip.prepare(ktab=False, lcp=True)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    hip.lcp_range_dev(0, n, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.equal(out, core))
    _, _, hmx, hrow, htotal = hip.lcp_info()
    c64 = core.to(torch.int64)
    assert (hmx, htotal) == (mx, total) and hrow == int(torch.nonzero(c64 == mx)[0].item())
    hip.close()


@pytest.fixture(scope="module")
def words_truth():
    return golden_truth("words", True)


def test_memory_returns(words_truth):
    import torch
    rng = np.random.default_rng(9)
    text = bytes(rng.integers(1, 5, 1 << 24, dtype=np.uint8))
    findex_amd.lcp_from_text(text)                            # the runtime's own first-use allocations happen here
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info(0)[0]
    findex_amd.lcp_from_text(text)
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info(0)[0] - free0) <= 64 << 20
    hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    hip.prepare(ktab=False, lcp=True)
    assert hip.lcp_info()[0] == 4 * hip.n
    hip.drop_tables(jump=False, frontier=False, lcp=True)
    assert hip.lcp_info()[0] == 0
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info(0)[0] - free1) <= 64 << 20
    assert np.array_equal(hip.lcp(), words_truth[1])          # and it comes back by a first call
    hip.close()


def test_prepare_contract_and_capture(words_truth):
    import torch
    _, want = words_truth
    txt = open(os.path.join(TESTDATA, "words.txt"), "rb").read()
    hip = findex_amd.HipFMSearcher(os.path.join(TESTDATA, "words.bwt"), bigEndian=True)
    rng = np.random.default_rng(14)
    pats = [txt[i:i + 4][::-1] for i in rng.integers(0, len(txt) - 4, 2000).tolist()]
    pbuf = np.frombuffer(b"".join(pats), dtype=np.uint8).copy()
    off = np.arange(0, 4 * len(pats) + 1, 4, dtype=np.uint64)
    hip.prepare(ktab=True, jump=True)
    sp0, ep0 = hip.search_batch(pbuf, off)
    held0 = hip.stats()["tables_held_bytes"]
    k = 1 << 16
    hrows = rng.integers(0, hip.n, k, dtype=np.uint64)
    hrows[5] = hip.n + 3                                      # out of range: UINT32_MAX
    rows = torch.from_numpy(hrows.view(np.int64)).cuda()
    out = torch.zeros(k, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    # without the array, a device call under capture is refused
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            hip.lcp_dev(rows.data_ptr(), k, out.data_ptr(), stream=s.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        out.zero_()                                           # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert err is not None and err.code == 5 and "stream capture" in str(err)
    assert hip.lcp_info()[0] == 0
    del g
    hip.prepare(ktab=False, lcp=True)
    assert hip.stats()["tables_held_bytes"] == held0
    sp1, ep1 = hip.search_batch(pbuf, off)
    assert np.array_equal(sp0, sp1) and np.array_equal(ep0, ep1)
    with torch.cuda.stream(s):
        hip.lcp_dev(rows.data_ptr(), k, out.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        hip.lcp_dev(rows.data_ptr(), k, out.data_ptr(), stream=s.cuda_stream)
    keep = np.arange(k) != 5
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert got[5] == np.uint32(0xFFFFFFFF)
        assert np.array_equal(got[keep], want[hrows[keep].astype(np.int64)])
    del g
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.lcp(np.array([hip.n], dtype=np.uint64))
    assert ei.value.code == 3
    L = _lib.load()
    assert L.fmx_write_lcp(hip.handle, b"/nonexistent/dir/x.lcp") == 1
    o4 = np.zeros(4, dtype=np.uint32)
    assert L.fmx_lcp_range(hip.handle, hip.n - 3, 4, o4.ctypes.data) == 3
    assert L.fmx_lcp_range(hip.handle, hip.n - 4, 4, o4.ctypes.data) == 0 and np.array_equal(o4, want[-4:])
    hip.close()


def test_core_refuses_a_stream_capture():
    import torch
    dev = torch.device("cuda", 0)
    text = torch.full((1024,), 97, dtype=torch.uint8, device=dev)
    sa = torch.arange(1024, -1, -1, dtype=torch.int32, device=dev)
    lcp = torch.empty(1025, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            findex_amd.lcp_from_text_dev(text.data_ptr(), 1024, sa.data_ptr(), lcp.data_ptr(), device=0, stream=s.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        lcp.zero_()
        g.capture_end()
    assert err is not None and err.code == 5 and "stream capture" in str(err)
    # outside a capture the same call gives the array of 'a' x 1024: SA[r] = n - 1 - r, LCP[r] = r
    findex_amd.lcp_from_text_dev(text.data_ptr(), 1024, sa.data_ptr(), lcp.data_ptr(), device=0)
    torch.cuda.synchronize()
    want = np.arange(1025, dtype=np.uint32)
    want[-1] = 0
    assert np.array_equal(lcp.cpu().numpy().view(np.uint32), want)


def test_bwt_of_several_cycles_is_refused(tmp_path):
    bwt, eof, counts = synth_bwt(20000, 1, 4, seed=21)
    hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
    orc = oracle.NaiveFMSearcher(_mem=(bwt, bwt.size, eof, counts))
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.prepare(ktab=False, lcp=True)
    assert ei.value.code == 2 and "not the BWT of one text" in str(ei.value)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.getLCP(1)
    assert ei.value.code == 2
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.write_lcp(tmp_path / "never.lcp")
    assert ei.value.code == 2
    assert hip.lcp_info()[0] == 0
    rng = np.random.default_rng(1)
    pats = rng.integers(1, 5, 4000, dtype=np.uint8)
    off = np.arange(0, 4001, 4, dtype=np.uint64)
    sp, ep = hip.search_batch(pats, off)
    wsp, wep, _ = orc.search_batch(pats, off)
    hit = wsp < wep
    assert hit.sum() > 900
    assert np.array_equal(sp[hit], wsp[hit]) and np.array_equal(ep[hit], wep[hit]) and np.all(sp[~hit] >= ep[~hit])
    hip.close()


def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    L = _lib.load()
    out = (ctypes.c_uint32 * 1)()
    rows = (ctypes.c_uint64 * 1)(0)
    assert L.fmx_prepare(hip.handle, 64) == 6
    assert L.fmx_lcp_batch(hip.handle, rows, 1, out) == 6
    assert L.fmx_lcp_batch_dev(hip.handle, rows, 1, out, None) == 6
    assert L.fmx_lcp_range(hip.handle, 0, 1, out) == 6
    assert L.fmx_write_lcp(hip.handle, b"/tmp/never.lcp") == 6
    hip.close()


def test_cli_writes_the_four_siblings(words_truth, tmp_path):
    sa, want = words_truth
    src = tmp_path / "words.txt"
    shutil.copy(os.path.join(TESTDATA, "words.txt"), src)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", str(src), "--fm", "--sa", "--lcp"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "words.bwt").read_bytes() == open(os.path.join(TESTDATA, "words.bwt"), "rb").read()
    assert (tmp_path / "words.aux").read_bytes() == open(os.path.join(TESTDATA, "words.aux"), "rb").read()
    assert (tmp_path / "words.lcp").read_bytes() == lcp_checker.lcp_file_bytes(want)
    assert (tmp_path / "words.sa").read_bytes() == sa.astype(">u4").tobytes()
    n = sa.size
    assert (tmp_path / "words.fm").stat().st_size == 4 * n + 9            # FMLoader's own size check
    assert sorted(p.name for p in tmp_path.iterdir()) == ["words.aux", "words.bwt", "words.fm", "words.lcp", "words.sa", "words.txt"]
