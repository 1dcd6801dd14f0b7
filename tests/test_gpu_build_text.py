"""Index construction from text on the device (fmx_bwt_from_text*, fmx_open_text): the BWT of reverse(text) + EOF as
BWTMerger2.merge(FileBWTReader) writes it (bwtmerger.scala:782-810, 841-856, 1106-1108), checked against the reference's
own fixture files, an independent numpy suffix sort, the product's search, and -- at size, across the 2^31 boundary --
the linear suffix-array check on the device."""
import os
import sys

import numpy as np
import pytest

import findex_amd
import oracle
from conftest import ROOT
from helpers import bwt_of_text

pytestmark = pytest.mark.gpu

GOLDEN_NAMES = ["test1024", "test2048", "test2048-2", "test3072", "test", "test-part"]


def np_suffix_array(s):
    """Prefix doubling with numpy lexsort over (rank[i], rank[i + k]) -- independent of the library's radix sort.  s ends
    with its unique smallest symbol 0."""
    n = len(s)
    rank = s.astype(np.int64)
    k = 1
    while True:
        r2 = np.full(n, -1, dtype=np.int64)
        r2[: n - k] = rank[k:]
        sa = np.lexsort((r2, rank))
        a, b = rank[sa], r2[sa]
        diff = np.ones(n, dtype=bool)
        diff[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
        nr = np.cumsum(diff) - 1
        rank = np.empty(n, dtype=np.int64)
        rank[sa] = nr
        if nr[-1] == n - 1:
            return sa
        k *= 2


def np_bwt_of_text(text):
    """(bwt, eof, counts) of reverse(text) + EOF by np_suffix_array, sa2BWT's filler rule."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    s = np.concatenate([t[::-1], np.zeros(1, dtype=np.uint8)])
    sa = np_suffix_array(s)
    eof = int(np.nonzero(sa == 0)[0][0])
    bwt = s[sa - 1]
    bwt[eof] = bwt[eof - 1] if eof > 0 else bwt[eof + 1]
    return bwt, eof, np.bincount(t, minlength=256).astype(np.int64)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_goldens(testdata, name):
    txt = open(os.path.join(testdata, name + ".txt"), "rb").read()
    gbwt, size, geof = oracle.load_bwt_file(os.path.join(testdata, name + ".cmp.bwt"), bigEndian=False)
    gaux = oracle.load_aux_file(os.path.join(testdata, name + ".cmp.aux"), bigEndian=False)
    bwt, eof, counts = findex_amd.bwt_from_text(txt)
    assert bwt.size == size and eof == geof
    keep = np.arange(size) != eof
    assert np.array_equal(bwt[keep], gbwt[keep])
    assert np.array_equal(counts, gaux)
    want, weof, _ = bwt_of_text(txt[::-1])            # the sa2BWT filler (the C tool used another in some goldens)
    assert weof == eof and np.array_equal(bwt, want)


def test_words_reproduces_words_bwt_entirely(testdata):
    txt = open(os.path.join(testdata, "words.txt"), "rb").read()
    gbwt, size, geof = oracle.load_bwt_file(os.path.join(testdata, "words.bwt"), bigEndian=True)
    gaux = oracle.load_aux_file(os.path.join(testdata, "words.aux"), bigEndian=True)
    bwt, eof, counts = findex_amd.bwt_from_text(txt)
    assert (size, geof) == (bwt.size, eof)
    assert np.array_equal(bwt, gbwt)                   # the eof filler included
    assert np.array_equal(counts, gaux)
    again = findex_amd.bwt_from_text(txt)              # deterministic
    assert again[1] == eof and np.array_equal(again[0], bwt)


def _fib(n):
    a, b = b"b", b"a"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _adversarial():
    rng = np.random.default_rng(7)
    cases = {}
    for n in (1, 2, 3, 63, 64, 65, (1 << 16) - 1, (1 << 16) + 1):
        cases["rand%d" % n] = bytes(rng.integers(1, 256, n, dtype=np.uint8))
    cases["a_x_2^20"] = b"a" * (1 << 20)
    cases["ab_repeated"] = b"ab" * 50000
    cases["fibonacci"] = _fib(100000)
    cases["sigma2"] = bytes(rng.integers(1, 3, 200000, dtype=np.uint8))
    cases["sigma255"] = bytes(rng.integers(1, 256, 300000, dtype=np.uint8))
    cases["a_then_b"] = b"a" * 5000 + b"b" + b"a" * 5000
    return cases


@pytest.mark.parametrize("name,text", list(_adversarial().items()))
def test_adversarial_against_numpy_sort(name, text):
    bwt, eof, counts = findex_amd.bwt_from_text(text)
    want, weof, wcounts = np_bwt_of_text(text)
    assert eof == weof
    assert np.array_equal(bwt, want)
    assert np.array_equal(counts, wcounts)


def _overlapping_count(text, p):
    c, i = 0, text.find(p)
    while i >= 0:
        c += 1
        i = text.find(p, i + 1)
    return c


def test_counts_through_the_product(testdata):
    txt = open(os.path.join(testdata, "words.txt"), "rb").read()
    hip = findex_amd.HipFMSearcher.from_text(txt)
    orc = oracle.NaiveFMSearcher(os.path.join(testdata, "words.bwt"), bigEndian=True)
    assert hip.n == orc.n == len(txt) + 1
    rng = np.random.default_rng(3)
    pats = []
    for _ in range(200):
        m = int(rng.integers(1, 9))
        i = int(rng.integers(0, len(txt) - m))
        pats.append(txt[i:i + m])
    pats += [b"aardvark", b"zzzzq", b"\n", b"the"]
    for p in pats[:60]:
        r = hip.search(p[::-1])
        got = 0 if r is None else r[1] - r[0]
        assert got == _overlapping_count(txt, p), p
    rev = [p[::-1] for p in pats]
    off = np.zeros(len(rev) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in rev])
    buf = np.frombuffer(b"".join(rev), dtype=np.uint8).copy()
    sp, ep = hip.search_batch(buf, off)
    wsp, wep, _ = orc.search_batch(buf, off)
    hit = wsp < wep
    assert np.array_equal(sp[hit], wsp[hit]) and np.array_equal(ep[hit], wep[hit])
    assert np.all(sp[~hit] >= ep[~hit])
    assert hip.search(b"aardvark"[::-1]) == (1044943, 1044945)


def _verify_sa_on_device(torch, d_text, length, d_sa32, d_bwt, eof):
    """The linear check: SA is a permutation of 0..n-1 and, for each i, (s[SA[i]], ISA[SA[i] + 1]) < (s[SA[i + 1]],
    ISA[SA[i + 1] + 1]) -- then SA is THE suffix array; and the BWT and eof follow from it."""
    dev = d_text.device
    n = length + 1
    s = torch.cat([torch.flip(d_text, dims=[0]), torch.zeros(1, dtype=torch.uint8, device=dev)])
    sa = d_sa32.to(torch.int64) & 0xFFFFFFFF                # u32 held in int32
    assert int(sa.max().item()) == n - 1 and int(sa.min().item()) == 0
    isa = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)          # isa[n] = -1: past the sentinel
    isa[sa] = torch.arange(n, dtype=torch.int64, device=dev)
    assert int((isa[:n] < 0).sum().item()) == 0, "not a permutation"
    chunk = 1 << 28
    for lo in range(0, n - 1, chunk):
        hi = min(n - 1, lo + chunk)
        a, b = sa[lo:hi], sa[lo + 1:hi + 1]
        sa_, sb = s[a], s[b]
        ok = (sa_ < sb) | ((sa_ == sb) & (isa[a + 1] < isa[b + 1]))
        assert bool(ok.all().item()), "suffixes out of order in [%d, %d)" % (lo, hi)
        del a, b, sa_, sb, ok
    assert int(sa[eof].item()) == 0
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        p = sa[lo:hi]
        want = s[torch.clamp(p - 1, min=0)]
        got = d_bwt[lo:hi]
        mask = p != 0
        assert bool((got[mask] == want[mask]).all().item()), "BWT does not follow from SA in [%d, %d)" % (lo, hi)
    fill = int(s[int(sa[eof - 1 if eof > 0 else 1].item()) - 1].item())
    assert int(d_bwt[eof].item()) == fill


@pytest.mark.parametrize("kind", ["iid128", "text"])
def test_at_size_across_2_31(kind):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import text_bwt
    dev = torch.device("cuda", 0)
    length = (1 << 31) + 4099
    if kind == "iid128":
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        text = torch.randint(1, 129, (length,), generator=g, device=dev, dtype=torch.uint8)
    else:       # the generator in pieces of at most 2^30 bytes (its torch.searchsorted takes fewer than 2^31 positions)
        parts, left, seed = [], length, 5
        while left:
            parts.append(text_bwt.make_text(torch, min(left, 1 << 30), seed, dev))
            left -= parts[-1].numel()
            seed += 1
        text = torch.cat(parts)
        del parts
        torch.cuda.empty_cache()
    bwt = torch.empty(length + 1, dtype=torch.uint8, device=dev)
    sa = torch.empty(length + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eof, counts = findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), sa.data_ptr(), device=0,
                                               stream=torch.cuda.current_stream().cuda_stream)
    assert int(counts.sum()) == length and counts[0] == 0
    hist = torch.bincount(text, minlength=256).cpu().numpy()
    assert np.array_equal(hist, counts)
    _verify_sa_on_device(torch, text, length, sa, bwt, eof)


def test_against_the_torch_tool():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import text_bwt
    dev = torch.device("cuda", 0)
    length = (1 << 30) - 1
    text = text_bwt.make_text(torch, length, 11, dev)
    want, weof = text_bwt.bwt_of_reversed_text(torch, text)
    torch.cuda.empty_cache()
    bwt = torch.empty(length + 1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eof, _ = findex_amd.bwt_from_text_dev(text.data_ptr(), length, bwt.data_ptr(), 0, device=0,
                                          stream=torch.cuda.current_stream().cuda_stream)
    assert eof == weof
    assert bool(torch.equal(bwt, want))


def test_device_memory_returns():
    import torch
    rng = np.random.default_rng(9)
    text = bytes(rng.integers(1, 5, 1 << 26, dtype=np.uint8))
    findex_amd.bwt_from_text(text)                     # the runtime's own first-use allocations happen here
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    findex_amd.bwt_from_text(text)
    h = findex_amd.HipFMSearcher.from_text(text[: 1 << 20])
    h.close()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    assert abs(free0 - free1) <= 64 << 20, (free0, free1)


def test_construction_refuses_a_stream_capture():
    import torch
    dev = torch.device("cuda", 0)
    text = torch.full((1024,), 97, dtype=torch.uint8, device=dev)
    bwt = torch.empty(1025, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            findex_amd.bwt_from_text_dev(text.data_ptr(), 1024, bwt.data_ptr(), 0, device=0, stream=s.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        bwt.zero_()                                    # (the graph is not empty; it is never replayed)
        g.capture_end()
    assert err is not None and err.code == 5 and "stream capture" in str(err)


def test_device_text_with_byte_0_is_refused():
    import torch
    dev = torch.device("cuda", 0)
    text = torch.full((4096,), 97, dtype=torch.uint8, device=dev)
    text[1000] = 0
    bwt = torch.empty(4097, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(findex_amd.FmxError) as e:
        findex_amd.bwt_from_text_dev(text.data_ptr(), 4096, bwt.data_ptr(), 0, device=0)
    assert e.value.code == 6


def test_cli_writes_files_both_searchers_open(testdata, tmp_path):
    """python -m findex_amd.index on a copy of words.txt: X.bwt / X.aux next to it, equal to the reference's words.bwt /
    words.aux, opened by fmx_open and by the oracle with the reference's answer."""
    import shutil
    import subprocess
    src = tmp_path / "words.txt"
    shutil.copy(os.path.join(testdata, "words.txt"), src)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", str(src)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "words.bwt").read_bytes() == open(os.path.join(testdata, "words.bwt"), "rb").read()
    assert (tmp_path / "words.aux").read_bytes() == open(os.path.join(testdata, "words.aux"), "rb").read()
    hip = findex_amd.HipFMSearcher(str(src), bigEndian=True)
    orc = oracle.NaiveFMSearcher(str(tmp_path / "words.bwt"), bigEndian=True)
    assert hip.search(b"aardvark"[::-1]) == orc.search(b"aardvark"[::-1]) == (1044943, 1044945)
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", str(src), "--little-endian"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert findex_amd.HipFMSearcher(str(src), bigEndian=False).search(b"aardvark"[::-1]) == (1044943, 1044945)
