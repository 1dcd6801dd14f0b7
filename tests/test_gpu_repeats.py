"""fmx_repeats on the device against tests/repeats_ref.py, the count written from the definition in text coordinates
(DESIGN.md 18): fixture indexes in both layouts, adversarial texts, the edges of the scan's tile, several thresholds per
call, the capacity rules, the device form, the refusals, one text of 2^20 bytes and a corpus."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import findex_amd
import oracle
import repeats_ref
from corpus_ref import RefCorpus
from findex_amd import _lib
from helpers import ends_at_a_fault, synth_bwt
from test_gpu_build_text import _adversarial
from test_gpu_lcp import golden_indexes, golden_truth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")
T = _lib.FMX_REPEATS_TILE
OVERFLOW, HIP_ERR = 9, 5
LAYOUTS = ["onehot", "bytes"]


def reference(text, L, later, stop):
    """brute for the small texts, hashed for the others (tests/test_repeats_cpu.py holds the two to each other)"""
    return (repeats_ref.brute if len(text) <= 600 else repeats_ref.hashed)(text, L, later, stop)


def check(hip, text, levels, stops=(0,), what=""):
    """one call per (mode, stop byte) with all the thresholds, every range and every summary field against the reference"""
    for stop in stops:
        for later in (False, True):
            got = hip.repeats(list(levels), keep_first=later, stop=stop)
            assert len(got) == len(levels)
            for L, (ranges, summary) in zip(levels, got):
                want_r, want_s = reference(text, L, later, stop)
                print(what, "L", L, "later", later, "stop", stop, "got", summary, "want", want_s)
                assert summary == want_s, (what, L, later, stop)
                assert ranges.dtype == np.uint64 and ranges.shape == want_r.shape and np.array_equal(ranges, want_r), (what, L, later, stop)


def open_text(text, layout="auto"):
    findex_amd.set_layout(layout)
    try:
        return findex_amd.HipFMSearcher.from_text(text)
    finally:
        findex_amd.set_layout("auto")


# ---------------------------------------------------------------- 1. the fixture indexes
def golden_text(name, be):
    """The text of a fixture index, recovered as test_gpu_lcp.golden_truth recovers s: bwt[r] = s[SA[r] - 1], text = reverse(s)."""
    sa, lcp = golden_truth(name, be)
    bwt, size, eof = oracle.load_bwt_file(os.path.join(TESTDATA, name + ".bwt"), bigEndian=be)
    s = np.zeros(size, dtype=np.uint8)
    keep = np.arange(size) != eof
    s[sa[keep] - 1] = np.asarray(bwt)[keep]
    return s[:size - 1][::-1].tobytes(), int(lcp.max())


@pytest.mark.parametrize("name,be", golden_indexes())
@ends_at_a_fault
def test_goldens(name, be):
    text, max_lcp = golden_text(name, be)
    levels = [1, 2, 3, 8, max_lcp, max_lcp + 1]
    values, counts = np.unique(np.frombuffer(text, dtype=np.uint8), return_counts=True)
    stop = int(values[np.argsort(counts)[len(counts) // 2]])              # a byte that occurs, neither the rarest nor the commonest
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
        check(hip, text, levels, stops=(0, stop), what="%s/%s" % (name, lay))
        info1 = hip.lcp_info()
        assert info1[0] == 4 * hip.n and info1[2] == max_lcp
        if lay == "bytes":
            assert info1 == info0
        assert hip.stats()["patterns_seen"] == seen0 and hip.stats()["launches"] > launches0
        sp1, ep1 = hip.search_batch(pats, off)
        assert np.array_equal(sp0, sp1) and np.array_equal(ep0, ep1)
        hip.close()


# ---------------------------------------------------------------- 2. adversarial texts
ADVERSARIAL = ["ab_repeated", "fibonacci", "sigma2", "a_then_b", "rand1", "rand2", "rand3"]


@pytest.mark.parametrize("name", ADVERSARIAL)
@ends_at_a_fault
def test_adversarial(name):
    text = _adversarial()[name]
    hip = open_text(text)
    check(hip, text, [1, 2, 3, 7, 64, 5000], stops=(0, text[0]), what=name)
    hip.close()


# ---------------------------------------------------------------- 3. the tile's edges
@pytest.mark.parametrize("m", [T - 1, T, T + 1, 3 * T + 5])
@ends_at_a_fault
def test_one_letter_is_one_class_of_every_row(m):
    text = b"a" * m
    hip = open_text(text)
    check(hip, text, [1, 2, T // 2, m - 1, m, m + 1], what="a x %d" % m)
    ranges, summary = hip.repeats(3)
    assert ranges.tolist() == [[0, m]] and summary["classes"] == 1 and summary["largest_class"] == m - 2
    hip.close()


def sigma4(rng, m):
    return bytearray((rng.integers(0, 3, m, dtype=np.uint8) + 97).tobytes())          # a, b, c: 'd' is placed by hand


def has_range(text, L, later, stop, a, b):
    return [a, b] in reference(bytes(text), L, later, stop)[0].tolist()


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_planted_copies_at_tile_edges(layout):
    m = 3 * T + 5
    rng = np.random.default_rng(23)
    # (a) with 'd' as the stop byte: "ab" on a tile's last byte and the next tile's first, a stop byte on either side of it,
    #     and stop bytes on a tile's last and first byte
    ta = sigma4(rng, m)
    ta[T - 2:T + 2] = b"dabd"
    ta[100:102] = b"ab"
    ta[2 * T - 1:2 * T + 1] = b"dd"
    ta[0], ta[m - 1] = ord("d"), ord("d")
    assert has_range(ta, 2, False, ord("d"), T - 1, T + 1)
    hip = open_text(bytes(ta), layout)
    check(hip, bytes(ta), [1, 2, 3, 9], stops=(ord("d"), 0), what="stops at tile edges")
    hip.close()
    # (b) a copy of 2 T + 3 bytes at 0 and at T + 2 (the text has that period), searched with L = 2 T: L exceeds a tile
    block = bytes(sigma4(rng, T + 2))
    tb = (block * 3)[:m]
    assert tb[:2 * T + 3] == tb[T + 2:] and has_range(tb, 2 * T, False, 0, 0, m) and has_range(tb, 2 * T, True, 0, T + 2, m)
    hip = open_text(tb, layout)
    check(hip, tb, [2 * T, 2 * T + 3, 2 * T + 4, T], what="L above a tile")
    hip.close()
    # (c) L = 20: X twice in a row with the second copy on a tile's first byte -- two flagged windows exactly L apart, one
    #     range; Y, one byte, Y with that byte on a tile's last byte -- two flagged windows L + 1 apart, two ranges
    L = 20
    tc = sigma4(rng, m)
    x, y = b"abcabbcacbbacabcbbca", b"ccabacbbcabaacbcacba"
    tc[T - L - 1:T + L + 1] = b"d" + x + x + b"d"              # (a 'd' on either side: the windows next to the copies stay unique)
    tc[2 * T - 1 - L:2 * T + L] = y + b"d" + y
    tc = bytes(tc)
    assert has_range(tc, L, False, 0, T - L, T + L) and has_range(tc, L, True, 0, T, T + L)
    assert has_range(tc, L, False, 0, 2 * T - 1 - L, 2 * T - 1) and has_range(tc, L, False, 0, 2 * T, 2 * T + L)
    hip = open_text(tc, layout)
    check(hip, tc, [L, L - 1, L + 1], stops=(0, ord("d")), what="L and L + 1 apart")
    hip.close()


# ---------------------------------------------------------------- 4. thresholds, capacity, determinism
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


def raw_call(hip, levels, later, stop, out, cap, dev=None):
    """fmx_repeats itself -> (status, n_out, out_off, summaries)"""
    L = _lib.load()
    lv = np.array(levels, dtype=np.uint32)
    opts = _lib.fmx_repeat_opts(1 if later else 0, stop, (0, 0, 0))
    n_out = ctypes.c_size_t(12345)
    off = np.full(len(levels) + 1, 77, dtype=np.uint64)
    sums = (_lib.fmx_repeat_summary * len(levels))()
    rc = L.fmx_repeats(hip.handle, lv.ctypes.data, len(levels), ctypes.byref(opts), off.ctypes.data,
                       out.ctypes.data if out is not None else None, cap, ctypes.byref(n_out), sums)
    return rc, int(n_out.value), off, [{f: int(getattr(x, f)) for f in repeats_ref.FIELDS} for x in sums]


@ends_at_a_fault
def test_thresholds_capacity_and_determinism(planted):
    text, hip = planted
    levels = [64, 12, 300, 50000, 29]                          # in no order, one of them longer than the text
    many = hip.repeats(levels, keep_first=True)
    singles = [hip.repeats(L, keep_first=True) for L in levels]
    total = 0
    for L, (r, s), (r1, s1) in zip(levels, many, singles):
        want_r, want_s = reference(text, L, True, 0)
        assert np.array_equal(r, r1) and s == s1 and np.array_equal(r, want_r) and s == want_s, L
        total += r.shape[0]
    assert many[3][0].shape == (0, 2) and total > 10
    want_off = np.cumsum([0] + [r.shape[0] for r, _ in many]).astype(np.uint64)
    # the counting call: the exact total, the offsets complete, the summaries valid
    rc, n, off, sums = raw_call(hip, levels, True, 0, None, 0)
    assert rc == OVERFLOW and n == total and np.array_equal(off, want_off) and sums == [s for _, s in many]
    assert str(total).encode() in _lib.load().fmx_last_error()
    guard = 8
    out = np.full((total + guard, 2), 0xABABABABABABABAB, dtype=np.uint64)
    rc, n, off, sums = raw_call(hip, levels, True, 0, out, total)
    assert rc == 0 and n == total and np.array_equal(off, want_off) and (out[total:] == 0xABABABABABABABAB).all()
    assert np.array_equal(out[:total], np.concatenate([r for r, _ in many]))
    first = out[:total].tobytes()
    # one record short: the exact total again, nothing at or behind out[cap]
    out[:] = 0xABABABABABABABAB
    rc, n, off, sums = raw_call(hip, levels, True, 0, out, total - 1)
    assert rc == OVERFLOW and n == total and np.array_equal(off, want_off) and sums == [s for _, s in many]
    assert (out[total - 1:] == 0xABABABABABABABAB).all()
    # the same bytes on a second run
    out[:] = 0
    rc, n, off2, sums2 = raw_call(hip, levels, True, 0, out, total)
    assert rc == 0 and out[:total].tobytes() == first and np.array_equal(off2, want_off) and sums2 == sums
    assert all(x >= 0 for x in hip.repeats_last()) and hip.repeats_last()[0] > 0


# ---------------------------------------------------------------- 5. the device form
@ends_at_a_fault
def test_device_form_and_a_capture(planted):
    import torch
    text, hip = planted
    levels = [12, 5, 300, 8]                                   # (with 'd' as the stop byte few long windows are eligible)
    host = hip.repeats(levels, keep_first=False, stop=ord("d"))
    for L, (r, s) in zip(levels, host):
        want_r, want_s = reference(text, L, False, ord("d"))
        assert np.array_equal(r, want_r) and s == want_s, L
    total = sum(r.shape[0] for r, _ in host)
    assert total > 100 and host[0][0].shape[0] > 0
    d_off = torch.zeros(len(levels) + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((2 * total + 16,), -1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        n, sums = hip.repeats_dev(levels, d_off.data_ptr(), d_out.data_ptr(), total, stop=ord("d"), stream=st.cuda_stream)
    st.synchronize()
    assert n == total and sums == [s for _, s in host]
    raw = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(raw[:2 * total].reshape(-1, 2), np.concatenate([r for r, _ in host])) and (raw[2 * total:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), np.cumsum([0] + [r.shape[0] for r, _ in host]).astype(np.uint64))
    # one record short
    d_out.fill_(-1)
    torch.cuda.synchronize()
    with pytest.raises(findex_amd.FmxError) as err:
        hip.repeats_dev(levels, d_off.data_ptr(), d_out.data_ptr(), total - 1, stop=ord("d"))
    assert err.value.code == OVERFLOW
    raw = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(raw[:2 * (total - 1)].reshape(-1, 2), np.concatenate([r for r, _ in host])[:-1]) and (raw[2 * (total - 1):] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
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
            hip.repeats_dev(levels, d_off.data_ptr(), d_out.data_ptr(), total, stop=ord("d"), stream=st.cuda_stream)
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


# ---------------------------------------------------------------- 6. refusals
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
    d_out = torch.zeros(64, dtype=torch.int64, device="cuda")

    def refused(hip, code, needle):
        for dev in (False, True):
            with pytest.raises(findex_amd.FmxError) as err:
                if dev:
                    hip.repeats_dev(4, d_off.data_ptr(), d_out.data_ptr(), 32)
                else:
                    hip.repeats(4)
            assert err.value.code == code and needle in str(err.value), str(err.value)

    for hip, code, needle in ((block, 6, "fmx_open_block"), (synth, 2, "not the BWT of one text")):
        refused(hip, code, needle)                              # (the handle's stream and the runtime's first-use memory)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        refused(hip, code, needle)
        torch.cuda.synchronize()
        # Every temporary of the call on the big handle is 4 n bytes or more (the smallest: the suffix array, the LCP array),
        # so one that stayed would show as at least that; the runtime's own memory for a stream's queue comes in 2 MiB pieces.
        assert abs(torch.cuda.mem_get_info()[0] - free0) < 4 * n
        assert hip.lcp_info()[0] == 0
    block.close()
    synth.close()


# ---------------------------------------------------------------- 7. one text of 2^20 bytes
@ends_at_a_fault
def test_a_megabyte_with_planted_copies():
    rng = np.random.default_rng(47)
    m = 1 << 20
    t = bytearray((rng.integers(0, 4, m, dtype=np.uint8) + 97).tobytes())
    plants = [(1000, 40), (20000, 41), (50000, 100), (90000, 777), (200000, 5000), (300000, 2048), (400000, 2049), (500000, 24)]
    for i, (src, ln) in enumerate(plants):
        dst = 600000 + 40000 * i + 7 * i
        t[dst:dst + ln] = t[src:src + ln]
    t[1040000:1040777] = t[90000:90777]                         # one of them a third time
    text = bytes(t)
    hip = findex_amd.HipFMSearcher.from_text(text)
    for later in (False, True):
        ranges, summary = hip.repeats(24, keep_first=later)
        want_r, want_s = repeats_ref.hashed(text, 24, later, 0)
        print("2^20 later", later, "got", summary, "want", want_s)
        assert summary == want_s and np.array_equal(ranges, want_r)
        assert summary["largest_class"] == 3 and summary["ranges"] >= len(plants)
    hip.close()


# ---------------------------------------------------------------- 8. a corpus
def corpus_documents():
    rng = np.random.default_rng(53)

    def words(k):
        return b" ".join(bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(k))

    shared = b"It was the best of times, it was the worst of times, it was the age of wisdom."
    special = b"raw zero \x00 raw one \x01 raw max \xff in a stretch that occurs twice"
    twin = words(30)
    return [words(20) + shared + words(12), twin, b"", words(8) + shared, twin, words(25),
            words(5) + special + words(6), special + words(9)]


def expected_rows(ref, L, later):
    """brute over the stream with the separator as the stop byte, the two ends of every range through the per-position table"""
    ranges, _ = repeats_ref.brute(ref.stream, L, later, 1)
    rows = [(ref.map(int(a))[0], ref.map(int(a))[2], ref.map(int(b) - 1)[2] + 1) for a, b in ranges]
    assert all(ref.map(int(a))[0] == ref.map(int(b) - 1)[0] for a, b in ranges)
    return np.array(sorted(rows), dtype=np.uint64).reshape(-1, 3)


@ends_at_a_fault
def test_corpus_duplicate_passages(tmp_path):
    docs = corpus_documents()
    ref = RefCorpus(docs)
    L = 12
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    rows = {}
    for later in (False, True):
        rows[later] = cs.duplicate_passages(L, keep_first=later)
        want = expected_rows(ref, L, later)
        print("corpus later", later, rows[later].tolist())
        assert rows[later].dtype == np.uint64 and np.array_equal(rows[later], want)
        assert (rows[later][:, 2] <= np.array([len(docs[int(d)]) for d in rows[later][:, 0]], dtype=np.uint64)).all()   # within its document
        per_doc = cs.duplicate_bytes(L, keep_first=later)
        assert per_doc.dtype == np.uint64 and per_doc.size == len(docs)
        for d in range(len(docs)):
            assert int(per_doc[d]) == sum(int(r[2] - r[1]) for r in rows[later] if int(r[0]) == d)
    assert np.array_equal(cs.duplicate_passages(L), rows[True])                      # keep-first is the default
    # the second twin goes whole in keep-first mode, the first stays; the empty document has no row
    assert [4, 0, len(docs[4])] in rows[True].tolist() and not (rows[True][:, 0] == 1).any() and not (rows[False][:, 0] == 2).any()
    assert (rows[True][:, 0] == 7).any() and (rows[False][:, 0] == 6).any()          # the stretch with the raw 0, 1 and 255
    cs.close()
    # the documents without special bytes, as a corpus of their own, against the raw files joined with a boundary byte
    plain = [d for d in docs if not any(c in d for c in (0, 1, 255))]
    assert len(plain) == 6
    joined = b"\x01".join(plain) + b"\x01"
    starts = np.cumsum([0] + [len(d) + 1 for d in plain])
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(plain))
    for later in (False, True):
        want = []
        for a, b in repeats_ref.brute(joined, L, later, 1)[0].tolist():
            d = int(np.searchsorted(starts, a, side="right")) - 1
            assert b <= starts[d + 1] - 1
            want.append((d, a - starts[d], b - starts[d]))
        assert cs.duplicate_passages(L, keep_first=later).tolist() == [list(w) for w in sorted(want)]
    cs.close()
    # the command line writes the keep-first rows, by name
    src = tmp_path / "docs"
    src.mkdir()
    for d, raw in enumerate(docs):
        (src / ("d%d" % d)).write_bytes(raw)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", "--dir", str(src), "--out", str(tmp_path / "x"), "--no-filter-binary",
                        "--dups", str(L)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = (tmp_path / "x.dups").read_bytes().split(b"\n")
    assert lines[-1] == b"" and lines[:-1] == [b"d%d\t%d\t%d" % (d, a, b) for d, a, b in rows[True].tolist()]
    # and the single-file form the ranges of the file, no stop byte
    one = tmp_path / "one.txt"
    one.write_bytes(docs[0] + docs[3])
    r = subprocess.run([sys.executable, "-m", "findex_amd.index", str(one), "--dups", str(L)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want = repeats_ref.brute(docs[0] + docs[3], L, False, 0)[0].tolist()
    assert (tmp_path / "one.dups").read_text() == "".join("%d\t%d\n" % (a, b) for a, b in want) and want
