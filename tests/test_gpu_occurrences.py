"""fmx_occurrences on the device (include/fmx.h) against tests/occ_ref.py, byte for byte: regexes end to end,
the tile edges of the scans and the sort, the key widths, duplicates and limits, the corpus, the routes that existed before,
and the contract's refusals."""
import ctypes
import os

import numpy as np
import pytest

import corpus_ref
import findex_amd
import occ_ref
from conftest import TESTDATA
from findex_amd import _lib
from helpers import ends_at_a_fault

pytestmark = pytest.mark.gpu

ARG, HIP, UNSUPPORTED, OVERFLOW = 3, 5, 6, 9
H = findex_amd.HipFMSearcher
OCC = occ_ref.OCC
MODES = ("all", "longest", "disjoint")


def same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0][:10], want[0][:10])
    assert got[1].dtype == OCC and got[1].tobytes() == want[1].tobytes()


def interval(hip, Q):
    r = hip.search(bytes(Q)[::-1])
    assert r is not None, Q
    return int(r[0]), int(r[1])


def closed_form(per_group):
    """[(pos array, len)] per group, ascending by pos -> (off, OCC array) without a corpus."""
    off = np.zeros(len(per_group) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([sum(p.size for p, _ in g) for g in per_group])
    occ = np.zeros(int(off[-1]), dtype=OCC)
    for g, parts in enumerate(per_group):
        pos = np.concatenate([p for p, _ in parts]) if parts else np.zeros(0, np.uint64)
        ln = np.concatenate([np.full(p.size, l_) for p, l_ in parts]) if parts else np.zeros(0, np.uint64)
        order = np.lexsort((ln, pos))
        sl = occ[int(off[g]):int(off[g + 1])]
        sl["group"], sl["pos"], sl["len"] = g, pos[order], ln[order]
    occ["doc"], occ["raw_len"], occ["raw_off"] = 0xFFFFFFFF, occ["len"], occ["pos"]
    return off, occ


# ---------------------------------------------------------------- 1. regexes end to end
@pytest.fixture(scope="module")
def words():
    T = occ_ref.word_text()
    tabs = occ_ref.regex_tables()
    want = {mode: occ_ref.brute_csr(tabs, T, occ_ref.MAX_LEN, mode) for mode in MODES}
    hip = H.from_text(T)
    yield T, hip, want
    hip.close()


@pytest.mark.parametrize("mode", MODES)
@ends_at_a_fault
def test_regexes_end_to_end(words, mode):
    T, hip, want = words
    trees = findex_amd.ReTree.compile_batch(list(occ_ref.REGEXES))
    off, occ, truncated = hip.finditer(trees, mode=mode, max_steps=occ_ref.MAX_LEN)
    print(mode, np.diff(off).tolist())
    same((off, occ), want[mode])
    assert truncated                                         # b.*b is still alive at 12 bytes
    # the host form on the downloaded results: the same bytes; and again: the same bytes
    res, _ = findex_amd.ReTree.prepare_batch(hip, trees).match_raw(max_steps=occ_ref.MAX_LEN, cap=1 << 16)
    for _ in range(2):
        same(hip.occurrences(res, n_groups=len(occ_ref.REGEXES), mode=mode), want[mode])
    same(hip.finditer(list(occ_ref.REGEXES), mode=mode, max_steps=occ_ref.MAX_LEN)[:2], want[mode])
    same(hip.finditer(trees, mode=mode, max_steps=occ_ref.MAX_LEN, occ_cap=10)[:2], want[mode])      # too little room at first
    t = hip.occurrences_last()
    assert t[4] >= occ.size and all(x >= 0 for x in t[:4])


# ---------------------------------------------------------------- 2. tile edges, 3. key widths
N_A = 6000


@pytest.fixture(scope="module")
def run_of_a():
    hip = H.from_text(b"a" * N_A)
    aa, aaa = interval(hip, b"aa"), interval(hip, b"aaa")
    assert aa[1] - aa[0] == N_A - 1 and aaa[1] - aaa[0] == N_A - 2      # 11 997 rows: six scan tiles of 2048
    yield hip, aa, aaa
    hip.close()


def a_expect(mode, one_group):
    p2, p3 = np.arange(N_A - 1, dtype=np.uint64), np.arange(N_A - 2, dtype=np.uint64)
    if not one_group:
        if mode == "disjoint":
            p2, p3 = p2[::2], p3[::3]
            assert p2.size == 3000 and p3.size == 2000
        return [[(p2, 2)], [(p3, 3)]]
    if mode == "all":
        return [[(p2, 2), (p3, 3)]]
    if mode == "longest":
        return [[(p3, 3), (p2[-1:], 2)]]
    return [[(p3[::3], 3)]]


@pytest.mark.parametrize("one_group", (False, True))
@pytest.mark.parametrize("mode", MODES)
@ends_at_a_fault
def test_tile_edges(run_of_a, mode, one_group):
    hip, aa, aaa = run_of_a
    rec = H.pack_records([0, 0 if one_group else 1], [2, 3], [aa[0], aaa[0]], [aa[1], aaa[1]])
    want = closed_form(a_expect(mode, one_group))
    same(hip.occurrences(rec, n_groups=1 if one_group else 2, mode=mode), want)
    same(hip.occurrences(rec[::-1], n_groups=1 if one_group else 2, mode=mode), want)
    assert hip.occurrences_last()[4] == 2 * N_A - 3


@pytest.mark.parametrize("mode", MODES)
@ends_at_a_fault
def test_key_width_many_groups(run_of_a, mode):
    """Groups 0, 65535, 65536 and 70000 of 70001: the group takes 17 bits of the key, beside 13 of pos and 2 of len."""
    hip, aa, aaa = run_of_a
    groups = [0, 65535, 65536, 70000]
    rec = H.pack_records(groups, [2, 3, 2, 3], [aa[0], aaa[0]] * 2, [aa[1], aaa[1]] * 2)
    two = a_expect(mode, False)
    per = [[] for _ in range(70001)]
    for j, g in enumerate(groups):
        per[g] = two[j & 1]
    want = closed_form(per)
    same(hip.occurrences(rec, n_groups=70001, mode=mode), want)


@pytest.fixture(scope="module")
def big():
    """A text of 2^21 bytes: n takes 22 bits."""
    rng = np.random.Generator(np.random.PCG64(11))
    T = rng.choice(np.frombuffer(b"abcd\n", dtype=np.uint8), 1 << 21).tobytes()
    hip = H.from_text(T)
    yield T, hip
    hip.close()


def find_all(T, q):
    out, at = [], T.find(q)
    while at >= 0:
        out.append(at)
        at = T.find(q, at + 1)
    return np.array(out, dtype=np.uint64)


@ends_at_a_fault
def test_two_sort_form(big):
    """22 bits of pos, 16 of len (a record of 65535 bytes, with no rows) and 27 of group (n_groups = 2^26) are 65: the form
    with two stable sorts.  The expectation is bytes.find."""
    T, hip = big
    n_groups = 1 << 26
    qs = {0: (b"abcab", b"bca"), 12345678: (b"dd\nd",), n_groups - 1: (b"abcab", b"abcabd")}
    g, ln, sp, ep = [5], [65535], [7], [7]
    for grp, strings in qs.items():
        for q in strings:
            a, b = interval(hip, q)
            g, ln, sp, ep = g + [grp], ln + [len(q)], sp + [a], ep + [b]
    rec = H.pack_records(g, ln, sp, ep)
    off, occ = hip.occurrences(rec, n_groups=n_groups, mode="longest")
    want_off = np.zeros(n_groups + 1, dtype=np.uint64)
    parts = []
    for grp in sorted(qs):
        best = {}
        for q in qs[grp]:
            for p in find_all(T, q).tolist():
                best[p] = max(best.get(p, 0), len(q))
        part = np.zeros(len(best), dtype=OCC)
        part["group"], part["pos"], part["len"] = grp, sorted(best), [best[p] for p in sorted(best)]
        parts.append(part)
        want_off[grp + 1:] += np.uint64(len(best))
    want = np.concatenate(parts)
    want["doc"], want["raw_len"], want["raw_off"] = 0xFFFFFFFF, want["len"], want["pos"]
    assert want.size > 5000 and len(set(want[want["group"] == n_groups - 1]["len"].tolist())) == 2
    same((off, occ), (want_off, want))


# ---------------------------------------------------------------- 4. duplicates, empty records, max_per
@pytest.mark.parametrize("max_per", (None, 1, 3))
@pytest.mark.parametrize("mode", MODES)
@ends_at_a_fault
def test_duplicates_empty_records_and_max_per(words, mode, max_per):
    T, hip, _ = words
    sa = occ_ref.suffix_array(T)
    iv = {q: interval(hip, q) for q in (b"ab", b"abc", b"cab", b"b", b"aab", b"ca b", b"b\n")}
    recs = [(2, 3) + iv[b"cab"], (0, 2) + iv[b"ab"], (2, 1) + iv[b"b"], (0, 2) + iv[b"ab"], (4, 3, 9, 9), (0, 3) + iv[b"abc"],
            (1, 0) + iv[b"b"], (3, 4) + iv[b"ca b"], (2, 3) + iv[b"aab"], (3, 2) + iv[b"b\n"], (2, 3) + iv[b"cab"], (4, 2, 5, 5)]
    rec = np.array(recs, dtype=H.RESULT)
    want = occ_ref.from_records(T, sa, recs, mode, max_per, n_groups=6)
    assert want[0][2] == want[0][1] and want[0][5] == want[0][4] and want[1].size > (6 if max_per else 500)
    same(hip.occurrences(rec, n_groups=6, mode=mode, max_per=max_per), want)


# ---------------------------------------------------------------- 5. the corpus
DOCS = [b"abba\x00cab b", b"", b"ab\x01\xffabcab", b"b", b"cab\nab\xff"]


@pytest.fixture(scope="module")
def small_corpus():
    ref = corpus_ref.RefCorpus(DOCS)
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(DOCS))
    yield ref, cs
    cs.close()


@pytest.mark.parametrize("mode", MODES)
@ends_at_a_fault
def test_corpus_records(small_corpus, mode):
    ref, cs = small_corpus
    S, hip = ref.stream, cs.searcher
    sa = occ_ref.suffix_array(S)
    strings = [(0, b"b\x01"), (0, b"b"), (1, b"ab"), (1, b"b\x01\x01ab"), (1, b"a\\0c"), (1, b"b\\1\\fa"), (2, b"\x01b\x01"),
               (2, b"\\f"), (2, b"\\f\x01"), (0, b"bb")]
    recs = [(g, len(q)) + interval(hip, q) for g, q in strings]
    want = occ_ref.from_records(S, sa, recs, mode, docs=ref, n_groups=3)
    got = hip.occurrences(np.array(recs, dtype=H.RESULT), n_groups=3, mode=mode, corpus=cs.corpus)
    same(got, want)
    occ = got[1]
    # the record with the separator is dropped, the shorter one at its start survives
    ends = [p for p in range(len(S) - 1) if S[p:p + 2] == b"b\x01"]
    g0 = occ[int(got[0][0]):int(got[0][1])]
    assert len(ends) == 3 and all(int(o["len"]) == 1 for o in g0 if int(o["pos"]) in ends)
    assert not any(b"\x01" in S[int(o["pos"]):int(o["pos"] + o["len"])] for o in occ)
    # doc, raw_off and raw_len are the corpus map of both ends
    d0, _, r0 = cs.corpus.map(occ["pos"])
    d1, _, r1 = cs.corpus.map(occ["pos"] + occ["len"] - np.uint64(1))
    assert np.array_equal(occ["doc"], d0) and np.array_equal(d0, d1) and np.array_equal(occ["raw_off"], r0)
    assert np.array_equal(occ["raw_len"], r1 + np.uint64(1) - r0)
    # without the corpus nothing is dropped
    same(hip.occurrences(np.array(recs, dtype=H.RESULT), n_groups=3, mode=mode), occ_ref.from_records(S, sa, recs, mode, n_groups=3))


@pytest.mark.parametrize("mode", MODES)
@ends_at_a_fault
def test_corpus_grep(small_corpus, mode):
    ref, cs = small_corpus
    regexes = ("ab", "b.*b", "[a-c]+", "c(a|b)*")
    want = occ_ref.brute_csr(occ_ref.regex_tables(regexes), ref.stream, 8, mode, docs=ref)
    off, occ, truncated, texts = cs.grep(list(regexes), mode=mode, max_steps=8, text=True)
    same((off, occ), want)
    assert occ.size > 10 and texts == [DOCS[int(o["doc"])][int(o["raw_off"]):int(o["raw_off"] + o["raw_len"])] for o in occ]
    assert cs.grep(list(regexes), mode=mode, max_steps=8)[1].tobytes() == occ.tobytes()


@ends_at_a_fault
def test_directory_and_command_line(tmp_path, capfdbinary):
    from findex_amd import grep
    root = os.path.join(TESTDATA, "t1")
    ref = corpus_ref.RefCorpus.from_dir(root)
    corpus = findex_amd.Corpus.from_dir(root)
    bwt, eof, counts = findex_amd.bwt_from_text(ref.stream)
    findex_amd.write_bwt(tmp_path / "x.bwt", tmp_path / "x.aux", bwt, eof, counts)
    corpus.save(tmp_path / "x.docs")
    cs = findex_amd.HipCorpusSearcher(corpus)
    regexes = ("ab", "q(u|a)+", "x[a-c]y")
    tabs = occ_ref.regex_tables(regexes)
    for mode in MODES:
        want = occ_ref.brute_csr(tabs, ref.stream, 16, mode, docs=ref)
        off, occ, truncated = cs.grep(list(regexes), mode=mode, max_steps=16)
        same((off, occ), want)
        assert not truncated and all(c > 0 for c in np.diff(off).tolist())
    cs.close()
    capfdbinary.readouterr()
    assert grep.main([str(tmp_path / "x"), *regexes, "--count"]) == 0
    assert capfdbinary.readouterr().out.split() == [b"%d" % c for c in np.diff(want[0]).tolist()]
    assert grep.main([str(tmp_path / "x"), "x[a-c]y", "-C", "4"]) == 0
    lines = capfdbinary.readouterr().out.splitlines()
    sel = want[1][int(want[0][2]):]
    assert len(lines) == sel.size
    for line, o in zip(lines, sel):
        name, at, text = line.split(b":", 2)
        raw = ref.docs[ref.names.index(name)]
        a = int(at)
        assert a == int(o["raw_off"]) and text == raw[max(a - 4, 0):a + 3 + 4] and b"\n" not in text


# ---------------------------------------------------------------- 6. the routes that existed before
@ends_at_a_fault
def test_against_locate_text(words):
    T, hip, _ = words
    for q in (b"ab", b"cab", b"b\n", b" "):
        sp, ep = interval(hip, q)
        off, occ = hip.occurrences(H.pack_records(0, len(q), [sp], [ep]))
        assert off.tolist() == [0, ep - sp] and np.array_equal(occ["pos"], hip.locate_text(q))
        off, occ = hip.occurrences(H.pack_records(0, len(q), [sp], [ep]), mode="disjoint")
        assert occ.size == T.count(q)                       # bytes.count counts from the left without overlaps


@pytest.mark.parametrize("max_hits", (None, 2))
@ends_at_a_fault
def test_against_locate_docs_edits(small_corpus, max_hits):
    ref, cs = small_corpus
    for q, e in ((b"cab", 1), (b"ab\xff", 2), (b"abba", 1)):
        esc = findex_amd.escape(q)
        doc, raw, ln, _ = cs.locate_docs_edits(q, e, max_hits=max_hits)
        _, hits = cs.searcher.search_edit_batch(np.frombuffer(esc[::-1], dtype=np.uint8), np.array([0, len(esc)], dtype=np.uint64),
                                                e, sub=(2, 254))
        rec = H.pack_records(0, hits["len"], hits["sp"], hits["ep"])
        off, occ = cs.searcher.occurrences(rec, n_groups=1, mode="all", max_per=max_hits, corpus=cs.corpus)
        assert occ.size > 3 and occ.size == doc.size
        assert sorted(zip(occ["doc"].tolist(), occ["raw_off"].tolist(), occ["len"].tolist())) == list(zip(doc.tolist(), raw.tolist(), ln.tolist()))


# ---------------------------------------------------------------- 7. the contract
@ends_at_a_fault
def test_capacity_device_form_and_stream_capture(run_of_a):
    import torch
    hip, aa, aaa = run_of_a
    rec = H.pack_records([0, 1], [2, 3], [aa[0], aaa[0]], [aa[1], aaa[1]])
    want = closed_form(a_expect("disjoint", False))
    T = want[1].size
    d_rec = torch.from_numpy(rec.view(np.int64)).cuda()
    d_off = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    guard = 256
    d_out = torch.full((T * 32 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    assert hip.occurrences_dev(d_rec.data_ptr(), 2, 2, d_off.data_ptr(), 0, 0, mode="disjoint") == T       # the counting call
    assert (d_out.cpu().numpy() == 0xCD).all()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert hip.occurrences_dev(d_rec.data_ptr(), 2, 2, d_off.data_ptr(), d_out.data_ptr(), T, mode="disjoint",
                                   stream=st.cuda_stream) == T
    st.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:T * 32].tobytes() == want[1].tobytes() and (raw[T * 32:] == 0xCD).all()
    assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want[0])
    # too small: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrences_dev(d_rec.data_ptr(), 2, 2, d_off.data_ptr(), d_out.data_ptr(), T - 1, mode="disjoint")
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert raw[:(T - 1) * 32].tobytes() == want[1][:T - 1].tobytes() and (raw[(T - 1) * 32:] == 0xCD).all()
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrences(rec, n_groups=2, mode="disjoint", cap=T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    # a record of 65536 bytes: the device form finds it on the device, and nothing is reported
    bad = rec.copy()
    bad["len"][1] = 65536
    d_bad = torch.from_numpy(bad.view(np.int64)).cuda()
    d_off.fill_(7)
    d_out.fill_(0xCD)
    n_out = ctypes.c_size_t(77)
    opts = _lib.fmx_occ_opts(0, 0, 0)
    vp = ctypes.c_void_p
    assert _lib.load().fmx_occurrences_dev(hip.handle, None, vp(d_bad.data_ptr()), 2, 2, ctypes.byref(opts), vp(d_off.data_ptr()),
                                           vp(d_out.data_ptr()), T, ctypes.byref(n_out), None) == ARG
    torch.cuda.synchronize()
    assert n_out.value == 77 and d_off.cpu().tolist() == [7, 7, 7] and (d_out.cpu().numpy() == 0xCD).all()
    # under a stream capture the call is refused before it allocates or launches, and the capture goes on
    launches = hip.stats()["launches"]
    torch.cuda.empty_cache()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g.capture_begin()
        try:
            hip.occurrences_dev(d_rec.data_ptr(), 2, 2, d_off.data_ptr(), d_out.data_ptr(), T, stream=st.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        d_off.zero_()
        g.capture_end()
    assert err is not None and err.code == HIP and "stream capture" in str(err)
    d_off.fill_(7)
    g.replay()                                               # the capture is valid: its one node runs
    torch.cuda.synchronize()
    assert not d_off.cpu().numpy().any()
    del g
    assert hip.stats()["launches"] == launches


@ends_at_a_fault
def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = H.from_block(bwt, bs, 3)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrences(H.pack_records(0, 1, [0], [2]))
    assert ei.value.code == UNSUPPORTED
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrences_dev(0, 0, 1, 8, 0, 0)
    assert ei.value.code == UNSUPPORTED
    hip.close()


@ends_at_a_fault
def test_rows_overflow_allocates_nothing_row_sized(big):
    """2^17 records of 2^15 rows each are 2^32 rows: refused after the scan, before the 36 bytes per row are asked for."""
    import torch
    T, hip = big
    k = 1 << 17
    rec = H.pack_records(0, 1, np.ones(k, dtype=np.uint64), np.full(k, 1 + (1 << 15), dtype=np.uint64))
    hip.occurrences(rec[:4], n_groups=1, max_per=1)          # (the locate samples are built)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.occurrences(rec, n_groups=1)
    assert ei.value.code == OVERFLOW and "max_per" in str(ei.value) and str(1 << 32) in str(ei.value)
    assert abs(before - torch.cuda.mem_get_info()[0]) < (64 << 20)
    assert hip.occurrences_last()[4] == 1 << 32
    # with max_per the same records are 2^17 rows of one occurrence
    off, occ = hip.occurrences(rec, n_groups=1, max_per=1)
    assert off.tolist() == [0, 1] and int(occ["len"][0]) == 1 and hip.occurrences_last()[4] == k


@ends_at_a_fault
def test_the_locate_samples_are_built_once():
    hip = H.from_text(occ_ref.word_text())
    assert hip.locate_info()[1] == 0
    sp, ep = interval(hip, b"cab")
    rec = H.pack_records(0, 3, [sp], [ep])
    a = hip.occurrences(rec)
    rate, nbytes, ms = hip.locate_info()
    assert nbytes > 0
    same(hip.occurrences(rec), a)
    assert hip.locate_info() == (rate, nbytes, ms)
    hip.close()
