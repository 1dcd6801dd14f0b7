"""The search under string classes on the device (fmx_search_classes_batch) against tests/classes_ref.py, in both
layouts, offsets and record bytes exactly: every spelling of queries on a mixed-script text, members of 1 .. 4 bytes and classes
of 1, 2, 9 and 16 on synthetic BWTs around the block edges, the one-row rule (the EOF row, a row whose symbol ends no member,
members that share their last byte), a stack 254 deep and one with 15 pushes per element, batches of three times as many
patterns as a grid can have waves, capacity and determinism, the device form with its flags and a stream capture, all-literal
patterns against the exact search and a fold-map table against the fold search; then the layers above on a small corpus:
locate_docs, rank and rank_passages under ignore_case="unicode" against Python's re.IGNORECASE.  Where a test passes `steps`,
the backward steps fmx_classes_last reports are held to classes_ref.walk -- never to a count read off the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import approx_ref
import classes_ref as C
import corpus_ref
import findex_amd
import fold_ref
import oracle
import rank_ref
import words_ref
from conftest import TESTDATA
from findex_amd import _lib, unicode_fold
from helpers import bwt_of_text, ends_at_a_fault, pack_patterns, synth_bwt
from test_classes_cpu import SYNTH_TABLE, golden_patterns, golden_text, synth_patterns

pytestmark = pytest.mark.gpu

LAYOUTS = ["onehot", "bytes"]
REC = findex_amd.HipFMSearcher.RESULT
ARG, HIP, UNSUPPORTED, OVERFLOW = 3, 5, 6, 9


def waves_max():
    """More waves than a launch of k_classes can have resident: a CU holds at most 2048 threads, 8 workgroups of 256, four
    waves each.  An upper bound, not the occupancy query the library makes."""
    import torch
    return 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count


def open_index(index, layout):
    findex_amd.set_layout(layout)
    try:
        return findex_amd.HipFMSearcher.from_mem(*index)
    finally:
        findex_amd.set_layout("auto")


def open_text(s, layout):
    return open_index(bwt_of_text(s), layout)


def expected_arrays(per_pattern):
    off, rows = C.expected_csr(per_pattern)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=REC) if rows else np.zeros(0, dtype=REC)


def check(hip, pats, table, per_pattern, what=None, steps=None):
    """One batch against its expectation, per-pattern lists of (len, sp, ep); with `steps`, the backward steps
    classes_ref.walk makes for the batch, also what fmx_classes_last reports of the call and what each of its two launches
    adds to the handle."""
    el, off = C.pack(pats)
    st0 = hip.stats()
    got_off, got = hip.search_classes_batch(el, off, C.abi(table))
    st1 = hip.stats()
    exp_off, exp = expected_arrays(per_pattern)
    assert np.array_equal(got_off, exp_off), what
    assert got.tobytes() == exp.tobytes(), what
    assert st1["patterns_seen"] == st0["patterns_seen"] and st1["tables_held_bytes"] == st0["tables_held_bytes"]
    if steps is not None:
        _, _, got_steps, requests = hip.classes_last()
        print("%s: %d hits, %d steps (walk: %d), %d requests" % (what, got.size, got_steps, steps, requests))
        assert got_steps == steps, (what, got_steps, steps)
        assert requests <= 4 * steps, (what, requests, steps)
        launches = st1["launches"] - st0["launches"]         # the counting call, and the call that fetched the hits if any
        assert launches == (2 if got.size else 1), what
        assert st1["backward_steps"] - st0["backward_steps"] == launches * steps, what


def walks(orc, pats, table, deaths=None):
    """(per-pattern hits, total steps, deepest stack) of classes_ref.walk, the hits held to dfs_hits on the way."""
    full, total, deepest = [], 0, 0
    for p in pats:
        hits, steps, depth = C.walk(orc, p, table, deaths)
        assert hits == C.dfs_hits(orc, p, table), p
        full.append(hits)
        total += steps
        deepest = max(deepest, depth)
    return full, total, deepest


# ---------------------------------------------------------------- every spelling on the mixed-script text
@pytest.fixture(scope="module")
def golden():
    """The golden text as an index holds it for text queries (reversed), queries of 0 .. 24 code points in several spellings,
    their table from unicode_fold.class_table, and the expectations."""
    text = golden_text()
    rev = text[::-1]
    orc = approx_ref.index_of(rev)[0]
    queries = golden_patterns(text, np.random.default_rng(303), per_len=2)
    el, off, cls_off, mem_off, mem_bytes = unicode_fold.class_table(queries)
    table, pats = C.table_of(cls_off, mem_off, mem_bytes), C.unpack(el, off)
    full, steps, depth = walks(orc, pats, table)
    return text, rev, queries, table, pats, full, steps


def test_golden_expectations_are_the_ones_the_kernel_needs(golden):
    text, rev, queries, table, pats, full, steps = golden
    per = [len(h) for h in full]
    print("golden: %d patterns, %d classes, %d hits, most of one pattern %d, %d steps" % (len(pats), len(table), sum(per), max(per), steps))
    assert max(len(p) for p in pats) >= 24 and min(len(p) for p in pats) == 0
    assert sum(1 for n in per if n >= 2) >= 40 and sum(1 for n in per if n == 0) >= 4
    assert sum(1 for h in full if len({x[0] for x in h}) >= 2) >= 6                     # spellings of different lengths
    assert {len(m) for cl in table for m in cl} == {1, 2, 3}
    for p, h in zip(pats[::5], full[::5]):                                             # the sliding window sees the same
        assert C.window_hits(rev, p, table) == h, p


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_spellings_on_the_golden_text(golden, layout):
    text, rev, queries, table, pats, full, steps = golden
    hip = open_text(rev, layout)
    check(hip, pats, table, full, what="golden", steps=steps)
    # one pattern at a time, the empty pattern, no table at all
    assert hip.search_classes([], None) == [(0, 0, len(text) + 1)]
    j = max(range(len(pats)), key=lambda j: len(full[j]))
    assert hip.search_classes(pats[j], C.abi(table)) == sorted(full[j], key=lambda h: h[1])
    # the pruned table of the index finds the same, and positions in the text are re.IGNORECASE's
    s = text.decode("utf-8")
    for q in ("kelvin", "MISS", "σοφίας", "über", "ıki", "ångström", "zebra"):
        el, off, tab = hip.unicode_table([q.encode()])
        _, hits = hip.search_classes_batch(el, off, tab)
        e2, o2, c2, m2, b2 = unicode_fold.class_table([q.encode()])
        _, all_hits = hip.search_classes_batch(e2, o2, (c2, m2, b2))
        assert hits.tobytes() == all_hits.tobytes(), q
        at, lens = hip.locate_classes(q.encode())
        want = [(len(s[:m.start()].encode()), len(m.group(1).encode())) for m in re.finditer("(?=(" + re.escape(q) + "))", s, re.IGNORECASE)]
        assert list(zip(at.tolist(), lens.tolist())) == sorted(want), q
    assert hip.locate_classes(b"kelvin")[1].max() == 8 and hip.locate_classes(b"kelvin", max_hits=3)[0].size == 3
    hip.close()


# ---------------------------------------------------------------- member shapes and class sizes on synthetic BWTs
def synth_shapes():
    for sizes in ((447, 448, 449), (127, 128, 129)):
        for n in sizes:
            for eof in (0, n // 2, n - 1):
                yield n, eof


@pytest.fixture(scope="module")
def synth():
    out = []
    deaths = {}
    for n, eof in synth_shapes():
        index = synth_bwt(n, 97, 112, seed=n, eof=eof)
        orc = oracle.NaiveFMSearcher.from_mem(*index)
        rng = np.random.default_rng(n + eof)
        pats = [p for m in (1, 2, 3, 5) for p in synth_patterns(orc, rng, SYNTH_TABLE, 8, m)]
        pats += [[256 + c] for c in range(len(SYNTH_TABLE))] + [[261, 261], [256, 257], [257, 0], [260, 258, 259]]
        full, steps, depth = walks(orc, pats, SYNTH_TABLE, deaths)
        out.append((index, (n, eof), pats, full, steps))
    # ... and a text made of the members themselves, in which the members of 3 and 4 bytes go through
    rng = np.random.default_rng(308)
    parts = [m for cl in SYNTH_TABLE for m in cl]
    s = b"".join(parts[int(j)] for j in rng.integers(0, len(parts), 160))
    orc = approx_ref.index_of(s)[0]
    pats = [[256 + c] for c in range(len(SYNTH_TABLE))] + [[256, 256], [262, 256], [257, 262, 256], [256, 257, 258, 259]]
    full, steps, depth = walks(orc, pats, SYNTH_TABLE, deaths)
    out.append((bwt_of_text(s), ("members", len(s)), pats, full, steps))
    print("synthetic: members of branching nodes by (bytes, step they died at; 0: went through):", sorted(deaths.items()))
    # a member of every length dies at each of its steps, and one of every length goes through
    assert all(deaths.get((ln, j), 0) > 0 for ln in (1, 2, 3, 4) for j in range(ln + 1)), sorted(deaths.items())
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_member_shapes_and_class_sizes_on_synthetic_bwts(synth, layout):
    found = most = 0
    sizes = set()
    for index, shape, pats, full, steps in synth:
        hip = open_index(index, layout)
        check(hip, pats, SYNTH_TABLE, full, what=shape, steps=steps)
        found += sum(len(h) for h in full)
        most = max(most, max(len(h) for h in full))
        for c in range(len(SYNTH_TABLE)):
            sizes.add((len(SYNTH_TABLE[c]), len(full[pats.index([256 + c])])))
        hip.close()
    print("synthetic: %d hits, most of one pattern %d, (class size, members that occur) %s" % (found, most, sorted(sizes)))
    assert found > 3000 and most >= 100
    assert {(1, 1), (2, 2), (9, 9), (16, 16)} <= sizes and any(s == 4 and 2 <= o for s, o in sizes)


# ---------------------------------------------------------------- the one-row rule
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_one_row_rule(golden, layout):
    """A class in front of a string that has one row.  On the EOF row (the whole text) BWT' is 0, which ends no member: the node
    dies without a step.  On another row only the members that end with the row's symbol are stepped: none -- no step; two
    that share it (and a two-byte suffix) -- both, to their first empty interval."""
    text, rev = golden[0], golden[1]
    orc = approx_ref.index_of(rev)[0]
    m = 30
    whole = rev[:m]
    assert C.dfs_hits(orc, C.literals(whole), []) == [(m, orc.eof, orc.eof + 1)]
    at = 40
    inner = rev[at:at + m]
    row = C.dfs_hits(orc, C.literals(inner), [])
    assert len(row) == 1 and row[0][2] - row[0][1] == 1
    x, xy, xyz = rev[at - 1:at], rev[at - 2:at], rev[at - 3:at]
    other = bytes([xy[0] ^ 1]) + x
    far = bytes([xyz[0] ^ 1]) + xy
    assert len({x, xy, xyz, other, far}) == 5 and 0 not in other + far
    table = [[b"q", b"Qz"],                                  # ends with neither symbol
             [xyz, far, b"q"],                               # two members share the row's symbol and a two-byte suffix; one occurs
             [xy, other]]                                    # ... share the symbol alone
    pats = [C.literals(whole), [256] + C.literals(whole), [257] + C.literals(whole),
            C.literals(inner), [256] + C.literals(inner), [257] + C.literals(inner), [258] + C.literals(inner), [258, 257] + C.literals(inner)]
    w = [C.walk(orc, p, table) for p in pats]
    assert w[1][1] == w[2][1] == w[0][1] and not w[1][0] and not w[2][0]               # the EOF row: no step
    assert w[4][1] == w[3][1] and not w[4][0]                                          # no member ends with the row's symbol: no step
    assert w[5][1] == w[3][1] + 3 + 3 and [h[0] for h in w[5][0]] == [m + 3]            # xyz goes through, far dies at its last step; q is not tried
    assert w[6][1] == w[3][1] + 2 + 2 and [h[0] for h in w[6][0]] == [m + 2]
    full = [h for h, _, _ in w]
    assert full == [C.dfs_hits(orc, p, table) for p in pats]
    hip = open_text(rev, layout)
    check(hip, pats, table, full, what="one row", steps=sum(s for _, s, _ in w))
    hip.close()


# ---------------------------------------------------------------- the stack
@pytest.fixture(scope="module")
def deep():
    """tests/test_gpu_fold.py's text for a pattern of 255 capitals: at every level the capital goes on and the lower-case
    sibling waits on the stack until the whole pattern is through -- 254 entries.  And a text over a .. p in which every
    pair occurs, for a class of 16: 15 pushes per element."""
    rng = np.random.default_rng(283)
    P = bytes(rng.integers(65, 91, 255, dtype=np.uint8))
    s = b"#".join(bytes([P[254 - j] + 32]) + P[255 - j:] for j in range(1, 255))
    table, cid = C.fold_table(fold_ref.ASCII)
    pats = [C.folded(P, cid), C.folded(P.lower(), cid), C.literals(P)]
    full, steps, depth = walks(approx_ref.index_of(s)[0], pats, table)
    assert depth >= 254
    s16 = bytes(np.random.default_rng(304).integers(97, 113, 4096, dtype=np.uint8))
    t16 = [[bytes([c]) for c in range(97, 113)]]
    p16 = [[256, 256], [256, 256, 256], [256]]
    full16, steps16, depth16 = walks(approx_ref.index_of(s16)[0], p16, t16)
    assert 30 <= depth16 <= 45 and len(full16[0]) == 256 and len(full16[1]) > 2000     # [256, 256]: 15 pushes per element
    return (s, table, pats, full, steps), (s16, t16, p16, full16, steps16)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_deep_and_wide_stacks(deep, layout):
    for s, table, pats, full, steps in deep:
        hip = open_text(s, layout)
        check(hip, pats, table, full, what="stack", steps=steps)
        batch = [pats[1], [97, 98], pats[0], [], pats[1]] * 3                          # a full stack next to short patterns in one wave's loop
        orc = approx_ref.index_of(s)[0]
        check(hip, batch, table, [C.dfs_hits(orc, p, table) for p in batch], what="stack, mixed")
        hip.close()


# ---------------------------------------------------------------- several patterns per wave
@pytest.fixture(scope="module")
def many(golden):
    """k = 3 * waves_max() + 5 patterns drawn with repetition from the golden batch: ragged lengths, the empty pattern,
    patterns without a hit, patterns with several spellings."""
    text, rev, queries, table, pats, full, _ = golden
    orc = approx_ref.index_of(rev)[0]
    steps = np.array([C.walk(orc, p, table)[1] for p in pats])
    k = 3 * waves_max() + 5
    return rev, table, pats, full, steps, np.random.default_rng(305).integers(0, len(pats), k)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_several_patterns_per_wave(many, layout):
    rev, table, pool, hits, steps, idx = many
    assert idx.size >= 3 * waves_max() and idx.size % 4 != 0
    pats = [pool[j] for j in idx.tolist()]
    exp_off, exp = expected_arrays([hits[j] for j in idx.tolist()])
    print("several patterns per wave: k = %d, %d hits" % (idx.size, exp.size))
    assert exp.size > 20_000
    hip = open_text(rev, layout)
    el, off = C.pack(pats)
    st0 = hip.stats()
    got_off, got = hip.search_classes_batch(el, off, C.abi(table))
    st1 = hip.stats()
    assert np.array_equal(got_off, exp_off)
    assert got.tobytes() == exp.tobytes()
    total = int(steps[idx].sum())
    assert hip.classes_last()[2] == total
    assert st1["launches"] == st0["launches"] + 2 and st1["backward_steps"] - st0["backward_steps"] == 2 * total
    hip.close()


# ---------------------------------------------------------------- capacity, order, determinism
def raw_call(L, hip, el, off, table, cap, guard=64):
    arrays = C.abi(table)
    tab = _lib.fmx_class_table()
    tab.cls_off, tab.mem_off, tab.mem_bytes = (a.ctypes.data for a in arrays)
    tab.n_classes = len(table)
    out = np.full((cap + guard) * REC.itemsize, 0xAB, dtype=np.uint8)
    out_off = np.zeros(off.size, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    rc = L.fmx_search_classes_batch(hip.handle, el.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(tab), out_off.ctypes.data,
                                    out.ctypes.data if cap else None, cap, ctypes.byref(n_out))
    assert (out[cap * REC.itemsize:] == 0xAB).all()          # nothing behind out[cap - 1]
    return rc, int(n_out.value), out_off, out[: cap * REC.itemsize].view(REC)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_capacity_order_and_determinism(golden, layout):
    text, rev, queries, table, pats, full, _ = golden
    exp_off, exp = expected_arrays(full)
    T = exp.size
    assert T > 200
    hip = open_text(rev, layout)
    el, off = C.pack(pats)
    L = _lib.load()
    rc, n, o, h = raw_call(L, hip, el, off, table, T)
    assert rc == 0 and n == T and np.array_equal(o, exp_off) and h.tobytes() == exp.tobytes()
    for cap in (T - 1, 1, 0):                                # one short; the counting call
        rc, n, _, _ = raw_call(L, hip, el, off, table, cap)
        assert rc == OVERFLOW and n == T, cap
        assert str(T).encode() in L.fmx_last_error()
    rc, n2, o2, h2 = raw_call(L, hip, el, off, table, n)     # the retry at n_out
    assert rc == 0 and n2 == T and h2.tobytes() == h.tobytes() and np.array_equal(o2, o)   # two calls, identical bytes
    rc, n3, o3, h3 = raw_call(L, hip, el, off, table, T + 1000)
    assert rc == 0 and n3 == T and h3[:T].tobytes() == h.tobytes()
    seg = np.repeat(np.arange(len(pats)), np.diff(o.astype(np.int64)))
    assert np.array_equal(h["regex"], seg)
    same = seg[1:] == seg[:-1]
    assert (h["sp"][1:][same] >= h["ep"][:-1][same]).all() and (h["sp"] < h["ep"]).all()      # disjoint, ascending
    hip.close()


# ---------------------------------------------------------------- the device form
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_flags_and_stream_capture(golden, layout):
    import torch
    text, rev, queries, table, pats, full, _ = golden
    hip = open_text(rev, layout)
    el, off = C.pack(pats)
    tab = C.abi(table)
    h_off, h_hits = expected_arrays(full)
    T, k = h_hits.size, len(pats)
    d_el = torch.from_numpy(el.view(np.int16)).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * REC.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        n = hip.search_classes_batch_dev(d_el.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T, tab, stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * REC.itemsize].tobytes() == h_hits.tobytes() and (raw[T * REC.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), h_off)
    # too small: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_classes_batch_dev(d_el.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T - 1, tab)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy()[(T - 1) * REC.itemsize:] == 0xCD).all()
    # a pattern of 256 elements: the host form refuses it before the device, the device form's kernel skips it and raises its
    # flag; so with an element that names a class the table does not have
    for bad, word in (([97] * 256, "255"), ([97, 256 + len(table)], "not in the table")):
        lel, loff = C.pack([pats[4], bad, [97] * 255])
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.search_classes_batch(lel, loff, tab)
        assert ei.value.code == ARG
        d_lel = torch.from_numpy(lel.view(np.int16)).cuda()
        d_loff = torch.from_numpy(loff.view(np.int64)).cuda()
        with pytest.raises(findex_amd.FmxError) as ei:
            hip.search_classes_batch_dev(d_lel.data_ptr(), d_loff.data_ptr(), 3, d_out_off.data_ptr(), d_out.data_ptr(), T, tab)
        assert ei.value.code == ARG and word in str(ei.value)
        torch.cuda.synchronize()
    # under a stream capture the call is refused before it allocates or launches, and the capture goes on
    launches = hip.stats()["launches"]
    torch.cuda.empty_cache()
    g = torch.cuda.CUDAGraph()
    err = None
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g.capture_begin()
        try:
            hip.search_classes_batch_dev(d_el.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T, tab, stream=st.cuda_stream)
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


@ends_at_a_fault
def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_classes([97, 98], None)
    assert ei.value.code == UNSUPPORTED
    hip.close()


# ---------------------------------------------------------------- against the exact search and the fold search
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_all_literal_patterns_are_the_exact_search(golden, layout):
    text, rev = golden[0], golden[1]
    rng = np.random.default_rng(306)
    pats = [b"", b"#", b"\0", rev[:40], rev[-9:] + b"\0"]
    for m in (1, 3, 8, 20, 60):
        for at in rng.integers(0, 4000, 8).tolist():
            pats += [rev[at:at + m], rev[at:at + m].swapcase()]
    hip = open_text(rev, layout)
    hip.config_set("jump", "off")
    hip.config_set("ktab", "off")
    buf, off = pack_patterns(pats)
    hip.stats_reset()
    sp, ep = hip.search_batch(buf, off)
    exact_steps = hip.stats()["backward_steps"]
    orc = approx_ref.index_of(rev)[0]
    assert exact_steps == int(orc.search_batch(buf, off)[2].sum())
    found = sp < ep
    got_off, got = hip.search_classes_batch(buf.astype(np.uint16), off, C.abi(SYNTH_TABLE))      # a table no element uses
    assert np.array_equal(np.diff(got_off.astype(np.int64)), found.astype(np.int64))
    assert np.array_equal(got["regex"], np.nonzero(found)[0])
    assert np.array_equal(got["len"], np.array([len(p) for p in pats])[found])
    assert np.array_equal(got["sp"], sp[found]) and np.array_equal(got["ep"], ep[found])
    assert hip.classes_last()[2] == exact_steps              # the one relation DESIGN.md 30 holds the kernel to
    hip.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_fold_map_table_is_the_fold_search(layout):
    with open(os.path.join(TESTDATA, "test3072.txt"), "rb") as f:
        s = fold_ref.mixed_case(f.read())
    rng = np.random.default_rng(307)
    general = fold_ref.make_map([b"abcdefgh", b"ij", b"xyz", b"TU"])
    pats = [b"", b"#", b"\0"]
    for m in (1, 2, 5, 12, 24):
        for at in rng.integers(0, len(s) - m, 12).tolist():
            pats += [s[at:at + m], s[at:at + m].swapcase()]
    buf, off = pack_patterns(pats)
    hip = open_text(s, layout)
    for fold in (fold_ref.ASCII, general):
        cid, cls_off, mem_off, mem_bytes = unicode_fold.fold_map_table(fold)
        el = np.array([c if cid[c] < 0 else 256 + cid[c] for c in buf.tolist()], dtype=np.uint16)
        want_off, want = hip.search_fold_batch(buf, off, fold)
        got_off, got = hip.search_classes_batch(el, off, (cls_off, mem_off, mem_bytes))
        assert want.size > 100 and np.array_equal(got_off, want_off) and got.tobytes() == want.tobytes()
    hip.close()


# ---------------------------------------------------------------- end to end on a small corpus
DOCS = ["Über den Wolken. über uns, ÜBER ALLES",
        "σοφία και λόγος. ΣΟΦΙΑ! Ο ΛΌΓΟΣ, ο λόγος των λόγων",
        "The Kelvin scale: 273 K, kelvin, \u212aelvin. MISS mi\u017fs miss",   # the Kelvin sign, the long s
        "ışık IŞIK isik; café CAFÉ cafe Café",
        "nothing of the kind here",
        "Ångström ångström ÅNGSTRÖM; uber Uber UBER",
        "kelvin kelvin kelvin KELVIN"]


@pytest.fixture(scope="module")
def files():
    docs = [d.encode("utf-8") for d in DOCS]
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    yield cs, rank_ref.RankRef(corpus_ref.RefCorpus(docs))
    cs.close()


def re_starts(q, flags=re.IGNORECASE):
    """[(doc, byte offset, bytes)] of the occurrences of q in DOCS, overlapping ones included, as Python's re finds them."""
    out = []
    for d, s in enumerate(DOCS):
        for m in re.finditer("(?=(" + re.escape(q) + "))", s, flags):
            out.append((d, len(s[:m.start()].encode()), len(m.group(1).encode())))
    return sorted(out)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


@ends_at_a_fault
def test_locate_docs_unicode(files):
    cs, _ = files
    for q in ("über", "ÜBER", "kelvin", "miss", "λόγοσ", "ΣΟΦΊΑ", "ışık", "ISIK", "café", "ångström", "zebra", "e"):
        doc, raw, lens = cs.locate_docs(q.encode(), ignore_case="unicode")
        assert list(zip(doc.tolist(), raw.tolist(), lens.tolist())) == re_starts(q), q
    assert len(re_starts("kelvin")) == 7 and {n for _, _, n in re_starts("kelvin")} == {6, 8}
    assert len(re_starts("über")) == 3 and len(re_starts("λόγοσ")) == 3 and len(re_starts("ISIK")) == 1
    # ASCII folding finds less: the status quo that ignore_case=True keeps
    assert cs.locate_docs("über".encode(), ignore_case=True)[0].size == 1
    # precomposed accented forms of a letter
    doc, raw, lens = cs.locate_docs(b"cafe", ignore_case="unicode", ignore_marks=True)
    assert doc.tolist() == [3, 3, 3, 3] and sorted(lens.tolist()) == [4, 5, 5, 5]
    doc, _, _ = cs.locate_docs(b"uber", ignore_case="unicode", ignore_marks=True)
    assert doc.tolist() == [0, 0, 0, 5, 5, 5]
    assert cs.locate_docs(b"kelvin", ignore_case="unicode", max_hits=2)[0].size == 2
    with pytest.raises(ValueError):
        cs.locate_docs(b"the", ignore_case="unicode", max_mismatches=1)
    with pytest.raises(ValueError):
        cs.locate_docs(b"the", ignore_marks=True)


@ends_at_a_fault
def test_rank_unicode_against_re(files):
    """rank(ignore_case="unicode") bit for bit against tests/rank_ref.py with the term counts taken by re.IGNORECASE on str."""
    cs, rr = files
    queries = [["über"], ["kelvin", "miss"], ["λόγοσ", "ΣΟΦΊΑ", "café"], ["ışık", "zebra"], ["e"], [], ["ångström", "UBER"]]
    post = []
    for q in queries:
        for t in q:
            tf = {}
            for d, _, _ in re_starts(t):
                tf[d] = tf.get(d, 0) + 1
            post.append(tf)
    raw = [[t.encode() for t in q] for q in queries]
    for match in ("any", "all"):
        off, doc, score, df, w = cs.rank(raw, top=5, match=match, ignore_case="unicode")
        assert df.tolist() == [len(p) for p in post]
        for got, want in zip(w.tolist(), rr.weights(post)):
            assert abs(got - want) <= 1e-12 * abs(want)
        eo, ed, es = rr.rank([len(q) for q in queries], post, w.tolist(), top=5, match=match)
        assert off.tolist() == eo and doc.tolist() == ed and bits(score) == bits(es)
    exact = cs.rank(raw, top=5)
    ascii_ = cs.rank(raw, top=5, ignore_case=True)
    docs = [d.encode("utf-8") for d in DOCS]                                           # on bytes re.IGNORECASE folds A..Z alone
    terms = [t for q in raw for t in q]
    assert ascii_[3].tolist() == [sum(1 for d in docs if re.search(re.escape(t), d, re.IGNORECASE)) for t in terms]
    assert exact[3].tolist() == [sum(1 for d in docs if t in d) for t in terms]
    assert (df >= ascii_[3]).all() and (ascii_[3] >= exact[3]).all() and df.sum() > ascii_[3].sum()
    assert df[terms.index("ΣΟΦΊΑ".encode())] == 1 and ascii_[3][terms.index("ΣΟΦΊΑ".encode())] == 0      # the ASCII map does not reach Greek
    assert [n for n, _ in cs.rank_files([b"KELVIN"], top=3, ignore_case="unicode")] == [n for n, _ in cs.rank_files([b"kelvin"], top=3, ignore_case="unicode")]
    # accented forms
    _, doc, _, df, _ = cs.rank([[b"cafe"]], ignore_case="unicode", ignore_marks=True)
    assert df.tolist() == [1] and doc.tolist() == [3]


@ends_at_a_fault
def test_rank_passages_unicode(files):
    """One length per term: allowed where every spelling of a term has the same number of bytes, refused with the term and
    two lengths otherwise."""
    cs, _ = files
    q = [["über".encode(), "café".encode()]]
    off, doc, score, df, w, psg, tf = cs.rank_passages(q, top=3, window=40, ignore_case="unicode")
    r_off, r_doc, r_score, _, _ = cs.rank(q, top=3, ignore_case="unicode")
    assert doc.tolist() == r_doc.tolist() and bits(score) == bits(r_score) and sorted(doc.tolist()) == [0, 3]
    by_doc = {int(d): row for d, row in zip(doc, tf.tolist())}
    assert by_doc[0] == [3, 0] and by_doc[3] == [0, 3]                                 # the counts of every spelling
    assert all(int(p["n_occ"]) >= 1 for p in psg)
    with pytest.raises(ValueError) as ei:
        cs.rank_passages([[b"kelvin"]], ignore_case="unicode")
    assert "kelvin" in str(ei.value) and "6" in str(ei.value) and "8" in str(ei.value)
    cs.rank([[b"kelvin"]], ignore_case="unicode")                                      # the ranking alone takes it


class _Stdout:
    """sys.stdout for a command line's main(): its bytes are kept."""

    def __init__(self):
        import io
        self.buffer = io.BytesIO()

    def write(self, text):
        self.buffer.write(text.encode())

    def flush(self):
        pass


@ends_at_a_fault
def test_rank_command_line(tmp_path, monkeypatch):
    """rank --unicode-case [--ignore-marks] against re on DOCS as a directory; the mains run in this process."""
    import sys
    from findex_amd import index as index_cli, rank as rank_cli
    root = tmp_path / "d"
    root.mkdir()
    for j, d in enumerate(DOCS):
        (root / ("f%d.txt" % j)).write_bytes(d.encode("utf-8"))
    base = str(tmp_path / "x")

    def run(cli, *args):
        out = _Stdout()
        monkeypatch.setattr(sys, "stdout", out)
        try:
            assert cli.main(list(args)) == 0
        finally:
            monkeypatch.undo()
        return out.buffer.getvalue().split(b"\n")[:-1]

    def holding(q):
        return sorted({b"f%d.txt" % d for d, _, _ in re_starts(q)})

    run(index_cli, "--dir", str(root), "--out", base)
    names = lambda rows: sorted(ln.split(b"\t")[1] for ln in rows)
    assert names(run(rank_cli, base, "über", "--unicode-case")) == holding("über") == [b"f0.txt"]
    assert names(run(rank_cli, base, "KELVIN", "--unicode-case")) == holding("kelvin") == [b"f2.txt", b"f6.txt"]
    assert names(run(rank_cli, base, "λόγοσ", "--unicode-case")) == [b"f1.txt"]
    assert names(run(rank_cli, base, "uber", "--unicode-case")) == [b"f5.txt"]
    assert names(run(rank_cli, base, "uber", "--unicode-case", "--ignore-marks")) == [b"f0.txt", b"f5.txt"]
    assert names(run(rank_cli, base, "UBER", "--unicode-case", "-w")) == [b"f5.txt"]
    assert names(run(rank_cli, base, "BER", "--unicode-case")) == [b"f0.txt", b"f5.txt"] and not run(rank_cli, base, "BER", "--unicode-case", "-w")
    assert names(run(rank_cli, base, "KELVIN", "-i")) == [b"f2.txt", b"f6.txt"] and names(run(rank_cli, base, "ÜBER", "-i")) == [b"f0.txt"]      # -i stays ASCII
    assert run(rank_cli, base, "über", "-i") != run(rank_cli, base, "über", "--unicode-case")      # ... one spelling against three


# ---------------------------------------------------------------- whole words on top
def variants(q, classes):
    """Every spelling of the text string q (bytes, read as UTF-8) under a mapping code point -> members."""
    import itertools
    parts = [[chr(m).encode("utf-8") for m in classes[cp]] if cp in classes else [raw] for cp, raw in unicode_fold.tokens(q)]
    return [b"".join(v) for v in itertools.product(*parts)]


# space and hyphen in one class (both boundary bytes), k with the hyphen (a word byte with a boundary byte), on top of the case classes
def odd_classes():
    classes = dict(unicode_fold.case_classes())
    classes[0x20] = classes[0x2D] = (0x20, 0x2D)
    return classes


WORD_QUERIES = ["über", "kelvin", "miss", "the", "STOP", "ok", "σοφία", "λόγοσ", "iki", "zebra", "ber", "elvin", "o"]
_word_refs = {}


@pytest.fixture(scope="module", params=LAYOUTS)
def words_world(request, golden):
    text = golden[0]
    if "ref" not in _word_refs:                              # one checker for both layouts, left unchanged
        _word_refs["ref"] = words_ref.SuffixRef(text)
    ref = _word_refs["ref"]
    findex_amd.set_layout(request.param)
    try:
        hip = findex_amd.HipFMSearcher.from_text(text)
    finally:
        findex_amd.set_layout("auto")
    assert hip.n == ref.n
    yield hip, ref, text
    hip.close()


def rows_of(off, runs, j):
    mine = runs[int(off[j]):int(off[j + 1])]
    return [(r, int(n)) for a, b, n in zip(mine["sp"].tolist(), mine["ep"].tolist(), mine["len"].tolist()) for r in range(a, b)]


@ends_at_a_fault
def test_context_and_classes(words_world):
    """fmx_search_context_classes_batch against tests/words_ref.py: per query the rows of every spelling that stand as whole
    words, each with the bytes of its spelling; a class that holds boundary bytes folds INSIDE a pattern while the step with the
    left neighbour stays exact."""
    hip, ref, text = words_world
    B = words_ref.BOUNDARY
    classes = unicode_fold.case_classes()
    pats = [q.encode("utf-8") for q in WORD_QUERIES]
    off, runs = hip.search_words(pats, classes="unicode")
    assert off.size == len(pats) + 1
    found = 0
    for i, q in enumerate(pats):
        mine = runs[int(off[i]):int(off[i + 1])]
        assert (mine["regex"] == i).all()
        sp, ep = mine["sp"].tolist(), mine["ep"].tolist()
        assert all(a < b for a, b in zip(sp, ep)) and all(b <= a for b, a in zip(ep, sp[1:]))      # ascending, disjoint
        want = sorted((r, len(v)) for v in variants(q, classes) for r in ref.context_rows(v, B, B))
        assert rows_of(off, runs, i) == want, q
        starts = sorted((p, len(v)) for v in variants(q, classes) for p in words_ref.literal_word_starts(text, v))
        at, lens = hip.locate_words(q, classes="unicode")
        assert list(zip(at.tolist(), lens.tolist())) == starts, q
        found += len(want)
    assert found > 100
    kel = pats.index(b"kelvin")
    assert {n for _, n in rows_of(off, runs, kel)} == {6, 8}                             # the Kelvin sign's spelling is two bytes longer
    for q in ("zebra", "ber", "elvin"):                                                # occur, if at all, never as words
        j = WORD_QUERIES.index(q)
        assert int(off[j]) == int(off[j + 1])
    assert hip.locate_classes(b"ber")[0].size > 0
    # bit 0 of left cleared: the occurrence at offset 0 goes
    first = text.split(b" ")[0]
    el, el_off, table = hip.unicode_table([first])
    no_start = bytes(c for c in B if c != 0)
    o1, r1 = hip.search_context_batch(el, el_off, B, B, classes=table)
    o2, r2 = hip.search_context_batch(el, el_off, no_start, B, classes=table)
    row0 = ref.interval(first)[0] if len(ref.context_rows(first, B, B)) else None
    at0 = [r for r, _ in rows_of(o1, r1, 0) if r not in [x for x, _ in rows_of(o2, r2, 0)]]
    assert len(at0) == 1 and 0 in hip.locate_words(first, classes="unicode")[0].tolist()
    # boundary bytes in a class
    odd = odd_classes()
    j = text.find(b" - ")
    a = text.rfind(b" ", 0, j) + 1
    b = text.find(b" ", j + 3)
    phrase = text[a:b].rstrip(b",.;")                                                 # word - word
    assert phrase.count(b" - ") == 1
    for q in (phrase, phrase.replace(b" - ", b"---"), phrase.replace(b" - ", b"   ")):
        want = sorted((p, len(v)) for v in variants(q, odd) for p in words_ref.literal_word_starts(text, v))
        at, lens = hip.locate_words(q, classes=odd)
        assert want and list(zip(at.tolist(), lens.tolist())) == want, q
    # the left neighbour is compared as it is: "-word" under {space, hyphen} is no word "word" more than before
    w2 = phrase.split(b" - ")[1]
    assert hip.locate_words(w2, classes=odd)[0].tolist() == sorted(p for v in variants(w2, odd) for p in words_ref.literal_word_starts(text, v))
    o3, r3 = hip.search_words([b"zebra", b"qqq"], classes="unicode")                   # no spelling occurs: no record reaches the filter
    assert o3.tolist() == [0, 0, 0] and r3.size == 0


@ends_at_a_fault
def test_context_and_classes_device_form(words_world):
    """fmx_search_context_classes_batch_dev on a side stream: the host form's bytes, guard bytes behind the capacity, a capacity
    one short, and the refusal under a stream capture."""
    import torch
    from findex_amd.searcher import class_words
    hip, ref, text = words_world
    B = words_ref.BOUNDARY
    pats = [q.encode("utf-8") for q in WORD_QUERIES]
    el, el_off, table = hip.unicode_table(pats)
    h_off, h_runs = hip.search_context_batch(el, el_off, B, B, classes=table)
    T, k = h_runs.size, len(pats)
    assert T > 20
    opts = _lib.fmx_context_opts()
    for j, w in enumerate(class_words(B)):
        opts.left[j] = opts.right[j] = int(w)
    tab, keep = hip._class_table(table)
    entry = hip._L.fmx_search_context_classes_batch_dev
    d_el = torch.from_numpy(np.ascontiguousarray(el).view(np.int16)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(el_off).view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * REC.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")

    def call(cap, stream=0):
        n_out = ctypes.c_size_t(0)
        rc = entry(hip._h, ctypes.c_void_p(d_el.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), k, ctypes.byref(opts), ctypes.byref(tab),
                   ctypes.c_void_p(d_out_off.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.byref(n_out), ctypes.c_void_p(stream))
        return rc, int(n_out.value), (hip._L.fmx_last_error() or b"").decode()

    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rc, n, msg = call(T, st.cuda_stream)
    st.synchronize()
    assert rc == 0 and n == T, msg
    raw = d_out.cpu().numpy()
    assert raw[: T * REC.itemsize].tobytes() == h_runs.tobytes() and (raw[T * REC.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), h_off)
    d_out.fill_(0xCD)
    rc, n, msg = call(T - 1)
    torch.cuda.synchronize()
    assert rc == OVERFLOW and n == T and str(T) in msg
    assert (d_out.cpu().numpy()[(T - 1) * REC.itemsize:] == 0xCD).all()
    launches = hip.stats()["launches"]
    torch.cuda.empty_cache()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g.capture_begin()
        rc, n, msg = call(T, st.cuda_stream)
        d_out_off.zero_()
        g.capture_end()
    assert rc == HIP and "stream capture" in msg
    d_out_off.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert not d_out_off.cpu().numpy().any()
    del g, keep
    assert hip.stats()["launches"] == launches


@ends_at_a_fault
def test_rank_and_locate_words_unicode(files):
    """rank(words=True, ignore_case="unicode") bit for bit against tests/rank_ref.py, the term counts being the whole-word
    occurrences of every spelling (tests/words_ref.py); locate_docs(words=True) against the same."""
    cs, rr = files
    docs = [d.encode("utf-8") for d in DOCS]
    classes = unicode_fold.case_classes()
    queries = [["über"], ["kelvin", "miss"], ["λόγοσ", "uber"], ["ber", "elvin"], ["k", "the"], []]
    post = []
    for q in queries:
        for t in q:
            tf = {}
            for d, s in enumerate(docs):
                c = sum(len(words_ref.literal_word_starts(s, v)) for v in variants(t.encode(), classes))
                if c:
                    tf[d] = c
            post.append(tf)
    assert post[1] == {2: 3, 6: 4} and not post[5] and not post[6] and post[7] == {2: 1}
    raw = [[t.encode() for t in q] for q in queries]
    for match in ("any", "all"):
        off, doc, score, df, w = cs.rank(raw, top=5, match=match, words=True, ignore_case="unicode")
        assert df.tolist() == [len(p) for p in post]
        eo, ed, es = rr.rank([len(q) for q in queries], post, w.tolist(), top=5, match=match)
        assert off.tolist() == eo and doc.tolist() == ed and bits(score) == bits(es)
    for t in ("kelvin", "über", "ber", "k"):
        doc, rawo, lens = cs.locate_docs(t.encode(), words=True, ignore_case="unicode")
        want = sorted((d, p, len(v)) for d, s in enumerate(docs) for v in variants(t.encode(), classes) for p in words_ref.literal_word_starts(s, v))
        assert list(zip(doc.tolist(), rawo.tolist(), lens.tolist())) == want, t


# ---------------------------------------------------------------- regexes and grep
from test_classes_cpu import REGEX_TEXT                      # noqa: E402

FIND_REGEXES = ["über", "k", "kelvin", "mis+", "σοφίασ", "(the|σ+)", "caf(é|e)", "[a-k]elvin", "ü+ber", "s?top", "an(d|D)?", "ı",
                "[s-u]h?e", "zebra"]


def re_hits_str(s, rx, flags, word=None, max_len=10):
    """[(byte start, byte length)] of every match of rx in the str s, every start and every end up to max_len characters;
    with `word` only those whose neighbouring BYTES are no word bytes."""
    pat = re.compile(rx, flags | re.DOTALL)
    data = s.encode("utf-8")
    at = [len(s[:j].encode("utf-8")) for j in range(len(s) + 1)]
    out = []
    for a in range(len(s)):
        if word is not None and at[a] > 0 and data[at[a] - 1] in word:
            continue
        for b in range(a + 1, min(len(s), a + max_len) + 1):
            if word is not None and at[b] < len(data) and data[at[b]] in word:
                continue
            if pat.fullmatch(s, a, b):
                out.append((at[a], at[b] - at[a]))
    return out


@pytest.fixture(scope="module")
def find_world():
    word = set(words_ref.WORD_BYTES)
    hits = {(rx, w): re_hits_str(REGEX_TEXT, rx, re.IGNORECASE, word if w else None) for rx in FIND_REGEXES for w in (False, True)}
    exact = {rx: re_hits_str(REGEX_TEXT, rx, 0) for rx in FIND_REGEXES}
    hip = findex_amd.HipFMSearcher.from_text(REGEX_TEXT.encode("utf-8"))
    yield hip, hits, exact
    hip.close()


@ends_at_a_fault
@pytest.mark.parametrize("mode", ["all", "longest", "disjoint"])
def test_finditer_unicode(find_world, mode):
    hip, hits, exact = find_world
    reduce = {"all": lambda h: sorted(set(h)), "longest": words_ref.longest, "disjoint": words_ref.disjoint}[mode]
    for words in (False, True):
        off, occ, truncated = hip.finditer(FIND_REGEXES, mode=mode, ignore_case="unicode", words=words)
        assert off.size == len(FIND_REGEXES) + 1
        for i, rx in enumerate(FIND_REGEXES):
            mine = occ[int(off[i]):int(off[i + 1])]
            assert list(zip(mine["pos"].tolist(), mine["len"].tolist())) == reduce(hits[(rx, words)]), (rx, words)
    assert sum(len(hits[(rx, False)]) > len(exact[rx]) for rx in FIND_REGEXES) >= 10  # the flag finds more than the plain regex
    assert not hits[("zebra", False)] and {n for _, n in hits[("kelvin", False)]} == {6, 8}
    for bad in ("^the", "[ü]"):
        with pytest.raises(ValueError):
            hip.finditer([bad], ignore_case="unicode")


@ends_at_a_fault
def test_grep_command_line(tmp_path, monkeypatch):
    """grep --unicode-case, with -n, -w and --not, against re.IGNORECASE on str; the mains run in this process."""
    import sys
    from findex_amd import grep as grep_cli, index as index_cli
    files = {"a.txt": "Über uns\nder Kelvin\nuber\n", "b.txt": "ÜBERALL über\nΣΟΦΊΑΣ\nKELVIN skala\n", "c.txt": "σοφίας\nmiſs Miss\nnichts\n"}
    root = tmp_path / "d"
    root.mkdir()
    for name, data in files.items():
        (root / name).write_bytes(data.encode("utf-8"))
    base = str(tmp_path / "x")

    def run(cli, *args):
        out = _Stdout()
        monkeypatch.setattr(sys, "stdout", out)
        try:
            assert cli.main(list(args)) == 0
        finally:
            monkeypatch.undo()
        return out.buffer.getvalue().split(b"\n")[:-1]

    def lines(rx, word=False, without=None):
        pat = re.compile(("(?<![0-9A-Za-z_\\u0080-\\U0010ffff])" + rx + "(?![0-9A-Za-z_\\u0080-\\U0010ffff])") if word else rx, re.IGNORECASE)
        no = re.compile(without, re.IGNORECASE) if without else None
        return [("%s:%d:%s" % (name, j + 1, ln)).encode("utf-8") for name, data in sorted(files.items())
                for j, ln in enumerate(data.split("\n")[:-1]) if pat.search(ln) and not (no and no.search(ln))]

    run(index_cli, "--dir", str(root), "--out", base)
    got = run(grep_cli, base, "über", "kelvin", "--unicode-case", "-n")
    assert got == lines("über") + lines("kelvin") and len(lines("über")) == 2 and len(lines("kelvin")) == 2
    assert run(grep_cli, base, "σοφίασ", "--unicode-case", "-n") == lines("σοφίασ") == ["b.txt:2:ΣΟΦΊΑΣ".encode(), "c.txt:1:σοφίας".encode()]
    got = run(grep_cli, base, "über", "miss", "--unicode-case", "-w", "-n")
    assert got == lines("über", True) + lines("miss", True) and "b.txt:1:ÜBERALL über".encode() in got and len(got) == 3
    got = run(grep_cli, base, "ÜBERALL", "--unicode-case", "-n", "--not", "UNS")
    assert got == lines("überall", without="uns") == ["b.txt:1:ÜBERALL über".encode()]
    assert run(grep_cli, base, "miss", "-i") == ["c.txt:19:Miss".encode()]                # -i stays ASCII: the long s is not met
    got = run(grep_cli, base, "miss", "--unicode-case")                                 # by occurrences: name:raw_off:text
    assert got == ["c.txt:13:miſs".encode(), "c.txt:19:Miss".encode()]
