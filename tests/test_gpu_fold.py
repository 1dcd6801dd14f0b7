"""The search under a fold map on the device (fmx_search_fold_batch) against tests/fold_ref.py, in both layouts,
offsets and record bytes exactly: a mixed-case text in every case spelling, the identity map against the exact search,
classes of 1, 2 and 8 on synthetic BWTs around the block edges, the one-row rule on the EOF row, a text in which every
variant occurs, a stack with a pending sibling at every level of a 255-byte pattern, batches of three times as many patterns
as a grid can have waves, capacity and determinism, the device form, its flag and a stream capture; then the layers above:
folding together with whole words against tests/words_ref.py, rank(ignore_case=True) against the ranking over the
reference's interval sets, finditer(ignore_case=True) and the command lines against Python's re.  Where a test passes
`steps`, the backward steps fmx_fold_last reports are held to fold_ref.walk -- never to a count read off the library."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import approx_ref
import findex_amd
import fold_ref
import oracle
import words_ref
from conftest import TESTDATA
from findex_amd import _lib
from helpers import bwt_of_text, ends_at_a_fault, lf_walk_patterns, pack_patterns, synth_bwt

pytestmark = pytest.mark.gpu

LAYOUTS = ["onehot", "bytes"]
REC = findex_amd.HipFMSearcher.RESULT
ASCII = fold_ref.ASCII
ARG, HIP, UNSUPPORTED, OVERFLOW = 3, 5, 6, 9


def waves_max():
    """More waves than a launch of k_fold can have resident: a CU holds at most 2048 threads, 8 workgroups of 256, four waves
    each.  An upper bound, not the occupancy query the library makes."""
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


def expected_arrays(pats, per_pattern):
    off, rows = fold_ref.expected_csr(pats, per_pattern)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=REC) if rows else np.zeros(0, dtype=REC)


def check(hip, pats, fold, per_pattern, what=None, steps=None):
    """One batch against its expectation, per-pattern lists of (sp, ep); with `steps`, the backward steps fold_ref.walk makes
    for the batch, also what fmx_fold_last reports of the call and what each of its two launches adds to the handle."""
    buf, off = pack_patterns(pats)
    st0 = hip.stats()
    got_off, got = hip.search_fold_batch(buf, off, fold)
    st1 = hip.stats()
    exp_off, exp = expected_arrays(pats, per_pattern)
    assert np.array_equal(got_off, exp_off), what
    assert got.tobytes() == exp.tobytes(), what
    assert st1["patterns_seen"] == st0["patterns_seen"] and st1["tables_held_bytes"] == st0["tables_held_bytes"]
    if steps is not None:
        _, _, got_steps, requests = hip.fold_last()
        print("%s: %d hits, %d steps (walk: %d), %d requests" % (what, got.size, got_steps, steps, requests))
        assert got_steps == steps, (what, got_steps, steps)
        assert requests <= 4 * steps, (what, requests, steps)
        launches = st1["launches"] - st0["launches"]         # the counting call, and the call that fetched the hits if any
        assert launches == (2 if got.size else 1), what
        assert st1["backward_steps"] - st0["backward_steps"] == launches * steps, what


def walk_steps(orc, pats, fold, per_pattern):
    """The steps fold_ref.walk makes for the batch; its hits must be the expectation's on the way."""
    total = 0
    for p, want in zip(pats, per_pattern):
        hits, steps, _ = fold_ref.walk(orc, p, fold)
        assert hits == sorted(want), p
        total += steps
    return total


def spellings(p):
    return [p, p.lower(), p.upper(), p.swapcase()]


# ---------------------------------------------------------------- a mixed-case text
@pytest.fixture(scope="module")
def mixed_text():
    with open(os.path.join(TESTDATA, "test3072.txt"), "rb") as f:
        return fold_ref.mixed_case(f.read())


@pytest.fixture(scope="module")
def mixed(mixed_text):
    """Patterns of 0 .. 24 bytes taken from the text, in every case spelling, and patterns that do not occur in any."""
    s = mixed_text
    rng = np.random.default_rng(281)
    orc = approx_ref.index_of(s)[0]
    pats = []
    for m in range(25):
        for _ in range(3):
            at = int(rng.integers(0, len(s) - m + 1))
            pats += spellings(s[at:at + m])
    pats += [b"#", b"zq#x", s[10:16] + b"#", b"#" + s[10:16], s[40:44] + b"0" + s[45:50], b"\0", s[-3:] + b"\0"]
    full = [fold_ref.dfs_hits(orc, p, ASCII) for p in pats]
    return pats, full, walk_steps(orc, pats, ASCII, full)


def test_mixed_expectations_are_the_ones_the_kernel_needs(mixed, mixed_text):
    pats, full, steps = mixed
    s = mixed_text
    assert sum(1 for c in s if 65 <= c <= 90) > 800 and sum(1 for c in s if 97 <= c <= 122) > 1800
    per = [len(h) for h in full]
    print("mixed: %d patterns, %d hits, most of one pattern %d, %d steps" % (len(pats), sum(per), max(per), steps))
    assert max(per) >= 2 and sum(1 for n in per if n >= 2) >= 20      # several spellings of one string occur
    assert sum(1 for n in per if n == 0) >= 4
    for p, h in zip(pats, full):                             # the sliding window sees the same
        assert fold_ref.window_hits(s, p, ASCII) == h, p
    # every spelling of a string finds the same intervals
    for j in range(0, 25 * 3 * 4, 4):
        assert full[j] == full[j + 1] == full[j + 2] == full[j + 3] and full[j]


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_mixed_case_text(mixed, mixed_text, layout):
    pats, full, steps = mixed
    hip = open_text(mixed_text, layout)
    check(hip, pats, ASCII, full, what="mixed", steps=steps)
    # opts == NULL is ASCII case folding
    buf, off = pack_patterns(pats)
    exp_off, exp = expected_arrays(pats, full)
    L = _lib.load()
    n_out = ctypes.c_size_t()
    o2 = np.zeros(off.size, dtype=np.uint64)
    h2 = np.zeros(exp.size, dtype=REC)
    assert L.fmx_search_fold_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, None, o2.ctypes.data,
                                   h2.ctypes.data, h2.size, ctypes.byref(n_out)) == 0
    assert n_out.value == exp.size and np.array_equal(o2, exp_off) and h2.tobytes() == exp.tobytes()
    # one pattern at a time, and its positions in the text
    s = mixed_text
    assert hip.search_fold(b"") == [(0, len(s) + 1)]
    q = s[100:104]
    assert hip.search_fold(q.swapcase()) == fold_ref.dfs_hits(approx_ref.index_of(s)[0], q, ASCII)
    hip.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_identity_map_is_the_exact_search(mixed, mixed_text, layout):
    pats, _, _ = mixed
    hip = open_text(mixed_text, layout)
    hip.config_set("jump", "off")
    hip.config_set("ktab", "off")
    buf, off = pack_patterns(pats)
    hip.stats_reset()
    sp, ep = hip.search_batch(buf, off)
    exact_steps = hip.stats()["backward_steps"]
    orc = approx_ref.index_of(mixed_text)[0]
    assert exact_steps == int(orc.search_batch(buf, off)[2].sum())
    found = sp < ep
    got_off, got = hip.search_fold_batch(buf, off, fold_ref.IDENTITY)
    assert np.array_equal(np.diff(got_off.astype(np.int64)), found.astype(np.int64))
    assert np.array_equal(got["regex"], np.nonzero(found)[0])
    assert np.array_equal(got["len"], np.array([len(p) for p in pats])[found])
    assert np.array_equal(got["sp"], sp[found]) and np.array_equal(got["ep"], ep[found])
    assert hip.fold_last()[2] == exact_steps                 # the one relation DESIGN.md 28 holds the kernel to
    hip.close()


# ---------------------------------------------------------------- classes of 1, 2 and 8 on synthetic BWTs
GENERAL = fold_ref.make_map([range(97, 105), (105, 106), (120, 121, 122)])      # 107 .. 112 fold to themselves; 120 .. 122 are absent


def synth_shapes():
    for sizes in ((447, 448, 449), (127, 128, 129)):
        for n in sizes:
            for eof in (0, n // 2, n - 1):
                yield n, eof


@pytest.fixture(scope="module")
def synth():
    out = []
    for n, eof in synth_shapes():
        index = synth_bwt(n, 97, 112, seed=n, eof=eof)
        orc = oracle.NaiveFMSearcher.from_mem(*index)
        rng = np.random.default_rng(n + eof)
        classes = {}
        for c in range(97, 113):
            classes.setdefault(GENERAL[c], []).append(c)
        pats = []
        for m in (1, 2, 3, 5):
            for p in lf_walk_patterns(orc, rng, 8, m, 0.3, alphabet=list(range(97, 113))):
                # another spelling of a string that occurs (a walk through the EOF row holds byte 0)
                pats.append(bytes(int(rng.choice(classes.get(GENERAL[c], [c]))) for c in p))
        full = [fold_ref.dfs_hits(orc, p, GENERAL) for p in pats]
        out.append((index, (n, eof), pats, full, walk_steps(orc, pats, GENERAL, full)))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_general_map_on_synthetic_bwts(synth, layout):
    found = most = 0
    for index, shape, pats, full, steps in synth:
        hip = open_index(index, layout)
        check(hip, pats, GENERAL, full, what=shape, steps=steps)
        found += sum(len(h) for h in full)
        most = max(most, max(len(h) for h in full))
        hip.close()
    print("synthetic: %d hits, most of one pattern %d" % (found, most))
    assert found > 2000 and most >= 30


# ---------------------------------------------------------------- the one-row rule on the EOF row
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_one_row_rule_on_the_eof_row(mixed_text, layout):
    """y + s[0:m], one byte more than the text has in front: when s[0:m] has been matched the interval is the one row of the
    whole text, the EOF row, whose BWT' symbol is 0 -- in no class of two, so the node dies without a step."""
    s = mixed_text
    orc = approx_ref.index_of(s)[0]
    m = 24
    base = s[:m]
    assert fold_ref.dfs_hits(orc, base, ASCII) == [(orc.eof, orc.eof + 1)]
    pats = [base, base.swapcase(), b"q" + base, b"Q" + base, b"q" + base.swapcase(), b"#" + base]
    full = [fold_ref.dfs_hits(orc, p, ASCII) for p in pats]
    assert full[0] == full[1] and not any(full[2:])
    walks = [fold_ref.walk(orc, p, ASCII) for p in pats]
    assert walks[2][1] == walks[0][1] and walks[5][1] == walks[0][1] + 1      # the letter costs no step, the singleton one
    check(hip := open_text(s, layout), pats, ASCII, full, what="eof row", steps=sum(w[1] for w in walks))
    hip.close()


# ---------------------------------------------------------------- every variant occurs
@pytest.fixture(scope="module")
def aa_text():
    return bytes(np.random.default_rng(282).choice([97, 65], 4096).astype(np.uint8))


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_every_variant_occurs(aa_text, layout):
    orc = approx_ref.index_of(aa_text)[0]
    pats = [b"a" * 10, b"A" * 10, b"aAaAaAaAaA", b"a" * 3, b"a" * 16]
    full = [fold_ref.dfs_hits(orc, p, ASCII) for p in pats]
    assert len(full[0]) > 900 and full[0] == full[1] == full[2] and len(full[3]) == 8
    assert fold_ref.window_hits(aa_text, pats[0], ASCII) == full[0]
    hip = open_text(aa_text, layout)
    check(hip, pats, ASCII, full, what="aA", steps=walk_steps(orc, pats, ASCII, full))
    hip.close()


# ---------------------------------------------------------------- a pending sibling at every level
@pytest.fixture(scope="module")
def deep():
    """A pattern P of 255 capitals and a text that holds, for j = 1 .. 254, the j + 1 bytes of P that the search has processed
    by then with the last processed one (the leftmost) in lower case, separated by '#': at every level the capital goes on --
    the smaller symbol -- and the lower-case sibling waits on the stack until the whole pattern is through."""
    rng = np.random.default_rng(283)
    P = bytes(rng.integers(65, 91, 255, dtype=np.uint8))
    parts = [bytes([P[254 - j] + 32]) + P[255 - j:] for j in range(1, 255)]
    s = b"#".join(parts)
    orc = approx_ref.index_of(s)[0]
    pats = [P.lower(), P]
    walks = [fold_ref.walk(orc, p, ASCII) for p in pats]
    full = [fold_ref.dfs_hits(orc, p, ASCII) for p in pats]
    assert [w[0] for w in walks] == full
    return s, pats, full, walks


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_deep_stack(deep, layout):
    s, pats, full, walks = deep
    print("deep: text of %d bytes, stack depths %s, steps %s" % (len(s), [w[2] for w in walks], [w[1] for w in walks]))
    assert max(w[2] for w in walks) >= 254 and all(len(p) == 255 for p in pats)
    hip = open_text(s, layout)
    check(hip, pats, ASCII, full, what="deep", steps=sum(w[1] for w in walks))
    # a full stack next to short patterns, over and over in one wave's loop
    batch = [pats[1], b"abc", pats[0], b"", pats[1]] * 3
    orc = approx_ref.index_of(s)[0]
    check(hip, batch, ASCII, [fold_ref.dfs_hits(orc, p, ASCII) for p in batch], what="deep, mixed")
    hip.close()


# ---------------------------------------------------------------- several patterns per wave
@pytest.fixture(scope="module")
def many(mixed_text, aa_text):
    """k = 3 * waves_max() + 5 patterns drawn with repetition from a pool of about 250 over the mixed-case text followed by
    the {a, A} text: ragged lengths, the empty pattern, patterns without a hit, patterns with hundreds of hits."""
    s = mixed_text + b"#" + aa_text[:1024]
    rng = np.random.default_rng(284)
    orc = approx_ref.index_of(s)[0]
    pool = [b"", b"#", b"zzzz", b"q#q", b"a" * 7, b"A" * 9, b"aA" * 4]
    while len(pool) < 250:
        m = int(rng.choice([1, 2, 3, 6, 12, 24]))
        at = int(rng.integers(0, len(mixed_text) - m))
        pool.append(spellings(s[at:at + m])[int(rng.integers(0, 4))])
    pool = sorted(set(pool))
    hits, steps = [], []
    for p in pool:
        h, st, _ = fold_ref.walk(orc, p, ASCII)
        assert h == fold_ref.dfs_hits(orc, p, ASCII)
        hits.append(h)
        steps.append(st)
    k = 3 * waves_max() + 5
    return s, pool, hits, np.array(steps), rng.integers(0, len(pool), k)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_several_patterns_per_wave(many, layout):
    s, pool, hits, steps, idx = many
    W = waves_max()
    lens = np.array([len(p) for p in pool])
    assert idx.size >= 3 * W and idx.size % 4 != 0 and 200 <= len(pool) <= 260
    assert (lens[idx[:-4]] != lens[idx[4:]]).mean() > 0.4 and max(len(h) for h in hits) > 100
    pats = [pool[j] for j in idx.tolist()]
    exp_off, exp = expected_arrays(pats, [hits[j] for j in idx.tolist()])
    print("several patterns per wave: k = %d, waves_max = %d, %d hits" % (idx.size, W, exp.size))
    assert 50_000 < exp.size < 2_000_000
    hip = open_text(s, layout)
    buf, off = pack_patterns(pats)
    st0 = hip.stats()
    got_off, got = hip.search_fold_batch(buf, off)
    st1 = hip.stats()
    assert np.array_equal(got_off, exp_off)
    assert got.tobytes() == exp.tobytes()
    total = int(steps[idx].sum())
    assert hip.fold_last()[2] == total
    assert st1["launches"] == st0["launches"] + 2 and st1["backward_steps"] - st0["backward_steps"] == 2 * total
    hip.close()


# ---------------------------------------------------------------- capacity, order, determinism
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_capacity_order_and_determinism(aa_text, mixed_text, layout):
    s = mixed_text + b"#" + aa_text[:1024]
    orc = approx_ref.index_of(s)[0]
    rng = np.random.default_rng(285)
    pats = [b"a" * int(m) for m in rng.integers(1, 9, 40)] + [s[at:at + 3].swapcase() for at in rng.integers(0, 3000, 60).tolist()]
    exp_off, exp = expected_arrays(pats, [fold_ref.dfs_hits(orc, p, ASCII) for p in pats])
    T = exp.size
    assert T > 2000
    hip = open_text(s, layout)
    buf, off = pack_patterns(pats)
    L = _lib.load()
    guard = 64

    def call(cap):
        out = np.full((cap + guard) * REC.itemsize, 0xAB, dtype=np.uint8)
        out_off = np.zeros(off.size, dtype=np.uint64)
        n_out = ctypes.c_size_t()
        rc = L.fmx_search_fold_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, None, out_off.ctypes.data,
                                     out.ctypes.data if cap else None, cap, ctypes.byref(n_out))
        assert (out[cap * REC.itemsize:] == 0xAB).all()      # nothing behind out[cap - 1]
        return rc, int(n_out.value), out_off, out[: cap * REC.itemsize].view(REC)

    rc, n, o, h = call(T)
    assert rc == 0 and n == T and np.array_equal(o, exp_off) and h.tobytes() == exp.tobytes()
    for cap in (T - 1, 1, 0):
        rc, n, _, _ = call(cap)
        assert rc == OVERFLOW and n == T, cap
        assert str(T).encode() in L.fmx_last_error()
    rc, n2, o2, h2 = call(n)                                 # the retry at n_out
    assert rc == 0 and n2 == T and h2.tobytes() == h.tobytes() and np.array_equal(o2, o)   # two calls, identical bytes
    rc, n3, o3, h3 = call(T + 1000)
    assert rc == 0 and n3 == T and h3[:T].tobytes() == h.tobytes()
    seg = np.repeat(np.arange(len(pats)), np.diff(o.astype(np.int64)))
    assert np.array_equal(h["regex"], seg)
    same = seg[1:] == seg[:-1]
    assert (h["sp"][1:][same] >= h["ep"][:-1][same]).all() and (h["sp"] < h["ep"]).all()      # disjoint, ascending
    hip.close()


# ---------------------------------------------------------------- the device form
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_device_form_flag_and_stream_capture(mixed, mixed_text, layout):
    import torch
    pats, full, _ = mixed
    hip = open_text(mixed_text, layout)
    buf, off = pack_patterns(pats)
    h_off, h_hits = expected_arrays(pats, full)
    T, k = h_hits.size, len(pats)
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * REC.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        n = hip.search_fold_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T, stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * REC.itemsize].tobytes() == h_hits.tobytes() and (raw[T * REC.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), h_off)
    # too small: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_fold_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T - 1)
    assert ei.value.code == OVERFLOW and str(T) in str(ei.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy()[(T - 1) * REC.itemsize:] == 0xCD).all()
    # a pattern of 256 bytes: the host form refuses it before the device, the device form's kernel skips it and raises its flag
    long_pats = [pats[4], mixed_text[:256], mixed_text[:255]]
    lbuf, loff = pack_patterns(long_pats)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_fold_batch(lbuf, loff)
    assert ei.value.code == ARG and "255" in str(ei.value)
    d_lpat = torch.from_numpy(lbuf).cuda()
    d_loff = torch.from_numpy(loff.view(np.int64)).cuda()
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_fold_batch_dev(d_lpat.data_ptr(), d_loff.data_ptr(), 3, d_out_off.data_ptr(), d_out.data_ptr(), T)
    assert ei.value.code == ARG and "255" in str(ei.value)
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
            hip.search_fold_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, d_out_off.data_ptr(), d_out.data_ptr(), T, stream=st.cuda_stream)
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


def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_fold(b"abr")
    assert ei.value.code == UNSUPPORTED
    hip.close()


# ---------------------------------------------------------------- folding together with whole words
H = findex_amd.HipFMSearcher
VOCAB = [b"he", b"The", b"THEN", b"a", b"An", b"and", b"x_1", b"Hello", b"END", b"the", b"tHe", b"AND", b"X_1"]
SEPS = [b" ", b" ", b", ", b"-", b".\n", b"\t"]
ABSENT = [b"zebra", b"th", b"X_", b"Nd"]                        # the last three occur, but never as words


def case_words_text():
    """About 6 KB of words in mixed case: "The" at offset 0, "THEN" at the very end, "xhe" where a map that folds the space
    with x would find a word if the step with the left neighbour were folded too."""
    rng = np.random.default_rng(287)
    parts = [b"The", b" ", b"xhe", b" ", b"he xhe", b" "]
    size = sum(len(p) for p in parts)
    while size < 6000:
        w, s = VOCAB[int(rng.integers(len(VOCAB)))], SEPS[int(rng.integers(len(SEPS)))]
        parts += [w, s]
        size += len(w) + len(s)
    parts.append(b"THEN")
    return b"".join(parts)


def variants(q, fold):
    """Every string that equals q under the map."""
    members = {}
    for c in range(256):
        members.setdefault(fold[c], []).append(c)
    return [bytes(v) for v in itertools.product(*[members[fold[c]] for c in q])]


_refs = {}


@pytest.fixture(scope="module", params=LAYOUTS)
def words_world(request):
    text = case_words_text()
    if "words" not in _refs:                                 # one checker for both layouts, left unchanged
        _refs["words"] = words_ref.SuffixRef(text)
    ref = _refs["words"]
    findex_amd.set_layout(request.param)
    try:
        hip = H.from_text(text)
    finally:
        findex_amd.set_layout("auto")
    assert hip.n == ref.n and hip.search(b"ehT") == ref.interval(b"The")
    yield hip, ref
    hip.close()


@ends_at_a_fault
def test_context_and_fold(words_world):
    hip, ref = words_world
    B = words_ref.BOUNDARY
    text = ref.text
    pats = VOCAB + ABSENT
    off, runs = hip.search_words(pats, fold=ASCII)
    assert off.size == len(pats) + 1
    for i, q in enumerate(pats):
        mine = runs[int(off[i]):int(off[i + 1])]
        assert (mine["regex"] == i).all() and (mine["len"] == len(q)).all()
        sp, ep = mine["sp"].tolist(), mine["ep"].tolist()
        assert all(a < b for a, b in zip(sp, ep)) and all(b <= a for b, a in zip(ep, sp[1:]))      # ascending, disjoint
        rows = [r for a, b in zip(sp, ep) for r in range(a, b)]
        want_rows = sorted(r for v in variants(q, ASCII) for r in ref.context_rows(v, B, B))
        assert rows == want_rows, q
        starts = sorted(p for v in variants(q, ASCII) for p in words_ref.literal_word_starts(text, v))
        assert hip.locate_words(q, fold=ASCII).tolist() == starts, q
    i = pats.index(b"the")
    assert 0 in hip.locate_words(b"the", fold=ASCII).tolist()                         # the word at offset 0: "The"
    assert len(text) - 4 in hip.locate_words(b"then", fold=ASCII).tolist()            # the word at the text's end: "THEN"
    assert hip.locate_words(b"then").size == 0 and hip.locate_words(b"the").size > 0
    assert int(off[len(VOCAB)]) == int(off[-1])                                       # no absent one is a word in any spelling
    # bit 0 of left cleared: the occurrence at offset 0 goes
    pat, poff = pack_patterns([q[::-1] for q in pats])
    no_start = bytes(c for c in B if c != 0)
    o2, runs2 = hip.search_context_batch(pat, poff, no_start, B, fold=ASCII)
    the0 = ref.interval(b"The")[0]
    rows_of = lambda o, r, j: [x for a, b in zip(r["sp"][int(o[j]):int(o[j + 1])].tolist(), r["ep"][int(o[j]):int(o[j + 1])].tolist()) for x in range(a, b)]
    assert the0 in rows_of(off, runs, i) and the0 not in rows_of(o2, runs2, i)
    assert rows_of(o2, runs2, i) == sorted(r for v in variants(b"the", ASCII) for r in ref.context_rows(v, no_start, B))
    # a map that folds a boundary byte with a word byte: the step with the left neighbour stays exact -- "xhe" holds no word
    # "he" -- while a space INSIDE a pattern folds
    odd = fold_ref.make_map([b" x"])
    assert hip.locate_words(b"he", fold=odd).tolist() == words_ref.literal_word_starts(text, b"he")
    assert text.find(b"xhe") + 1 not in hip.locate_words(b"he", fold=odd).tolist()
    both = sorted(p for v in variants(b"he xhe", odd) for p in words_ref.literal_word_starts(text, v))
    assert both and hip.locate_words(b"he xhe", fold=odd).tolist() == both
    assert hip.locate_words(b"hexxhe", fold=odd).tolist() == both
    # the fold search alone, through locate
    for q in (b"the", b"HE", b"x_1", b"zebra"):
        want = [m.start() for m in re.finditer(b"(?=" + re.escape(q.lower()) + b")", text.lower())]
        assert hip.locate_fold(q).tolist() == want, q
    assert hip.locate_fold(b"he", max_hits=5).size == 5
    assert hip.search_context_batch(pat[:0], poff[:1], B, B, fold=ASCII)[0].tolist() == [0]
    o3, runs3 = hip.search_words([b"zebra", b"qqq"], fold=ASCII)                      # no spelling occurs: no record reaches the filter
    assert o3.tolist() == [0, 0, 0] and runs3.size == 0


@ends_at_a_fault
def test_context_and_fold_device_form(words_world):
    """fmx_search_context_fold_batch_dev on a side stream: the host form's bytes (which test_context_and_fold holds against the
    reference), guard bytes behind the capacity, a capacity one short, the flag of a pattern that is too long once its left
    byte stands in front, and the refusal under a stream capture."""
    import torch
    from findex_amd.searcher import class_words
    hip, ref = words_world
    B = words_ref.BOUNDARY
    pats = VOCAB + ABSENT
    pat, poff = pack_patterns([q[::-1] for q in pats])
    h_off, h_runs = hip.search_context_batch(pat, poff, B, B, fold=ASCII)
    T, k = h_runs.size, len(pats)
    assert T > 20
    opts = _lib.fmx_context_opts()
    for j, w in enumerate(class_words(B)):
        opts.left[j] = opts.right[j] = int(w)
    fopts = hip._fold_opts(ASCII)
    entry = hip._L.fmx_search_context_fold_batch_dev

    def call(d_p, d_o, kk, cap, stream=0):
        n_out = ctypes.c_size_t(0)
        rc = entry(hip._h, ctypes.c_void_p(d_p.data_ptr()), ctypes.c_void_p(d_o.data_ptr()), kk, ctypes.byref(opts), ctypes.byref(fopts),
                   ctypes.c_void_p(d_out_off.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.byref(n_out), ctypes.c_void_p(stream))
        return rc, int(n_out.value), (hip._L.fmx_last_error() or b"").decode()

    d_pat = torch.from_numpy(np.ascontiguousarray(pat)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(poff).view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * REC.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    launches = hip.stats()["launches"]
    with torch.cuda.stream(st):
        rc, n, msg = call(d_pat, d_off, k, T, st.cuda_stream)
    st.synchronize()
    assert rc == 0 and n == T, msg
    assert hip.stats()["launches"] > launches
    raw = d_out.cpu().numpy()
    assert raw[: T * REC.itemsize].tobytes() == h_runs.tobytes() and (raw[T * REC.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), h_off)
    # too small: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    rc, n, msg = call(d_pat, d_off, k, T - 1)
    torch.cuda.synchronize()
    assert rc == OVERFLOW and n == T and str(T) in msg
    assert (d_out.cpu().numpy()[(T - 1) * REC.itemsize:] == 0xCD).all()
    # 254 bytes is the longest pattern: with a left byte in front it has 255.  One of 255 is skipped by the kernel, which
    # raises its flag; the host form refuses it before the device
    text = ref.text
    for m, want in ((254, 0), (255, ARG)):
        lbuf, loff = pack_patterns([b"eh", text[:m][::-1]])
        d_lpat = torch.from_numpy(np.ascontiguousarray(lbuf)).cuda()
        d_loff = torch.from_numpy(np.ascontiguousarray(loff).view(np.int64)).cuda()
        rc, n, msg = call(d_lpat, d_loff, 2, T)
        torch.cuda.synchronize()
        assert rc == want, (m, rc, msg)
        if want:
            assert "255" in msg
            with pytest.raises(findex_amd.FmxError) as ei:
                hip.search_context_batch(lbuf, loff, B, B, fold=ASCII)
            assert ei.value.code == ARG and "254" in str(ei.value)
        else:
            o, runs = hip.search_context_batch(lbuf, loff, B, B, fold=ASCII)
            assert n == runs.size and np.array_equal(d_out_off[:3].cpu().numpy().view(np.uint64), o)
            assert d_out.cpu().numpy()[: n * REC.itemsize].tobytes() == runs.tobytes()
            assert int(o[2]) - int(o[1]) == (1 if text[254] in B else 0)      # the text's beginning: a word if it ends at a boundary
    # under a stream capture the call is refused before it allocates or launches, and the capture goes on
    launches = hip.stats()["launches"]
    torch.cuda.empty_cache()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g.capture_begin()
        rc, n, msg = call(d_pat, d_off, k, T, st.cuda_stream)
        d_out_off.zero_()
        g.capture_end()
    assert rc == HIP and "stream capture" in msg
    d_out_off.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert not d_out_off.cpu().numpy().any()
    del g
    assert hip.stats()["launches"] == launches


# ---------------------------------------------------------------- ranking
def case_docs():
    rng = np.random.default_rng(288)
    docs = []
    for d in range(60):
        parts = []
        for _ in range(int(rng.integers(0, 25))):
            parts += [VOCAB[int(rng.integers(len(VOCAB)))], SEPS[int(rng.integers(len(SEPS)))]]
        docs.append(b"".join(parts))
    docs[5] = b"THE"                                                                # a whole file; a word that ends one file
    docs[6] = b"and then The"                                                       # and begins the next
    docs[7] = b"tHe end \x00 He"
    return docs


@pytest.fixture(scope="module")
def files():
    docs = case_docs()
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_documents(docs))
    ref = words_ref.SuffixRef(bytes(cs.corpus.stream()))
    yield cs, ref, docs
    cs.close()


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@ends_at_a_fault
def test_rank_ignore_case(files):
    """rank(ignore_case=True) against fmx_corpus_rank_sets over the REFERENCE's interval sets: per term the intervals of its
    spellings that occur (a naive suffix array of the stream), with words=True the runs of their rows that stand as words."""
    from findex_amd import escape
    cs, ref, docs = files
    B = words_ref.BOUNDARY
    assert cs.searcher.n == ref.n and cs.searcher.search(b"eht") == ref.interval(b"the")      # the same rows
    queries = [[b"he"], [b"the", b"then"], [b"A", b"an", b"AND"], [b"x_1", b"zebra"], [b"e"], [b"\x00"], []]
    terms = [t for q in queries for t in q]
    q_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.uint64)
    for words in (False, True):
        sp, ep, set_off = [], [], [0]
        for t in terms:
            if words:
                rows = sorted(r for v in variants(escape(t), ASCII) for r in ref.context_rows(v, B, B))
                ivs = [(r, r + 1) for r in rows]
            else:
                ivs = sorted(iv for iv in (ref.interval(v) for v in variants(escape(t), ASCII)) if iv[0] < iv[1])
            sp += [a for a, _ in ivs]
            ep += [b for _, b in ivs]
            set_off.append(len(sp))
        assert set_off[2] - set_off[1] >= 3                                          # "the" occurs in several spellings
        for match in ("any", "all"):
            want = cs.rank_sets_intervals(sp, ep, set_off, q_off, top=10, match=match)
            got = cs.rank(queries, top=10, match=match, words=words, ignore_case=True)
            same_bytes(got, want)
            exact = cs.rank(queries, top=10, match=match, words=words)
            assert (got[3] >= exact[3]).all() and got[3].sum() > exact[3].sum()      # df: more files hold a term in some spelling
    with pytest.raises(ValueError):
        cs.locate_docs(b"the", max_mismatches=1, ignore_case=True)
    # positions, against a scan of the files
    for words in (False, True):
        doc, raw = cs.locate_docs(b"the", ignore_case=True, words=words)
        scan = words_ref.literal_word_starts if words else (lambda s, q: [m.start() for m in re.finditer(b"(?=" + q + b")", s)])
        want = [(d, p) for d, s in enumerate(docs) for p in scan(s.lower(), b"the")]
        assert list(zip(doc.tolist(), raw.tolist())) == want and (5, 0) in want and (7, 0) in want
    assert [n for n, _ in cs.rank_files([b"THE"], top=3, ignore_case=True)] == [n for n, _ in cs.rank_files([b"the"], top=3, ignore_case=True)]


# ---------------------------------------------------------------- regexes and the command lines
FIND_REGEXES = ["he", "The", "x_1", "th(e|en)", "a+n?", ".he", "[s-u]h[a-e]", "an(d|D)?", "hel*o", "zebra", "\\w_\\d",
                "[ab].", "[a-c]\\w", "[x-z]_\\d", "([ab]|c)."]                 # a class or a dot after a set


def re_hits(text, rx, flags, word=None, max_len=6):
    """[(start, length)] of every match of rx in text, every start and every end up to max_len; with `word` only those whose
    neighbours are no word bytes."""
    rx = re.compile(rx.replace("\\w", "[A-y]").replace("\\d", "[0-8]").encode("latin-1"), flags | re.DOTALL)
    out = []
    for a in range(len(text)):
        if word is not None and a > 0 and text[a - 1] in word:
            continue
        for b in range(a + 1, min(len(text), a + max_len) + 1):
            if word is not None and b < len(text) and text[b] in word:
                continue
            if rx.fullmatch(text, a, b):
                out.append((a, b - a))
    return out


@pytest.fixture(scope="module")
def find_world():
    text = case_words_text()
    flags = re.IGNORECASE | re.ASCII
    hits = {(rx, w): re_hits(text, rx, flags, set(words_ref.WORD_BYTES) if w else None) for rx in FIND_REGEXES for w in (False, True)}
    exact = {rx: re_hits(text, rx, 0) for rx in FIND_REGEXES}
    hip = H.from_text(text)
    yield hip, text, hits, exact
    hip.close()


@ends_at_a_fault
@pytest.mark.parametrize("mode", ["all", "longest", "disjoint"])
def test_finditer_ignore_case(find_world, mode):
    hip, text, hits, exact = find_world
    reduce = {"all": lambda h: sorted(set(h)), "longest": words_ref.longest, "disjoint": words_ref.disjoint}[mode]
    for words in (False, True):
        off, occ, truncated = hip.finditer(FIND_REGEXES, mode=mode, ignore_case=True, words=words)
        assert off.size == len(FIND_REGEXES) + 1
        for i, rx in enumerate(FIND_REGEXES):
            mine = occ[int(off[i]):int(off[i + 1])]
            assert list(zip(mine["pos"].tolist(), mine["len"].tolist())) == reduce(hits[(rx, words)]), (rx, words)
            assert (mine["group"] == i).all()
    assert sum(len(hits[(rx, False)]) > len(exact[rx]) for rx in FIND_REGEXES) >= 7   # the flag finds more than the plain regex
    assert not hits[("zebra", False)] and hits[("\\w_\\d", False)]
    with pytest.raises(ValueError):
        hip.finditer(["^the"], ignore_case=True)


class _Stdout:
    """sys.stdout for a command line's main(): its bytes are kept."""

    def __init__(self):
        import io
        self.buffer = io.BytesIO()

    def write(self, text):
        self.buffer.write(text.encode())

    def flush(self):
        pass


def test_command_lines(tmp_path, monkeypatch):
    """grep -i, grep -i -w -n and rank -i against re on a corpus of three files.  The mains run in this process (one index
    build, one open per call); `python -m findex_amd.grep` is started once, for the way in."""
    from findex_amd import grep as grep_cli, index as index_cli, rank as rank_cli
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = {"a.txt": b"The cat\nconCATenate\nthen\n", "b.txt": b"CAT the\nTHE\nno\n", "c.txt": b"catcat Theme\n"}
    root = tmp_path / "d"
    root.mkdir()
    for name, data in files.items():
        (root / name).write_bytes(data)
    base = str(tmp_path / "x")

    def run(cli, *args):
        out = _Stdout()
        monkeypatch.setattr(sys, "stdout", out)
        try:
            assert cli.main(list(args)) == 0
        finally:
            monkeypatch.undo()
        return out.buffer.getvalue().split(b"\n")[:-1]

    def lines(rx, word=False, flags=re.IGNORECASE | re.ASCII, without=None):
        """name:line_no:line of the lines that hold a match of rx (and none of `without`), in (file, line) order, as re finds
        them."""
        pat = re.compile((b"\\b" + rx + b"\\b") if word else rx, flags)
        no = re.compile(without, flags) if without else None
        return [name.encode() + b":%d:" % (j + 1) + ln for name, data in sorted(files.items())
                for j, ln in enumerate(data.split(b"\n")[:-1]) if pat.search(ln) and not (no and no.search(ln))]

    def holding(rx, word=False, flags=re.IGNORECASE | re.ASCII):
        return sorted({ln.split(b":")[0] for ln in lines(rx, word, flags)})

    run(index_cli, "--dir", str(root), "--out", base)
    got = run(grep_cli, base, "the", "cat", "-i", "-n")
    assert got == lines(b"the") + lines(b"cat") and b"b.txt:2:THE" in got and b"a.txt:2:conCATenate" in got
    got = run(grep_cli, base, "the", "cat", "-i", "-w", "-n")
    assert got == lines(b"the", True) + lines(b"cat", True) and b"b.txt:2:THE" in got and b"a.txt:2:conCATenate" not in got
    assert run(grep_cli, base, "the", "-n") == lines(b"the", flags=0)                  # without -i: as before
    assert b"b.txt:2:THE" not in lines(b"the", flags=0)
    got = run(grep_cli, base, "cat", "-i", "-n", "--not", "the")                      # -i reaches the --not regex too
    assert got == lines(b"cat", without=b"the") == [b"a.txt:2:conCATenate"]
    got = [ln.split(b"\t")[1] for ln in run(rank_cli, base, "cat", "-i")]
    assert sorted(got) == holding(b"cat") == [b"a.txt", b"b.txt", b"c.txt"]
    got = [ln.split(b"\t")[1] for ln in run(rank_cli, base, "cat", "-i", "-w")]
    assert sorted(got) == holding(b"cat", True) == [b"a.txt", b"b.txt"]               # not c.txt: catcat is no word
    got = [ln.split(b"\t")[1] for ln in run(rank_cli, base, "cat")]
    assert sorted(got) == holding(b"cat", flags=0) == [b"a.txt", b"c.txt"]
    env = dict(os.environ)
    env["PYTHONPATH"] = root_dir + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "findex_amd.grep", base, "the", "-i", "-w", "-n"], cwd=root_dir, env=env,
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split(b"\n")[:-1] == lines(b"the", True)
