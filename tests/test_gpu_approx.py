"""Approximate search on the device (fmx_search_approx_batch) against tests/approx_ref.py, in both layouts:
real texts with dense and wide alphabets against the sliding window, synthetic BWTs around the block edges against the
walk over getPrevRange, the one-row rule and the EOF row, e = 0 against the exact search, batches of three times as many
patterns as a grid can have waves (e = 0 .. 3), patterns of up to 3001 bytes, degenerate shapes, capacity, order and
determinism, the device form and a stream capture, and the corpus searcher.  Where a test passes `steps`, the backward steps
fmx_approx_last reports are held to approx_ref.walk, the walk of DESIGN.md 15 restated over the oracle -- never to a count
read off the library."""
import ctypes
import os

import numpy as np
import pytest

import approx_ref
import findex_amd
import oracle
from conftest import TESTDATA
from findex_amd import _lib
from helpers import bwt_of_text, lf_walk_patterns, pack_patterns, synth_bwt

pytestmark = pytest.mark.gpu

LAYOUTS = ["onehot", "bytes"]
HIT = findex_amd.HipFMSearcher.APPROX_HIT
OVERFLOW = 9


def waves_max():
    """More waves than a launch of k_approx can have resident: a CU holds at most 2048 threads, 8 workgroups of 256, four
    waves each.  An upper bound, not the occupancy query the library makes: a batch of 3 * waves_max() patterns and more
    makes every wave's loop over the batch go round at least three times."""
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
    off, rows = approx_ref.expected_csr(per_pattern)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=HIT) if rows else np.zeros(0, dtype=HIT)


def check(hip, pats, e, per_pattern, sub=(1, 255), what=None, steps=None):
    """One batch against its expectation, per-pattern lists of (sp, ep, d); with `steps`, the backward steps approx_ref.walk
    makes for the batch, also what fmx_approx_last reports of the call."""
    buf, off = pack_patterns(pats)
    got_off, got = hip.search_approx_batch(buf, off, e, sub=sub)
    exp_off, exp = expected_arrays(per_pattern)
    assert np.array_equal(got_off, exp_off), (what, e)
    assert got.tobytes() == exp.tobytes(), (what, e)
    if steps is not None:
        _, _, got_steps, requests = hip.approx_last()
        print("%s e=%d: %d steps (walk: %d), %d requests" % (what, e, got_steps, steps, requests))
        assert got_steps == steps, (what, e, got_steps, steps)
        assert 0 < requests <= 4 * steps, (what, e, requests, steps)


def walk_steps(orc, pats, e, per_pattern, sub=(1, 255)):
    """The steps approx_ref.walk makes for the batch; its hits must be the expectation's on the way."""
    total = 0
    for p, want in zip(pats, per_pattern):
        hits, steps = approx_ref.walk(orc, p, e, *sub)
        assert hits == sorted(want), (p, e)
        total += steps
    return total


def mutated(rng, s, m, alphabet, k=200):
    """k patterns of m bytes taken from s, 0, 1 or 2 of their bytes replaced by letters of the alphabet."""
    pats = []
    for j in range(k):
        at = int(rng.integers(0, len(s) - m + 1))
        p = bytearray(s[at:at + m])
        for pos in rng.choice(m, size=min(j % 3, m), replace=False).tolist():
            p[pos] = int(rng.choice(alphabet))
        pats.append(bytes(p))
    return pats


# ---------------------------------------------------------------- real text, dense alphabet
DENSE_M = (1, 2, 6, 12, 24)


@pytest.fixture(scope="module")
def dense():
    """text name -> (text, {m: (patterns, their hits at e = 3)}); the hits of a smaller budget are those with d <= e."""
    rng = np.random.default_rng(20)
    with open(os.path.join(TESTDATA, "test1024.txt"), "rb") as f:
        t1024 = f.read()
    texts = {"test1024": t1024, "abcd": bytes(rng.integers(97, 101, 3000, dtype=np.uint8))}
    out = {}
    for name, s in texts.items():
        alphabet = sorted(set(s))
        per_m = {}
        for m in DENSE_M:
            pats = mutated(rng, s, m, alphabet)
            per_m[m] = (pats, [approx_ref.window_hits(s, p, 3) for p in pats])
        out[name] = (s, per_m)
    return out


def test_dense_expectations_are_the_ones_the_kernel_needs(dense):
    """Before any comparison: the batches hold what they are there for."""
    assert len(set(dense["test1024"][0])) == 26
    _, ab = dense["abcd"]
    per = [len(h) for h in ab[6][1]]
    print("abcd m=6 e=3: most hits of one pattern %d, batch total %d" % (max(per), sum(per)))
    assert max(per) >= 300 and 50_000 <= sum(per) <= 100_000
    assert all(len(approx_ref.within(h, 1)) >= 3 for h in ab[6][1])
    _, tt = dense["test1024"]
    none = sum(1 for m in (12, 24) for h in tt[m][1] if not approx_ref.within(h, 1))
    print("test1024 m>=12 e=1: %d patterns without a hit" % none)
    assert none >= 50


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["test1024", "abcd"])
def test_dense_alphabet_against_the_sliding_window(dense, name, layout):
    s, per_m = dense[name]
    hip = open_text(s, layout)
    for m in DENSE_M:
        pats, full = per_m[m]
        for e in range(4):
            check(hip, pats, e, [approx_ref.within(h, e) for h in full], what=(name, m))
    hip.close()


# ---------------------------------------------------------------- wide alphabet
@pytest.fixture(scope="module")
def wide():
    rng = np.random.default_rng(21)
    s = bytes(rng.integers(1, 256, 5000, dtype=np.uint8))
    assert len(set(s)) == 255 and max(s) >= 0x80
    alphabet = list(range(1, 256))
    cases = []                                               # (m, e, patterns, hits)
    for m, e, k in ((1, 1, 64), (2, 1, 100), (6, 3, 100), (12, 3, 100), (24, 3, 100), (2, 2, 20)):
        pats = mutated(rng, s, m, alphabet, k)
        cases.append((m, e, pats, [approx_ref.window_hits(s, p, e) for p in pats]))
    return s, cases


@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_alphabet_against_the_sliding_window(wide, layout):
    s, cases = wide
    assert all(len(h) == 255 for h in cases[0][3])           # m = 1, e = 1: every symbol, 16 symbol rounds per node
    assert min(len(h) for h in cases[5][3]) > 4000           # m = 2, e = 2: every pair that occurs
    hip = open_text(s, layout)
    for m, emax, pats, full in cases:
        for e in (range(emax + 1) if m >= 6 else [emax]):
            check(hip, pats, e, [approx_ref.within(h, e) for h in full], what=("wide", m))
    hip.close()


# ---------------------------------------------------------------- synthetic BWTs against the walk over getPrevRange
def synth_shapes():
    """The smallest shapes that put sp and ep in one block, in two, and at a block's edge, in each layout (448 positions
    per one-hot block, 128 per bytes block), and one of several blocks; the EOF slot first, in the middle and last."""
    for lo, hi, sizes, k in ((97, 100, (447, 448, 449, 4500), 10), (1, 200, (127, 128, 129, 4500), 5)):
        for n in sizes:
            for eof in (0, n // 2, n - 1):
                yield lo, hi, n, eof, k


@pytest.fixture(scope="module")
def synth():
    out = []
    for lo, hi, n, eof, k in synth_shapes():
        index = synth_bwt(n, lo, hi, seed=n + lo, eof=eof)
        orc = oracle.NaiveFMSearcher.from_mem(*index)
        rng = np.random.default_rng(n + eof)
        pats = [p for m in (8, 16) for p in lf_walk_patterns(orc, rng, k, m, 0.5, alphabet=list(range(lo, hi + 1)))]
        full = [approx_ref.dfs_hits(orc, p, 2) for p in pats]
        steps = [walk_steps(orc, pats, e, [approx_ref.within(h, e) for h in full]) for e in range(3)]
        out.append((index, (lo, hi, n, eof), pats, full, steps))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_synthetic_bwts_against_the_walk(synth, layout):
    found = 0
    for index, shape, pats, full, steps in synth:
        hip = open_index(index, layout)
        for e in range(3):
            check(hip, pats, e, [approx_ref.within(h, e) for h in full], what=shape, steps=steps[e])
        found += sum(len(h) for h in full)
        hip.close()
    assert found > 800


# ---------------------------------------------------------------- the one-row rule and the EOF row
@pytest.fixture(scope="module")
def prefix_case():
    """Patterns at the beginning of the text: s[0:m] whole and with its first, a middle and its last byte replaced, and
    y + s[0:m] -- one byte more than the text has in front: when s[0:m] has been matched the interval is the one row of
    the whole text, the EOF row, whose BWT' symbol is 0, and nothing may extend it."""
    with open(os.path.join(TESTDATA, "test1024.txt"), "rb") as f:
        s = f.read()
    pats, kind = [], []
    for m in (8, 24):
        base = s[:m]
        pats.append(base)
        kind.append("base")
        for pos in (0, m // 2, m - 1):
            p = bytearray(base)
            p[pos] = 122 if p[pos] != 122 else 121
            pats.append(bytes(p))
            kind.append("first" if pos == 0 else "other")
        for y in (s[m], 122):
            pats.append(bytes([y]) + base)
            kind.append("extended")
    full = [approx_ref.window_hits(s, p, 2) for p in pats]
    orc = approx_ref.index_of(s)[0]
    return s, pats, kind, full, [walk_steps(orc, pats, e, [approx_ref.within(h, e) for h in full]) for e in range(3)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_row_rule_and_the_eof_row(prefix_case, layout):
    s, pats, kind, full, steps = prefix_case
    for e in (1, 2):
        exp = [approx_ref.within(h, e) for h in full]
        # the text's own beginning is found, exactly and behind one replaced byte; one byte further in front it is not
        assert all(any(d == 0 for _, _, d in h) for h, kd in zip(exp, kind) if kd == "base")
        assert all(h and min(d for _, _, d in h) == 1 for h, kd in zip(exp, kind) if kd in ("first", "other"))
        assert all(not h for h, kd in zip(exp, kind) if kd == "extended")
    assert all(not approx_ref.within(h, 0) for h, kd in zip(full, kind) if kd == "first")
    hip = open_text(s, layout)
    for e in (0, 1, 2):
        check(hip, pats, e, [approx_ref.within(h, e) for h in full], what="prefix", steps=steps[e])
    hip.close()


# ---------------------------------------------------------------- e = 0 is the exact search
@pytest.mark.parametrize("layout", LAYOUTS)
def test_budget_zero_is_the_exact_search(layout):
    index = synth_bwt(4500, 97, 100, seed=31)
    orc = oracle.NaiveFMSearcher.from_mem(*index)
    rng = np.random.default_rng(32)
    walks = lf_walk_patterns(orc, rng, 5000, 16, 0.5, alphabet=[97, 98, 99, 100])
    # more patterns than three times the waves any grid can have: the 5000 walks over and over, each time in another order
    k = 3 * waves_max() + 5
    order = np.concatenate([rng.permutation(len(walks)) for _ in range(-(-k // len(walks)))])[:k]
    assert k > len(walks) and sorted(order[:len(walks)].tolist()) == list(range(len(walks)))
    pats = [walks[j] for j in order.tolist()]
    print("e = 0: k = %d patterns, at most %d waves" % (k, waves_max()))
    buf, off = pack_patterns(pats)
    hip = open_index(index, layout)
    hip.config_set("jump", "off")
    hip.config_set("ktab", "off")
    hip.stats_reset()
    sp, ep = hip.search_batch(buf, off)
    st = hip.stats()
    exact_steps = st["backward_steps"]
    assert st["ktab_lookups"] == 0 and st["jump_lookups"] == 0 and st["row_lookups"] == 0
    osp, oep, osteps = orc.search_batch(buf, off)
    assert exact_steps == int(osteps.sum())
    seen, launches = st["patterns_seen"], st["launches"]
    got_off, hits = hip.search_approx_batch(buf, off, 0)
    found = sp < ep
    assert 1000 < int(found[:len(walks)].sum()) < 4500       # (the first 5000 are the walks themselves, each once)
    assert np.array_equal(np.diff(got_off.astype(np.int64)), found.astype(np.int64))
    assert np.array_equal(hits["pattern"], np.nonzero(found)[0]) and not hits["mismatches"].any()
    assert np.array_equal(hits["sp"], sp[found]) and np.array_equal(hits["ep"], ep[found])
    _, _, steps, requests = hip.approx_last()
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
    assert L.fmx_search_approx_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, None, o2.ctypes.data,
                                     h2.ctypes.data, h2.size, ctypes.byref(n_out)) == 0
    assert n_out.value == hits.size and np.array_equal(o2, got_off) and h2.tobytes() == hits.tobytes()
    hip.close()


# ---------------------------------------------------------------- several patterns per wave, e >= 1
class Pool:
    """Distinct patterns with their hits at e = 3 (flat arrays, each pattern's by ascending sp) and their walk steps per
    budget: a batch is an array of pool indices, and its expectation is expanded from the pool's with numpy."""

    def __init__(self, s, pats, budgets):
        orc = approx_ref.index_of(s)[0]
        self.pats = pats
        self.len = np.array([len(p) for p in pats])
        full = [approx_ref.window_hits(s, p, 3) for p in pats]
        self.hits = np.array([h for hs in full for h in hs], dtype=np.int64).reshape(-1, 3)      # (sp, ep, d)
        self.owner = np.repeat(np.arange(len(pats)), [len(hs) for hs in full])
        self.steps = {e: np.array([walk_steps(orc, [p], e, [approx_ref.within(hs, e)]) for p, hs in zip(pats, full)],
                                  dtype=np.int64) for e in budgets}

    def expected(self, idx, e):
        """-> (off, records, steps) of the batch [pats[j] for j in idx] at budget e."""
        keep = self.hits[:, 2] <= e
        hits, owner = self.hits[keep], self.owner[keep]
        cnt = np.bincount(owner, minlength=len(self.pats))
        first = np.cumsum(cnt) - cnt
        per = cnt[idx]
        off = np.concatenate([[0], np.cumsum(per)])
        src = np.repeat(first[idx] - off[:-1], per) + np.arange(int(off[-1]))
        rows = np.zeros(int(off[-1]), dtype=HIT)
        rows["pattern"] = np.repeat(np.arange(idx.size), per)
        rows["sp"], rows["ep"], rows["mismatches"] = hits[src, 0], hits[src, 1], hits[src, 2]
        return off.astype(np.uint64), rows, int(self.steps[e][idx].sum())


@pytest.fixture(scope="module")
def many(abcd_text):
    """k = 3 * waves_max() + 5 patterns drawn with repetition from a pool over the abcd text: lengths 1, 6, 12 and 24 with
    0 - 2 bytes replaced, the empty pattern, and patterns that have no hit at any budget; and a second draw from the pool's
    patterns of at most 12 bytes for e = 3 (a pattern of 6 bytes has some 350 hits there)."""
    s = abcd_text
    rng = np.random.default_rng(38)
    pats = [b"", b"z" * 4, b"z" * 8, b"z" * 24, s[5:9] + b"zzzz" + s[13:17]]
    for m in (1, 6, 12, 24):
        pats += mutated(rng, s, m, [97, 98, 99, 100], 80)
    pats = sorted(set(pats))
    short = [p for p in pats if len(p) <= 12]
    pool = Pool(s, pats, (1, 2))
    pool3 = Pool(s, short, (3,))
    W = waves_max()
    k = 3 * W + 5
    idx = rng.integers(0, len(pats), k)
    idx3 = rng.integers(0, len(short), k)
    return pool, idx, pool3, idx3, W


def test_many_expectations_are_the_ones_the_kernel_needs(many):
    pool, idx, pool3, idx3, W = many
    k = idx.size
    print("several patterns per wave: k = %d, waves_max = %d, pool of %d (%d of at most 12 bytes)"
          % (k, W, len(pool.pats), len(pool3.pats)))
    assert k >= 3 * W and k % 4 != 0 and 200 <= len(pool.pats) <= 400
    for p, ix in ((pool, idx), (pool3, idx3)):
        # a wave takes the patterns q, q + its stride, ...: whatever the stride (at most W), neighbours in that order differ
        assert (ix[:-W] != ix[W:]).mean() > 0.95 and (p.len[ix[:-W]] != p.len[ix[W:]]).mean() > 0.4
        assert (ix[:-4] != ix[4:]).mean() > 0.95
        assert (p.len[ix] == 0).sum() >= 10
    none = np.setdiff1d(np.arange(len(pool.pats)), pool.owner)
    assert none.size >= 4 and np.isin(idx, none).sum() >= 50          # patterns without a hit at e = 3, and so at any budget
    assert len({len(p) for p in pool.pats}) >= 7
    for e in (1, 2):
        _, rows, steps = pool.expected(idx, e)
        print("e = %d: %d hits, %d steps" % (e, rows.size, steps))
        assert rows.size > 50_000 and (rows["mismatches"] == e).sum() > 25_000
    _, rows, steps = pool3.expected(idx3, 3)
    print("e = 3: %d hits, %d steps" % (rows.size, steps))
    assert 1_000_000 < rows.size < 5_000_000 and (rows["mismatches"] == 3).sum() > 500_000


@pytest.mark.parametrize("layout", LAYOUTS)
def test_several_patterns_per_wave(many, abcd_text, layout):
    """Every wave's loop over the batch goes round three times and more, with e = 1, 2 and 3: the wave starts each pattern
    from the root, whatever depth, round and frames the one before left behind.  Offsets and record bytes exactly, the
    call's steps those of approx_ref.walk, and the handle's counters moved by them once per launch."""
    pool, idx, pool3, idx3, W = many
    hip = open_text(abcd_text, layout)
    for p, ix, budgets in ((pool, idx, (1, 2)), (pool3, idx3, (3,))):
        buf, off = pack_patterns([p.pats[j] for j in ix.tolist()])
        for e in budgets:
            exp_off, exp, steps = p.expected(ix, e)
            assert 50_000 < exp.size < 5_000_000                    # asserted before the call: 24 bytes a record
            st0 = hip.stats()
            got_off, got = hip.search_approx_batch(buf, off, e)
            st1 = hip.stats()
            assert np.array_equal(got_off, exp_off), e
            assert got.tobytes() == exp.tobytes(), e
            _, _, got_steps, requests = hip.approx_last()
            print("%s e = %d: k = %d, %d hits, %d steps (walk: %d), %d requests" % (layout, e, ix.size, got.size, got_steps, steps, requests))
            assert got_steps == steps and 0 < requests <= 4 * steps, (e, got_steps, steps, requests)
            # the counting call and the call that fetched the hits
            assert st1["launches"] == st0["launches"] + 2
            assert st1["backward_steps"] - st0["backward_steps"] == 2 * steps, e
    hip.close()


# ---------------------------------------------------------------- step counts on real texts, e = 1 .. 3
@pytest.fixture(scope="module")
def counted(dense, wide):
    """One dense and one wide-alphabet batch with the steps of approx_ref.walk: 40 patterns each of 6 and of 24 bytes over
    the abcd text, 8 each of 6 and of 12 bytes over the text of 255 symbols (a node of several rows steps 254 candidates
    there, so the walk is not cheap on the host)."""
    s, per_m = dense["abcd"]
    pats = per_m[6][0][:40] + per_m[24][0][:40]
    full = per_m[6][1][:40] + per_m[24][1][:40]
    ws, cases = wide
    by_m = {m: (p, f) for m, e, p, f in cases if e == 3}
    wpats = by_m[6][0][:8] + by_m[12][0][:8]
    wfull = by_m[6][1][:8] + by_m[12][1][:8]
    out = []
    for name, text, pp, ff in (("abcd", s, pats, full), ("wide", ws, wpats, wfull)):
        orc = approx_ref.index_of(text)[0]
        out.append((name, text, pp, ff, {e: walk_steps(orc, pp, e, [approx_ref.within(h, e) for h in ff]) for e in (1, 2, 3)}))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_step_counts_on_a_dense_and_a_wide_alphabet(counted, layout):
    for name, text, pats, full, steps in counted:
        hip = open_text(text, layout)
        for e in (1, 2, 3):
            check(hip, pats, e, [approx_ref.within(h, e) for h in full], what=name, steps=steps[e])
        hip.close()


# ---------------------------------------------------------------- long and ragged patterns
LONG_M = (0, 1, 25, 64, 65, 255, 256, 257, 1000, 2999, 3000, 3001)


@pytest.fixture(scope="module")
def long_case(abcd_text):
    """Per length the text's own substring and copies with one, two and three bytes replaced, at the first, a middle and
    the last position; 3000 is the whole text, and 3001 -- as long as the index, its sentinel included -- the text with
    byte 0 behind it and in front of it (the loop steps from the row of the whole text to the sentinel's: both occur), and a
    pattern of that length that does not occur.  In mixed order."""
    s = abcd_text
    rng = np.random.default_rng(39)
    pats = []
    for m in LONG_M:
        if m > len(s):
            bases = [s + b"\0", b"\0" + s, s[1:] + b"ab"]
        else:
            at = 0 if m >= len(s) - 1 else int(rng.integers(1, len(s) - m))
            bases = [s[at:at + m]]
        for base in bases:
            pats.append(base)
            where = sorted({0, m // 2, m - 1}) if m else []
            for pos in [(p,) for p in where] + ([(where[0], where[-1]), tuple(where[:2])] if len(where) >= 2 else []) + \
                    ([tuple(where)] if len(where) == 3 else []):
                p = bytearray(base)
                for j in pos:
                    p[j] = 97 + (p[j] - 97 + 1 + int(rng.integers(0, 3))) % 4 if p[j] else 97
                pats.append(bytes(p))
    pats = [pats[j] for j in rng.permutation(len(pats)).tolist()]
    full = [approx_ref.window_hits(s, p, 3) for p in pats]
    orc = approx_ref.index_of(s)[0]
    steps = [walk_steps(orc, pats, e, [approx_ref.within(h, e) for h in full]) for e in range(4)]
    return pats, full, steps


@pytest.mark.parametrize("layout", LAYOUTS)
def test_long_and_ragged_patterns(long_case, abcd_text, layout):
    """An exact tail walks i - 1 steps in one lane group and a long pattern lives under the one-row rule: up to 3001 bytes,
    hits behind three replaced bytes 1000 and more bytes apart, the whole text, and the text with its sentinel."""
    s = abcd_text
    pats, full, steps = long_case
    assert {len(p) for p in pats} == set(LONG_M)
    deep = [len(p) for p, h in zip(pats, full) if len(p) >= 1000 and any(d == 3 for _, _, d in h)]
    print("long patterns: %d of %d bytes in all, with a hit at d = 3: lengths %s; steps %s"
          % (len(pats), sum(len(p) for p in pats), sorted(deep), steps))
    assert deep and max(deep) >= 3000
    eof = approx_ref.index_of(s)[0].eof
    assert full[pats.index(s)] == full[pats.index(s + b"\0")] == [(eof, eof + 1, 0)]      # the row of the whole text
    assert full[pats.index(b"\0" + s)] == [(0, 1, 0)]                                      # the sentinel's row
    assert not full[pats.index(s[1:] + b"ab")]
    hip = open_text(s, layout)
    for e in range(4):
        check(hip, pats, e, [approx_ref.within(h, e) for h in full], what="long", steps=steps[e])
    hip.close()


# ---------------------------------------------------------------- degenerate shapes
@pytest.fixture(scope="module")
def abcd_text():
    rng = np.random.default_rng(33)
    return bytes(rng.integers(97, 101, 3000, dtype=np.uint8))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_degenerate_shapes(abcd_text, layout):
    s = abcd_text
    hip = open_text(s, layout)
    n = len(s) + 1
    off, hits = hip.search_approx_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 2)        # k = 0
    assert off.tolist() == [0] and hits.size == 0
    assert hip.search_approx(b"", 2) == [(0, n, 0)]                                                          # k = 1, empty
    assert hip.search_approx(s[10:16], 0) == [approx_ref.window_hits(s, s[10:16], 0)[0]]
    for e in range(4):
        pats = [b"", s[5:11], b"", b"", s[100:103], b""]                                                      # empty ones between
        check(hip, pats, e, [approx_ref.window_hits(s, p, e) for p in pats], what="empties")
    pats = [b"a", b"d", b"z", b"\x00"]                       # m = 1, e = 3: every string over the range is a candidate
    check(hip, pats, 3, [approx_ref.window_hits(s, p, 3) for p in pats], what="m1e3")
    assert all(len(approx_ref.window_hits(s, p, 3)) == 4 for p in pats[:3])
    pats = [s[20:26] + b"z" + s[27:30], b"z" * 5, s[40:44] + b"\x00" + s[45:50], s[-4:] + b"\x00", b"\x00" + s[:3]]
    for e in range(3):                                       # a byte the index does not hold, and byte 0
        exp = [approx_ref.window_hits(s, p, e) for p in pats]
        assert e == 0 or (exp[0] and exp[2])
        assert exp[3] and exp[4]                             # the end of the text, and its beginning behind the sentinel
        check(hip, pats, e, exp, what="absent")
    rng = np.random.default_rng(34)
    pats = mutated(rng, s, 6, [97, 98, 99, 100], 100)
    for sub in ((98, 99), (2, 254), (100, 255), (1, 96)):
        for e in (1, 2):
            exp = [approx_ref.window_hits(s, p, e, *sub) for p in pats]
            check(hip, pats, e, exp, sub=sub, what=sub)
    narrow = sum(len(approx_ref.window_hits(s, p, 2, 98, 99)) for p in pats)
    assert 0 < narrow < sum(len(approx_ref.window_hits(s, p, 2)) for p in pats)
    hip.close()


def test_block_handles_are_unsupported():
    bwt = np.frombuffer(b"abracadabra", dtype=np.uint8).copy()
    bs = np.zeros(256, dtype=np.int64)
    for c in range(1, 256):
        bs[c] = bs[c - 1] + int((bwt == c - 1).sum())
    hip = findex_amd.HipFMSearcher.from_block(bwt, bs, 3)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_approx(b"abr", 1)
    assert ei.value.code == 6
    hip.close()


# ---------------------------------------------------------------- capacity, order, determinism
@pytest.mark.parametrize("layout", LAYOUTS)
def test_capacity_order_and_determinism(abcd_text, layout):
    s = abcd_text
    rng = np.random.default_rng(35)
    pats = mutated(rng, s, 6, [97, 98, 99, 100], 300)
    exp_off, exp = expected_arrays([approx_ref.window_hits(s, p, 2) for p in pats])
    T = exp.size
    assert T > 20_000
    hip = open_text(s, layout)
    buf, off = pack_patterns(pats)
    L = _lib.load()
    opts = _lib.fmx_approx_opts(2, 0, 0, 0)
    guard = 64

    def call(cap):
        out = np.full((cap + guard) * HIT.itemsize, 0xAB, dtype=np.uint8)
        out_off = np.zeros(off.size, dtype=np.uint64)
        n_out = ctypes.c_size_t()
        rc = L.fmx_search_approx_batch(hip.handle, buf.ctypes.data, off.ctypes.data, off.size - 1, ctypes.byref(opts),
                                       out_off.ctypes.data, out.ctypes.data if cap else None, cap, ctypes.byref(n_out))
        assert (out[cap * HIT.itemsize:] == 0xAB).all()      # nothing behind out[cap - 1]
        return rc, int(n_out.value), out_off, out[: cap * HIT.itemsize].view(HIT)

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
    # order: sp ascends strictly inside every pattern, and `pattern` is the CSR segment
    seg = np.repeat(np.arange(len(pats)), np.diff(o.astype(np.int64)))
    assert np.array_equal(h["pattern"], seg)
    same = seg[1:] == seg[:-1]
    assert (h["sp"][1:][same] > h["sp"][:-1][same]).all() and (h["sp"] < h["ep"]).all()
    assert int(o[-1]) == T
    hip.close()


# ---------------------------------------------------------------- the device form
@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_form_and_stream_capture(abcd_text, layout):
    import torch
    s = abcd_text
    rng = np.random.default_rng(36)
    pats = mutated(rng, s, 12, [97, 98, 99, 100], 500)
    hip = open_text(s, layout)
    buf, off = pack_patterns(pats)
    h_off, h_hits = hip.search_approx_batch(buf, off, 2)
    T, k = h_hits.size, len(pats)
    assert T > 500
    d_pat = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    guard = 256
    d_out_off = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    d_out = torch.full((T * HIT.itemsize + guard,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        n = hip.search_approx_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T,
                                        stream=st.cuda_stream)
    st.synchronize()
    assert n == T
    raw = d_out.cpu().numpy()
    assert raw[: T * HIT.itemsize].tobytes() == h_hits.tobytes() and (raw[T * HIT.itemsize:] == 0xCD).all()
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64), h_off)
    # too small: the exact total, nothing behind the capacity
    d_out.fill_(0xCD)
    with pytest.raises(findex_amd.FmxError) as ei:
        hip.search_approx_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T - 1)
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
            hip.search_approx_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), k, 2, d_out_off.data_ptr(), d_out.data_ptr(), T,
                                        stream=st.cuda_stream)
        except findex_amd.FmxError as e:
            err = e
        d_out_off.zero_()
        g.capture_end()
    assert err is not None and err.code == 5 and "stream capture" in str(err)
    d_out_off.fill_(7)
    g.replay()                                               # the capture is valid: its one node runs
    torch.cuda.synchronize()
    assert not d_out_off.cpu().numpy().any()
    del g
    assert hip.stats()["launches"] == launches
    hip.close()


# ---------------------------------------------------------------- the corpus
def test_corpus_locate_docs_with_mismatches(tmp_path):
    rng = np.random.default_rng(37)
    q = b"needlework"
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxy", dtype=np.uint8)
    names = ["a.txt", "b.txt", "c.txt", "d.txt", "e.txt"]
    docs = {nm: bytearray(rng.choice(letters, 300 + 17 * j).tobytes()) for j, nm in enumerate(names)}
    for nm in names:
        (tmp_path / nm).write_bytes(bytes(docs[nm]))
    order = [os.fsdecode(x) for x in findex_amd.list_files(str(tmp_path))]
    assert sorted(order) == names

    def plant(nm, at, text):
        docs[nm][at:at + len(text)] = text

    plant(order[0], 0, q)                                    # exact, at the beginning of the first file
    plant(order[0], 100, b"needlewerk")
    plant(order[1], 50, b"zeedlework")                       # the first byte
    plant(order[1], 150, b"needleworz")                      # the last byte
    plant(order[1], 200, b"nzzdlework")                      # two bytes: not within one
    plant(order[3], 30, q)
    plant(order[4], len(docs[order[4]]) - 10, b"needlewxrk")  # at the end of the last file
    # one that straddles two files: only the separator between them differs from the query
    docs[order[1]][-5:] = b"needl"
    docs[order[2]][:4] = b"work"
    for nm in names:
        (tmp_path / nm).write_bytes(bytes(docs[nm]))
    cs = findex_amd.HipCorpusSearcher(findex_amd.Corpus.from_dir(str(tmp_path)))
    assert [os.fsdecode(x) for x in cs.corpus.names] == order

    def scan(e):
        out = []
        for j, nm in enumerate(order):
            d = bytes(docs[nm])
            for at in range(len(d) - len(q) + 1):
                dist = sum(1 for x, y in zip(d[at:at + len(q)], q) if x != y)
                if dist <= e:
                    out.append((j, at, dist))
        return out

    exp = scan(1)
    assert len(exp) == 6 and sum(1 for x in exp if x[2] == 0) == 2
    doc, raw, mism = cs.locate_docs(q, max_mismatches=1)
    assert list(zip(doc.tolist(), raw.tolist(), mism.tolist())) == exp
    assert (1, len(docs[order[1]]) - 5) not in set(zip(doc.tolist(), raw.tolist()))      # the straddling window
    exp2 = scan(2)
    assert len(exp2) == 7
    doc, raw, mism = cs.locate_docs(q, max_mismatches=2)
    assert list(zip(doc.tolist(), raw.tolist(), mism.tolist())) == exp2
    # max_mismatches = 0 is what the call returned before: two arrays, the exact occurrences
    r0 = cs.locate_docs(q, max_mismatches=0)
    r1 = cs.locate_docs(q)
    assert len(r0) == 2 and len(r1) == 2
    assert list(zip(r0[0].tolist(), r0[1].tolist())) == [(j, at) for j, at, d in exp if d == 0]
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])
    cs.close()
