"""tests/planted_text.py against the from-the-definition references, without a device: the closed forms that
tests/test_gpu_top_bit.py takes for its expectations at 3 * 2^30 bytes are held here, on the same geometry scaled down to
about 3 * 2^12 bytes (line 2^11, tile 64, L0 = 24: two of 12 419 positions share 24 bytes over four symbols with a chance
below m^2 / 2 * 4^-24 = 2^-21), to repeats_ref.brute, to bytes.find through occ_ref.reduce_pairs, and to lcp_checker.kasai
over a numpy suffix sort; and the plan of the device test is held to the conditions its inputs must meet, which need the
offsets alone."""
import numpy as np
import pytest

import lcp_checker
import ngrams_ref
import occ_ref
import planted_text as pt
import repeats_ref
from test_gpu_build_text import np_suffix_array

SEEDS = (1, 2, 3, 4, 5)
MODES = ("all", "longest", "disjoint")


_made = {}


def scaled(seed):
    """(plan, text bytes) of the scaled geometry, made once per seed."""
    if seed not in _made:
        plan = pt.geometry(3 << 12, 1 << 11, 64, 24, 40, seed=seed)
        pt.check_blocks(plan)
        _made[seed] = (plan, pt.write(plan, pt.background(plan.m, 1000 + seed)).tobytes())
    return _made[seed]


def find_all(text, q):
    out, at = [], text.find(q)
    while at >= 0:
        out.append(at)
        at = text.find(q, at + 1)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_write_lays_blocks_and_flanks(seed):
    plan, text = scaled(seed)
    assert len(text) == plan.m == (3 << 12) + 131 and plan.thresholds == [24, 25, 40, 41, 128, 131, 132]
    planted = np.zeros(plan.m, dtype=bool)
    for b in plan.blocks:
        for i, t in enumerate(b.copies):
            assert text[t:t + len(b)] == b.data
            planted[t:t + len(b)] = True
            for at, f in ((t - 1, b.before[i]), (t + len(b), b.after[i])):
                if f is not None:
                    assert text[at] == f and f not in pt.SYMS and f not in (0, 1, pt.STOP)
                    planted[at] = True
                else:
                    assert at < 0 or at == plan.m or any(c <= at < c + len(o) for o in plan.blocks for c in o.copies)      # the copy that abuts
    rest = np.frombuffer(text, dtype=np.uint8)[~planted]
    assert set(rest.tolist()) == set(pt.SYMS) and np.array_equal(rest, pt.background(plan.m, 1000 + seed)[~planted])
    x, z, zp = plan.block["X"], plan.block["Z"], plan.block["Z'"]
    assert x.data.count(bytes([pt.STOP])) == 1 and x.before[0] is None and x.after[-1] is None and x.copies[-1] + len(x) == plan.m
    assert z.copies[2] == z.copies[1] + plan.L0 and z.after[1] is None and z.before[2] is None
    assert zp.copies[2] == zp.copies[1] + plan.L0 + 1 and zp.after[1] == zp.before[2] and zp.after[1] is not None


@pytest.mark.parametrize("seed", SEEDS)
def test_repeat_ranges_against_the_definition(seed):
    plan, text = scaled(seed)
    for stop in (0, pt.STOP):
        for keep_first in (False, True):
            for L in plan.thresholds:
                got_r, got_s = pt.repeat_ranges(plan, L, keep_first, stop)
                want_r, want_s = repeats_ref.brute(text, L, keep_first, stop)
                assert got_s == want_s, (L, keep_first, stop)
                assert got_r.dtype == np.uint64 and np.array_equal(got_r, want_r), (L, keep_first, stop)
                assert list(got_s) == list(repeats_ref.FIELDS) == list(pt.FIELDS)
                # the flagged windows themselves, from the text: every window whose bytes stand twice or more
                starts = pt.window_starts(plan, L, keep_first, stop).tolist()
                assert len(starts) == want_s["windows"] and all(len(find_all(text, text[t:t + L])) >= 2 for t in starts[:40] + starts[-40:])
    # the cases the geometry is there for
    r64 = pt.repeat_ranges(plan, plan.L0)[0].tolist()
    z, zp = plan.block["Z"], plan.block["Z'"]
    assert [z.copies[1], z.copies[2] + plan.L0] in r64                                  # two abutting copies: one range
    assert [zp.copies[1], zp.copies[1] + plan.L0] in r64 and [zp.copies[2], zp.copies[2] + plan.L0] in r64
    assert pt.repeat_ranges(plan, 2 * plan.tile, stop=pt.STOP)[1]["ranges"] == 0 and pt.repeat_ranges(plan, 2 * plan.tile)[1]["ranges"] == 5
    assert pt.repeat_ranges(plan, plan.L0)[1]["largest_class"] == 7 and pt.repeat_ranges(plan, 41)[1]["largest_class"] == 5


def slices_of(plan):
    """[(block, lo, hi)]: chains of overlapping slices of X, Y whole and in parts, Z and Z', the text's two ends."""
    x, y = plan.block["X"], plan.block["Y"]
    k = plan.min_slice
    out = [(x, o, o + k + 1) for o in range(0, len(x) - k - 1, k // 2) if pt.STOP not in x.data[o:o + k + 1]]
    out += [(y, 0, len(y)), (y, 3, 3 + k), (y, len(y) - k, len(y)), (x, 0, k), (x, len(x) - k, len(x))]
    return out + [(plan.block[name], 0, plan.L0) for name in ("Z", "Z'") if plan.L0 >= k]


@pytest.mark.parametrize("seed", SEEDS)
def test_occurrence_pairs_against_bytes_find(seed):
    plan, text = scaled(seed)
    assert plan.min_slice == 27
    got, want = [], []
    for b, lo, hi in slices_of(plan):
        at = pt.occurrence_pairs(plan, b, lo, hi)
        assert at == find_all(text, b.data[lo:hi]) and len(at) == len(b.copies), (b.name, lo, hi)
        got += [(p, hi - lo) for p in at]
        want += [(p, hi - lo) for p in find_all(text, b.data[lo:hi])]
    assert len(got) > 50
    for mode in MODES:
        assert occ_ref.reduce_pairs(got, mode) == occ_ref.reduce_pairs(want, mode)
    assert len(occ_ref.reduce_pairs(got, "disjoint")) < len(occ_ref.reduce_pairs(got, "longest")) <= len(occ_ref.reduce_pairs(got, "all"))
    with pytest.raises(AssertionError):
        pt.occurrence_pairs(plan, plan.block["X"], 0, plan.min_slice - 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_lcp_rows_against_kasai(seed):
    plan, text = scaled(seed)
    s = lcp_checker.s_of_text(text)
    sa = np_suffix_array(np.frombuffer(s, dtype=np.uint8))
    lcp = lcp_checker.kasai(s, sa)
    row_of = np.empty(sa.size, dtype=np.int64)
    row_of[sa] = np.arange(sa.size)
    planted = set()
    for b in plan.blocks:
        for o in range(plan.L0 - 1, len(b)):
            values, want = pt.lcp_rows(plan, b, o)
            rows = row_of[values]
            assert want == o + 1 and np.array_equal(rows, rows[0] + np.arange(len(values))), (b.name, o)
            assert (lcp[rows[:-1]] == want).all() and lcp[rows[-1]] < want and (rows[0] == 0 or lcp[rows[0] - 1] < want), (b.name, o)
            planted.update(rows[:-1].tolist())
    # ... and no other row reaches L0: the array form names the same rows and values
    assert sorted(planted) == np.nonzero(lcp >= plan.L0)[0].tolist()
    v, nxt, val = pt.lcp_planted(plan)
    assert sorted(row_of[v.astype(np.int64)].tolist()) == sorted(planted)
    assert np.array_equal(lcp[row_of[v.astype(np.int64)]], val) and np.array_equal(sa[row_of[v.astype(np.int64)] + 1], nxt.astype(np.int64))
    assert int(lcp.max()) == len(plan.block["X"]) == int(val.max())


def class_rows(plan, classes, L, row_of):
    """sp of every class from the inverse suffix array: the rows of its copies, which must be consecutive."""
    sp = np.zeros(classes.size, dtype=np.int64)
    for j, at in enumerate(pt.ngram_occurrences(plan, classes, L)):
        rows = np.sort(row_of[at])
        assert np.array_equal(rows, rows[0] + np.arange(rows.size)), (L, j)
        sp[j] = rows[0]
    return sp


@pytest.mark.parametrize("seed", SEEDS)
def test_ngram_classes_against_the_definition(seed):
    plan, text = scaled(seed)
    s = lcp_checker.s_of_text(text)
    sa = np_suffix_array(np.frombuffer(s, dtype=np.uint8))
    row_of = np.empty(sa.size, dtype=np.int64)
    row_of[sa] = np.arange(sa.size)
    a = np.frombuffer(text, dtype=np.uint8)
    seen = set()
    for stop in (0, pt.STOP):
        for L in plan.thresholds:
            classes, summary = pt.ngram_classes(plan, L, stop)
            sp = class_rows(plan, classes, L, row_of)
            # the eligible window of the smallest row, for a length without a class
            t = plan.m - L - sa[sa <= plan.m - L]
            t = t[np.array([stop not in text[x:x + L] for x in t.tolist()], dtype=bool)] if stop else t
            lone = (int(row_of[plan.m - L - t[0]]), int(t[0])) if t.size else None
            rec, _ = ngrams_ref.brute(text, L, 1, "row", 0, stop)       # every eligible class, from the definition, once
            every = tuple(rec[f].astype(np.int64) for f in ("sp", "count", "first_pos"))
            for order in ("row", "count"):
                for top in (0, 3):
                    got_r, got_s = pt.ngram_result(classes, summary, sp, order, top, lone)
                    want_r, want_s = ngrams_ref.result(every, 2, order, top, 9)
                    assert got_r.dtype == ngrams_ref.RECORD and got_r.tobytes() == want_r.tobytes(), (L, stop, order, top)
                    assert list(got_s) == list(ngrams_ref.FIELDS) and got_s == {f: want_s[f] for f in ngrams_ref.FIELDS}, (L, stop, order, top, got_s, want_s)
            for bins in (1, 2, 6, 9):                             # 6: Y's seven copies are the overflow
                assert np.array_equal(pt.ngram_spectrum(classes, summary, bins), ngrams_ref.result(every, 2, "row", 0, bins)[1]["spectrum"]), (L, stop, bins)
            assert summary["windows"] == sum(not stop or stop not in text[x:x + L] for x in range(plan.m - L + 1))
            seen.add((classes.size > 0, summary["largest_pos"] is None))
            for c in classes[:3]:                                 # an entry is the window it names
                b = plan.blocks[int(c["block"])]
                assert text[int(c["first_pos"]):int(c["first_pos"]) + L] == b.data[int(c["offset"]):int(c["offset"]) + L]
    assert seen == {(True, False), (False, True)} and a.size == plan.m
    assert pt.ngram_classes(plan, plan.L0)[1]["largest_count"] == 7 and pt.ngram_classes(plan, 2 * plan.tile, pt.STOP)[0].size == 0


def test_the_device_plan_meets_its_input_conditions():
    """From the offsets alone: what tests/test_gpu_top_bit.py asserts again before it compares anything."""
    plan = pt.gpu_plan()
    line, m, T = 1 << 31, (3 << 30) + 4099, 2048
    assert (plan.m, plan.line, plan.tile, plan.L0) == (m, line, T, 64) and m + 1 < 1 << 32
    assert plan.thresholds == [64, 65, 300, 301, 4096, 4099, 4100] and plan.min_slice <= 40
    pt.check_blocks(plan)
    x, y, z, zp = (plan.block[k] for k in ("X", "Y", "Z", "Z'"))
    assert len(x) == 2 * T + 3 and x.data.find(bytes([pt.STOP])) == 1500 and x.data.count(bytes([pt.STOP])) == 1
    a = x.copies
    assert a[0] == 0 and a[1] < m - line < a[1] + len(x) and a[2] < line < a[2] + len(x) and a[3] > line and a[4] + len(x) == m
    assert len(y) == 300 and len(y.copies) == 7 and min(y.copies) > line
    assert len(z) == len(zp) == 64 and z.copies[2] - z.copies[1] == 64 and z.copies[2] % T == 0 and z.copies[2] > line
    assert zp.copies[2] - zp.copies[1] == 65 and zp.copies[2] == 5 << 29 and z.copies[0] < line and zp.copies[0] < line
    fig = pt.check_inputs(plan)
    print("device plan:", fig)
    r, s = pt.repeat_ranges(plan, 64)
    assert s["largest_class"] == 7 and s["largest_class_pos"] >= line
    assert pt.repeat_ranges(plan, 4096, stop=pt.STOP)[1]["ranges"] == 0 and pt.repeat_ranges(plan, 4096)[1]["ranges"] == 5
    assert pt.repeat_ranges(plan, 4100)[1] == dict.fromkeys(pt.FIELDS, 0)
    # occurrences: the chain of 40-byte slices of X has 100 positions and more on either side of the line
    pos = [p for j in range(201) if pt.STOP not in x.data[20 * j:20 * j + 40] for p in pt.occurrence_pairs(plan, x, 20 * j, 20 * j + 40)]
    assert sum(p >= line for p in pos) >= 100 and sum(p < line for p in pos) >= 100 and any(p < line < p + 40 for p in pos)
    # the u32 fields that carry their top bit: class ids r + 1 and positions above the line, the summary's size << 32 | ~t
    assert fig["lcp_sa_above"] > 1000 and fig["lcp_sa_below"] > 1000 and fig["lcp_rows"] == 4 * 4036 + 6 * 237 + 2 + 2
