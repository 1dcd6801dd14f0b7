"""tests/top_bit_ref.py -- the torch references tests/test_gpu_top_bit.py runs on 3 * 2^30 bytes on the device -- on CPU tensors,
against lines_ref.Lines, lines_ref.occurrence_lines, linequery_ref.line_query and ngrams_ref.brute: the planted text of
tests/test_planted_text_cpu.py's scaled geometry (12 419 bytes), walked in steps of 1000 bytes so that every chunked pass
crosses many chunk edges; the suffix array from a numpy suffix sort."""
import numpy as np
import pytest
import torch

import lcp_checker
import linequery_ref
import lines_ref
import ngrams_ref
import occ_ref
import planted_text as pt
import top_bit_ref as tb
from test_gpu_build_text import np_suffix_array

STEP = 1000
SETS = (bytes([10]), bytes([10, 97, 98, 99]))


@pytest.fixture(scope="module")
def made():
    plan = pt.geometry(3 << 12, 1 << 11, 64, 24, 40, seed=3)
    pt.check_blocks(plan)
    text = pt.write(plan, pt.background(plan.m, 1003)).tobytes()
    assert len(text) == 12419 and text.count(b"\n") == 5
    s = lcp_checker.s_of_text(text)
    sa = np_suffix_array(np.frombuffer(s, dtype=np.uint8))
    row_of = np.empty(sa.size, dtype=np.int64)
    row_of[sa] = np.arange(sa.size)
    return plan, text, torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()), row_of


def occurrences(plan, text):
    """(off, occ): three groups -- slices of X, Y whole, none -- as fmx_occurrences would leave them."""
    x, y = plan.block["X"], plan.block["Y"]
    k = plan.min_slice
    xs = sorted(p for o in range(0, len(x) - k, 7) if pt.STOP not in x.data[o:o + k] for p in pt.occurrence_pairs(plan, x, o, o + k))
    ys = pt.occurrence_pairs(plan, y, 0, len(y))
    occ = np.zeros(len(xs) + len(ys), dtype=occ_ref.OCC)
    occ["pos"] = xs + ys
    occ["group"] = [0] * len(xs) + [1] * len(ys)
    occ["len"] = [k] * len(xs) + [len(y)] * len(ys)
    return np.array([0, len(xs), len(xs) + len(ys), len(xs) + len(ys)], dtype=np.uint64), occ


@pytest.mark.parametrize("breaks", SETS, ids=("newline", "newline_a_b_c"))
def test_lines_stand_in_against_lines_ref(made, breaks):
    plan, text, t, _ = made
    want = lines_ref.Lines(text, breaks)
    got = tb.Lines(t, breaks, step=STEP)
    assert got.brk.dtype == torch.int64 and np.array_equal(got.brk.numpy(), want.brk) and (got.len, got.n_brk) == (want.len, want.n_brk)
    assert torch.equal(got.brk, tb.break_positions(t, breaks[::-1], step=plan.m + 5))
    assert want.n_brk == 5 if len(breaks) == 1 else want.n_brk > plan.m // 2
    rng = np.random.default_rng(9)
    edge = np.concatenate([want.brk[:40], want.brk[:40] + 1, np.maximum(want.brk[:40] - 1, 0), want.brk[-3:], [0, plan.m - 1]])
    pos = np.concatenate([rng.integers(0, plan.m, 3000), edge[edge < plan.m]]).astype(np.int64)
    L = want.line(pos)
    for form in (lambda a: a, torch.from_numpy):                 # numpy in, numpy out; tensors in, tensors out
        back = (lambda a: a) if form(pos) is pos else (lambda a: a.numpy())
        assert np.array_equal(back(got.line(form(pos))), L)
        assert np.array_equal(back(got.start(form(L))), want.start(L)) and np.array_equal(back(got.end(form(L))), want.end(L))
    assert isinstance(got.line(pos), np.ndarray) and got.line(pos).dtype == np.int64 and torch.is_tensor(got.line(torch.from_numpy(pos)))
    # lookup and spans, with what lies outside
    far = np.concatenate([pos.astype(np.uint64), np.array([plan.m, plan.m + 1, 1 << 32, 1 << 63, 2 ** 64 - 1], dtype=np.uint64)])
    for a, b in zip(got.lookup(far), want.lookup(far)):
        assert a.dtype == np.uint64 and np.array_equal(a, b)
    for a, b in zip(got.lookup(torch.from_numpy(far.view(np.int64))), want.lookup(far)):
        assert np.array_equal(a.numpy().view(np.uint64), b)
    lines = np.concatenate([np.arange(0, min(want.n_brk + 4, 60)), [want.n_brk - 1, want.n_brk, want.n_brk + 1, 1 << 31, 1 << 63]]).astype(np.uint64)
    for a, b in zip(got.spans(lines), want.spans(lines)):
        assert a.dtype == np.uint64 and np.array_equal(a, b)
    for a, b in zip(got.spans(torch.from_numpy(lines.view(np.int64))), want.spans(lines)):
        assert np.array_equal(a.numpy().view(np.uint64), b)
    assert (want.spans(lines)[0][-2:] == lines_ref.NONE).all() and (want.lookup(far)[0][-5:] == lines_ref.NONE).all()
    # the directory entries between which dir[] crosses a line index
    if want.n_brk > 100:
        for shift in (4, 7):
            d = want.directory(shift).astype(np.int64)
            for line in (want.n_brk // 2, want.n_brk // 3 + 1):
                p = got.directory_crossings(shift, line)
                b = p[0] >> shift
                assert d[b] < line <= d[b + 1] and p == [b << shift, ((b + 1) << shift) - 1, (b + 1) << shift, ((b + 2) << shift) - 1]


@pytest.mark.parametrize("breaks", SETS, ids=("newline", "newline_a_b_c"))
def test_occurrence_lines_and_line_queries_over_the_stand_in(made, breaks):
    plan, text, t, _ = made
    want_lines, got_lines = lines_ref.Lines(text, breaks), tb.Lines(t, breaks, step=STEP)
    off, occ = occurrences(plan, text)
    want = lines_ref.occurrence_lines(want_lines, off, occ)
    got = lines_ref.occurrence_lines(got_lines, off, occ)
    assert np.array_equal(got[0], want[0]) and got[1].dtype == lines_ref.LINE_HIT and got[1].tobytes() == want[1].tobytes()
    assert want[0].tolist()[-1] == want[0].tolist()[-2] and want[1].size >= (5 if len(breaks) == 1 else 50)
    hoff, hits = want
    # anchored queries need no lines; ALL_LINES through the adapter: the candidates cut down to the lines near the positive term
    queries = [(0, [(1, 0, False)]), (None, [(1, 2, False)]), (None, [(0, 1, False), (1, 3, True)]), (0, [(1, 5, True)]),
               (None, [(1, 0, True), (0, 0, False), (2, "file", True)])]
    want_q = linequery_ref.line_query(hoff, hits, queries, lines=want_lines)
    got_q = tb.line_query(hoff, hits, queries, got_lines)
    assert np.array_equal(got_q[0], want_q[0]) and got_q[1].tobytes() == want_q[1].tobytes()
    assert want_q[1].size > 10 and (np.diff(want_q[0].astype(np.int64)) > 0).sum() >= 3
    # the real-lines records themselves: every line but the empty piece behind a final break
    every = linequery_ref.real_lines(want_lines)
    assert tb.line_records(got_lines, np.arange(-2, want_lines.n_brk + 3)).tobytes() == every.tobytes()


@pytest.mark.parametrize("L", (1, 2, 3))
def test_gram_table_against_brute(made, L, monkeypatch):
    plan, text, t, row_of = made
    monkeypatch.setattr(tb, "HEAD", 100)                         # both steps of a scatter, in every chunk
    rec, summary = ngrams_ref.brute(text, L, min_count=1, order="row")
    for rows in (torch.from_numpy(row_of), torch.from_numpy(row_of.astype(np.uint32).view(np.int32))):
        g = tb.gram_table(t, L, rows, step=STEP)
        by_row = torch.argsort(g["sp"])
        assert rec.size == g["code"].numel() == summary["distinct"] > 4 ** L // 2
        for f, key in (("sp", "sp"), ("count", "count"), ("first_pos", "first")):
            assert np.array_equal(g[key][by_row].numpy(), rec[f].astype(np.int64)), (L, f)
        for c, p in zip(g["code"].tolist()[:50], g["first"].tolist()):
            assert text[p:p + L] == c.to_bytes(L, "big")
    plain = tb.gram_table(t, L, step=plan.m)
    assert "sp" not in plain and all(torch.equal(plain[k], g[k]) for k in plain)
    bad = row_of.copy()
    i = plan.m - 5 - L                                            # the window at t = 5, and the first behind it that begins otherwise
    j = plan.m - next(x for x in range(6, plan.m) if text[x] != text[5]) - L
    bad[[i, j]] = bad[[j, i]]                                     # their rows swapped: a window's rows are no run any more
    with pytest.raises(AssertionError):
        tb.gram_table(t, L, torch.from_numpy(bad), step=STEP)
