"""Pins tests/primitives_ref.py (Psi by a stable sort of the BWT bytes, LF its inverse, occ by searchsorted) before any
GPU test trusts it: against the CPU oracle -- the inverted lists and binary search of the project this one was modelled
on -- and against that project's own known answers.  No GPU."""
import os

import numpy as np
import pytest

import oracle
from helpers import (bwt_of_text, clustered_bwt, geometric_bwt, one_symbol_bwt, sparse_alphabet_bwt, synth_bwt)
from primitives_ref import PlainIndex

LENGTHS = (0, 1, 7, 40)


def compare_with_oracle(bwt, eof, counts, seed=0):
    """Every reference function against the oracle on one index: Psi and LF for every row (LF by getPrevI on every row
    of a small index and on a sample of a large one, and as the inverse of fm() everywhere), occ with its clamps, steps,
    class steps, both substring walks."""
    ref = PlainIndex(bwt, eof)
    orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
    n = ref.n
    assert orc.n == n and orc.eof == ref.eof
    assert [orc.cf(c) for c in range(256)] == ref.cf.tolist()
    fm = orc.fm().astype(np.int64)
    assert np.array_equal(ref.psi, fm) and ref.psi[0] == eof
    inv = np.empty(n, dtype=np.int64)
    inv[fm] = np.arange(n)
    assert np.array_equal(ref.lf, inv)
    rng = np.random.default_rng(seed)
    edge = np.array(sorted({0, eof, n - 1, min(eof + 1, n - 1), max(eof - 1, 0)}), dtype=np.int64)
    rows = np.arange(n) if n <= 5000 else np.unique(np.concatenate([rng.integers(0, n, 3000), edge]))
    assert [orc.getPrevI(int(r)) for r in rows] == ref.lf[rows].tolist()
    assert [orc.getNextI(int(r)) for r in rows[:2000]] == ref.psi[rows[:2000]].tolist()
    assert [orc.bwt_read(int(r)) for r in edge] == ref.B[edge].tolist()
    # occ: present symbols, 0, absent ones and 255; keys -1 .. n + 1
    present = np.nonzero(np.bincount(ref.B, minlength=256))[0]
    absent = np.setdiff1d(np.arange(256), present)
    syms = np.unique(np.concatenate([present, [0, 255], absent[:3], absent[-3:]])).astype(np.uint8)
    if n <= 449:
        c = np.repeat(syms, n + 3)
        i = np.tile(np.arange(-1, n + 2, dtype=np.int64), syms.size)
    else:
        c = rng.choice(syms, size=40_000)
        i = rng.integers(-1, n + 2, size=40_000, dtype=np.int64)
        i[:8] = [-1, 0, eof - 1, eof, min(eof + 1, n + 1), n - 1, n, n + 1]
    assert np.array_equal(ref.occ(c, i), orc.occ_batch(c, i))
    # steps on valid intervals, sp == ep and ep == n among them
    k = 6000
    a = rng.integers(0, n + 1, size=k)
    b = rng.integers(0, n + 1, size=k)
    sp, ep = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
    sp[:3], ep[:3] = [0, n, 0], [0, n, n]
    cc = rng.choice(syms, size=k)
    w1, w2 = orc.prev_range_batch(sp, ep, cc)
    g1, g2 = ref.prev_range(sp, ep, cc)
    assert np.array_equal(g1.astype(np.uint64), w1) and np.array_equal(g2.astype(np.uint64), w2)
    for x, y in ((0, n), (int(sp[5]), int(ep[5])), (n // 2, n)):
        for c0, c1 in ((0, 255), (97, 122), (255, 255), (5, 4), (int(present[-1]) + 1 if present[-1] < 255 else 255, 255)):
            assert ref.interval_prev_range(x, y, c0, c1) == orc.getIntervalPrevRange(x, y, c0, c1), (x, y, c0, c1)
    # the walks
    wrows = np.unique(np.concatenate([edge, rng.integers(0, n, 120)]))
    for length in LENGTHS:
        pb, pe = ref.prev_substr(wrows, length)
        nb = ref.next_substr_host(wrows, length)
        wo, wl = ref.next_substr(wrows, length)
        for q, r in enumerate(wrows.tolist()):
            assert bytes(pb[q]) == orc.prevSubstr(r, length), (r, length)
            assert int(pe[q]) == orc.lf_chain(r, length), (r, length)
            assert nb[q] == orc.nextSubstr(r, length), (r, length)
            assert bytes(wo[q, :wl[q]]) == nb[q][::-1] and (wl[q] == length or wo[q, wl[q] - 1] == 0)
    orc.close()


@pytest.mark.parametrize("n", [1, 2, 449, 5000, 300_007])
def test_synthetic_indexes_against_the_oracle(n):
    for eof in sorted({0, n // 3, n - 1}):
        lo, hi = (1, 6) if n < 5000 else (3, 250)                     # absent symbols below, between (n < 5000) and above
        compare_with_oracle(*synth_bwt(n, lo, hi, seed=n + eof, eof=eof), seed=n)


DESIGNED = [("clustered-0", lambda: clustered_bwt(0)), ("clustered-third", lambda: clustered_bwt(200_000 // 3)),
            ("clustered-last", lambda: clustered_bwt(199_999)), ("geometric", geometric_bwt), ("sparse_alphabet", sparse_alphabet_bwt)] + \
           [("one_symbol-%d" % n, lambda n=n: one_symbol_bwt(n)) for n in (127, 128, 129, 447, 448, 449, 896, 897, 40_000)]


@pytest.mark.parametrize("name,make", DESIGNED, ids=[d[0] for d in DESIGNED])
def test_designed_indexes_against_the_oracle(name, make):
    compare_with_oracle(*make(), seed=len(name))


def test_designed_indexes_are_what_they_claim():
    """The properties the GPU tests rely on, from the bytes themselves."""
    bwt, eof, counts = clustered_bwt(200_000 // 3)
    assert counts[200] == 5 and counts[7] == 1 and counts.sum() == bwt.size - 1
    bwt, eof, counts = sparse_alphabet_bwt()
    assert np.nonzero(counts)[0].tolist() == [1, 3, 128, 254, 255] and counts[254] == counts[255] == 1
    p254, p255 = int(np.nonzero(bwt == 254)[0][0]), int(np.nonzero(bwt == 255)[0][0])
    assert p254 % 448 == 0 and p254 % 128 == 0 and (p255 + 1) % 448 == 0 and (p255 + 1) % 128 == 0
    bwt, eof, counts = geometric_bwt()
    assert np.all(counts[1:17] > 0) and counts[17:].sum() == 0 and counts[1] > 100 * counts[9]
    bwt, eof, counts = one_symbol_bwt(448)
    assert counts[97] == 447 and counts.sum() == 447


def test_known_answers_of_the_reference(testdata):
    """The known answers test_reference_kats_through_the_product asks of the HIP path, asked of the plain reference."""
    bwt, eof, _ = bwt_of_text(b"abracadabra")
    ref = PlainIndex(bwt, eof)
    assert ref.cf[0] == 0 and ref.cf[ord("a")] == 1 and ref.cf[ord("b")] == 6
    assert ref.psi.tolist() == [3, 0, 6, 7, 8, 9, 10, 11, 5, 2, 1, 4]
    assert ref.lf[6] == 2 and ref.psi[6] == 10 and ref.psi[10] == 1
    rows = {0: [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1], ord("a"): [1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 5, 5],
            ord("b"): [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2], ord("r"): [0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2], ord("x"): [0] * 12}
    for c, want in rows.items():
        assert ref.occ(np.full(12, c, dtype=np.uint8), np.arange(12)).tolist() == want
    bwt, eof, _ = bwt_of_text(b"mmabcacadabbbca"[::-1])
    ref = PlainIndex(bwt, eof)
    assert ref.occ([ord("b")], [6]).tolist() == [3]
    assert [int(v[0]) for v in ref.prev_range([0], [16], [ord("a")])] == [1, 6]
    assert [int(v[0]) for v in ref.prev_range([1], [6], [ord("b")])] == [6, 8]
    bwt, n, eof = oracle.load_bwt_file(os.path.join(testdata, "test1024.cmp.bwt"), bigEndian=False)
    ref = PlainIndex(np.asarray(bwt)[:n], eof)
    assert eof == 462 and ref.B[0] == ord("u") and ref.B[eof] == 0
    assert ref.lf[eof] == 0 and ref.psi[eof] == 517 and ref.lf[1] == 48 and ref.lf[48] == 649
    assert ref.next_substr_host([1], 3) == [b"haa"] and bytes(ref.prev_substr([1], 5)[0][0]) == b"bqxxa"
    assert bytes(ref.prev_substr([eof], 5)[0][0]) == b"\0uexm" and bytes(ref.prev_substr([ref.lf[eof]], 4)[0][0]) == b"uexm"
    assert ref.next_substr_host([eof], 100) == [
        b"ajrtzbeqwbxdfpwjflmmsseewuudgfbtzqenjqafwzcnfanycigwsflfvxojxpqhhzekjdkhgsptqveavquuoqujbezdkarayoml"]
    bwt, eof, _ = bwt_of_text(b"ippisissim"[::-1])
    ref = PlainIndex(bwt, eof)
    assert ref.psi[[0, 5, 4, 10, 9]].tolist() == [5, 4, 10, 9, 3]
    assert ref.lf[[3, 9, 10, 4, 5, 0]].tolist() == [9, 10, 4, 5, 0, 1]
