"""Level K+1 of the k-mer table (fmx_ktab.hip, build_kext; k_search4<.., KX>): a search's first K+1 steps as one lookup.
Every result -- (sp, ep), the reference loop's step count and the rank queries it stands for -- must be the oracle's, with the
level on and off, by pairs of lanes and by quads.  Needs a real MI355X:  pytest -m gpu
"""
import os
import sys

import numpy as np
import pytest

import findex_amd
import oracle
from helpers import lf_walk_patterns, pack_patterns, synth_bwt
from helpers import table_default  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def search_checked(hip, orc, pats):
    """The batch on the device against the oracle: intervals, steps, rank queries.  Returns the device's stats."""
    buf, off = pack_patterns(pats)
    wsp, wep, wsteps = orc.search_batch(buf, off)
    hip.stats_reset()
    gsp, gep = hip.search_batch(buf, off)
    bad = np.nonzero((gsp != wsp) | (gep != wep))[0]
    assert bad.size == 0, [(pats[i], int(gsp[i]), int(gep[i]), int(wsp[i]), int(wep[i])) for i in bad[:5]]
    st = hip.stats()
    assert st["backward_steps"] == int(wsteps.sum()) and st["rank_queries"] == 2 * int(wsteps.sum())
    return st


def ke_of(k):
    """The k-mer level a search uses (fmx_search.hip, plan_of): the largest multiple of four up to K."""
    return 12 if k >= 12 else 8 if k >= 8 else 4 if k >= 4 else 0


def patterns_for(orc, syms, ke, seed):
    """Hits and misses of every length 1 .. KE+3, a miss at each of the first KE+1 steps, byte 0 and a foreign byte at
    each of those steps, walks from the rows next to the end of the text."""
    rng = np.random.default_rng(seed)
    syms = [int(s) for s in syms]
    foreign = next(b for b in range(1, 256) if b not in syms)
    pats = []
    for m in range(1, ke + 4):
        pats += lf_walk_patterns(orc, rng, 60, m, 0.3, alphabet=syms)
    base = lf_walk_patterns(orc, rng, 120, ke + 3, 0.0)
    for j in range(ke + 1):               # step j consumes the byte at len - 1 - j
        for i, p in enumerate(base):
            q = bytearray(p)
            q[len(q) - 1 - j] = [syms[int(rng.integers(0, len(syms)))], 0, foreign][i % 3]
            pats.append(bytes(q))
    for r0 in list(range(0, 6)) + [orc.n - 1]:      # the rows whose suffixes are the shortest
        for m in range(1, ke + 4):
            cs, r = [], r0
            for _ in range(m):
                cs.append(orc.bwt_read(r))
                r = orc.getPrevI(r)
            pats.append(bytes(reversed(cs)))
    pats += [b"", bytes([syms[0]]), b"\x00", bytes([foreign]) * (ke + 1)]
    return pats


def absent_neighbours(orc, syms, ke, seed):
    """Patterns whose Z is a KE-mer that does not occur (its X mostly does), and patterns whose X is one (their Z mostly
    occurs), with zero to two characters in front."""
    if len(syms) ** ke > 1 << 17:
        return []
    grid = np.array(np.meshgrid(*[syms] * ke, indexing="ij"), dtype=np.uint8).reshape(ke, -1).T
    mers = [bytes(r) for r in grid]
    buf, off = pack_patterns(mers)
    sp, ep, _ = orc.search_batch(buf, off)
    absent = [m for m, a, b in zip(mers, sp, ep) if a >= b][:40]
    rng = np.random.default_rng(seed)
    out = []
    for a in absent:
        for c in syms[:4]:
            lead = bytes(int(x) for x in rng.choice(syms, size=int(rng.integers(0, 3))))
            out += [lead + a + bytes([c]), lead + bytes([c]) + a]
    return out


def classify(orc, pats, ke):
    """How many patterns of length > KE have Z (the KE characters before the last) absent while X (the last KE) occurs,
    and how many the reverse."""
    def occurs(s):
        buf, off = pack_patterns([s])
        sp, ep, _ = orc.search_batch(buf, off)
        return int(ep[0]) > int(sp[0])
    za = xa = 0
    for p in pats:
        if len(p) > ke and 0 not in p[-ke - 1:]:
            x, z = occurs(p[-ke:]), occurs(p[-ke - 1:-1])
            za += (x and not z)
            xa += (z and not x)
    return za, xa


def run_both_ways(hip, orc, pats, lanes):
    """The batch with the level on and off on one handle (the per-handle key switches the kernel, the level stays)."""
    hip.config_set("search_lanes", lanes)
    hip.config_set("ktab_ext", "on")
    on = search_checked(hip, orc, pats)
    hip.config_set("ktab_ext", "off")
    off = search_checked(hip, orc, pats)
    hip.config_set("ktab_ext", "on")
    return on, off


def open_pair(bwt, eof, counts):
    return findex_amd.HipFMSearcher.from_mem(bwt, eof, counts), oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)


def biased_bwt(n, probs, seed):
    """Symbols 1 .. len(probs) drawn with those probabilities: a mildly biased text, whose rarest k-mers do not occur."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bwt = rng.choice(np.arange(1, len(probs) + 1, dtype=np.uint8), size=n, p=probs).astype(np.uint8)
    eof = n // 3
    counts = np.bincount(bwt, minlength=256).astype(np.int64)
    counts[bwt[eof]] -= 1
    return bwt, eof, counts


def kmer_rows(orc, syms, ke):
    """The number of rows of every one of the sigma^KE k-mers, by the oracle."""
    grid = np.array(np.meshgrid(*[syms] * ke, indexing="ij"), dtype=np.uint8).reshape(ke, -1).T
    buf = np.ascontiguousarray(grid).reshape(-1)
    sp, ep, _ = orc.search_batch(buf, np.arange(grid.shape[0] + 1, dtype=np.uint64) * ke)
    return np.where(ep > sp, ep - sp, 0).astype(np.int64)


EXT_MAX_LIST = 64       # kExtMaxList (fmx_ktab.hip): an index with a longer list gets no level K+1

# (n, lowest symbol, highest symbol, seed, symbol probabilities or None for uniform, the KE the shape must give).  K is the
# largest with sigma^K <= n / 8 (build_ktab) and KE the largest multiple of four up to it: 8^4 <= 2^13 < 8^5; 16^4 <= 2^16 <
# 16^5; 4^5 <= 2^10 < 4^6 (K = 5, used as 4); 3^8 = 6561 <= 2^13 < 3^9; 2^13 <= 2^13 (K = 13, used as 12); and the two
# biased texts, chosen with the oracle so that every KE-mer has at most 64 rows while more than 1 % of them have none
# (a stronger bias, or a Fibonacci word, would give lists longer than 64 and silently test the kernels without the level):
# 3^8 <= 2^13, and 2^12 <= 2^12 < 2^13.
SHAPES = {
    "sigma8-mean16": (1 << 16, 1, 8, 11, None, 4),
    "sigma16-mean8": (1 << 19, 1, 16, 12, None, 4),
    "sigma4-mean32": (1 << 13, 1, 4, 13, None, 4),
    "sigma3-ke8": (1 << 16, 1, 3, 14, None, 8),
    "sigma2-ke12": (1 << 16, 1, 2, 15, None, 12),
    "sigma3-ke8-biased": (1 << 16, 1, 3, 22, (0.39, 0.38, 0.23), 8),
    "sigma2-ke12-biased": (1 << 15, 1, 2, 24, (0.59, 0.41), 12),
}
ABSENT_KMERS = ("sigma16-mean8", "sigma3-ke8-biased", "sigma2-ke12-biased")      # the shapes with k-mers that do not occur


def test_shapes_reach_every_depth_the_level_is_compiled_for():
    assert {s[5] for s in SHAPES.values()} == {4, 8, 12}


@pytest.mark.parametrize("lanes", ["pairs", "quads"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_level_matches_oracle(table_default, lanes, name):
    n, lo, hi, seed, probs, want_ke = SHAPES[name]
    table_default("jump_pairs", "on")
    bwt, eof, counts = synth_bwt(n, lo, hi, seed) if probs is None else biased_bwt(n, probs, seed)
    syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
    assert len(syms) == hi - lo + 1
    table_default("ktab_ext", "off")
    without, _ = open_pair(bwt, eof, counts)
    without.prepare(ktab=True)
    table_default("ktab_ext", "on")
    hip, orc = open_pair(bwt, eof, counts)
    hip.prepare(ktab=True)
    # the level was built: sigma^KE entries of 32 bytes (and the overflow lists) beside the same levels
    assert hip.stats()["tables_held_bytes"] >= without.stats()["tables_held_bytes"] + 32 * len(syms) ** want_ke
    without.close()
    hip.prepare(ktab=True, jump=True)
    st = hip.stats()
    ke = ke_of(st["ktab_k"])
    assert ke == want_ke and st["jump_bytes"] == 32 * n, st
    pats = patterns_for(orc, syms, ke, seed) + absent_neighbours(orc, syms, ke, seed)
    za, xa = classify(orc, pats, ke)
    if probs is not None:
        rows = kmer_rows(orc, syms, ke)
        assert int(rows.max()) <= EXT_MAX_LIST and float((rows == 0).mean()) >= 0.01, (int(rows.max()), float((rows == 0).mean()))
    if name in ABSENT_KMERS:
        assert za > 0 and xa > 0, (za, xa)
    on, off = run_both_ways(hip, orc, pats, lanes)
    # the level serves the hits: fewer rank-dictionary lines, the same reference steps
    assert on["rank_queries"] == off["rank_queries"]
    assert on["search_requests"] < off["search_requests"], (on["search_requests"], off["search_requests"])
    # a batch of many patterns: several batches per wave, parked misses walked inside the batch loop too
    rng = np.random.default_rng(seed + 1)
    big = lf_walk_patterns(orc, rng, 6000, ke + 3, 0.5, alphabet=syms)
    run_both_ways(hip, orc, big, lanes)


def test_level_off_builds_nothing(table_default):
    table_default("jump_pairs", "on")
    bwt, eof, counts = synth_bwt(1 << 16, 1, 8, 11)
    table_default("ktab_ext", "on")
    a, _ = open_pair(bwt, eof, counts)
    a.prepare(ktab=True)
    table_default("ktab_ext", "off")
    b, _ = open_pair(bwt, eof, counts)
    b.prepare(ktab=True)
    sa, sb = a.stats(), b.stats()
    assert sa["ktab_k"] == sb["ktab_k"] == 4
    # 8^4 entries of 32 bytes, and the overflow lists, beside the same levels
    assert sa["tables_held_bytes"] >= sb["tables_held_bytes"] + 32 * 8 ** 4
    a.drop_tables(ktab=True)
    assert a.stats()["tables_held_bytes"] == 0


@pytest.mark.parametrize("lanes", ["pairs", "quads"])
def test_level_on_text(table_default, lanes):
    """The BWT of a text with the repeats of natural language (tools/text_bwt.py): its common words' k-mers have lists far
    longer than a lookup may scan (build_kext, kExtMaxList), so the handle gets no level K+1 -- and searches by both kernels
    stay the oracle's."""
    torch = pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import text_bwt
    table_default("jump_pairs", "on")
    text = text_bwt.make_text(torch, 1 << 23, 7, "cuda")      # (K = 4 over its ~28 symbols needs n >= 8 * 28^4)
    bwt_t, eof = text_bwt.bwt_of_reversed_text(torch, text)
    bwt = bwt_t.cpu().numpy().astype(np.uint8)
    eof = int(eof)
    counts = np.bincount(bwt, minlength=256).astype(np.int64)
    counts[bwt[eof]] -= 1
    held = []
    for ext in ("off", "on"):
        table_default("ktab_ext", ext)
        hip, orc = open_pair(bwt, eof, counts)
        hip.prepare(ktab=True, jump=True)
        assert ke_of(hip.stats()["ktab_k"]) >= 4
        held.append(hip.stats()["tables_held_bytes"])
    assert held[0] == held[1], "a level K+1 with lists longer than kExtMaxList"
    syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
    pats = patterns_for(orc, syms, 4, 5)
    on, off = run_both_ways(hip, orc, pats, lanes)
    assert on["search_requests"] == off["search_requests"]
