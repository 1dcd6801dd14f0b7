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


@pytest.mark.parametrize("lanes", ["pairs", "quads"])
@pytest.mark.parametrize("shape", [(1 << 16, 1, 8, 11), (1 << 19, 1, 16, 12), (1 << 13, 1, 4, 13)],
                         ids=["sigma8-mean16", "sigma16-mean8", "sigma4-mean32"])
def test_level_matches_oracle(table_default, lanes, shape):
    n, lo, hi, seed = shape
    table_default("jump_pairs", "on")
    table_default("ktab_ext", "on")
    bwt, eof, counts = synth_bwt(n, lo, hi, seed)
    hip, orc = open_pair(bwt, eof, counts)
    hip.prepare(ktab=True, jump=True)
    st = hip.stats()
    ke = ke_of(st["ktab_k"])
    assert ke >= 4 and st["jump_bytes"] == 32 * n, st
    syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
    pats = patterns_for(orc, syms, ke, seed) + absent_neighbours(orc, syms, ke, seed)
    za, xa = classify(orc, pats, ke)
    if shape[2] == 16:      # (only this shape has k-mers that do not occur: 16^4 of them for a mean of 8 rows)
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
