"""Two independent expectations for the matching statistics (fmx_match_stats_batch), loop_stats and brute_stats, and
mems_of, the MEM rule over a length array; none uses the library.

For byte j of pattern q, with e = j - off[q] + 1 and L = min(e, max_len): the reference's loop from (0, n) over pat[j],
pat[j - 1], .., stopped before the first step whose result is empty and after L steps at the latest.  len[j] is the number of
steps completed, (sp[j], ep[j]) the interval after the last of them."""
import numpy as np


def limits(off, n_bytes, max_len):
    """Per position: its pattern, e, and L = min(e, max_len)."""
    off = np.asarray(off, dtype=np.int64)
    j = np.arange(n_bytes, dtype=np.int64)
    q = np.searchsorted(off, j, side="right") - 1
    e = j - off[q] + 1
    return q, e, np.minimum(e, int(max_len))


def loop_stats(orc, pat, off, max_len):
    """The definition over the oracle's getPrevRange, one prev_range_batch call per round: round r steps every position that
    is still walking by pat[j - r].  -> (len, sp, ep, steps) per position, steps = len + 1 where the walk ended on an
    emptying step and len otherwise."""
    pat = np.ascontiguousarray(pat, dtype=np.uint8)
    nb = pat.size
    _, _, L = limits(off, nb, max_len)
    ln = np.zeros(nb, dtype=np.uint32)
    steps = np.zeros(nb, dtype=np.uint32)
    sp = np.zeros(nb, dtype=np.uint64)
    ep = np.full(nb, orc.n, dtype=np.uint64)
    live = np.nonzero(L > 0)[0]
    r = 0
    while live.size:
        a, b = orc.prev_range_batch(sp[live], ep[live], pat[live - r])
        steps[live] += 1
        ok = a < b
        go = live[ok]
        sp[go], ep[go] = a[ok], b[ok]
        ln[go] += 1
        r += 1
        live = go[L[go] > r]
    return ln, sp, ep, steps


def loop_stats_scalar(orc, pat, off, max_len):
    """The same, one getPrevRange call per step (tiny inputs): -> (len, sp, ep, steps) as lists."""
    pat = bytes(pat)
    _, _, L = limits(off, len(pat), max_len)
    out = ([], [], [], [])
    for j in range(len(pat)):
        sp, ep, i, st = 0, orc.n, 0, 0
        while i < L[j]:
            st += 1
            r = orc.getPrevRange(sp, ep, pat[j - i])
            if r is None:
                break
            sp, ep = int(r[0]), int(r[1])
            i += 1
        for lst, v in zip(out, (i, sp, ep, st)):
            lst.append(v)
    return out


def brute_stats(s, pat, off, max_len, chained=False):
    """Substring tests on the text s (patterns without byte 0): len[j] = the longest l <= L with pat[j - l + 1 .. j] in s.
    chained: the tests of position j begin at len[j - 1] + 1 (a string that occurs has its first l - 1 bytes occur), which
    makes long matches affordable; tests/test_mstat_cpu.py holds the two forms to each other."""
    s, pat = bytes(s), bytes(pat)
    assert 0 not in pat
    _, e, L = limits(off, len(pat), max_len)
    ln = np.zeros(len(pat), dtype=np.uint32)
    for j in range(len(pat)):
        l = int(L[j])
        if chained and e[j] > 1:
            l = min(l, int(ln[j - 1]) + 1)
        while l > 0 and pat[j - l + 1:j + 1] not in s:
            l -= 1
        ln[j] = l
    return ln


def text_stats(orc, s, pat, off, max_len, threads=1):
    """(len, sp, ep, steps) as loop_stats gives them, by another route: the lengths from the substring tests on the text s
    (chained), each position's interval from ONE exact search of the oracle for its matched suffix (orc.search_batch, on
    `threads` cores), the steps from the lengths: a walk that ends below its limit L made one emptying step more."""
    pat = np.ascontiguousarray(pat, dtype=np.uint8)
    ln = brute_stats(s, pat, off, max_len, chained=True)
    _, _, L = limits(off, pat.size, max_len)
    l64 = ln.astype(np.int64)
    soff = np.zeros(pat.size + 1, dtype=np.uint64)
    soff[1:] = np.cumsum(l64)
    total = int(soff[-1])
    # the suffix of position j is pat[j - len + 1 .. j]: byte t of the concatenation belongs to position j = owner[t]
    owner = np.repeat(np.arange(pat.size, dtype=np.int64), l64)
    within = np.arange(total, dtype=np.int64) - np.repeat(soff[:-1].astype(np.int64), l64)
    sbuf = pat[owner - l64[owner] + 1 + within] if total else np.zeros(0, dtype=np.uint8)
    sp, ep, st = orc.search_batch(sbuf, soff, threads=threads)
    assert (sp < ep).all() and np.array_equal(st.astype(np.int64), l64)
    steps = np.where(l64 < L, l64 + 1, l64).astype(np.uint32)
    return ln, sp, ep, steps


def mems_of(ln, off, min_len):
    """Byte j ends a reported match iff len[j] >= min_len and (j is the last byte of its pattern or len[j + 1] <= len[j]).
    -> (out_off[k + 1], [(pattern, len, end)]) with a pattern's hits by ascending end."""
    assert min_len >= 1
    off = [int(x) for x in off]
    out_off, rows = [0], []
    for q in range(len(off) - 1):
        for j in range(off[q], off[q + 1]):
            if ln[j] >= min_len and (j + 1 == off[q + 1] or ln[j + 1] <= ln[j]):
                rows.append((q, int(ln[j]), j - off[q] + 1))
        out_off.append(len(rows))
    return out_off, rows
