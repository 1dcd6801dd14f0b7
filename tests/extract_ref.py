"""Extraction by text position, restated in Python over the oracle's LF (CPU only): the inverse-SA samples by a
bwt_fm2sa-style walk, a range cut into pieces as include/fmx.h (extract) defines them, every piece a walk on a counter.

Definitions (fmx.h, locate): s = reverse(text) + sentinel, n = len + 1 rows; SA[0] = n - 1, SA[LF r] = SA[r] - 1; the row with
SA == v (v >= 1) holds the BWT byte s[v - 1] = text[n - 1 - v].  isa[j] = the row with SA == j * rate.  To emit from text
offset t: v = n - 1 - t, up = ceil(v / rate) * rate; up <= n - 1: start at isa[up / rate], skip up - v steps; otherwise start
at row 0 and skip n - 1 - v.  A range is cut at every t with (n - 1 - t) % rate == 0 and, as the kernel does, at every
multiple of `tile` in the batch's output."""
import numpy as np


def lf_of_fm(fm):
    """LF from the oracle's inverted list (fm = LF's inverse: Util.bwtFm2sa walks i = fm(i) upwards in SA)."""
    fm = np.asarray(fm, dtype=np.int64)
    lf = np.empty(fm.size, dtype=np.int64)
    lf[fm] = np.arange(fm.size, dtype=np.int64)
    return lf


def index_arrays(orc, bwt):
    """(BWT' as a list with 0 at the EOF row, LF as a list) of an oracle searcher and its BWT bytes."""
    b = np.array(bwt, dtype=np.uint8)
    b[orc.eof] = 0
    return b.tolist(), lf_of_fm(orc.fm()).tolist()


def isa_samples(lf, rate):
    """isa[j] = the row with SA == j * rate: one walk down from row 0 (SA n - 1)."""
    n = len(lf)
    isa = [0] * ((n - 1) // rate + 1)
    r = 0
    for v in range(n - 1, -1, -1):
        if v % rate == 0:
            isa[v // rate] = r
        r = lf[r]
    assert r == 0, "the LF cycle through row 0 is shorter than n"
    return isa


def isa_from_locate_samples(lf, rate):
    """The same array by the scatter: marked rows (SA % rate == 0) in row order with their SA."""
    n = len(lf)
    sa = [0] * n
    r = 0
    for v in range(n - 1, -1, -1):
        sa[r] = v
        r = lf[r]
    isa = [0] * ((n - 1) // rate + 1)
    for row in range(n):
        if sa[row] % rate == 0:
            isa[sa[row] // rate] = row
    return isa


def pieces(n, rate, pos, lengths, tile):
    """The pieces of a batch as (output offset, bytes, text offset): cut at range starts, at tile edges of the output and at
    every t with (n - 1 - t) % rate == 0."""
    out, j = [], 0
    for p0, ln in zip(pos, lengths):
        t, end = int(p0), int(p0) + int(ln)
        assert end <= n - 1
        while t < end:
            v = n - 1 - t
            take = min(end - t, tile - j % tile, rate if v % rate == 0 else v % rate)
            out.append((j, take, t))
            t += take
            j += take
    return out


def walk(bwt, lf, isa, rate, t, take):
    """One piece: (bytes, LF steps made).  A loop on a counter, no other exit."""
    n = len(lf)
    v = n - 1 - t
    assert 1 <= v and take >= 1
    up = -(-v // rate) * rate
    if up <= n - 1:
        row, skip = isa[up // rate], up - v
    else:
        row, skip = 0, n - 1 - v
    assert skip <= rate - 1 and take <= rate
    got = bytearray()
    for i in range(skip + take):
        if i >= skip:
            got.append(bwt[row])
        row = lf[row]
    return bytes(got), skip + take


def extract_batch(bwt, lf, isa, rate, pos, lengths, tile=1 << 60):
    """(the batch's bytes, LF steps, pieces, the longest walk)."""
    n = len(lf)
    out, steps, longest = bytearray(), 0, 0
    ps = pieces(n, rate, pos, lengths, tile)
    for j, take, t in ps:
        assert j == len(out)
        got, st = walk(bwt, lf, isa, rate, t, take)
        out += got
        steps += st
        longest = max(longest, st)
    return bytes(out), steps, len(ps), longest


def step_bounds(rate, lengths, tile):
    """What fmx.h promises of a batch's steps: n_bytes <= steps <= n_bytes + (rate - 1) (non-empty ranges + tiles +
    n_bytes / rate + 1)."""
    nb = int(sum(int(x) for x in lengths))
    ranges = sum(1 for x in lengths if int(x))
    return nb, nb + (rate - 1) * (ranges + -(-nb // tile) + nb // rate + 1)
