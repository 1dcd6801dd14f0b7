"""A text whose repeats, occurrences and LCP rows are closed forms: blocks over a..d planted into i.i.d. a..d bytes.

Plain Python and numpy; no torch and nothing of the library.  A PLAN is the text length m, a line (the position whose two
sides a test wants to reach: 2^31 on the device), the scan tile T, a base threshold L0 and a list of blocks; a block is its
bytes (a..d, and at most a stop byte), the ascending text offsets of its copies and, per copy, the flank byte written before
and after it.  A side that is the text's start, the text's end or an abutting copy has no flank (None); two copies one byte
apart share that byte as a flank.  Flank bytes lie outside a..d and are never 0, 1 or the stop byte 10; among the copies of
one block the bytes in front of the copies are pairwise distinct (a flank, the last byte of an abutting copy, or nothing at
t = 0, where the index has its sentinel), and so are the bytes behind them.

What the closed forms rest on.  (1) The background holds no window of L0 bytes twice and none that a block holds: for i.i.d.
bytes over four symbols the chance is below m^2 / 2 * 4^-L0 (2^-66 at m = 3.2 * 10^9, L0 = 64).  (2) No two places inside the
blocks hold the same L0 - 1 bytes, and a window that runs from a copy into an abutting one occurs once: check_blocks()
decides this from the block bytes.  (3) A window that holds a flank byte is unique: a second one would have to hold the same byte at
the same place with equal bytes of background or of another block around it.  With these, a window of L >= L0 bytes occurs
twice or more iff it lies inside one copy of a block that has two or more copies, and then once per copy.  The tests hold
the closed forms to the from-the-definition references on scaled-down plans (tests/test_planted_text_cpu.py); a test on the
device does not assume (1): a natural repeat makes it fail."""
import math

import numpy as np

SYMS = b"abcd"
STOP = 10
FLANKS = bytes(x for pair in zip(range(101, 109), range(0xF0, 0xF8)) for x in pair)      # e, 0xF0, f, 0xF1, ...
FIELDS = ("ranges", "covered_bytes", "classes", "windows", "largest_class", "largest_class_pos")


class Block:
    def __init__(self, name, data, copies):
        self.name, self.data, self.copies = name, bytes(data), sorted(int(t) for t in copies)
        self.before = [None] * len(self.copies)
        self.after = [None] * len(self.copies)

    def __len__(self):
        return len(self.data)


class Plan:
    def __init__(self, m, line, tile, L0, blocks):
        self.m, self.line, self.tile, self.L0, self.blocks = int(m), int(line), int(tile), int(L0), list(blocks)
        self.block = {b.name: b for b in self.blocks}
        _assign_flanks(self)
        check_plan(self)

    @property
    def thresholds(self):
        """L0, L0 + 1, |Y|, |Y| + 1, 2 T, |X| = 2 T + 3, |X| + 1 -- the list of the device test, at the plan's scale."""
        y, x = len(self.block["Y"]), len(self.block["X"])
        return [self.L0, self.L0 + 1, y, y + 1, 2 * self.tile, x, x + 1]

    @property
    def min_slice(self):
        """The shortest slice occurrence_pairs answers for: the background holds a given slice of k bytes with a chance
        below m * 4^-k, 2^-40 from this length on."""
        return int(math.ceil((math.log2(self.m) + 40) / 2))


def _copies(plan):
    """Every copy as (start, end, block, index), ascending."""
    return sorted((t, t + len(b), b, i) for b in plan.blocks for i, t in enumerate(b.copies))


def _assign_flanks(plan):
    """Greedy: every flank position takes the first byte of FLANKS that the block behind it does not have in front of
    another copy and the block in front of it does not have behind another copy."""
    cs = _copies(plan)
    for j, (a, e, b, i) in enumerate(cs):
        prev_end = cs[j - 1][1] if j else None
        next_start = cs[j + 1][0] if j + 1 < len(cs) else None
        if a > 0 and prev_end != a:
            if prev_end == a - 1:                                 # the byte shared with the copy in front
                b.before[i] = cs[j - 1][2].after[cs[j - 1][3]]
            else:
                b.before[i] = next(f for f in FLANKS if f not in b.before)
        if e < plan.m and next_start != e:
            nb = cs[j + 1][2] if next_start == e + 1 else None
            b.after[i] = next(f for f in FLANKS if f not in b.after and (nb is None or f not in nb.before))


def byte_before(plan, b, i):
    """The byte in front of copy i of block b: its flank, the last byte of the copy that abuts, None at the text's start."""
    t = b.copies[i]
    if b.before[i] is not None or t == 0:
        return b.before[i]
    return next(o.data[-1] for a, e, o, _ in _copies(plan) if e == t)


def byte_after(plan, b, i):
    e = b.copies[i] + len(b)
    if b.after[i] is not None or e == plan.m:
        return b.after[i]
    return next(o.data[0] for a, _, o, _ in _copies(plan) if a == e)


def check_plan(plan):
    """The rules of the module's docstring that the offsets and flanks alone decide."""
    cs = _copies(plan)
    assert cs and cs[0][0] >= 0 and cs[-1][1] <= plan.m
    for (a0, e0, _, _), (a1, e1, _, _) in zip(cs, cs[1:]):
        assert e0 <= a1, "copies overlap at %d" % a1
    for b in plan.blocks:
        assert len(b) >= plan.L0 and set(b.data) <= set(SYMS) | {STOP}
        for i, t in enumerate(b.copies):
            assert (b.before[i] is None) == (t == 0 or any(e == t for _, e, _, _ in cs))
            assert (b.after[i] is None) == (t + len(b) == plan.m or any(a == t + len(b) for a, _, _, _ in cs))
            for f in (b.before[i], b.after[i]):
                assert f is None or (f in FLANKS and f not in SYMS and f not in (0, 1, STOP))
        front = [byte_before(plan, b, i) for i in range(len(b.copies))]
        back = [byte_after(plan, b, i) for i in range(len(b.copies))]
        assert len(set(front)) == len(front) and len(set(back)) == len(back), b.name


def runs(plan):
    """The maximal stretches of abutting copies: [(start, [(block, index), ...])]."""
    out = []
    for a, e, b, i in _copies(plan):
        if out and out[-1][2] == a:
            out[-1][1].append((b, i))
            out[-1][2] = e
        else:
            out.append([a, [(b, i)], e])
    return [(a, members) for a, members, _ in out]


def check_blocks(plan, k=None):
    """Rule (2): no two places inside the blocks hold the same k bytes (k = L0 - 1 by default, one byte less than any
    threshold: a window with a flank byte at its edge differs from another by its other L0 - 1 bytes), and a window of k
    bytes that runs from one copy into an abutting one is none of them and occurs once."""
    k = plan.L0 - 1 if k is None else k
    seen = {}
    for b in plan.blocks:
        for o in range(len(b) - k + 1):
            w = b.data[o:o + k]
            assert w not in seen, "blocks %s and %s share %d bytes" % (seen[w], b.name, k)
            seen[w] = b.name
    crossing = set()
    for _, members in runs(plan):
        if len(members) < 2:
            continue
        data = b"".join(b.data for b, _ in members)
        inside, at = set(), 0
        for b, _ in members:
            inside.update(range(at, at + len(b) - k + 1))
            at += len(b)
        for o in range(len(data) - k + 1):
            if o not in inside:
                w = data[o:o + k]
                assert w not in seen and w not in crossing, "a window across abutting copies occurs twice"
                crossing.add(w)


def pieces(plan):
    """[(offset, bytes)]: what write() lays over the background, in any order (no two overlap but a shared flank byte,
    which both carry with the same value)."""
    out = []
    for b in plan.blocks:
        for i, t in enumerate(b.copies):
            out.append((t, b.data))
            if b.before[i] is not None:
                out.append((t - 1, bytes([b.before[i]])))
            if b.after[i] is not None:
                out.append((t + len(b), bytes([b.after[i]])))
    return out


def background(m, seed):
    return (np.random.default_rng(seed).integers(0, len(SYMS), m, dtype=np.uint8) + SYMS[0]).astype(np.uint8)


def write(plan, bg):
    """The planted text: a copy of the background (uint8[m], a..d) with every piece laid over it."""
    text = np.array(bg, dtype=np.uint8, copy=True)
    assert text.shape == (plan.m,)
    for at, data in pieces(plan):
        text[at:at + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return text


# ---------------------------------------------------------------- repeats
def eligible(b, L, stop):
    """The offsets o in [0, |b| - L] whose window b[o : o + L] holds no stop byte, ascending (int64)."""
    if L > len(b):
        return np.zeros(0, dtype=np.int64)
    o = np.arange(len(b) - L + 1, dtype=np.int64)
    if stop:
        hits = np.concatenate(([0], np.cumsum(np.frombuffer(b.data, dtype=np.uint8) == stop)))
        o = o[hits[o + L] == hits[o]]
    return o


def window_starts(plan, L, keep_first=False, stop=0):
    """The text offsets of the flagged windows, ascending (int64)."""
    assert L >= plan.L0
    out = [np.zeros(0, dtype=np.int64)]
    for b in plan.blocks:
        o = eligible(b, L, stop)
        if len(b.copies) >= 2 and o.size:
            out += [t + o for t in b.copies[1 if keep_first else 0:]]
    return np.sort(np.concatenate(out))


def repeat_ranges(plan, L, keep_first=False, stop=0):
    """-> (ranges uint64[r, 2], summary dict) as fmx_repeats defines them, for a threshold L >= L0."""
    assert L >= plan.L0
    classes = windows = largest = pos = 0
    spans = []
    for b in plan.blocks:
        c = len(b.copies)
        o = eligible(b, L, stop)
        if c < 2 or not o.size:
            continue
        classes += int(o.size)
        windows += int(o.size) * (c - 1 if keep_first else c)
        first = b.copies[0] + int(o[0])
        if c > largest or (c == largest and first < pos):
            largest, pos = c, first
        cut = np.nonzero(np.diff(o) > L)[0]                       # windows more than L apart leave a byte uncovered
        lo = o[np.concatenate(([0], cut + 1))]
        hi = o[np.concatenate((cut, [o.size - 1]))] + L
        for t in b.copies[1 if keep_first else 0:]:
            spans += [(t + int(a), t + int(e)) for a, e in zip(lo, hi)]
    ranges = []
    for a, e in sorted(spans):
        if ranges and a <= ranges[-1][1]:                         # overlapping or abutting: one range
            ranges[-1][1] = max(ranges[-1][1], e)
        else:
            ranges.append([a, e])
    summary = dict(ranges=len(ranges), covered_bytes=sum(e - a for a, e in ranges), classes=classes, windows=windows,
                   largest_class=largest, largest_class_pos=pos)
    return np.array(ranges, dtype=np.uint64).reshape(-1, 2), summary


# ---------------------------------------------------------------- occurrences
def occurrence_pairs(plan, b, lo, hi):
    """The text positions of b.data[lo:hi], ascending: p_i + lo for every copy.  The slice has min_slice bytes or more,
    holds no stop byte and stands nowhere else in the blocks or across abutting copies (asserted here)."""
    q = b.data[lo:hi]
    assert 0 <= lo < hi <= len(b) and len(q) >= plan.min_slice and STOP not in q
    for o in plan.blocks:
        at, found = o.data.find(q), []
        while at >= 0:
            found.append(at)
            at = o.data.find(q, at + 1)
        assert found == ([lo] if o is b else []), (b.name, lo, hi, o.name)
    for _, members in runs(plan):
        if len(members) > 1:
            data = b"".join(x.data for x, _ in members)
            n_in = sum(1 for x, _ in members if x is b)
            count, at = 0, data.find(q)
            while at >= 0:
                count, at = count + 1, data.find(q, at + 1)
            assert count == n_in
    return [t + lo for t in b.copies]


# ---------------------------------------------------------------- n-grams
NGRAM_CLASS = np.dtype([("block", np.int64), ("offset", np.int64), ("count", np.int64), ("first_pos", np.int64)])
NGRAM_RECORD = np.dtype([("sp", np.uint64), ("count", np.uint64), ("first_pos", np.uint64)])
NGRAM_FIELDS = ("records", "selected", "distinct", "windows", "singletons", "largest_count", "largest_sp", "largest_pos")


def stop_positions(plan, stop):
    """The text positions of the stop byte, ascending: the background and the flanks hold none."""
    return sorted(t + o for b in plan.blocks for t in b.copies for o, x in enumerate(b.data) if stop and x == stop)


def eligible_windows(plan, L, stop=0):
    """How many of the m - L + 1 windows of L bytes hold no stop byte: the windows that hold position p begin in
    [p - L + 1, p]; the union of these stretches, cut at the text's two ends, is taken off."""
    if L > plan.m:
        return 0
    held, reach = 0, -1                                           # reach: the last window start already taken off
    for p in stop_positions(plan, stop):
        lo, hi = max(p - L + 1, 0, reach + 1), min(p, plan.m - L)
        if hi >= lo:
            held, reach = held + hi - lo + 1, hi
    return plan.m - L + 1 - held


def ngram_classes(plan, L, stop=0):
    """The windows of L >= L0 bytes that occur twice or more, and the closed forms of the n-gram summary.

    -> (classes, summary).  classes: a NGRAM_CLASS array, one entry per distinct repeated window -- by (1)-(3) of the
    module's docstring the windows that lie inside one copy of a block with two or more copies, once per copy -- as (index
    of the block in plan.blocks, offset in the block, count = the block's copies, first position = first copy + offset),
    eligibility as eligible() has it.  The entries stand in the order of their rows: the suffix array of
    s = reverse(T) + sentinel lists the windows by their reversed bytes, and no two classes share them.
    summary: windows (the eligible ones), distinct = windows - sum(count - 1), singletons = windows - sum(count),
    largest_count and largest_pos (the first position of the first class, in row order, of that count).  Without a class
    every eligible window is a singleton: largest_count is 1 and largest_pos None -- the window of the smallest row, which
    the plan does not name."""
    assert L >= plan.L0
    rows = []
    for k, b in enumerate(plan.blocks):
        if len(b.copies) >= 2:
            rows += [(b.data[o:o + L][::-1], k, int(o), len(b.copies), b.copies[0] + int(o)) for o in eligible(b, L, stop).tolist()]
    rows.sort()
    assert all(x[0] != y[0] for x, y in zip(rows, rows[1:]))
    classes = np.array([r[1:] for r in rows], dtype=np.int64).reshape(-1, 4)
    out = np.zeros(len(rows), dtype=NGRAM_CLASS)
    for j, f in enumerate(NGRAM_CLASS.names):
        out[f] = classes[:, j]
    windows = eligible_windows(plan, L, stop)
    total = int(out["count"].sum())
    summary = dict(windows=windows, distinct=windows - total + out.size, singletons=windows - total,
                   largest_count=int(out["count"].max()) if out.size else int(windows > 0), largest_pos=None if windows else 0)
    if out.size:
        summary["largest_pos"] = int(out["first_pos"][np.argmax(out["count"])])      # argmax: the first of the largest
    return out, summary


def ngram_occurrences(plan, classes, L):
    """int64[classes, copies as a ragged list]: per class the positions in s = reverse(T) + sentinel of its windows,
    m - t - L for every copy t + offset -- whose rows must be consecutive, the smallest of them the class's sp."""
    return [plan.m - (np.array(plan.blocks[int(c["block"])].copies, dtype=np.int64) + int(c["offset"])) - L for c in classes]


def ngram_result(classes, summary, sp, order="count", top=0, lone=None):
    """(records, summary) as fmx_ngrams defines them at min_count = 2, from ngram_classes' pair and the classes' sp (int64,
    in their order; ascending, as that is the row order).  lone: (sp, first_pos) of the eligible window in the smallest row,
    for a length without a class."""
    sp = np.asarray(sp, dtype=np.int64).reshape(-1)
    assert sp.size == classes.size and (np.diff(sp) > 0).all()
    pick = np.arange(sp.size) if order == "row" else np.lexsort((sp, -classes["count"]))
    kept = pick[:top] if top else pick
    rec = np.zeros(kept.size, dtype=NGRAM_RECORD)
    rec["sp"], rec["count"], rec["first_pos"] = sp[kept], classes["count"][kept], classes["first_pos"][kept]
    full = dict(summary, records=int(kept.size), selected=int(sp.size), largest_sp=0)
    if sp.size:
        full["largest_sp"] = int(sp[np.argmax(classes["count"])])
    elif summary["windows"]:
        full["largest_sp"], full["largest_pos"] = int(lone[0]), int(lone[1])
    return rec, {f: full[f] for f in NGRAM_FIELDS}


def ngram_spectrum(classes, summary, bins):
    """uint64[bins]: entry c the classes of count c, singletons included, entry 0 those of count >= bins."""
    spec = np.bincount(np.where(classes["count"] < bins, classes["count"], 0), minlength=bins).astype(np.uint64)
    spec[1 if bins > 1 else 0] += np.uint64(summary["singletons"])
    return spec


# ---------------------------------------------------------------- LCP
def row_order(plan, b):
    """The copies of b in the order their suffixes stand in the suffix array of s = reverse(T) + sentinel: a suffix that
    begins inside a copy reads the block backwards to its first byte and then the byte in front of the copy, which is
    different for every copy (the sentinel, the smallest, for a copy at t = 0)."""
    key = [byte_before(plan, b, i) for i in range(len(b.copies))]
    return sorted(range(len(b.copies)), key=lambda i: -1 if key[i] is None else key[i])


def lcp_rows(plan, b, o):
    """The suffixes of s that begin at offset o of each copy of b (o + 1 >= L0): -> (their SA values in row order, o + 1).
    They stand in consecutive rows; LCP of every such row but the last is o + 1, LCP of the last and of the row in front of
    the first is below o + 1."""
    assert plan.L0 - 1 <= o < len(b)
    return [plan.m - 1 - (b.copies[i] + o) for i in row_order(plan, b)], o + 1


def lcp_planted(plan):
    """Every row with LCP >= L0, as (sa uint64[k], sa_next uint64[k], lcp uint64[k]): the row holds SA value sa, the row
    below it sa_next, and its LCP is lcp -- lcp_rows for every block and every o, as arrays."""
    sa, nxt, val = [], [], []
    for b in plan.blocks:
        order = row_order(plan, b)
        o = np.arange(plan.L0 - 1, len(b), dtype=np.int64)
        for i, j in zip(order, order[1:]):
            sa.append(plan.m - 1 - (b.copies[i] + o))
            nxt.append(plan.m - 1 - (b.copies[j] + o))
            val.append(o + 1)
    return tuple(np.concatenate(x).astype(np.uint64) for x in (sa, nxt, val))


# ---------------------------------------------------------------- the geometry of the tests
def geometry(base, line, tile, L0, y_len, seed, stop_at=None):
    """The plan of tests/test_gpu_top_bit.py at any scale: m = base + 2 T + 3, line < base.

    X: 2 T + 3 bytes with one stop byte; copies at 0, around m - line (where SA values cross the line), around the line
       (a tile edge as well), wholly above it, and ending at m.
    Y: y_len bytes, seven copies above the line -- the largest class.
    Z: L0 bytes; one copy alone below the line, two that abut on the tile edge line + 3 line / 8: one range.
    Z': L0 bytes; one copy alone below the line, two copies L0 + 1 apart with one flank byte between them, which is the
       last byte of the tile that ends at line + line / 4: two ranges."""
    x_len = 2 * tile + 3
    m = base + x_len
    rng = np.random.default_rng(seed)

    def draw(k):
        return bytearray((rng.integers(0, len(SYMS), k, dtype=np.uint8) + SYMS[0]).tobytes())

    x = draw(x_len)
    x[x_len * 1500 // 4099 if stop_at is None else stop_at] = STOP
    up = m - line
    ez, ezp = line + 3 * (line // 8), line + line // 4
    assert line % tile == 0 and ez % tile == 0 and ezp % tile == 0 and L0 < y_len < 2 * tile
    blocks = [Block("X", x, [0, up - x_len // 2, line - x_len // 3, line + up // 3, m - x_len]),
              Block("Y", draw(y_len), [line + k * (up // 9) + up // 27 + 333 for k in range(1, 8)]),
              Block("Z", draw(L0), [line // 2 + 5, ez - L0, ez]),
              Block("Z'", draw(L0), [line // 2 + 5 + 4 * L0, ezp - L0 - 1, ezp])]
    return Plan(m, line, tile, L0, blocks)


def gpu_plan():
    """m = 3 * 2^30 + 4099, the line 2^31, T = 2048 (FMX_REPEATS_TILE), L0 = 64, Y of 300 bytes, X's stop byte at 1500."""
    return geometry(3 << 30, 1 << 31, 2048, 64, 300, seed=20, stop_at=1500)


def input_figures(plan):
    """What a test at the plan's scale must reach, from the expectation alone: a dict of counts."""
    line, m = plan.line, plan.m
    fig = dict(below=0, above=0, straddling=0, ends_at_m=0, starts_at_0=0, p_below=0, p_above=0, no_ranges=0, pos_above=0)
    for stop in (0, STOP):
        for keep_first in (False, True):
            for L in plan.thresholds:
                r, s = repeat_ranges(plan, L, keep_first, stop)
                a, e = r[:, 0].astype(np.int64), r[:, 1].astype(np.int64)
                fig["below"] += int((e <= line).sum())
                fig["above"] += int((a >= line).sum())
                fig["straddling"] += int(((a < line) & (e > line)).sum())
                fig["ends_at_m"] += int((e == m).sum())
                fig["starts_at_0"] += int((a == 0).sum())
                fig["no_ranges"] += int(r.shape[0] == 0)
                fig["pos_above"] += int(s["largest_class"] > 0 and s["largest_class_pos"] >= line)
                p = m - window_starts(plan, L, keep_first, stop) - L
                fig["p_below"] += int((p < line).sum())
                fig["p_above"] += int((p >= line).sum())
    sa, nxt, val = lcp_planted(plan)
    fig["lcp_rows"] = int(sa.size)
    fig["lcp_sa_below"] = int((sa < line).sum())
    fig["lcp_sa_above"] = int((sa >= line).sum())
    fig["lcp_max"] = int(val.max())
    return fig


def check_inputs(plan, fig=None):
    fig = input_figures(plan) if fig is None else fig
    for key in ("below", "above", "straddling", "ends_at_m", "starts_at_0", "p_below", "p_above", "no_ranges", "pos_above",
                "lcp_sa_below", "lcp_sa_above"):
        assert fig[key] > 0, (key, fig)
    assert fig["lcp_max"] == len(plan.block["X"])
    return fig
