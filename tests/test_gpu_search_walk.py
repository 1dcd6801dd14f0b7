"""The last walk of a k_search4 wave (fmx_search4.h, walk_last): the patterns a table lookup found to miss, finished behind the
batch loops -- one lane per parked pattern for everything that is not a rank step, lane groups for the rank steps.  Needs a
real MI355X:  pytest -m gpu -s

Every case runs in a child process with FMX_SEARCH_WGS=1 FMX_TRACE=1 (1024 waves; the child asserts it from its launch line)
and compares with oracle.NaiveFMSearcher over the same bytes: (sp, ep) bit for bit, misses' values included, the executed
steps, and -- on the same battery -- the 8-byte form and FMX_SEARCH_MISS_NONE.  The counters beside the steps
(`search_requests`, `ktab_lookups`, `jump_lookups`, `row_lookups`) are held to tests/golden/search_walk_counters.json: what the
commit before the new walk counted on these very inputs, recorded for every case whose counters repeated between two runs of
that commit.

Indexes: `iid` synth_bwt(300 000, 1, 12) and `text`, a real text of 3000 bytes (the head of README.md), whose LF walks cross
the EOF row.  In the first every one of the 12^4 four-character strings occurs (2 .. 33 rows each) and the second has no k-mer
level of four characters, so neither can hold a level K + 1 park whose last KT characters do not occur; `rare` is the first
index over eleven symbols with a twelfth in 30 rows, which the mixed waves below put into a pattern's last KT characters.
Forms (P = patterns per batch of a wave): `pairs` one-hot, pairs of lanes, pairs of row jump entries, level K + 1 (P = 32);
`quads` its quads twin (16); `single` single row jump entries by quads (16); `jumps` the same without the three-step table (16:
a miss at byte j of an entry is walked by j + 1 rank steps, so one behind the eighth outlives the eight characters the last
walk stages and is put back on the list); `rows3` one-hot with the three-step row table alone (16); `bytes3` the bytes layout with it (8).  `pairs` and `single` also run with `jump_chars` 8 and 11 on the first index, `jumps`
with 11 too; the
third index is searched by `pairs` and `quads`, the forms with level K + 1.

The battery is laid out BY WAVE.  Batch b of a launch goes to wave b mod 1024 while the rounds are strided, and wave w's class
is w mod 8: its batches hold, counted over its strided rounds and filled from the first round on, exactly
1, P - 1, P, P + 1, 64, 65 or 0 patterns that miss on one row (classes 0 .. 6; as many as its rounds can hold), the rest hits; the
misses sit at the front of a batch in even waves' batches, at the back in odd ones'.  Such a miss is an LF walk of 20 .. 60
characters with the character of one step s in 12 .. length - 1 replaced (by then the interval is one row on the first index):
by another symbol of the alphabet, by byte 0 or by a byte outside the alphabet.  s is uniform, so the misses fall on every byte of
a row jump entry, of the first and of the second one of a pair, on every byte of a three-step word, on the pattern's first
character (s = length - 1: the pattern ends exactly at the failing step) and fewer than eight characters before it.  Class 7 is
mixed: hits, such misses, patterns whose step KT (the fifth from the end on the first index) is replaced -- level K + 1 finds
the last KT + 1 characters absent, the last KT occur --, patterns with one of the last KT replaced (on `rare` by the rare
symbol: the last KT characters do not occur either), patterns of 0 .. 7 characters, and patterns of 4 .. 7 characters whose
first one is replaced (on the text they miss on one row at their last step: a parked pattern of fewer than eight characters).
Rounds: 3 for `pairs` (a class-5 wave holds 65 after its third batch, past the in-loop flush threshold of 64: the walk inside
the batch loop and the last one handle patterns parked by the same lookups); 5 for `quads`, `single` and `jumps` (no ticket pool);
`rows3` 5 and `bytes3` 9 strided rounds followed by two pooled rounds of hits of 1 .. 4 characters, which no wave hands to its
rows list, so what a wave parks does not depend on which batches it draws."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 120      # seconds
NW = 1024                # waves of a launch with FMX_SEARCH_WGS=1 on the 256 CUs of an MI355X
MAXLEN = 60
MINLEN = 20
ONE_ROW = 12             # the first step whose character is replaced in a one-row miss
GOLDEN = os.path.join(TESTS, "golden", "search_walk_counters.json")
# form -> (layout, per-handle keys, patterns per batch, strided rounds, pooled rounds, (JT, RW, R3T, G2) of the launch line)
FORMS = {
    "pairs": ("onehot", {"jump": "auto", "jump_pairs": "on", "search_lanes": "pairs", "ktab": "auto", "ktab_ext": "on"}, 32, 3, 0, (2, 0, 1, 1)),
    "quads": ("onehot", {"jump": "auto", "jump_pairs": "on", "search_lanes": "quads", "ktab": "auto", "ktab_ext": "on"}, 16, 5, 0, (2, 0, 1, 0)),
    "single": ("onehot", {"jump": "auto", "jump_pairs": "off", "search_lanes": "quads", "ktab": "auto", "ktab_ext": "off"}, 16, 5, 0, (1, 0, 1, 0)),
    "jumps": ("onehot", {"jump": "jumps", "jump_pairs": "off", "search_lanes": "quads", "ktab": "auto", "ktab_ext": "off"}, 16, 5, 0, (1, 0, 0, 0)),
    "rows3": ("onehot", {"jump": "rows3", "jump_pairs": "off", "search_lanes": "quads", "ktab": "auto", "ktab_ext": "off"}, 16, 5, 2, (0, 3, 0, 0)),
    "bytes3": ("bytes", {"jump": "rows3", "jump_pairs": "off", "ktab": "auto"}, 8, 9, 2, (0, 3, 0, 0)),
}
CASES = (["iid-%s-9" % f for f in FORMS] + ["text-%s-9" % f for f in FORMS] +
         ["iid-pairs-8", "iid-pairs-11", "iid-single-8", "iid-single-11", "rare-pairs-9", "rare-quads-9", "iid-jumps-11"])


def targets(per_wave, rounds):
    """Misses on one row a wave of classes 0 .. 6 holds after its strided rounds."""
    cap = per_wave * rounds
    return [min(v, cap) for v in (1, per_wave - 1, per_wave, per_wave + 1, 64, 65, 0)]


def battery(hip, syms, foreign, kt, per_wave, rounds, pooled, seed, rare=None):
    """(buf, off, kinds): the module's battery; kinds[i] = 0 hit, 1 miss on one row, 2 step KT replaced, 3 one of the last
    KT replaced, 4 short, 5 a pooled round's short hit, 6 short with its first character replaced."""
    rng = np.random.default_rng(seed)
    k = (rounds + pooled) * NW * per_wave
    idx = np.arange(k)
    batch, grp = idx // per_wave, idx % per_wave
    wave, rnd = batch % NW, batch // NW
    cls = wave % 8
    tgt = np.asarray(targets(per_wave, rounds) + [0])[cls]
    inb = np.clip(tgt - rnd * per_wave, 0, per_wave)                      # misses of this pattern's batch
    pos = np.where(wave % 2 == 0, grp, per_wave - 1 - grp)
    kinds = np.where(pos < inb, 1, 0)
    mixed = cls == 7
    u = rng.random(k)
    kinds = np.where(mixed, np.select([u < 0.35, u < 0.70, u < 0.85, u < 0.95, u < 0.975], [0, 1, 2, 3, 4], 6), kinds)
    kinds = np.where(rnd >= rounds, 5, kinds)
    lens = rng.integers(MINLEN, MAXLEN + 1, k)
    lens = np.where(kinds == 4, rng.integers(0, 8, k), lens)
    lens = np.where(kinds == 5, rng.integers(1, 5, k), lens)
    lens = np.where(kinds == 6, rng.integers(4, 8, k), lens)
    rows = rng.integers(0, hip.n, k).astype(np.uint64)
    b, _ = hip.lf_walk_batch(rows, MAXLEN)
    full = np.ascontiguousarray(b[:, ::-1])                               # step j of pattern i reads full[i, MAXLEN - 1 - j]
    step = np.zeros(k, dtype=np.int64)
    m1 = kinds == 1
    step[m1] = ONE_ROW + (rng.random(int(m1.sum())) * (lens[m1] - ONE_ROW)).astype(np.int64)
    step[kinds == 2] = kt
    m3 = kinds == 3
    step[m3] = rng.integers(0, max(kt, 1), int(m3.sum()))
    step[kinds == 6] = lens[kinds == 6] - 1
    mut = np.nonzero(((kinds >= 1) & (kinds <= 3)) | (kinds == 6))[0]
    old = full[mut, MAXLEN - 1 - step[mut]]
    sy = np.asarray(syms, dtype=np.uint8)
    other = sy[(np.searchsorted(sy, old) + rng.integers(1, len(syms), mut.size)) % len(syms)]      # a symbol that is not `old` (when old is one)
    v = rng.random(mut.size)
    new = np.where((kinds[mut] == 1) & (v < 0.1), 0, np.where((kinds[mut] == 1) & (v < 0.2), foreign, other))
    if rare is not None:
        new = np.where(kinds[mut] == 3, rare, new)
    new = new.astype(np.uint8)
    full[mut, MAXLEN - 1 - step[mut]] = new
    keep = np.arange(MAXLEN)[None, :] >= (MAXLEN - lens)[:, None]
    buf = np.ascontiguousarray(full[keep])
    off = np.zeros(k + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return buf, off, kinds


def child(index, form, jc):
    import findex_amd
    import oracle
    import search_forms as sf
    from helpers import bwt_of_text, index_of_bwt, lf_walk_patterns, pack_patterns, synth_bwt
    from test_gpu_search_ends import counters_of, traced
    findex_amd.config_set("tables_after", "0")
    layout, keys, per_wave, rounds, pooled, want_form = FORMS[form]
    rare = None
    if index == "iid":
        bwt, eof, counts = synth_bwt(300_000, 1, 12, 77)
    elif index == "rare":
        bwt, eof, _ = synth_bwt(300_000, 1, 11, 77)
        rare = 12
        bwt[np.random.default_rng(3).choice(bwt.size, 30, replace=False)] = rare
        bwt, eof, counts = index_of_bwt(bwt, eof)
    else:
        with open(os.path.join(ROOT, "README.md"), "rb") as f:
            text = f.read().replace(b"\0", b" ")
        text = (text * (3000 // max(1, len(text)) + 1))[:3000]
        bwt, eof, counts = bwt_of_text(text)
    orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
    syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
    foreign = next(b for b in range(1, 256) if b not in syms)
    findex_amd.set_layout(layout)
    hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
    for key, value in keys.items():
        # (the text's k-mer table is shallower than four characters: no level K + 1 to insist on)
        hip.config_set(key, "auto" if key == "ktab_ext" and index == "text" else value)
    hip.config_set("jump_chars", str(jc))
    hip.prepare(ktab=True, jump=True)
    st = hip.stats()
    kt = sf.kt_of(st["ktab_k"])
    assert st["jump_chars"] == (jc if want_form[0] else st["jump_chars"]), st["jump_chars"]
    buf, off, kinds = battery(hip, syms, foreign, kt, per_wave, rounds, pooled, 5, rare)
    # the edges by hand, behind the battery (a last, partial round of the launch): a pattern that ends exactly at the failing
    # step, one with fewer than eight characters left at the walk, byte 0 and a foreign byte at the failing step
    rng = np.random.default_rng(9)
    extra = []
    for base in lf_walk_patterns(orc, rng, 12, 40, 0.0):
        for at, c in ((0, syms[0]), (0, 0), (0, foreign), (3, 0), (6, foreign), (7, syms[-1]), (8, syms[1 % len(syms)])):
            q = bytearray(base)
            q[at] = c if q[at] != c else syms[2 % len(syms)]
            extra.append(bytes(q))
    if pooled == 0:      # (behind pooled rounds they would be drawn: the waves' lists would depend on the draw)
        eb, eo = pack_patterns(extra)
        off = np.concatenate([off, off[-1] + eo[1:]])
        buf = np.concatenate([buf, eb])
    out = orc.search_batch(buf, off, threads=min(16, len(os.sched_getaffinity(0))))
    wsp, wep, wsteps = out
    hit = wsp < wep
    nk = kinds.size
    fig = {"patterns": int(hit.size), "hits": int(hit.sum()), "kinds": np.bincount(kinds, minlength=7).tolist(),
           "misses_by_kind": np.bincount(kinds[~hit[:nk]], minlength=7).tolist()}
    assert 0.15 < hit.mean() < 0.9, fig
    assert index != "text" or fig["misses_by_kind"][6] > 100, fig
    if index != "text":
        # the battery is what the module says it is: hits hit, designed misses fail at their step, on one row from ONE_ROW on
        # (all but the few walks that reach the end of the text)
        assert hit[:nk][kinds == 0].mean() > 0.99 and (~hit[:nk][kinds == 1]).mean() > 0.99, fig
        assert fig["misses_by_kind"][2] > 0, fig
        # level K + 1 parks: the last KT + 1 characters absent with the last KT present (kind 2), and with those absent too
        def absent(kind, m):
            sel = np.nonzero((kinds == kind) & (np.diff(off[:nk + 1].astype(np.int64)) > m))[0][:3000]
            tb, to = pack_patterns([bytes(buf[int(off[i + 1]) - m:int(off[i + 1])]) for i in sel])
            a, b, _ = orc.search_batch(tb, to)
            return int((a >= b).sum())
        fig["kx_parks"] = [absent(2, kt + 1), absent(2, kt), absent(3, kt)]
        assert fig["kx_parks"][0] > 100 and fig["kx_parks"][1] == 0 and (rare is None or fig["kx_parks"][2] > 100), fig
    _, lines = traced(lambda: sf._compare(hip, out, buf, off, "walk"))
    assert len(lines) == 1, lines
    name, nb, nw, drawn, area = lines[0]
    got = tuple(int(x) for x in name[len("k_search4<"):-1].split(","))
    assert nw == NW and nb == (hit.size + per_wave - 1) // per_wave, lines
    assert (got[3], got[4], got[5], got[6]) == want_form and (index == "text" or got[7] == (1 if keys.get("ktab_ext") == "on" else 0)), name
    assert drawn == (pooled * NW if pooled else 0), lines
    fig["form"] = name
    fig["counters"] = counters_of(hip)
    sf._lean_forms(hip, out, buf, off)
    hip.close()
    findex_amd.set_layout("auto")
    print("RESULT " + json.dumps(fig))
    print("DONE")


_FAULT = []      # why no further child is started


@pytest.mark.gpu
@pytest.mark.timeout(CHILD_TIMEOUT + 60)
@pytest.mark.parametrize("case", CASES)
def test_search_walk(case):
    if _FAULT:
        pytest.fail("not started: " + _FAULT[0])
    env = dict(os.environ, FMX_SEARCH_WGS="1", FMX_TRACE="1")
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), case], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired as e:
        _FAULT.append("the child of %s did not end within %d s" % (case, CHILD_TIMEOUT))
        pytest.fail(_FAULT[0] + "\n" + str(e.stderr)[-2000:])
    if p.returncode < 0 or p.returncode in (134, 139):      # a signal: nothing more is started on the device
        _FAULT.append("the child of %s ended with status %d" % (case, p.returncode))
    assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), "status %d\n%s\n%s" % (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    got = None
    for ln in p.stdout.splitlines():
        if ln.startswith("RESULT "):
            print(case, ln[7:])
            got = json.loads(ln[7:])["counters"]
    assert got is not None
    with open(GOLDEN) as f:
        want = json.load(f)
    if case in want:      # (a case whose counters did not repeat between two runs of the commit before is not in the file)
        assert got == want[case], "%s: (search_requests, ktab_lookups, jump_lookups, row_lookups) = %s, the commit before the new walk counted %s" % (case, got, want[case])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    _index, _form, _jc = sys.argv[1].split("-")
    child(_index, _form, int(_jc))
