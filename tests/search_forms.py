"""Every instantiation of k_search4 (findex_amd/csrc/fmx_search4.h, FMX_SEARCH4_LIST) and the recipe that makes
select_plan / plan_of (fmx_search.hip) choose it.

RECIPES maps a form -- the template arguments (WIDE, LAYOUT, KT, JT, RW, R3T, G2, KX) as integers, the way FMX_TRACE prints
them -- to the list of recipes that launch it: the index, the layout, the per-handle keys, the fmx_prepare flags, the batch
size and the environment of the process.  tests/test_search_forms_cpu.py holds the table's keys to the header's list;
tests/test_gpu_search_forms.py runs every recipe in a child process (this file, run as a program) under FMX_TRACE=1 and
compares what it finds with an oracle over the same bytes.

Run as a program (the child):  python tests/search_forms.py small|many|wide GROUP
"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ONEHOT, BYTES = 0, 1      # kLayoutOneHot, kLayoutBytes (fmx_device.h; header_forms reads the values from there)
LAYOUT_NAME = {ONEHOT: "onehot", BYTES: "bytes"}
JUMP_CHARS = 9            # the default "jump_chars": characters per row-jump entry
SMALL_N = 1 << 16
# about 2^32 + 2^29 rows plus an odd remainder: a ninth of the rows lie above 2^32
WIDE_N = (1 << 32) + (1 << 29) + 12345
WIDE_SIGMA = 4
WIDE_MAXLEN = 40
RAGGED = 6000             # the ragged part of the small battery
# launch_form (fmx_search.hip) spreads a batch over min(k / (256 / G), CUs x resident workgroups) workgroups, so a battery of a
# few thousand patterns is ONE lockstep batch per wave: the small battery tests the edges of a search, not the batch loop.
# The loop -- the next batch staged while this one is searched, parked misses walked "when 48 have come together", the rows
# phase -- runs in the children started with FMX_SEARCH_WGS=1 (one workgroup per CU: 1024 waves on the 256 CUs of an MI355X)
# over MANY_BATCHES batches of 64 / G patterns; the parent asserts from the trace line that a wave had MIN_ROUNDS or more.
MANY_BATCHES = 4608
MIN_ROUNDS = 3
# above 2^32 rows: at least the 100 000 patterns per form, and enough that the pairs of lanes (32 patterns per batch) draw too
WIDE_PATTERNS = MANY_BATCHES * 32


def form_str(f):
    """The form as FMX_TRACE prints it (fmx_search.hip, launch_form)."""
    return "k_search4<%d,%d,%d,%d,%d,%d,%d,%d>" % tuple(f)


def twin(f):
    """The same form served by the other lane grouping (fmx_prepare calibrates both where there are both)."""
    return f[:6] + (1 - f[6],) + f[7:]


def ktab_rule(n, sigma):
    """build_ktab (fmx_ktab.hip): the largest K <= 16 with sigma^K <= n / 8 (the memory bounds do not bind at these sizes)."""
    k, entries = 0, 1
    while k < 16 and entries * sigma <= n // 8 and entries * sigma <= 1 << 32:
        entries *= sigma
        k += 1
    return k


def kt_of(k):
    """The level a search uses (fmx_search.hip, plan_of): the largest multiple of four up to K."""
    return 12 if k >= 12 else 8 if k >= 8 else 4 if k >= 4 else 0


# ---------------------------------------------------------------- the header's list
def header_forms(workdir):
    """The tuples of FMX_SEARCH4_LIST, by the preprocessor: a three-line unit that includes fmx_search4.h and expands the
    list with a macro that prints its arguments, compiled with findex_amd/build.py's compiler, architecture and include
    paths.  Returns a list (duplicates kept, for the test to find)."""
    from findex_amd import build as fb
    unit = os.path.join(str(workdir), "search_forms_unit.hip")
    with open(unit, "w") as f:
        f.write('#include "fmx_search4.h"\n'
                "#define FMX_FORM_ROW_(W, L, KT, JT, RW, R3T, G2, KX) fmx_form_row W L KT JT RW R3T G2 KX fmx_form_end\n"
                "FMX_SEARCH4_LIST(FMX_FORM_ROW_)\n")
    cmd = [fb._hipcc(), "-E", "-P", "-x", "hip", "--cuda-host-only", "-std=c++17", "--offload-arch=" + fb.ARCH,
           "-I" + os.path.join(fb.ROOT, "include"), "-I" + fb.CSRC] + fb._extra_flags() + [unit]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    with open(os.path.join(fb.CSRC, "fmx_device.h")) as f:
        dev = f.read()
    names = {"true": 1, "false": 0}
    for name in ("kLayoutOneHot", "kLayoutBytes"):
        names[name] = int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, dev).group(1))
    assert names["kLayoutOneHot"] == ONEHOT and names["kLayoutBytes"] == BYTES
    forms = []
    for m in re.finditer(r"fmx_form_row\s+(.*?)\s+fmx_form_end", out.stdout, re.S):
        tok = m.group(1).split()
        assert len(tok) == 8, tok
        forms.append(tuple(names[t] if t in names else int(t) for t in tok))
    return forms


# ---------------------------------------------------------------- the recipes
# (JT, RW, R3T) -> the "jump" / "jump_pairs" keys that leave exactly those tables on the handle (fmx_jump.hip: build_jump,
# row3_get, row1_get), and whether fmx_prepare is asked for the frontier's row table R1
ROW_TABLES = {
    (2, 0, 1): ({"jump": "auto", "jump_pairs": "on"}, False),      # pairs of entries (built from R3) + R3
    (1, 0, 1): ({"jump": "auto", "jump_pairs": "off"}, False),     # single entries + R3
    (1, 0, 0): ({"jump": "jumps", "jump_pairs": "off"}, False),    # single entries, no R3
    (0, 3, 0): ({"jump": "rows3", "jump_pairs": "off"}, False),    # R3 alone
    (0, 1, 0): ({"jump": "rows", "jump_pairs": "off"}, True),      # the frontier's R1 alone
    (0, 0, 0): ({"jump": "off", "jump_pairs": "off"}, False),      # none
}
# KT -> the i.i.d. indexes of SMALL_N rows whose k-mer table has that depth by ktab_rule: (sigma, "ktab" key)
SMALL_KT = {
    12: [(2, "auto")],                      # 2^13 = 8192 <= 8192: K = 13
    8: [(3, "auto")],                       # 3^8 = 6561 <= 8192 < 3^9
    4: [(5, "auto")],                       # 5^5 = 3125 <= 8192 < 5^6: K = 5
    0: [(5, "off"), (128, "auto")],         # no table; a table that is there but shallower than 4 (K = 1)
}
# level K+1 is refused when a KE-mer has more than 64 rows (kExtMaxList): sigma 5 has 105 rows per 4-mer on average, so KT 4
# takes sigma 8 (16 rows per 4-mer; 8^4 = 4096 <= 8192 < 8^5)
KX_SIGMA = {12: 2, 8: 3, 4: 8}


def _recipe(rid, group, f, index, keys, frontier, env=None):
    wide, layout, kt, jt, rw, r3t, g2, kx = f
    return {"id": rid, "group": group, "form": f, "index": index, "layout": LAYOUT_NAME[layout], "keys": keys,
            "prepare": {"ktab": True, "jump": True, "frontier": frontier}, "batch": RAGGED if not wide else WIDE_PATTERNS,
            "env": env or {}, "pool": bool(g2 or rw)}


def _build_recipes():
    table = {}

    def add(r):
        table.setdefault(r["form"], []).append(r)

    rows_onehot = [(2, 0, 1, 1), (2, 0, 1, 0), (1, 0, 1, 1), (1, 0, 1, 0), (1, 0, 0, 0), (0, 3, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0)]
    rows_bytes = [(1, 0, 1, 0), (1, 0, 0, 0), (0, 3, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0)]
    for layout, rows in ((ONEHOT, rows_onehot), (BYTES, rows_bytes)):
        for kt in (0, 4, 8, 12):
            group = "%s-kt%d" % (LAYOUT_NAME[layout], kt)
            for jt, rw, r3t, g2 in rows:
                f = (1 if layout == BYTES else 0, layout, kt, jt, rw, r3t, g2, 0)
                tkeys, frontier = ROW_TABLES[(jt, rw, r3t)]
                variants = [({"kind": "iid", "n": SMALL_N, "sigma": s, "seed": 100 + s}, ktab) for s, ktab in SMALL_KT[kt]]
                if kt == 4:     # one repetitive text per layout: intervals that stay a few rows wide for many steps
                    variants.append(({"kind": "rep"}, "auto"))
                for index, ktab in variants:
                    keys = dict(tkeys, ktab=ktab, ktab_ext="off", search_lanes="pairs" if g2 else "quads")
                    tag = index["kind"] + (str(index["sigma"]) if index["kind"] == "iid" else "") + ("" if ktab == "auto" else "-ktaboff")
                    add(_recipe("%s-jt%d-rw%d-r3t%d-g%d-%s" % (group, jt, rw, r3t, g2, tag), group, f, index, keys, frontier))
    for kt in (4, 8, 12):       # level KT + 1: pairs of row jump entries, one-hot, up to 2^32 rows
        for g2 in (1, 0):
            f = (0, ONEHOT, kt, 2, 0, 1, g2, 1)
            keys = dict(ROW_TABLES[(2, 0, 1)][0], ktab="auto", ktab_ext="on", search_lanes="pairs" if g2 else "quads")
            index = {"kind": "iid", "n": SMALL_N, "sigma": KX_SIGMA[kt], "seed": 100 + KX_SIGMA[kt]}
            add(_recipe("kx-kt%d-g%d" % (kt, g2), "kx", f, index, keys, False))
    # above 2^32 rows: one index, sigma 4 (K = 14 by the rule); FMX_KTAB in the process environment gives the shallower levels
    for kt in (0, 4, 8, 12):
        group = "wide-kt%d" % kt
        for jt, rw, r3t, g2 in rows_onehot:
            f = (1, ONEHOT, kt, jt, rw, r3t, g2, 0)
            tkeys, frontier = ROW_TABLES[(jt, rw, r3t)]
            keys = dict(tkeys, ktab="auto" if kt else "off", ktab_ext="off", search_lanes="pairs" if g2 else "quads")
            index = {"kind": "wide", "n": WIDE_N, "sigma": WIDE_SIGMA, "seed": 4321}
            add(_recipe("%s-jt%d-rw%d-r3t%d-g%d" % (group, jt, rw, r3t, g2), group, f, index, keys, frontier,
                        env={"FMX_KTAB": str(kt)} if kt else {}))
    return table


RECIPES = _build_recipes()
SMALL_GROUPS = ["%s-kt%d" % (lay, kt) for lay in ("onehot", "bytes") for kt in (0, 4, 8, 12)] + ["kx"]
WIDE_GROUPS = ["wide-kt%d" % kt for kt in (0, 4, 8, 12)]


def recipes_of(group):
    return [r for rs in RECIPES.values() for r in rs if r["group"] == group]


# ---------------------------------------------------------------- indexes and batteries (CPU: numpy and the oracle)
def rep_text():
    """The first generator of test_row_tables_on_repetitive_texts: a unit repeated with a few point mutations, so that the
    repeats split into families of two to eight rows."""
    rng = np.random.default_rng(2024)
    unit = bytes(rng.integers(97, 100, 37).astype(np.uint8))
    rep = bytearray(unit * 60)
    for j in rng.integers(0, len(rep), 70):
        rep[int(j)] = int(rng.integers(97, 101))
    return bytes(rep)


def small_index(spec):
    """(bwt, eof, counts) of a recipe's index (not the one above 2^32 rows, which is generated on the device)."""
    from helpers import bwt_of_text, synth_bwt
    if spec["kind"] == "iid":
        return synth_bwt(spec["n"], 1, spec["sigma"], spec["seed"])
    assert spec["kind"] == "rep"
    return bwt_of_text(rep_text())


def battery(orc, syms, kt, jc, seed, ragged=RAGGED):
    """The patterns every small recipe searches, from the oracle: hits and misses of every length 0 .. KT + 2 jc + 4; a
    miss at every step up to past the second row-jump lookup (so at each of the first KT + 1 steps and inside and just past
    each lookup), by a symbol of the alphabet, byte 0 and a byte outside the alphabet in turn; walks from rows 0 .. 5 and
    n - 1; the buffer begins with short patterns (inside its first 16 bytes); then the ragged batch."""
    from helpers import lf_walk_patterns
    rng = np.random.default_rng(seed)
    syms = [int(s) for s in syms]
    foreign = next(b for b in range(1, 256) if b not in syms)
    lmax = kt + 2 * jc + 4
    one_row = 1                             # steps after which an interval of an i.i.d. index is one row, roughly
    while len(syms) ** one_row < orc.n:
        one_row += 1
    lbig = max(lmax, one_row + 2 * jc + 8)
    pats = [b"", bytes([syms[0]])] + lf_walk_patterns(orc, rng, 3, 3, 0.0)
    for m in range(0, lmax + 1):
        pats += lf_walk_patterns(orc, rng, 24, m, 0.3, alphabet=syms)
    base = lf_walk_patterns(orc, rng, 30, lbig, 0.0)
    for j in range(lbig):                   # step j consumes the byte at len - 1 - j
        for i, p in enumerate(base):
            q = bytearray(p)
            q[len(q) - 1 - j] = [syms[int(rng.integers(0, len(syms)))], 0, foreign][(i + j) % 3]
            pats.append(bytes(q))
    for r0 in list(range(0, 6)) + [orc.n - 1]:
        for m in range(1, lmax + 1):
            cs, r = [], r0
            for _ in range(m):
                cs.append(orc.bwt_read(r))
                r = orc.getPrevI(r)
            pats.append(bytes(reversed(cs)))
    pats += [b"\x00", bytes([foreign]), bytes([foreign]) * (kt + 1)]
    for m in rng.integers(0, lbig + 1, ragged):
        pats += lf_walk_patterns(orc, rng, 1, int(m), 0.5, alphabet=syms + [foreign])
    return pats


def miss_regions(orc, buf, off, wsp, wep, wsteps, kdepth):
    """Where the oracle's misses fail: (in the k-mer lookup, on one row, on a wider interval).  A miss that executed s steps
    failed at step s - 1; its last s - 1 characters hit, and the width of their interval says whether the failing step was
    taken from one row or on the rank dictionary.  "On one row" is where the kernels consult the row jump table and the row
    tables, but it is coarser than "inside a lookup": a one-row miss with fewer than jump_chars characters left is served by
    R3 or the dictionary.  The batteries do not rely on this split for coverage (they place a miss at every step up to past
    the second lookup, or at a random one); it only keeps a battery from passing without any miss of a kind."""
    from helpers import pack_patterns
    miss = np.nonzero(wsp >= wep)[0]
    fail = wsteps[miss].astype(np.int64) - 1
    ends = off[1:][miss].astype(np.int64)
    tails = [bytes(buf[int(e) - int(f):int(e)]) for e, f in zip(ends, fail)]
    tb, to = pack_patterns(tails)
    tsp, tep, _ = orc.search_batch(tb, to)
    width = (tep - tsp).astype(np.int64)
    assert bool((width > 0).all())
    in_k = fail < kdepth
    return int(in_k.sum()), int((~in_k & (width == 1)).sum()), int((~in_k & (width > 1)).sum())


def check_conditions(f, orc, buf, off, wsp, wep, wsteps):
    """On the oracle's own outputs, so that a degenerate battery cannot pass: at least 20 % of the patterns hit and 20 %
    miss, and at least one miss falls in each region the form has."""
    wide, layout, kt, jt, rw, r3t, g2, kx = f
    k = wsp.size
    hits = int((wsp < wep).sum())
    in_k, one_row, wider = miss_regions(orc, buf, off, wsp, wep, wsteps, kt + kx)
    fig = {"patterns": k, "hits": hits, "misses": k - hits, "miss_in_kmer": in_k, "miss_on_one_row": one_row, "miss_on_dictionary": wider}
    assert hits >= 0.2 * k and k - hits >= 0.2 * k, fig
    assert wider > 0, fig
    assert not kt or in_k > 0, fig
    assert not (jt or rw) or one_row > 0, fig
    return fig


# ---------------------------------------------------------------- the child process
def _mark(what, rid):
    os.write(2, ("[forms] %s %s\n" % (what, rid)).encode())


def _emit(obj):
    sys.stdout.write("RESULT " + json.dumps(obj) + "\n")
    sys.stdout.flush()


def _apply(hip, recipe):
    for key, value in recipe["keys"].items():
        hip.config_set(key, value)
    hip.prepare(**recipe["prepare"])


def _compare(hip, orc_out, buf, off, what, threads=1):
    """One search of (buf, off) against the oracle's (sp, ep, steps): intervals bit for bit, the reference loop's steps."""
    wsp, wep, wsteps = orc_out
    hip.stats_reset()
    gsp, gep = hip.search_batch(buf, off)
    bad = np.nonzero((gsp != wsp) | (gep != wep))[0]
    assert bad.size == 0, "%s: %d of %d intervals differ, first %s" % (
        what, bad.size, wsp.size, [(int(i), bytes(buf[int(off[i]):int(off[i + 1])]), int(gsp[i]), int(gep[i]), int(wsp[i]), int(wep[i])) for i in bad[:4]])
    st = hip.stats()
    steps = int(wsteps.sum())
    assert st["backward_steps"] == steps and st["rank_queries"] == 2 * steps, (what, st["backward_steps"], st["rank_queries"], steps)


def _lean_forms(hip, orc_out, buf, off):
    """The 8-byte form and FMX_SEARCH_MISS_NONE: both are written by the kernel itself."""
    wsp, wep, _ = orc_out
    k = wsp.size
    hit = wsp < wep
    esc = 64
    usp, uep = hip.unpack_intervals(hip.search_batch_ex(buf, off, packed=True, escape_cap=esc), k, esc)
    assert np.array_equal(usp, wsp) and np.array_equal(uep, wep), "packed form"
    for packed in (False, True):
        if packed:
            msp, mep = hip.unpack_intervals(hip.search_batch_ex(buf, off, packed=True, escape_cap=esc, miss_none=True), k, esc)
        else:
            msp, mep = hip.search_batch_ex(buf, off, miss_none=True)
        assert np.array_equal(msp[hit], wsp[hit]) and np.array_equal(mep[hit], wep[hit]), "miss_none hits (packed %d)" % packed
        assert bool((msp[~hit] >= mep[~hit]).all()), "miss_none misses (packed %d)" % packed


def _device_walks(hip, rng, k, maxlen, syms, minlen=1, replaced=1.0 / 3):
    """k ragged patterns from LF walks of the device: lengths minlen .. maxlen, a share of them with one byte replaced by one of
    `syms`."""
    rows = rng.integers(0, hip.n, k).astype(np.uint64)
    b, _ = hip.lf_walk_batch(rows, maxlen)
    full = np.ascontiguousarray(b[:, ::-1])
    lens = rng.integers(minlen, maxlen + 1, k)
    mut = np.nonzero(rng.random(k) < replaced)[0]
    pos = maxlen - 1 - (rng.random(mut.size) * lens[mut]).astype(np.int64)       # inside the pattern's own bytes
    full[mut, pos] = np.asarray(syms, dtype=np.uint8)[rng.integers(0, len(syms), mut.size)]
    keep = np.arange(maxlen)[None, :] >= (maxlen - lens)[:, None]
    buf = np.ascontiguousarray(full[keep])
    off = np.zeros(k + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return buf, off


def child_small(group, many):
    """The recipes of one group on indexes of about 2^16 rows, each against oracle.NaiveFMSearcher over the same bytes: the
    battery of edges (one batch per wave), or -- `many`, in a process started with FMX_SEARCH_WGS=1 -- MANY_BATCHES batches of
    ragged patterns from LF walks of the device."""
    import findex_amd
    import oracle
    from helpers import pack_patterns
    findex_amd.config_set("tables_after", "0")      # (tests/conftest.py does this for the pytest process)
    cache = {}
    for recipe in recipes_of(group):
        f = recipe["form"]
        rid = recipe["id"]
        t0 = time.time()
        key = json.dumps(recipe["index"], sort_keys=True)
        if key not in cache:
            bwt, eof, counts = small_index(recipe["index"])
            orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
            syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
            cache[key] = [bwt, eof, counts, orc, syms, {}]
        bwt, eof, counts, orc, syms, runs = cache[key]
        res = {"id": rid, "ok": False}
        _mark("begin", rid)
        try:
            findex_amd.set_layout(recipe["layout"])
            hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
            _apply(hip, recipe)
            st = hip.stats()
            want_k = ktab_rule(orc.n, len(syms)) if recipe["keys"]["ktab"] == "auto" else 0
            assert st["ktab_k"] == want_k and kt_of(want_k) == f[2], (st["ktab_k"], want_k, f)
            foreign = next(b for b in range(1, 256) if b not in syms)
            if not many:
                if f[2] not in runs:
                    pats = battery(orc, syms, f[2], JUMP_CHARS, 7 + f[2], ragged=recipe["batch"])
                    buf, off = pack_patterns(pats)
                    runs[f[2]] = (buf, off, orc.search_batch(buf, off))
                buf, off, out = runs[f[2]]
                res["figures"] = check_conditions(f, orc, buf, off, *out)
                _compare(hip, out, buf, off, rid)
                _lean_forms(hip, out, buf, off)
            else:
                per_wave = 32 if f[6] else 8 if f[1] == BYTES else 16      # patterns of one batch: 64 / G
                k = MANY_BATCHES * per_wave
                if ("many", k) not in runs:
                    rng = np.random.default_rng(11)
                    one_row = 1
                    while len(syms) ** one_row < orc.n:
                        one_row += 1
                    buf, off = _device_walks(hip, rng, k, max(f[2] + 2 * JUMP_CHARS + 4, one_row + 2 * JUMP_CHARS + 8), syms + [foreign] * len(syms), minlen=0, replaced=0.6)
                    runs[("many", k)] = (buf, off, orc.search_batch(buf, off, threads=min(16, len(os.sched_getaffinity(0)))))
                buf, off, out = runs[("many", k)]
                res["figures"] = check_conditions(f, orc, buf, off, *out)
                _compare(hip, out, buf, off, rid)
                _lean_forms(hip, out, buf, off)
            hip.close()
            res["ok"] = True
        except AssertionError as e:
            res["error"] = "AssertionError: " + str(e)[:1500]
        finally:
            _mark("end", rid)
            findex_amd.set_layout("auto")
        res["seconds"] = round(time.time() - t0, 2)
        _emit(res)
    print("DONE")


def child_wide(group):
    """The eight one-hot forms of one KT on an index of WIDE_N rows, against oracle.SampledFMSearcher over the same bytes.  The
    process is started with FMX_SEARCH_WGS=1: WIDE_PATTERNS are 4608 batches of pairs or 9216 of quads over 1024 waves, so the
    batch loop's carried state and the pool are exercised with 64-bit rows too."""
    import torch
    import findex_amd
    import bench
    findex_amd.config_set("tables_after", "0")
    recipes = recipes_of(group)
    spec = recipes[0]["index"]
    n, sigma = spec["n"], spec["sigma"]
    t0 = time.time()
    g = torch.Generator(device="cuda")
    g.manual_seed(spec["seed"])
    bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, n, step):
        b = min(n, a + step)
        bwt[a:b] = torch.randint(1, sigma + 1, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
    eof = n // 3
    torch.cuda.synchronize()
    findex_amd.set_layout("onehot")
    hip = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, None)
    cores = bench.effective_cores()
    orc, _ = bench.oracle_index(torch, bwt, eof, cores, 0)
    if orc is None or not hasattr(orc, "bytes") or orc.n != n:
        _emit({"id": group, "ok": False, "error": "the host cannot hold the reference (about 3 n bytes at n = %d)" % n})
        print("DONE")
        return
    torch.cuda.empty_cache()
    syms = list(range(1, sigma + 1))
    rng = np.random.default_rng(5)
    buf, off = _device_walks(hip, rng, WIDE_PATTERNS - 20, WIDE_MAXLEN, syms + [sigma] * sigma)     # (half the replacements are the last symbol: its bucket crosses 2^32)
    short = [bytes([c]) for c in syms] + [bytes([c, d]) for c in syms for d in syms]                # one- and two-character patterns
    sb = np.frombuffer(b"".join(short), dtype=np.uint8)
    off = np.concatenate([off, off[-1] + np.cumsum([len(s) for s in short]).astype(np.uint64)])
    buf = np.concatenate([buf, sb])
    out = orc.search_batch(buf, off, threads=cores)
    wsp, wep, wsteps = out
    hit = wsp < wep
    line = np.uint64(1 << 32)
    fig = {"patterns": int(wsp.size), "hits": int(hit.sum()), "misses": int((~hit).sum()),
           "hits_above_2^32": int((hit & (wsp >= line)).sum()), "intervals_across_2^32": int((hit & (wsp < line) & (wep >= line)).sum()),
           "misses_above_2^32": int((~hit & (wsp >= line)).sum()), "setup_seconds": round(time.time() - t0, 1)}
    _emit({"id": group, "ok": True, "figures": fig})
    tables = None
    for recipe in recipes:
        rid = recipe["id"]
        t1 = time.time()
        res = {"id": rid, "ok": False}
        _mark("begin", rid)
        try:
            assert wsp.size == WIDE_PATTERNS
            assert fig["hits_above_2^32"] >= 0.05 * fig["hits"] and fig["intervals_across_2^32"] >= 1 and fig["misses_above_2^32"] >= 1000, fig
            want = (recipe["keys"]["jump"], recipe["keys"]["jump_pairs"])
            if tables is not None and tables != want:
                hip.drop_tables(jump=True, frontier=True)
            tables = want
            _apply(hip, recipe)
            st = hip.stats()
            res["figures"] = {"ktab_k": st["ktab_k"], "jump_bytes": st["jump_bytes"], "row_bytes": st["row_bytes"]}
            assert kt_of(st["ktab_k"]) == recipe["form"][2], st["ktab_k"]
            _compare(hip, out, buf, off, rid)
            res["ok"] = True
        except AssertionError as e:
            res["error"] = "AssertionError: " + str(e)[:1500]
        finally:
            _mark("end", rid)
        res["seconds"] = round(time.time() - t1, 2)
        _emit(res)
    print("DONE")


if __name__ == "__main__":
    if sys.argv[1] == "wide":
        child_wide(sys.argv[2])
    else:
        child_small(sys.argv[2], sys.argv[1] == "many")
