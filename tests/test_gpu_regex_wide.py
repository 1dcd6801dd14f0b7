"""The regex engines on an index of more than 2^32 rows (search_forms.WIDE_N = 2^32 + 2^29 + 12345 rows over a..d, i.i.d.).

launch_pass (fmx_frontier.hip) starts k_frontier<true, kLayoutOneHot> only when n > 2^32, and the reference-order kernels
k_match_ref_wave / k_match_ref (fmx_refmatch.hip) their <true, onehot> forms likewise; k_frontier<true, kLayoutBytes> runs for
every bytes-layout handle, but below this size none of its row fields ever held a value of 2^32 or more: the 40-bit sp / ep of
a work-queue granule, the one-row table entry with its byte at bit 40, the 56-bit k-mer table entry, the LDS pools, the
(len, sp, ep) order of the result groups, the device-resident export, RefSlot / HeapElem.  Here every one of them carries rows
on both sides of 2^32, in both layouts, and what comes back is compared with searches restated over cf + occ of
oracle.SampledFMSearcher (held to the inverted lists by tests/test_oracle_kat.py):
  * frontier mode: helpers.frontier_oracle, breadth-first with one prev_range_batch call per level;
  * reference order: oracle.retree.ReTree._matchSA, the pure-Python replay of the reference's priority-queue loop;
  * the Thompson and DFA engines: oracle.engines.
Nothing of the library produces an expectation.  The conditions the inputs must meet (results above, below and across 2^32,
one-row results at the line, a limit that binds) are computed from the expectations alone, printed and asserted before any
comparison.

The index, both handles and the oracle are made once for the module.  Searches run under a level cap throughout: on i.i.d.
bytes LF has short cycles, and a starred regex can follow one for ever.
"""
import gc
import time

import numpy as np
import pytest

import findex_amd
from oracle import retree as R
from helpers import _OIdx, ends_at_a_fault, forward_string, frontier_oracle
import search_forms as sf

pytestmark = pytest.mark.gpu

LINE = 1 << 32
SYMS = b"abcd"
MAIN_STEPS = 32             # the level cap of the main batch: beyond every result it has but those of a cycle
DEEP_STEPS = 9              # ... of the regexes whose frontier grows fourfold per level: about 4^7 * 5 elements at the cap
PREFIX_LENGTHS = (1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 17, 18, 19, 20, 21, 22, 23, 24)
VARIANT_LENGTHS = (4, 10, 16, 20, 24)
REF_LIMITS = ((1024, 1000), (16, 50), (1, 0), (1 << 14, 3000))      # the last: a heap that no wave's LDS holds (group kernel)
LAYOUTS = ("onehot", "bytes")

# results lie in the bucket of the byte stepped last: d's bucket crosses 2^32 (44 % of it lies above), a's lies below
FAMILIES = ["[a-d][a-d][a-d][a-d][a-d]d", "[a-d][a-d][a-d][a-d][a-d]a",                 # 1024 intervals each
            "[a-d][a-d][a-d][a-d][a-d][a-d]d", "[a-d][a-d][a-d][a-d][a-d][a-d]a",       # 4096: groups ordered on the host
            "d[a-d][a-d][a-d][a-d][a-d][a-d][a-d]d",                                    # 16384, and 4^7 elements alive at once
            "(ab|cd)+d", "(ab|cd)+a", "(a|b|d|c)", "d[a-d]*"]
# under DEEP_STEPS; ("[cd][a-d]*d" is a MatchError in the reference's ReTree: two regexes instead)
DEEP = ["d[a-d]*d", "c[a-d]*d", "a[a-d]*a", "a[ab]*d", "d[cd]*a", "d[a-d]*"]


# ---------------------------------------------------------------- inputs, from the oracle alone
def line_regexes(orc, line):
    """Regexes whose results hold the rows line - 1 and line.  A regex steps its first byte first, so the result of a
    literal is the interval of the suffixes that begin with the literal reversed: the prefixes of the two rows' suffixes,
    reversed -- plain, with one position widened to [a-d], and with `?` on one byte.  (An LF walk from the row, as the
    literal search's battery takes it, gives strings that hit at the row where the walk ENDS; the interval that holds a
    given row takes the walk forwards.)  -> (regexes, the plain ones)"""
    res, plain = [], []
    for row in (line - 1, line):
        t = forward_string(orc, row, max(PREFIX_LENGTHS)).decode("latin-1")
        for m in PREFIX_LENGTHS:
            s = t[:m][::-1]
            plain.append(s)
            res.append(s)
            if m in VARIANT_LENGTHS:
                j = m // 2
                res.append(s[:j] + "[a-d]" + s[j + 1:])
                res.append(s[:j] + s[j] + "?" + s[j + 1:])
    return res, plain


def oracle_tables(res):
    return [R.ReTree(R.re2post(re)).tables() for re in res]


def input_figures(main_want, deep_want, line):
    """What the issue asks of the inputs, from the expectations alone."""
    sp = np.concatenate([main_want["sp"], deep_want["sp"]]).astype(np.int64)
    ep = np.concatenate([main_want["ep"], deep_want["ep"]]).astype(np.int64)
    return {"results": int(sp.size), "sp>=2^32": int((sp >= line).sum()), "ep<=2^32": int((ep <= line).sum()),
            "sp<2^32<=ep": int(((sp < line) & (ep >= line)).sum()),
            "one_row_at_the_line": int(((ep - sp == 1) & (sp >= line - 1)).sum()),
            "largest_group": int(np.bincount(main_want["regex"]).max())}


def check_inputs(fig):
    assert fig["sp>=2^32"] >= 1000 and fig["ep<=2^32"] >= 1000 and fig["sp<2^32<=ep"] >= 5 and fig["one_row_at_the_line"] >= 10, fig
    assert fig["largest_group"] > 1024, fig


# ---------------------------------------------------------------- the index, once per module
class Wide:
    pass


@pytest.fixture(scope="module")
def wide():
    import torch
    import bench
    w = Wide()
    w.torch = torch
    t0 = time.time()
    gc.collect()
    torch.cuda.empty_cache()
    n = sf.WIDE_N
    g = torch.Generator(device="cuda")
    g.manual_seed(4322)
    bwt = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, n, step):
        b = min(n, a + step)
        bwt[a:b] = torch.randint(SYMS[0], SYMS[-1] + 1, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
    eof = n // 3
    torch.cuda.synchronize()
    w.n, w.eof, w.bwt = n, eof, bwt
    w.hip = {}
    try:
        for layout in LAYOUTS:
            findex_amd.set_layout(layout)
            w.hip[layout] = findex_amd.HipFMSearcher.from_device(bwt.data_ptr(), n, eof, None)
    finally:
        findex_amd.set_layout("auto")
    for layout, code in (("onehot", sf.ONEHOT), ("bytes", sf.BYTES)):
        st = w.hip[layout].stats()
        # the one-hot handle is the n > 2^32 one: launch_pass takes the k_frontier<true, kLayoutOneHot> branch for it
        assert st["layout"] == code and w.hip[layout].n == n > LINE, (layout, st["layout"], w.hip[layout].n)
    t1 = time.time()
    w.cores = bench.effective_cores()
    orc, _ = bench.oracle_index(torch, bwt, eof, w.cores, 0)
    if orc is None or not hasattr(orc, "prev_range_batch") or not hasattr(orc, "bytes") or orc.n != n:
        pytest.fail("the host cannot hold the reference of an index of %d rows (about 3 n bytes): no regex test above 2^32 rows ran" % n)
    w.orc = orc
    t2 = time.time()
    line, plain = line_regexes(orc, LINE)
    w.main, w.plain, w.deep = line + FAMILIES, plain, DEEP
    w.all = w.main + w.deep
    w.tables = {re: t for re, t in zip(w.all, oracle_tables(w.all))}
    w.main_want, w.main_calls, _ = frontier_oracle(orc, [w.tables[re] for re in w.main], MAIN_STEPS, threads=w.cores)
    w.deep_want, w.deep_calls, w.deep_cut = frontier_oracle(orc, [w.tables[re] for re in w.deep], DEEP_STEPS, threads=w.cores)
    w.fig = input_figures(w.main_want, w.deep_want, LINE)
    w.fig.update({"regexes": len(w.all), "oracle_evaluations": w.main_calls + w.deep_calls,
                  "seconds_index": round(t1 - t0, 1), "seconds_oracle_index": round(t2 - t1, 1), "seconds_expectations": round(time.time() - t2, 1)})
    print("wide regex inputs:", w.fig)
    w.trees = {}
    w.ref_want = {}
    yield w
    for h in w.hip.values():
        h.close()
    orc.close()
    del w.bwt, bwt
    gc.collect()
    torch.cuda.empty_cache()


def trees_of(w, res):
    for re in res:
        if re not in w.trees:
            w.trees[re] = findex_amd.ReTree(findex_amd.REParser.re2post(re))
    return [w.trees[re] for re in res]


def no_tables(hip):
    """The handle without derived tables: every step on the rank dictionary."""
    hip.config_set("ktab", "off")
    hip.config_set("jump", "off")
    hip.drop_tables(jump=True, frontier=True, ktab=True)


def with_tables(hip, n):
    """The k-mer table and the frontier's row table, and no other (the literal search's tables are 24 n bytes)."""
    st = hip.stats()
    if not (st["ktab_k"] and st["row_bytes"]):
        hip.config_set("ktab", "auto")
        hip.config_set("ktab_ext", "off")
        hip.config_set("jump", "rows")
        hip.drop_tables(jump=True, frontier=True, ktab=True)     # (a handle keeps its decision not to build a table until then)
        hip.prepare(ktab=True, frontier=True)
        st = hip.stats()
    assert st["ktab_k"] == sf.ktab_rule(n, len(SYMS)) and st["row_bytes"] > 0, (st["ktab_k"], st["row_bytes"])


def keys(arr):
    return list(zip(arr["regex"].tolist(), arr["len"].tolist(), arr["sp"].tolist(), arr["ep"].tolist()))


def per_regex(want, k):
    out = [[] for _ in range(k)]
    for r, ln, sp, ep in keys(want):
        out[r].append((ln, sp, ep))
    return out


def check_frontier_calls(w, hip, count_steps):
    """Both frontier calls through matchSA_batch: the result list of every regex equal to the oracle's, sorted by
    (len, sp, ep), multiplicity included."""
    check_inputs(w.fig)
    for res, steps, want, calls in ((w.main, MAIN_STEPS, w.main_want, w.main_calls), (w.deep, DEEP_STEPS, w.deep_want, w.deep_calls)):
        hip.stats_reset()
        got = findex_amd.ReTree.matchSA_batch(hip, trees_of(w, res), max_steps=steps, max_frontier=1 << 22, cap=1 << 20)
        st = hip.stats()
        exp = per_regex(want, len(res))
        assert len(got) == len(res)
        for re, g, e in zip(res, got, exp):
            assert [r.key() for r in g] == e, (re, steps, len(g), len(e))
        if count_steps:
            assert st["backward_steps"] == calls, (steps, st["backward_steps"], calls)
        if res is w.deep:
            assert findex_amd.ReTree.last_truncated and w.deep_cut
            # the 40-bit granules of the work queue did carry these rows
            assert st["frontier_queue_writes"] > 0, st


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_frontier_without_tables(wide, layout):
    """Frontier mode with neither k-mer table nor row table: results per regex, and as many backward steps as the oracle
    makes getPrevRange calls (the invariant test_regex_frontier_parity holds below 2^32 rows)."""
    hip = wide.hip[layout]
    no_tables(hip)
    check_frontier_calls(wide, hip, count_steps=True)
    st = hip.stats()
    assert st["ktab_k"] == 0 and st["row_bytes"] == 0 and st["jump_bytes"] == 0, st


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_frontier_with_tables(wide, layout):
    """The same with the tables prepared: start elements leave the k-mer table through its 56-bit entries, one-row elements
    step through the row table (a row index of 2^32 and more, the byte at bit 40)."""
    hip = wide.hip[layout]
    with_tables(hip, wide.n)
    hip.stats_reset()
    check_frontier_calls(wide, hip, count_steps=False)


@pytest.mark.parametrize("kernel", ["wave", "group"])
@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_reference_order(wide, layout, kernel, monkeypatch):
    """ReTree._matchSA's queue under the reference's limits and tighter ones, by both kernels (FMX_REFMATCH is read at
    every call): elements, their newest-first order, pops, and two rank queries per pop."""
    check_inputs(wide.fig)
    monkeypatch.setenv("FMX_REFMATCH", kernel)
    hip = wide.hip[layout]
    with_tables(hip, wide.n)
    trees = trees_of(wide, wide.all)
    idx = _OIdx(wide.orc)
    for mb, mi in REF_LIMITS:
        if (mb, mi) not in wide.ref_want:
            wide.ref_want[(mb, mi)] = [R.ReTree(R.re2post(re))._matchSA(idx, mb, mi) for re in wide.all]
        want = wide.ref_want[(mb, mi)]
        if (mb, mi) == (16, 50):
            cut = sum(1 for _, front, _ in want if front)
            print("reference order (16, 50): %d of %d regexes cut off by a limit" % (cut, len(want)))
            assert cut >= 1
        hip.stats_reset()
        got = findex_amd.ReTree.matchSA_batch(hip, trees, mode="reference", maxBranching=mb, maxIterations=mi, cap=1 << 20)
        st = hip.stats()
        assert len(got) == len(wide.all)
        for re, g, (ret, _, _) in zip(wide.all, got, want):
            assert [r.key() for r in g] == ret, (re, mb, mi)
        pops = sum(p for _, _, p in want)
        assert st["backward_steps"] == pops and st["rank_queries"] == 2 * pops, (mb, mi, st["backward_steps"], st["rank_queries"], pops)


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_resident_batch_and_device_resident_results(wide, layout):
    """prepare_batch + match_raw: the flat list equal to the oracle's, grouped by regex and ordered by (len, sp, ep) -- with
    groups of 4096 and 16384 results, ordered on the host by 64-bit keys; match_dev leaves the same bytes and the same
    per-regex counts in device memory."""
    from findex_amd.regex import RESULT_DTYPE
    check_inputs(wide.fig)
    torch = wide.torch
    hip = wide.hip[layout]
    with_tables(hip, wide.n)
    for res, steps, want in ((wide.main, MAIN_STEPS, wide.main_want), (wide.deep, DEEP_STEPS, wide.deep_want)):
        batch = findex_amd.ReTree.prepare_batch(hip, trees_of(wide, res))
        cap = 1 << 20
        out, per = batch.match_raw(max_steps=steps, cap=cap)
        assert out.size == want.size and all(np.array_equal(out[f], want[f]) for f in ("regex", "len", "sp", "ep")), (steps, out.size, want.size)
        assert np.array_equal(per, np.bincount(want["regex"], minlength=len(res)).astype(np.uint32))
        d_out = torch.zeros(cap * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_per = torch.full((len(res),), 7, dtype=torch.int32, device="cuda")
        k = batch.match_dev(d_out.data_ptr(), cap, d_per.data_ptr(), max_steps=steps)
        torch.cuda.synchronize()
        got = np.frombuffer(d_out[: k * RESULT_DTYPE.itemsize].cpu().numpy().tobytes(), dtype=RESULT_DTYPE)
        assert k == out.size and got.tobytes() == out.tobytes(), steps
        assert np.array_equal(d_per.cpu().numpy().astype(np.uint32), per)
        del batch, d_out, d_per


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_thompson_and_dfa_engines(wide, layout):
    """REParser.createNFA + REParser.matchSA and DFA.matchSA compile to tables of their own and search with k_frontier:
    one small case each, results in d's bucket and at the line."""
    from oracle import engines as E
    P = findex_amd.REParser
    hip = wide.hip[layout]
    with_tables(hip, wide.n)
    idx = _OIdx(wide.orc)
    at_line = wide.plain[len(PREFIX_LENGTHS):]            # the prefixes of row 2^32's suffix
    p8, p12 = at_line[PREFIX_LENGTHS.index(8)], at_line[PREFIX_LENGTHS.index(12)]
    above = across = 0
    # (results are the suffixes that begin with the regex reversed: those of d[cd]... lie above the line, d[ab]... below)
    for re in ("(a|b|c|d)(a|b|c|d)(a|b|c|d)(a|b|c|d)d", "a(c|d)+d", p8, p12, p12[:5] + "(a|b|c|d)" + p12[6:]):
        want = sorted(E.nfa_matchSA(E.createNFA(R.re2post(re)), idx, maxLength=12))
        got = [r.key() for r in P.matchSA(P.createNFA(P.re2post(re)), hip, maxLength=12)]
        assert got == want, re
        above += sum(1 for _, sp, _ in want if sp >= LINE)
        across += sum(1 for _, sp, ep in want if sp < LINE <= ep)
    assert above >= 50 and across >= 3, (above, across)      # (about 110 of the first regex's 256 intervals lie above)
    a, b = findex_amd.DFA(4), E.DFA(4)
    for f, t_, ch in [(0, 1, ord("a")), (1, 2, ord("c")), (2, 2, ord("c")), (2, 3, ord("d"))]:      # a c+ d
        a.addLink(f, t_, ch)
        b.addLink(f, t_, ch)
    a.finishStates = {3}
    b.finishStates = {3}
    a.compileBuckets()
    b.compileBuckets()
    want = sorted(b.matchSA(idx))
    assert [r.key() for r in a.matchSA(hip)] == want
    assert sum(1 for _, sp, _ in want if sp >= LINE) >= 3, want


@pytest.mark.parametrize("layout", LAYOUTS)
@ends_at_a_fault
def test_literal_regexes_equal_the_literal_search(wide, layout):
    """A literal regex steps its bytes from the first to the last, the literal search from the last to the first: the
    regex and search_batch of the reversed string must give the same interval (tests/test_gpu_search_forms.py holds
    search_batch to the oracle at this n), and both the oracle's."""
    from helpers import pack_patterns
    hip = wide.hip[layout]
    with_tables(hip, wide.n)
    res = wide.plain
    buf, off = pack_patterns([re.encode("latin-1")[::-1] for re in res])
    sp, ep = hip.search_batch(buf, off)
    wsp, wep, _ = wide.orc.search_batch(buf, off)
    assert np.array_equal(sp, wsp) and np.array_equal(ep, wep)
    assert bool((sp < ep).all())
    got = findex_amd.ReTree.matchSA_batch(hip, trees_of(wide, res), max_steps=MAIN_STEPS)
    for re, g, a, b in zip(res, got, sp.tolist(), ep.tolist()):
        assert [r.key() for r in g] == [(len(re), a, b)], re
    rows = [(a, b) for a, b in zip(sp.tolist(), ep.tolist())]
    assert sum(1 for a, b in rows if a < LINE <= b) >= 5 and sum(1 for a, b in rows if b - a == 1 and a >= LINE - 1) >= 5
