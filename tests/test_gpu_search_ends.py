"""The two ends of a k_search4 launch: its first batches, whose offsets are requested before the tables are in LDS and whose
symbol entries come from the table built with the handle, and its last rounds, drawn from the ticket pool.  Needs a real
MI355X:  pytest -m gpu -s

Every case runs in a child process with FMX_SEARCH_WGS=1 FMX_TRACE=1 (1024 waves, so the pool exists from four rounds of
batches: 131 072 patterns by pairs of lanes, 32 768 in the bytes layout) and compares with oracle.NaiveFMSearcher over the same
bytes: (sp, ep) bit for bit, misses' values included, and the executed steps.  The child reads its own launch lines ("N batches
over M waves, the last L drawn from ticket area A") and takes every batch size from them: the waves M and the pooled full
rounds kPoolRounds = what a launch of nine rounds draws.  One battery of patterns per index and layout, searched by the
oracle once; every shape is a prefix of it:

  exact      rounds exactly kPoolRounds + 2: the smallest launch with a pool, which holds kPoolRounds full rounds
  nopool     one batch fewer: nothing is drawn
  uneven     five batches more: the counters' shares of the pool differ (with 1024 waves there are 32 counters, fewer than
             the 64 there can be; a pool of fewer batches than counters cannot exist, it holds two rounds at least)
  onelast    a last batch of one pattern
  long       nine rounds and three batches: a wave parks misses through seven rounds or more, so its walk list is flushed
             inside the pool phase

The battery is ragged BY BATCH: of the wave-sized runs of patterns 15 % hold lengths 66 .. 70 (a span of more than 2 KiB:
the batch is read from global memory, unstaged), 15 % lengths 0 .. 3 (no batch of them reaches a row-table lookup), the rest
lengths 0 .. 70 with empty patterns among them; 30 % of the patterns have one byte replaced.  On the `exact` shape the 8-byte
form and FMX_SEARCH_MISS_NONE are compared too, and the same batch is launched three times in a row on one stream (the ticket
counters must be back at zero for each) and then alternately on two streams, every result equal to the oracle's.

Indexes: synth_bwt(300 000, 1, 12) and a real text of 3000 bytes (the head of README.md), whose LF walks cross the EOF row;
layouts: one-hot by pairs of lanes with pairs of row jump entries, and bytes with the three-step row table.  `sparse` is an
index of the symbols {1, 3, 128, 254, 255}, searched with the tables off and on in both layouts: the symbol entries built
with the handle against what the kernel used to work out from C[] and the slots.

The counters beside the steps -- `search_requests`, `ktab_lookups`, `jump_lookups`, `row_lookups` -- are held to
tests/golden/search_ends_counters.json: what the commit before the symbol table counted on these very inputs, recorded for every
shape whose counters repeated between two runs of that commit (a pooled launch that flushes its walk list inside the batch loop
walks a parked pattern by rank steps or by the three-step table depending on which wave drew its batch, so its split between
requests and lookups is not a function of the input; such shapes are not in the file)."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 120      # seconds; a child took 6-15 s on the MI355X, most of it the start of the interpreter and the oracle's search
CASES = ["iid-onehot", "iid-bytes", "text-onehot", "text-bytes", "sparse"]
KEYS = {"onehot": {"jump": "auto", "jump_pairs": "on", "search_lanes": "pairs", "ktab": "auto"},
        "bytes": {"jump": "rows3", "jump_pairs": "off", "ktab": "auto"}}
_LINE = re.compile(r"^\[fmx\] (k_search4<[\d,]+>): (\d+) batches over (\d+) waves, the last (\d+) drawn from ticket area (\d+)\s*$", re.M)
MAXLEN = 70
COUNTERS = ("search_requests", "ktab_lookups", "jump_lookups", "row_lookups")
GOLDEN = os.path.join(TESTS, "golden", "search_ends_counters.json")


def counters_of(hip):
    st = hip.stats()
    return [int(st[c]) for c in COUNTERS]


# ---------------------------------------------------------------- the child
def traced(fn):
    """fn() with the process's stderr (the library's FMX_TRACE lines) collected: (fn's result, the launch lines as tuples
    (form, batches, waves, drawn, area))."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    os.write(2, text.encode())
    return out, [(m.group(1),) + tuple(int(m.group(i)) for i in range(2, 6)) for m in _LINE.finditer(text)]


def battery(hip, per_wave, nbatches, syms, seed):
    """nbatches * per_wave patterns from LF walks of the device, ragged by batch (the module's text)."""
    rng = np.random.default_rng(seed)
    k = nbatches * per_wave
    rows = rng.integers(0, hip.n, k).astype(np.uint64)
    b, _ = hip.lf_walk_batch(rows, MAXLEN)
    full = np.ascontiguousarray(b[:, ::-1])
    mode = rng.random(nbatches)
    lo = np.where(mode < 0.15, 66, 0).repeat(per_wave)
    hi = np.where(mode < 0.15, MAXLEN, np.where(mode < 0.30, 3, MAXLEN)).repeat(per_wave)
    lens = lo + (rng.random(k) * (hi - lo + 1)).astype(np.int64)
    mut = np.nonzero((rng.random(k) < 0.3) & (lens > 0))[0]
    pos = MAXLEN - 1 - (rng.random(mut.size) * lens[mut]).astype(np.int64)      # inside the pattern's own bytes
    full[mut, pos] = np.asarray(syms, dtype=np.uint8)[rng.integers(0, len(syms), mut.size)]
    keep = np.arange(MAXLEN)[None, :] >= (MAXLEN - lens)[:, None]
    buf = np.ascontiguousarray(full[keep])
    off = np.zeros(k + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return buf, off


def prefix(buf, off, out, k):
    return buf[:int(off[k])], off[:k + 1], tuple(a[:k] for a in out)


def on_streams(hip, buf, off, out):
    """The batch three times in a row on one stream, then alternately on two: every launch's intervals are the oracle's."""
    import torch
    k = off.size - 1
    d_pat = torch.zeros(buf.size + 64, dtype=torch.uint8, device="cuda")
    d_pat[:buf.size] = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    order = [s1, s1, s1, s1, s2, s1, s2]
    res = [(torch.full((k,), -1, dtype=torch.int64, device="cuda"), torch.full((k,), -1, dtype=torch.int64, device="cuda")) for _ in order]
    torch.cuda.synchronize()

    def launches():
        for st, (sp, ep) in zip(order, res):
            hip.search_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k, st.cuda_stream)
        torch.cuda.synchronize()
    _, lines = traced(launches)
    assert len(lines) == len(order) and all(ln[3] > 0 and ln[4] > 0 for ln in lines), lines
    assert len({ln[4] for ln in lines}) == 2, ("two streams, two ticket areas", lines)
    wsp, wep = out[0].astype(np.int64), out[1].astype(np.int64)
    for i, (sp, ep) in enumerate(res):
        assert np.array_equal(sp.cpu().numpy(), wsp) and np.array_equal(ep.cpu().numpy(), wep), "launch %d of %d on streams" % (i, len(order))


def child_ends(index, layout):
    import findex_amd
    import oracle
    import search_forms as sf
    from helpers import bwt_of_text, synth_bwt
    findex_amd.config_set("tables_after", "0")
    if index == "iid":
        bwt, eof, counts = synth_bwt(300_000, 1, 12, 77)
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
    for key, value in KEYS[layout].items():
        hip.config_set(key, value)
    hip.prepare(ktab=True, jump=True)
    per_wave = 32 if layout == "onehot" else 8
    # the waves of a large launch and the full rounds it hands to the pool come from its own launch line (below)
    big = 9 * 1024
    buf, off = battery(hip, per_wave, big + 3, syms + [foreign], 2)
    out = orc.search_batch(buf, off, threads=min(16, len(os.sched_getaffinity(0))))
    hit = out[0] < out[1]
    assert 0.2 < hit.mean() < 0.9, hit.mean()
    (_, lines) = traced(lambda: sf._compare(hip, out, buf, off, "long"))
    counters = {"long": counters_of(hip)}
    form, nb, nw, drawn, area = lines[-1]
    assert nb == big + 3 and nb // nw >= 8 and area > 0 and drawn > 0 and (drawn - (nb % nw)) % nw == 0, lines
    pool_rounds = (drawn - nb % nw) // nw
    assert 1 <= pool_rounds <= 7, lines
    want_form = {"onehot": (2, 0, 1, 1), "bytes": (0, 3, 0, 0)}[layout]
    got = tuple(int(x) for x in form[len("k_search4<"):-1].split(","))
    assert (got[3], got[4], got[5], got[6]) == want_form, form
    exact = (pool_rounds + 2) * nw
    shapes = [("exact", exact * per_wave, pool_rounds * nw),
              ("nopool", (exact - 1) * per_wave, 0),
              ("uneven", (exact + 5) * per_wave, pool_rounds * nw + 5),
              ("onelast", (exact + 7) * per_wave + 1, pool_rounds * nw + 8)]
    figures = {"form": form, "waves": nw, "pool_rounds": pool_rounds, "hits": int(hit.sum()), "patterns": int(hit.size)}
    for name, k, want_drawn in shapes:
        pb, po, pout = prefix(buf, off, out, k)
        _, lines = traced(lambda: sf._compare(hip, pout, pb, po, name))
        assert len(lines) == 1 and lines[0][0] == form, (name, lines)
        _, nb, nw2, drawn, area = lines[0]
        assert nb == (k + per_wave - 1) // per_wave and nw2 == nw and drawn == want_drawn and (area > 0) == (want_drawn > 0), (name, lines)
        figures[name] = [k, drawn]
        counters[name] = counters_of(hip)
        if name == "exact":
            sf._lean_forms(hip, pout, pb, po)
            on_streams(hip, pb, po, pout)
    hip.close()
    findex_amd.set_layout("auto")
    figures["counters"] = counters
    print("RESULT " + json.dumps(figures))
    print("DONE")


def child_sparse():
    """Symbols {1, 3, 128, 254, 255}: the entries of byte 255 (whose bucket ends at n), of the absent symbols between them
    and of the EOF symbol, in both layouts, with the tables off and on."""
    import findex_amd
    import oracle
    import search_forms as sf
    from helpers import pack_patterns, sparse_alphabet_bwt
    findex_amd.config_set("tables_after", "0")
    bwt, eof, counts = sparse_alphabet_bwt()
    orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
    syms = [int(s) for s in np.nonzero(counts)[0] if s != 0]
    assert syms == [1, 3, 128, 254, 255]
    pats = sf.battery(orc, syms, 4, sf.JUMP_CHARS, 5, ragged=3000)
    pats += [bytes([c]) for c in (0, 2, 4, 127, 129, 253, 254, 255)] + [bytes([255, 1]), bytes([1, 255]), bytes([254, 255, 3])]
    buf, off = pack_patterns(pats)
    out = orc.search_batch(buf, off)
    figures, counters = {}, {}
    for layout in ("onehot", "bytes"):
        for tables in ("off", "on"):
            findex_amd.set_layout(layout)
            hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
            keys = dict(KEYS[layout]) if tables == "on" else {"jump": "off", "jump_pairs": "off", "ktab": "off"}
            for key, value in keys.items():
                hip.config_set(key, value)
            hip.prepare(ktab=True, jump=True)
            _, lines = traced(lambda: sf._compare(hip, out, buf, off, "%s tables %s" % (layout, tables)))
            assert lines, "no k_search4 launch"
            figures["%s-%s" % (layout, tables)] = lines[-1][0]
            counters["%s-%s" % (layout, tables)] = counters_of(hip)
            sf._lean_forms(hip, out, buf, off)
            hip.close()
    findex_amd.set_layout("auto")
    assert len(set(figures.values())) == 4, figures
    figures["counters"] = counters
    print("RESULT " + json.dumps(figures))
    print("DONE")


# ---------------------------------------------------------------- the tests
_FAULT = []      # why no further child is started


@pytest.mark.gpu
@pytest.mark.timeout(CHILD_TIMEOUT + 60)
@pytest.mark.parametrize("case", CASES)
def test_search_ends(case):
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
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    assert want and got is not None
    for shape, values in want.items():
        assert got[shape] == values, "%s %s: %s = %s, the commit before the symbol table counted %s" % (case, shape, COUNTERS, got[shape], values)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    if sys.argv[1] == "sparse":
        child_sparse()
    else:
        child_ends(*sys.argv[1].split("-"))
