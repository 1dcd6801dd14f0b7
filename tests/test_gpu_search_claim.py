"""Where a wave of k_search4's pool claims its next batch (fmx_search4.h, "the pool"): a drawn batch of the pairs-of-lanes
kernels draws the wave's next ticket beside its last row-jump lookup, or behind its loop when there was none to stand beside.
Moving the claim moves an atomic and no work: every pool batch is still searched exactly once, every counter is back at zero
for the stream's next launch, the results and the executed steps are the oracle's, and the lookups a launch makes are the ones
recorded from the commit before the claim moved (tests/golden/search_claim_counters.json)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

WGS = 3                       # workgroups per CU: 96 groups of 32 waves for 64 counters on 256 CUs, an uneven deal (2 : 1)
PER_WAVE = 32                 # patterns per wave: pairs of lanes
COUNTERS = ("search_requests", "ktab_lookups", "jump_lookups", "row_lookups", "rank_queries")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_claim_counters.json")

_CLAIM_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, findex_amd, oracle
from helpers import synth_bwt
case, wgs = sys.argv[2], int(sys.argv[3])
findex_amd.set_layout("onehot")
bwt, eof, counts = synth_bwt(500_000, 97, 120, 29)
hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
hip.config_set("jump_pairs", "on")
hip.config_set("search_lanes", "pairs")
hip.prepare(ktab=True, jump=True)
orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
# This index is too small for a k-mer table the search uses (24 symbols, 24^4 entries > n / 8: the table stops at depth 3 and the
# kernel's form has KT = 0): step 0 is taken from the symbol table, the step loop begins at step 1, and the first TABLE lookup a
# pattern can make is a row-jump lookup (pairs of entries of jc = 9 characters), issued once every live group of its wave holds at
# most four rows -- step 5 as a rule, 24^5 being 16 n.
per_wave = 32
nwaves = wgs * torch.cuda.get_device_properties(0).multi_processor_count * 4
k = nwaves * per_wave * 9 // 2 - 3                        # four and a half rounds, the last batch short: two and a half are the pool
rng = np.random.default_rng(11)
kind = case.split(":")
hits_lo, hits_hi = 0.0, 1.0                               # the share of patterns that occur, as the case is built
if kind[0] == "eq":                                       # equal lengths: every group of a batch ends on the same kind of step
    m = int(kind[1])
    lens = np.full(k, m, dtype=np.int64)
    frac = 0.1 if kind[2] == "miss" else 0.0
    hits_lo, hits_hi = (0.85, 0.95) if frac else (1.0, 1.0)
elif kind[0] == "ragged":                                 # tests/test_gpu_search_pool.py's inputs: most claims fall behind the loop
    m, frac = 24, 0.1
    lens = rng.integers(0, m + 1, size=k)
    hits_lo, hits_hi = 0.8, 0.95
elif kind[0] == "short":                                  # lengths 0 and 1: step 0 is not the loop's (KT = 0), which ends before its first step
    m, frac = 1, 0.0
    lens = rng.integers(0, 2, size=k)
    hits_lo, hits_hi = 1.0, 1.0
elif kind[0] == "minpool":                                # exactly four rounds: the smallest pool the host hands out, two batches per wave
    m, frac = 24, 0.1
    k = nwaves * per_wave * 4
    lens = rng.integers(0, m + 1, size=k)
    hits_lo, hits_hi = 0.8, 0.95
else:
    assert kind[0] == "allmiss"
    m, frac = 24, 0.0
walk, _ = hip.lf_walk_batch(rng.integers(0, bwt.size, size=k), m)
full = np.ascontiguousarray(walk[:, ::-1])
if kind[0] == "allmiss":
    # EVERY pattern is a text of 24 characters with the character of one of its steps 6 .. 14 (counted from its end) changed to
    # another symbol of the alphabet: its interval is one row (four at most) from step 5 on, so the first row-jump lookup of its
    # batch -- a pair of entries, steps 5 .. 22 as a rule, with 19 characters left: not the batch's last -- finds that it misses.
    # The batch loses all its groups to a lookup it did not claim beside and draws behind its loop.
    lens = np.full(k, m, dtype=np.int64)
    col = m - 1 - rng.integers(6, 15, size=k)
    full[np.arange(k), col] = (full[np.arange(k), col] - 97 + rng.integers(1, 24, size=k)) % 24 + 97
    hits_lo, hits_hi = 0.0, 0.001
else:
    if frac:                                              # a tenth of them with one character changed
        miss = (rng.random(k) < frac) & (lens > 0)
        col = m - 1 - (rng.random(k) * lens).astype(np.int64)
        full[miss, col[miss]] = (full[miss, col[miss]] + 1) % 120 + 1
off = np.zeros(k + 1, dtype=np.int64); off[1:] = np.cumsum(lens)
idx = np.repeat(np.arange(k), lens) * m + (m - np.repeat(lens, lens)) + (np.arange(off[-1]) - np.repeat(off[:-1], lens))
pats = full.reshape(-1)[idx] if off[-1] else np.zeros(0, dtype=np.uint8)
dev = torch.device("cuda", 0)
d_pat = torch.from_numpy(np.concatenate([pats, np.zeros(16, dtype=np.uint8)])).to(dev); d_off = torch.from_numpy(off).to(dev)
one = torch.cuda.Stream()
outs = []
def launch(stream):
    sp = torch.full((k,), -1, dtype=torch.int64, device=dev); ep = torch.full((k,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    hip.stats_reset()
    hip.search_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k, stream)
    torch.cuda.synchronize()
    st = hip.stats()
    outs.append((sp, ep, st["backward_steps"], {c: int(st[c]) for c in sys.argv[4].split(",")}))
for rep in range(3):          # one after the other on one stream: a counter that is not back at zero, or a batch nobody drew, leaves -1
    launch(one.cuda_stream)
launch(2)                     # hipStreamPerThread has no ticket area: every batch strided
print("CLAIM k=%d nwaves=%d" % (k, nwaves))
print("TABLES ktab_k=%d jump_chars=%d" % (hip.stats()["ktab_k"], hip.stats()["jump_chars"]))
for i, o in enumerate(outs):
    print("COUNTERS %d %s steps=%d" % (i, json.dumps(o[3], sort_keys=True), o[2]))
for sp, ep, steps, _ in outs[1:]:
    assert torch.equal(sp, outs[0][0]) and torch.equal(ep, outs[0][1]) and steps == outs[0][2], steps
sp, ep = outs[0][0].cpu().numpy().view(np.uint64), outs[0][1].cpu().numpy().view(np.uint64)
wsp, wep, wsteps = orc.search_batch(pats, off, threads=8)
assert np.array_equal(sp, wsp) and np.array_equal(ep, wep)
assert outs[0][2] == int(wsteps.sum()), (outs[0][2], int(wsteps.sum()))    # the steps the reference's loop executes, all patterns
assert hits_lo <= float(((sp < ep) | (lens == 0)).mean()) <= hits_hi, float(((sp < ep) | (lens == 0)).mean())
print("ok")
"""

CASES = (["eq:%d:%s" % (m, h) for m in list(range(19, 41, 3)) + [23, 32, 41] for h in ("hits", "miss")] +
         ["ragged", "allmiss", "short", "minpool"])


def run_case(case, env_extra=None):
    """One case in a child process (FMX_SEARCH_WGS is read once per process): asserts what every case asserts about results,
    steps and launch lines, and returns (k, nwaves, the counters of its four launches)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FMX_TRACE="1", FMX_SEARCH_WGS=str(WGS))
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, "-c", _CLAIM_SCRIPT, root, case, str(WGS), ",".join(COUNTERS)], capture_output=True, text=True,
                       timeout=600, env=env)
    for line in r.stdout.splitlines():
        if line.startswith(("CLAIM", "TABLES", "COUNTERS")):
            print(case, line)                                 # every figure before anything is asserted about it
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    k, nwaves = map(int, re.search(r"CLAIM k=(\d+) nwaves=(\d+)", r.stdout).groups())
    nbatch = (k + PER_WAVE - 1) // PER_WAVE
    lines = [tuple(map(int, m.groups())) for m in
             re.finditer(r"k_search4<[^>]*>: (\d+) batches over (\d+) waves, the last (\d+) drawn from ticket area (\d+)", r.stderr)]
    lines = [ln for ln in lines if ln[0] == nbatch]           # (the searches of this batch, not what fmx_prepare may launch)
    assert len(lines) == 4, r.stderr[-3000:]
    assert (nwaves // 32) % 64 != 0                           # the deal is uneven
    drawn = nbatch - (nbatch // nwaves - 2) * nwaves          # as launch_form computes it: all full rounds but two are strided
    area = lines[0][3]
    assert area > 0 and lines[:3] == [(nbatch, nwaves, drawn, area)] * 3, lines
    assert lines[3] == (nbatch, nwaves, 0, 0), lines
    counters = [json.loads(m.group(1)) for m in re.finditer(r"COUNTERS \d (\{.*?\}) steps", r.stdout)]
    assert len(counters) == 4
    return k, nwaves, counters


@pytest.mark.parametrize("case", CASES)
def test_claim_moves_no_work(case):
    """FMX_SEARCH_WGS = 3 (3072 waves on 256 CUs, counters with 64 and 32 drawers), the pairs-of-lanes kernel over pairs of row-jump
    entries, four and a half rounds of the grid so that two and a half are drawn.  The index (500 000 rows, 24 symbols) is too small
    for a k-mer table the search uses: the form has KT = 0, the step loop begins at step 1, and a batch's first row-jump lookup
    (jc = 9, pairs: up to 18 steps) goes out once every live group holds at most four rows, at step 5 as a rule.  Cases:
      * eq:M:hits / eq:M:miss -- equal lengths M = 19 .. 40 in steps of 3, all hits and with a tenth of the patterns changed in one
        character: batches that end on a pair lookup, a single lookup, a three-step word or a rank step, depending on the step at
        which the batch became narrow; and M = 23, 32, 41 (5 + 18, 5 + 27, 5 + 36), where a batch that is narrow at step 5 ends
        exactly on a lookup -- the lengths at which the claim beside a lookup is the rule (profiles/claim_c3_ab.md has the counts
        of claims beside a lookup and behind the loop for every case, from a logging build);
      * ragged -- the pool test's lengths 0 .. 24 with a tenth misses: most claims fall behind the loop;
      * allmiss -- every pattern is a text of 24 characters with one character changed 6 .. 14 steps from its end: the batch's first
        row-jump lookup, which is not its last (19 characters left), finds every group to miss, and the batch draws behind its loop;
      * short -- lengths 0 and 1: the loop of a KT = 0 form ends before its first step, the batch draws with no loop behind it;
      * minpool -- exactly four rounds, the smallest pool there is.  (A pool with fewer batches than waves, which the issue behind
        this test also asked for, does not exist: the host pools only from four rounds on and then always two full rounds or more,
        fmx_search.hip, kPoolRounds.)
    Three launches on one stream into outputs refilled with -1 and one on hipStreamPerThread (strided throughout): equal (sp, ep)
    and equal executed steps among the four; every (sp, ep) and the step total the oracle's; FMX_TRACE shows the pool the host
    computes on one ticket area for the first three and none for the fourth; and the requests and lookups of each of the three
    pooled launches are the ones the commit before the claim moved made on these inputs.
    In `allmiss` two of the five counters have no single value in the parent commit itself: 32 patterns are parked per batch, so a
    wave walks parked patterns in the middle of the launch, those of consecutive batches of its own together, and how many
    three-step words such a walk takes (each in place of one to three one-request rank steps) depends on which batches, and how
    many, a wave draws -- which differs from launch to launch and, on purpose, between the parent and this change.  Pooled launches
    of the parent gave row_lookups 213 194 .. 214 977 and search_requests 4 365 725 .. 4 371 074, of this change 209 322 .. 212 412 and
    4 373 420 .. 4 382 691 (0.2 % more requests), while jump_lookups, ktab_lookups, rank_queries and the executed steps were the same in
    every launch of both, and the STRIDED launch, whose batches are assigned statically, gave 216 952 and 4 359 800 every time in both.
    For such a case the golden file holds the counters that are the same in all four launches of the parent, which every pooled
    launch must equal, and the five counters of the parent's strided launch (`strided`), which the strided launch must equal."""
    k, nwaves, counters = run_case(case)
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert nwaves == gold["nwaves"], "the recorded counters are those of %d waves" % gold["nwaves"]
    want = gold["cases"][case]
    assert k == want["k"]
    for i in range(3):
        assert {c: counters[i][c] for c in want["counters"]} == want["counters"], (i, counters[i], want["counters"])
    if "strided" in want:
        assert counters[3] == want["strided"], (counters[3], want["strided"])
