"""k_search4's pool on grids whose groups of 32 waves do not divide evenly among the 64 ticket counters (fmx_search4.h, "the
pool"; fmx_pool_deal.h): every counter owns a share of the pool in proportion to its drawers, every pool batch is drawn exactly
once, and every counter is back at zero for the stream's next launch."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_POOL_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, findex_amd, oracle
from helpers import synth_bwt
layout, wgs = sys.argv[2], int(sys.argv[3])
findex_amd.set_layout(layout)
bwt, eof, counts = synth_bwt(500_000, 97, 120, 29)
hip = findex_amd.HipFMSearcher.from_mem(bwt, eof, counts)
if layout == "onehot":
    hip.config_set("jump_pairs", "on")
    hip.config_set("search_lanes", "pairs")
else:
    hip.config_set("jump", "rows3")
hip.prepare(ktab=True, jump=True)
per_wave = 32 if layout == "onehot" else 8                # patterns per wave: pairs of lanes, octets
nwaves = wgs * torch.cuda.get_device_properties(0).multi_processor_count * 4
k = nwaves * per_wave * 9 // 2 - 3                        # four and a half rounds, the last batch short: two and a half are the pool
m = 24
rng = np.random.default_rng(11)
walk, _ = hip.lf_walk_batch(rng.integers(0, bwt.size, size=k), m)
full = np.ascontiguousarray(walk[:, ::-1])
lens = rng.integers(0, m + 1, size=k)                     # ragged, 0 .. 24: the last `len` characters of each walk
miss = (rng.random(k) < 0.1) & (lens > 0)                 # ... a tenth of them with one character changed
col = m - 1 - (rng.random(k) * lens).astype(np.int64)
full[miss, col[miss]] = (full[miss, col[miss]] + 1) % 120 + 1
off = np.zeros(k + 1, dtype=np.int64); off[1:] = np.cumsum(lens)
idx = np.repeat(np.arange(k), lens) * m + (m - np.repeat(lens, lens)) + (np.arange(off[-1]) - np.repeat(off[:-1], lens))
pats = full.reshape(-1)[idx]
dev = torch.device("cuda", 0)
d_pat = torch.from_numpy(pats).to(dev); d_off = torch.from_numpy(off).to(dev)
one = torch.cuda.Stream()
outs = []
def launch(stream):
    sp = torch.full((k,), -1, dtype=torch.int64, device=dev); ep = torch.full((k,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    hip.stats_reset()
    hip.search_batch_dev(d_pat.data_ptr(), d_off.data_ptr(), sp.data_ptr(), ep.data_ptr(), k, stream)
    torch.cuda.synchronize()
    outs.append((sp, ep, hip.stats()["backward_steps"]))
for rep in range(3):          # one after the other on one stream: a counter that is not back at zero, or a batch nobody drew, leaves -1
    launch(one.cuda_stream)
launch(2)                     # hipStreamPerThread has no ticket area: every batch strided
print("POOL k=%d nwaves=%d" % (k, nwaves))
for sp, ep, steps in outs[1:]:
    assert torch.equal(sp, outs[0][0]) and torch.equal(ep, outs[0][1]) and steps == outs[0][2], steps
sp, ep = outs[0][0].cpu().numpy().view(np.uint64), outs[0][1].cpu().numpy().view(np.uint64)
orc = oracle.NaiveFMSearcher.from_mem(bwt, eof, counts)
wsp, wep, wsteps = orc.search_batch(pats, off, threads=8)
for lo, hi in ((0, 4000), (k - (nwaves * per_wave * 5 // 2 - 3), k)):      # the pool is the END of the batch list
    assert np.array_equal(sp[lo:hi], wsp[lo:hi]) and np.array_equal(ep[lo:hi], wep[lo:hi]), (lo, hi)
assert outs[0][2] == int(wsteps.sum()), (outs[0][2], int(wsteps.sum()))    # the steps the reference's loop executes, all patterns
assert 0.8 < float((sp < ep).mean()) < 0.95
print("ok")
"""


@pytest.mark.parametrize("layout,wgs", [("onehot", 3), ("onehot", 5), ("bytes", 3), ("bytes", 7)])
def test_pool_on_an_uneven_deal(layout, wgs):
    """FMX_SEARCH_WGS = 3, 5 or 7 workgroups per CU: on 256 CUs 96, 160 or 224 groups of 32 waves for 64 counters, so half
    of the counters have one more group of drawers than the others (2 : 1, 3 : 2, 4 : 3).  The pairs-of-lanes kernel (one-hot layout)
    and a row-table form of the bytes layout; ragged patterns of 0 .. 24 bytes, a tenth of them misses, four and a half rounds of
    the grid, so that two full rounds and the partial one are drawn.  Three launches on one stream into outputs refilled with
    -1 and one on hipStreamPerThread (strided throughout) give equal results and equal executed steps; the first 4000 and
    the last two and a half rounds of patterns are the oracle's, the executed steps the oracle's over the whole batch.
    FMX_TRACE must show the three pooled launches with the pool the host computes -- the batches past all full rounds but
    two -- on one ticket area, and the fourth with none.  (A child process: FMX_SEARCH_WGS is read once per process.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FMX_TRACE="1", FMX_SEARCH_WGS=str(wgs))
    r = subprocess.run([sys.executable, "-c", _POOL_SCRIPT, root, layout, str(wgs)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    k, nwaves = map(int, re.search(r"POOL k=(\d+) nwaves=(\d+)", r.stdout).groups())
    per_wave = 32 if layout == "onehot" else 8
    nbatch = (k + per_wave - 1) // per_wave
    lines = [tuple(map(int, m.groups())) for m in
             re.finditer(r"k_search4<[^>]*>: (\d+) batches over (\d+) waves, the last (\d+) drawn from ticket area (\d+)", r.stderr)]
    lines = [ln for ln in lines if ln[0] == nbatch]           # (the searches of this batch, not what fmx_prepare may launch)
    assert len(lines) == 4, r.stderr[-3000:]
    assert (nwaves // 32) % 64 != 0                           # the deal is uneven: what this test is for
    drawn = nbatch - (nbatch // nwaves - 2) * nwaves          # as launch_form computes it: all full rounds but two are strided
    area = lines[0][3]
    assert area > 0 and lines[:3] == [(nbatch, nwaves, drawn, area)] * 3, lines
    assert lines[3] == (nbatch, nwaves, 0, 0), lines
