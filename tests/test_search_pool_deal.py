"""How k_search4's pool of drawn batches is dealt to its ticket counters (findex_amd/csrc/fmx_pool_deal.h): the arithmetic the
kernel runs, compiled for the host into a stand-alone program and swept over grids and pool sizes.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "findex_amd", "csrc")

_PROGRAM = r"""
#include "fmx_pool_deal.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (bad++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the equal shares the kernel dealt before fmx_pool_deal.h (counter c owned pool batches c, c + nshards, ...)
static uint32_t equal_share(uint32_t npool, uint32_t nshards, uint32_t shard) {
  return npool > shard ? (npool - shard + nshards - 1u) / nshards : 0u;
}

static void sweep(uint32_t nwaves) {
  const uint32_t nshards = fmx::pool_shards(nwaves);
  CHECK(nshards == ((nwaves + 31u) / 32u < 64u ? (nwaves + 31u) / 32u : 64u), "nwaves %u: %u counters", nwaves, nshards);
  std::vector<uint32_t> brute(nshards, 0);
  for (uint32_t w = 0; w < nwaves; w++) {
    const uint32_t c = fmx::pool_shard_of(w, nwaves);
    CHECK(c == (w >> 5) % nshards, "wave %u of %u: counter %u", w, nwaves, c);
    brute[c]++;
  }
  const uint64_t pools[] = {0, 1, (uint64_t)nshards - 1, nshards, 2ull * nwaves, 2ull * nwaves + 1, 3ull * nwaves - 1};
  for (uint64_t np : pools) {
    const uint32_t npool = (uint32_t)np;
    uint64_t next = 0, drawers = 0;
    for (uint32_t c = 0; c < nshards; c++) {
      const fmx::PoolDeal d = fmx::pool_deal(nwaves, c, npool);
      // contiguous, in the counters' order: disjoint, and together [0, npool) when the last one ends there
      CHECK(d.first == next, "nwaves %u npool %u counter %u: first %u, the one before ends at %llu", nwaves, npool, c, d.first, (unsigned long long)next);
      next = (uint64_t)d.first + d.count;
      CHECK(d.drawers == brute[c], "nwaves %u counter %u: %u drawers, %u waves draw from it", nwaves, c, d.drawers, brute[c]);
      drawers += d.drawers;
      // |count - npool * drawers / nwaves| < 1, in integers
      const long long dev = (long long)d.count * nwaves - (long long)npool * d.drawers;
      CHECK(dev < (long long)nwaves && -dev < (long long)nwaves, "nwaves %u npool %u counter %u: %u batches for %u of %u drawers", nwaves, npool, c, d.count, d.drawers, nwaves);
    }
    CHECK(next == npool, "nwaves %u npool %u: the ranges end at %llu", nwaves, npool, (unsigned long long)next);
    CHECK(drawers == nwaves, "nwaves %u: %llu drawers", nwaves, (unsigned long long)drawers);
  }
}

int main() {
  unsigned swept = 0;
  bool saw[3] = {false, false, false};
  for (uint32_t nwaves = 4; nwaves <= 8192; nwaves += 4) {
    sweep(nwaves);
    swept++;
    saw[0] |= nwaves == 5120; saw[1] |= nwaves == 7168; saw[2] |= nwaves == 3072;
  }
  CHECK(saw[0] && saw[1] && saw[2], "5120, 7168 and 3072 waves were not all swept");
  // grids whose npool * drawers does not fit 32 bits: the 64-bit product and its long division
  const uint32_t big[] = {65536u * 3u + 4u, (1u << 20) + 36u, 1000003u};
  for (uint32_t nwaves : big) sweep(nwaves);
  CHECK(fmx::pool_muldiv(0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu) == 0xFFFFFFFEu && fmx::pool_muldiv(3000000000u, 7u, 11u) == 1909090909u, "pool_muldiv");
  // what this header is for: 5120 waves are 160 groups, three for counters 0..31 and two for the others.  Equal shares miss the
  // bound there; the deal in proportion keeps it.
  {
    const uint32_t nwaves = 5120, nshards = fmx::pool_shards(nwaves), npool = 2u * nwaves + 1u;
    unsigned missed = 0;
    for (uint32_t c = 0; c < nshards; c++) {
      const fmx::PoolDeal d = fmx::pool_deal(nwaves, c, npool);
      const long long dev = (long long)equal_share(npool, nshards, c) * nwaves - (long long)npool * d.drawers;
      missed += dev >= (long long)nwaves || -dev >= (long long)nwaves;
    }
    CHECK(nshards == 64 && missed == 64, "equal shares at 5120 waves miss the bound on %u of %u counters", missed, nshards);
    const fmx::PoolDeal a = fmx::pool_deal(nwaves, 0, npool), b = fmx::pool_deal(nwaves, 63, npool);
    CHECK(a.drawers == 96 && b.drawers == 64 && a.count == 192 && (b.count == 128 || b.count == 129), "5120 waves: %u for %u, %u for %u", a.count, a.drawers, b.count, b.drawers);
  }
  std::printf("%s: %u grids swept, %d checks failed\n", bad ? "FAILED" : "ok", swept, bad);
  return bad ? 1 : 0;
}
"""


def _compile(tmp_path, flags):
    src = tmp_path / "pool_deal.cpp"
    src.write_text(_PROGRAM)
    exe = tmp_path / "pool_deal"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags + [str(src), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_pool_is_dealt_in_proportion_to_drawers(tmp_path):
    """fmx_pool_deal.h, by the host compiler alone (the header includes nothing from HIP), under the undefined-behaviour and
    address sanitizers where the host has their runtimes: for 4 .. 8192 waves in steps of 4 (and a few grids past 2^16
    waves) and pools of 0, 1, nshards - 1, nshards, 2 nwaves, 2 nwaves + 1 and 3 nwaves - 1 batches, the
    counters' ranges are disjoint and together exactly [0, npool), their drawers are the waves that draw from them (a
    brute-force count) and sum to the grid, and every counter's share is within one batch of npool * drawers / nwaves --
    which equal shares miss at 5120 waves, the benchmark's grid."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe, r = _compile(tmp_path, ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:
        exe, r = _compile(tmp_path, [])          # a host without the sanitizers' runtimes: the same checks without them
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().startswith("ok: 2048 grids swept"), out.stdout[-3000:] + out.stderr[-3000:]


def test_the_kernel_deals_with_the_tested_header():
    """The kernel calls the function the program above sweeps, with the counters per area that program assumes."""
    with open(os.path.join(CSRC, "fmx_search4.h")) as f:
        kernel = f.read()
    assert '#include "fmx_pool_deal.h"' in kernel and "pool_deal(" in kernel and "pool_shard_of(" in kernel
    with open(os.path.join(CSRC, "fmx_device.h")) as f:
        assert re.search(r"constexpr uint32_t kTixShards = 64;", f.read())
    with open(os.path.join(CSRC, "fmx_pool_deal.h")) as f:
        header = f.read()
    assert re.search(r"constexpr uint32_t kPoolShards = 64;", header)
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", header)
    assert includes == ["stdint.h"], includes
